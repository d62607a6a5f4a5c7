// kern_transition.hip -- mjhip_transitionFDBatch's kernels: k_transition, one lane per
// evaluation of mj_stepSkip (csrc/step.h, csrc/transition.h), and k_transition_diff, the
// differencing into the transposed A and B. Its own translation unit of libmjhip.so, compiled
// without multiply-add contraction (__graft_entry__.UNIT_FLAGS) as kern_step.hip is.
#define MJHIP_KERNEL_UNIT 1
#include "kernels.h"
#include "transition_call.h"
#include "transition.h"

// the same 4,096 B kernel-argument segment as every other kernel (mjhip.hip)
static_assert(sizeof(mjhipModel) + sizeof(Mirror) + sizeof(TransitionCall) + 2*sizeof(int) <= 4096,
              "mjhipModel + Mirror + TransitionCall exceed the 4,096 B kernel-argument segment");

// Evaluation blocks [first, first + gridDim.x) of the call (transition.h): block g < nblk is a
// centre block, the others are perturbed evaluations. skipstage, the perturbation and the
// centre block are uniform over a block (one wave), so the stages skipped cost no divergence.
// The two kinds of block run as separate launches in stream order (centres first): a
// perturbed lane reads its centre's stage outputs, factor and status.
template <bool CONTACT>
__global__ __launch_bounds__(64) void k_transition(mjhipModel m, Mirror mr, TransitionCall a,
                                                   int first) {
  const int g = first + blockIdx.x, lane = threadIdx.x;
  const int nblk = a.nblk, cb = g % nblk, slot = g / nblk - 1;
  const long Bp = (long)nblk*64, b = (long)cb*64 + lane;
  if (b >= a.B) return;
  const int nq = m.nq, nv = m.nv, na = m.na, nu = m.nu, nx = 6*m.nbody;
  const mjh::TransitionPlan plan = mjh::transitionPlan(m, a.want_A != 0, a.want_B != 0,
                                                       a.centered != 0);
  Lane<64> d = lane_view(mr, g, lane);
  const mjh::StepLayout L = mjh::stepLayout(&m);
  mjh::StepScratch<64> sc = mjh::stepBind<64>(L, d, a.scratch + (long)g*64*L.total, lane);
  double* y = a.Y + (long)(slot + 1)*(nq + nv + na)*Bp + b;
  if (slot >= 0 && a.cstatus[b]) return;    // the base state's matrices are zeros already
  for (int k = 0; k < nq; k++) d.qpos[k] = a.qpos[b*nq + k];
  for (int k = 0; k < nv; k++) d.qvel[k] = a.qvel[b*nv + k];
  for (int k = 0; k < na; k++) d.act[k] = a.act ? a.act[b*na + k] : 0.0;
  for (int k = 0; k < nu; k++) d.ctrl[k] = a.ctrl ? a.ctrl[b*nu + k] : 0.0;
  for (int k = 0; k < nv; k++) d.qfrc_applied[k] = a.qfrc_applied ? a.qfrc_applied[b*nv + k] : 0.0;
  for (int k = 0; k < nx; k++) d.xfrc_applied[k] = a.xfrc_applied ? a.xfrc_applied[b*nx + k] : 0.0;
  int skipstage = mjhipSTAGE_NONE;
  if (slot >= 0) {
    int kind, i, s;
    mjh::transitionDecode(plan, slot, &kind, &i, &s);
    if (!mjh::transitionPerturb(m, d, kind, i, s, a.eps, a.centered != 0)) return;
    skipstage = mjh::transitionSkipstage(kind);
    Lane<64> c = lane_view(mr, cb, lane);
    mjh::aliasMocap(d, c);
    if (skipstage > mjhipSTAGE_NONE) {
      const mjh::StepScratch<64> csc =
          mjh::stepBind<64>(L, c, a.scratch + (long)cb*64*L.total, lane);
      mjh::aliasSkipped(d, c, skipstage);
      mjh::aliasFactor(m, d, sc, c, csc, skipstage);
    }
  }
  const int st = mjh::stepSkip<64, CONTACT>(m, d, sc, skipstage);
  if (slot < 0) {
    a.status[b] = st;
    if (a.cstatus) a.cstatus[b] = st;
  } else if (st) {
    atomicOr(a.status + b, st);
  }
  for (int k = 0; k < nq; k++) y[k*Bp] = d.qpos[k];
  for (int k = 0; k < nv; k++) y[(nq + k)*Bp] = d.qvel[k];
  for (int k = 0; k < na; k++) y[(nq + nv + k)*Bp] = d.act[k];
}

// Thread (b = blockIdx.x, column c): c < ncolA is column c of A[b] ([q | v | a]), the others
// column c - ncolA of B[b]. A wave's 64 columns of one output row are consecutive doubles.
__global__ __launch_bounds__(64) void k_transition_diff(mjhipModel m, TransitionCall a) {
  const int nv = m.nv, na = m.na, nu = m.nu, ndx = 2*nv + na;
  const int ncolA = a.want_A ? ndx : 0, ncol = ncolA + (a.want_B ? nu : 0);
  const int c = blockIdx.y*64 + threadIdx.x;
  const long b = blockIdx.x, Bp = (long)a.nblk*64;
  if (c >= ncol) return;
  const mjh::TransitionPlan plan = mjh::transitionPlan(m, a.want_A != 0, a.want_B != 0,
                                                       a.centered != 0);
  const bool isB = c >= ncolA;
  const int col = isB ? c - ncolA : c;
  const int kind = isB ? mjh::kTrCtrl : col < nv ? mjh::kTrQpos
                                      : col < 2*nv ? mjh::kTrQvel : mjh::kTrAct;
  const int i = isB ? col : col < nv ? col : col < 2*nv ? col - nv : col - 2*nv;
  const int width = isB ? nu : ndx;
  double* out = (isB ? a.Bm + b*ndx*nu : a.A + b*ndx*ndx) + col;
  if (a.status[b]) {
    for (int r = 0; r < ndx; r++) out[(long)r*width] = 0.0;
    return;
  }
  const long nstate = m.nq + nv + na;
  mjh::transitionColumn(
      m, plan, kind, i, a.eps, a.centered != 0, isB && a.ctrl ? a.ctrl[b*nu + i] : 0.0,
      [&](int slot) { return mjh::Strided{a.Y + (long)(slot + 1)*nstate*Bp + b, Bp}; },
      [&](int r, double v) { out[(long)r*width] = v; });
}

int mjhip_transitionSlots(const mjhipModel* hm, int want_A, int want_B, int centered) {
  return mjh::transitionPlan(*hm, want_A != 0, want_B != 0, centered != 0).P;
}

int mjhip_launchTransition(hipStream_t s, const mjhipModel& dmodel, const Mirror& mr,
                           const TransitionCall& call, int P, bool contact) {
  const dim3 block(64);
  const unsigned nblk = (unsigned)call.nblk;
  for (int pass = 0; pass < 2; pass++) {
    const dim3 grid(pass ? nblk*(unsigned)P : nblk);
    const int first = pass ? call.nblk : 0;
    if (!grid.x) continue;
    if (contact) hipLaunchKernelGGL(k_transition<true>, grid, block, 0, s, dmodel, mr, call, first);
    else hipLaunchKernelGGL(k_transition<false>, grid, block, 0, s, dmodel, mr, call, first);
    if (hipGetLastError() != hipSuccess) return 1;
  }
  const int ndx = 2*dmodel.nv + dmodel.na;
  const int ncol = (call.want_A ? ndx : 0) + (call.want_B ? dmodel.nu : 0);
  if (ncol) {
    hipLaunchKernelGGL(k_transition_diff, dim3(call.B, (ncol + 63)/64), block, 0, s, dmodel, call);
  }
  return hipGetLastError() != hipSuccess;
}
