// kern_solver.hip -- mjhip_forwardSolveBatch's kernel: k_forward_solve, mj_forward with the
// Newton constraint solver (csrc/solver.h), one lane per instance. Its own translation unit of
// libmjhip.so, compiled without multiply-add contraction (__graft_entry__.UNIT_FLAGS) as
// kern_step.hip is.
#define MJHIP_KERNEL_UNIT 1
#include "kernels.h"
#include "solver_call.h"
#include "solver.h"

// the same 4,096 B kernel-argument segment as every other kernel (mjhip.hip)
static_assert(sizeof(mjhipModel) + sizeof(Mirror) + sizeof(SolverCall) <= 4096,
              "mjhipModel + Mirror + SolverCall exceed the 4,096 B kernel-argument segment");

// One lane per instance, 64-instance blocks (k_forward's shape). A lane's iteration count
// depends on its own rows: a lane without rows is done after the smooth stages and then waits
// for the slowest lane of its wave.
template <bool CONTACT>
__global__ __launch_bounds__(64) void k_forward_solve(mjhipModel m, Mirror mr, SolverCall a) {
  const int blk = blockIdx.x, lane = threadIdx.x;
  const long inst = (long)blk*64 + lane;
  if (inst >= a.B) return;
  const int nq = m.nq, nv = m.nv, nu = m.nu, na = m.na;
  Lane<64> d = lane_view(mr, blk, lane);
  const mjh::SolverLayout L = mjh::solverLayout(&m, mr.efc_cap);
  const mjh::SolverScratch<64> sc =
      mjh::solverBind<64>(L, a.scratch + (long)blk*64*L.total, lane);
  if (a.qpos) for (int k = 0; k < nq; k++) d.qpos[k] = a.qpos[inst*nq + k];
  if (a.qvel) for (int k = 0; k < nv; k++) d.qvel[k] = a.qvel[inst*nv + k];
  if (a.ctrl) for (int k = 0; k < nu; k++) d.ctrl[k] = a.ctrl[inst*nu + k];
  if (a.act) for (int k = 0; k < na; k++) d.act[k] = a.act[inst*na + k];
  if (a.qacc_warmstart) {
    for (int k = 0; k < nv; k++) sc.qacc_warmstart[k] = a.qacc_warmstart[inst*nv + k];
  }
  mjh::SolverOpt opt;
  opt.tolerance = a.tolerance;
  opt.ls_tolerance = a.ls_tolerance;
  opt.meaninertia = a.meaninertia;
  opt.iterations = a.iterations;
  opt.ls_iterations = a.ls_iterations;
  int niter = 0;
  const int st = mjh::forward<64, CONTACT>(m, d, sc, opt, &niter);
  a.status[inst] = st;
  if (a.niter) a.niter[inst] = niter;
  if (a.qacc) for (int k = 0; k < nv; k++) a.qacc[inst*nv + k] = d.qacc[k];
  if (a.qfrc_constraint) {
    for (int k = 0; k < nv; k++) a.qfrc_constraint[inst*nv + k] = d.qfrc_constraint[k];
  }
  if (a.act_dot) for (int k = 0; k < na; k++) a.act_dot[inst*na + k] = d.act_dot[k];
  if (a.act_next) for (int k = 0; k < na; k++) a.act_next[inst*na + k] = d.act_next[k];
}

long mjhip_solverScratchDoubles(const mjhipModel* hm, int efc_cap) {
  return mjh::solverLayout(hm, efc_cap).total;
}

int mjhip_launchForwardSolve(hipStream_t s, const mjhipModel& dmodel, const Mirror& mr,
                             const SolverCall& call, bool contact) {
  const dim3 grid((call.B + 63)/64), block(64);
  if (contact) hipLaunchKernelGGL(k_forward_solve<true>, grid, block, 0, s, dmodel, mr, call);
  else hipLaunchKernelGGL(k_forward_solve<false>, grid, block, 0, s, dmodel, mr, call);
  return hipGetLastError() != hipSuccess;
}
