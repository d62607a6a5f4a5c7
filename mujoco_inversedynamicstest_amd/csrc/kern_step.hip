// kern_step.hip -- mjhip_rolloutBatch's kernel: T steps of mj_step (csrc/step.h) per instance
// in one launch, in its own translation unit of libmjhip.so, compiled without multiply-add
// contraction (__graft_entry__.UNIT_FLAGS) as the oracle is.
#define MJHIP_KERNEL_UNIT 1
#include "kernels.h"
#include "rollout.h"
#include "step.h"

// the same 4,096 B kernel-argument segment as every other kernel (mjhip.hip)
static_assert(sizeof(mjhipModel) + sizeof(Mirror) + sizeof(RolloutCall) + sizeof(int) <= 4096,
              "mjhipModel + Mirror + RolloutCall exceed the 4,096 B kernel-argument segment");

// columns of a block's rows collected in LDS per pass: 64 rows of kRollChunk doubles, one
// pad column against bank conflicts
constexpr int kRollChunk = 32;

// Row t of each of the block's instances (n doubles, get(k) the lane's k-th) into
// out[B][T][n]. A lane writing its own row scatters the wave over 64 rows T*n*8 bytes apart
// (direct); otherwise the block's rows go through LDS and half a wave writes one row's
// consecutive doubles. Every lane of the block calls this (the LDS form synchronizes; direct
// is uniform over the grid).
template <class Get>
__device__ __forceinline__ void writeRows(bool direct, double* __restrict__ out, double* lds,
                                          long inst0, int lane, bool valid, int B, int T,
                                          int t, int n, Get get) {
  if (direct) {
    if (valid) {
      double* row = out + ((inst0 + lane)*T + t)*n;
      for (int k = 0; k < n; k++) row[k] = get(k);
    }
  } else {
    for (int c0 = 0; c0 < n; c0 += kRollChunk) {
      const int nc = n - c0 < kRollChunk ? n - c0 : kRollChunk;
      if (valid) {
        for (int k = 0; k < nc; k++) lds[lane*(kRollChunk + 1) + k] = get(c0 + k);
      }
      __syncthreads();
      const int k = lane & (kRollChunk - 1);
      for (int r = lane / kRollChunk; r < 64; r += 64 / kRollChunk) {
        if (inst0 + r < B && k < nc) {
          out[((inst0 + r)*T + t)*n + c0 + k] = lds[r*(kRollChunk + 1) + k];
        }
      }
      __syncthreads();
    }
  }
}

// One lane per instance, 64-instance blocks (k_forward's shape). No lane returns before the
// last step: a stopped or padding lane still takes part in its block's LDS write-out.
// direct: the A/B form of the row stores. MJHIP_ROLLOUT_DIRECT_STORE makes it the build's
// default; MJHIP_ROLLOUT_DIRECT=1 in the environment asks for it at run time (mjhip.hip). It
// is a kernel argument and not a template parameter because each instantiation of the step
// compiles for minutes.
#ifdef MJHIP_ROLLOUT_DIRECT_STORE
constexpr bool kRolloutDirectDefault = true;
#else
constexpr bool kRolloutDirectDefault = false;
#endif
template <bool CONTACT>
__global__ __launch_bounds__(64) void k_rollout(mjhipModel m, Mirror mr, RolloutCall a,
                                                int direct_store) {
  __shared__ double lds[64*(kRollChunk + 1)];
  const bool direct = direct_store != 0;
  const int blk = blockIdx.x, lane = threadIdx.x;
  const long inst0 = (long)blk*64, inst = inst0 + lane;
  const bool valid = inst < a.B;
  const int nq = m.nq, nv = m.nv, na = m.na, nu = m.nu, nx = 6*m.nbody, T = a.T;
  Lane<64> d = lane_view(mr, blk, lane);
  const mjh::StepLayout L = mjh::stepLayout(&m);
  const mjh::StepScratch<64> sc = mjh::stepBind<64>(L, d, a.scratch + inst0*L.total, lane);
  if (valid) {
    if (a.qpos) for (int k = 0; k < nq; k++) d.qpos[k] = a.qpos[inst*nq + k];
    if (a.qvel) for (int k = 0; k < nv; k++) d.qvel[k] = a.qvel[inst*nv + k];
    if (a.act) for (int k = 0; k < na; k++) d.act[k] = a.act[inst*na + k];
    if (a.ctrl_mode == kRolloutHeld) for (int k = 0; k < nu; k++) d.ctrl[k] = a.ctrl[inst*nu + k];
    if (a.qfrc_mode == kRolloutHeld) {
      for (int k = 0; k < nv; k++) d.qfrc_applied[k] = a.qfrc_applied[inst*nv + k];
    }
    if (a.xfrc_mode == kRolloutHeld) {
      for (int k = 0; k < nx; k++) d.xfrc_applied[k] = a.xfrc_applied[inst*nx + k];
    }
  }
  bool active = valid;
  int done = 0, status = 0;
  for (int t = 0; t < T; t++) {
    bool stepped = false;
    double fwdinv = 0;
    if (active) {
      const long row = inst*T + t;
      if (a.ctrl_mode == kRolloutPerStep) for (int k = 0; k < nu; k++) d.ctrl[k] = a.ctrl[row*nu + k];
      if (a.qfrc_mode == kRolloutPerStep) {
        for (int k = 0; k < nv; k++) d.qfrc_applied[k] = a.qfrc_applied[row*nv + k];
      }
      if (a.xfrc_mode == kRolloutPerStep) {
        for (int k = 0; k < nx; k++) d.xfrc_applied[k] = a.xfrc_applied[row*nx + k];
      }
      const int st = mjh::step<64, CONTACT>(m, d, sc, a.fwdinv_on != 0, &fwdinv);
      status |= st;
      if (st & mjh::kStepStop) {
        active = false;
        fwdinv = 0;
      } else {
        stepped = true;
        done++;
      }
    }
    if (a.state) {
      writeRows(direct, a.state, lds, inst0, lane, valid, a.B, T, t, nq + nv + na, [&](int k) {
        return k < nq ? (double)d.qpos[k] : k < nq + nv ? (double)d.qvel[k - nq]
                                                        : (double)d.act[k - nq - nv];
      });
    }
    if (a.qacc) {
      const mjh::SP<64> q0 = mjh::firstQacc(m, d, sc);
      writeRows(direct, a.qacc, lds, inst0, lane, valid, a.B, T, t, nv,
                        [&](int k) { return stepped ? (double)q0[k] : 0.0; });
    }
    if (a.fwdinv && valid) a.fwdinv[inst*T + t] = fwdinv;
  }
  if (valid) {
    if (a.steps_done) a.steps_done[inst] = done;
    if (a.status) a.status[inst] = status;
  }
}

long mjhip_rolloutScratchDoubles(const mjhipModel* hm) { return mjh::stepLayout(hm).total; }

int mjhip_launchRollout(hipStream_t s, const mjhipModel& dmodel, const Mirror& mr,
                        const RolloutCall& call, bool contact, bool direct) {
  const dim3 grid((call.B + 63) / 64), block(64);
  const int ds = direct || kRolloutDirectDefault;
  if (contact) hipLaunchKernelGGL(k_rollout<true>, grid, block, 0, s, dmodel, mr, call, ds);
  else hipLaunchKernelGGL(k_rollout<false>, grid, block, 0, s, dmodel, mr, call, ds);
  return hipGetLastError() != hipSuccess;
}
