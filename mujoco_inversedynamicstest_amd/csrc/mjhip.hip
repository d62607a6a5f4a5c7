// mjhip.hip — libmjhip.so: HIP kernels for gfx950 + the C-ABI of include/mjhip.h.
//
// Device layout (DESIGN.md §Data layout):
//   * model: every mjhipModel array copied once into one device buffer; a device-side
//     mjhipModel (same struct, device pointers) is passed by value as a kernel argument, so
//     model reads are wave-uniform scalar loads.
//   * mirror: every per-instance field F of S doubles is F[(blk*S + k)*64 + lane] — 64-
//     instance blocks = one wavefront; a wavefront's access to component k is one 512-byte
//     contiguous segment (fully coalesced), and a block's whole field is contiguous.
//   * one lane per instance (north star), blockDim = 64, grid = ceil(B/64).
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "engine_device.h"
#include "fast_kernels.h"
#include "kernels.h"
#include "pair_program.h"
#include "rollout.h"
#include "transition_call.h"
#include "solver_call.h"
// lane-count variants of the cooperative kernel (kern_constraint.hip), measurement only
extern template __global__ void k_constraint_coop<8, true, false, false>(mjhipModel, Mirror, int, const int*, const int*, const CoopPair*, const mjh::ContactParam*, const unsigned long long*, int, double*, int*);
extern template __global__ void k_constraint_coop<32, true, false, false>(mjhipModel, Mirror, int, const int*, const int*, const CoopPair*, const mjh::ContactParam*, const unsigned long long*, int, double*, int*);
#include "post_pass.h"

// Every kernel takes mjhipModel and Mirror by value, and HIP's kernel-argument segment holds
// 4,096 B (a larger one compiles without a diagnostic and fails at launch). 160 B is the room
// the widest argument list beside the two (k_fd_expand, k_fd_diff, k_constraint_coop) takes.
static_assert(sizeof(mjhipModel) + sizeof(Mirror) + 160 <= 4096,
              "mjhipModel + Mirror leave no room in the 4,096 B kernel-argument segment");

//==================================== kernels ===============================================

// k_constraint, k_constraint_coop (kern_constraint.hip) and k_inverse (kern_inverse.hip):
// kernels.h

// fluid forces after the generated kernels (csrc/post_pass.h): one lane per instance
__global__ __launch_bounds__(64) void k_fluid_after(mjhipModel m, Mirror mr, int B) {
  const long inst = (long)blockIdx.x*64 + threadIdx.x;
  if (inst >= B) return;
  Lane<64> d = lane_view(mr, blockIdx.x, threadIdx.x);
  mjh::fluidAfter(m, d);
}

// spatial tendons, their transmissions and mj_passive after the generated kernels
// (csrc/post_pass.h): one lane per instance
__global__ __launch_bounds__(64) void k_tendon_after(mjhipModel m, Mirror mr, int B) {
  const long inst = (long)blockIdx.x*64 + threadIdx.x;
  if (inst >= B) return;
  Lane<64> d = lane_view(mr, blockIdx.x, threadIdx.x);
  mjh::tendonAfter(m, d);
}

// mjENBL_INVDISCRETE on the straight-line path (csrc/post_pass.h): mj_discreteAcc and the
// RNE over its qacc before the constraint kernel; the caller's qacc back after the sensors.
// trn: the slider-crank and site transmissions the generated kernels leave to the pass after
// the constraint kernel are formed here first (mj_discreteAcc's implicit damping reads their
// actuator_moment; the reference has them from mj_fwdPosition, before mj_discreteAcc)
__global__ __launch_bounds__(64) void k_discrete_before(mjhipModel m, Mirror mr, int B,
                                                        int trn) {
  const long inst = (long)blockIdx.x*64 + threadIdx.x;
  if (inst >= B) return;
  Lane<64> d = lane_view(mr, blockIdx.x, threadIdx.x);
  if (trn) mjh::transmissionAfter(m, d);
  mjh::discreteBefore(m, d);
}

__global__ __launch_bounds__(64) void k_discrete_restore(mjhipModel m, Mirror mr, int B) {
  const long inst = (long)blockIdx.x*64 + threadIdx.x;
  if (inst >= B) return;
  Lane<64> d = lane_view(mr, blockIdx.x, threadIdx.x);
  mjh::discreteRestore(m, d);
}

// Status checks of the straight-line path: mj_checkPos/Vel/Acc (engine_forward.c:53-102)
// on the inputs and the pivot test behind MJHIP_INST_INERTIA on qLD's diagonal, ORed into
// the status words the generated kernels and k_constraint wrote. A separate launch, run
// only when statuses are asked for: inside the generated kernels the extra live values
// cost spills (tools/kernel_resources.py).
__global__ __launch_bounds__(64) void k_check(mjhipModel m, Mirror mr, int B,
                                              int* __restrict__ status, int skipstage) {
  const long inst = (long)blockIdx.x*64 + threadIdx.x;
  if (inst >= B) return;
  Lane<64> d = lane_view(mr, blockIdx.x, threadIdx.x);
  int st = mjh::checkInputs(m, d, skipstage);
  for (int k = 0; skipstage == mjhipSTAGE_NONE && k < m.nv; k++) {
    if (!(d.qLD[m.C_rowadr[k] + m.C_rownnz[k] - 1] >= mjh::MINVAL)) st |= MJHIP_INST_INERTIA;
  }
  if (st) status[inst] |= st;
}

// Batched mj_inverseSkip(POS / VEL) on the straight-line path: the generated k_va (POS) or
// k_acc (VEL) ran the remaining stages and, for an instance with constraint rows (made by the
// previous call), left the raw mj_rne(flg_acc = 1) in qfrc_inverse. Here those instances
// finish as the reference does on the rows it kept: mj_referenceConstraint when the velocity
// stage ran (POS), mj_invConstraint, then the assembly (engine_inverse.c:169-252).
// all != 0: a model whose rows serve every instance (contacts): the straight-line stage
// stored the raw RNE for every instance, which is assembled here, rows or none
// (mj_invConstraint with nefc = 0 zeroes qfrc_constraint, engine_inverse.c:168-177)
__global__ __launch_bounds__(64) void k_skip_rows(mjhipModel m, Mirror mr, int B, int skipstage,
                                                  double* __restrict__ qfrc_out, int all) {
  const long inst = (long)blockIdx.x*64 + threadIdx.x;
  if (inst >= B) return;
  Lane<64> d = lane_view(mr, blockIdx.x, threadIdx.x);
  if (!d.efc_count[0] && !all) return;
  if (d.efc_count[0] && skipstage == mjhipSTAGE_POS) mjh::referenceConstraint(m, d);
  mjh::invConstraint(m, d);
  for (int i = 0; i < m.nv; i++) {
    d.qfrc_inverse[i] += m.dof_armature[i] * d.qacc[i] - d.qfrc_passive[i] -
                         d.qfrc_constraint[i];
  }
  if (qfrc_out) {
    for (int i = 0; i < m.nv; i++) qfrc_out[inst*m.nv + i] = d.qfrc_inverse[i];
  }
}

// slider-crank/site/body transmissions, sensors and energy after the generated kernels and
// the constraint kernel (mjh::transmissionAfter, mjh::sensorsAfter)
__global__ __launch_bounds__(64) void k_sensors(mjhipModel m, Mirror mr, int B, int sensors,
                                                int trn) {
  const int blk = blockIdx.x, lane = threadIdx.x;
  if ((long)blk*64 + lane >= B) return;
  Lane<64> d = lane_view(mr, blk, lane);
  mjh::sensorsAfter<64>(m, d, sensors != 0, trn != 0);
}

// row-major (B x n) <-> mirror block layout
__global__ void k_to_mirror(const double* __restrict__ src, double* __restrict__ dst, int B,
                            int n) {
  long t = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= (long)B*n) return;
  long inst = t / n, k = t % n;
  dst[((inst >> 6)*n + k)*64 + (inst & 63)] = src[t];
}

__global__ void k_from_mirror(const double* __restrict__ src, double* __restrict__ dst, int B,
                              int n) {
  long t = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= (long)B*n) return;
  long inst = t / n, k = t % n;
  dst[t] = src[((inst >> 6)*n + k)*64 + (inst & 63)];
}

// mjd_inverseFD expansion (engine_derivative_fd.c:611-719): base state b and perturbation
// p (0 = centre, 1..nv = qacc_i + eps, nv+1..2nv = qvel_i + eps, 2nv+1..3nv = qpos
// integrated along e_i by eps). Instances are base-major: inst = b*(3nv+1) + p.
// Layout 1 (stage skipping, mj_inverseSkip(mjSTAGE_POS) for the qvel/qacc perturbations):
// the instances that run the position stage first -- the centres b, then the qpos
// perturbations nbase + b*nv + i (dof i) -- then from A = nbase*(nv+1) the others,
// A + b*2nv + (p-1). The centres lead so that they fill whole waves: only their mirror slots
// keep every field (Mirror::fd_elide, codegen.FD_KEEP).
__device__ static inline long fd_inst(int layout, long nbase, long b, int p, int nv) {
  if (!layout) return b*(3*nv + 1) + p;
  if (p == 0) return b;
  if (p > 2*nv) return nbase + b*nv + (p - 2*nv - 1);
  return nbase*(nv + 1) + b*2*nv + (p - 1);
}

// instances [first, end) of the layout (first a multiple of 64), one block per 64 instances,
// its kExpandWaves waves taking turns over the input components: qvel[k], qacc[k] (k < nv), joint j's
// qpos (mj_integratePos on dof i for the qpos perturbations), ctrl[k], act[k]. The 64 lanes of a wave
// write one 512-byte mirror line per value. gate: the stage-skip fall-back's expansion (mjhip_inverseFDBatch): it runs only when
// k_vaskip found a centre with limit rows (fdflag[0]), and its first thread hands the range
// {first, end} -- or the empty {first, first} -- to the fall-back k_all (fdflag[1..2])
// the base state b and perturbation p of instance inst in the layout (the inverse of fd_inst)
__device__ static inline void fd_bp(int layout, long nbase, long inst, int nv, long* b, int* p) {
  const int P = 3*nv + 1;
  if (!layout) {
    *b = inst / P;
    *p = (int)(inst % P);
  } else if (inst < nbase) {
    *b = inst;
    *p = 0;
  } else if (inst < nbase*(nv + 1)) {
    const long t = inst - nbase;
    *b = t / nv;
    *p = 2*nv + 1 + (int)(t % nv);
  } else {
    const long t = inst - nbase*(nv + 1);
    *b = t / (2*nv);
    *p = 1 + (int)(t % (2*nv));
  }
}

constexpr int kExpandWaves = 16;   // 4 measured 13 us per 28,672 instances (latency-bound)
__global__ __launch_bounds__(64*kExpandWaves) void k_fd_expand(mjhipModel m, Mirror mr, int nbase,
                                                  const double* __restrict__ qpos,
                                                  const double* __restrict__ qvel,
                                                  const double* __restrict__ qacc,
                                                  const double* __restrict__ ctrl,
                                                  const double* __restrict__ act, double eps,
                                                  int layout, int* __restrict__ fdflag,
                                                  long first, long end, int gate) {
  const int nv = m.nv, nq = m.nq, P = 3*nv + 1;
  const int nctrl = ctrl ? m.nu : 0;
  const int ncomp = 2*nv + m.njnt + nctrl + (act ? m.na : 0);
  // blocks of blockDim.x / 64 waves, striding over the 64-instance blocks of [first, end)
  // (the main expansion: one block each; the gated one: a few one-wave blocks, so that the
  // usual empty launch dispatches little): wave w writes components w, w + waves, ...
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64, waves = blockDim.x / 64;
  if (gate) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      fdflag[1] = (int)first;
      fdflag[2] = fdflag[0] ? (int)end : (int)first;
    }
    if (!fdflag[0]) return;
  } else if (fdflag && blockIdx.x == 0 && threadIdx.x == 0) {
    fdflag[0] = 0;                       // k_vaskip raises it later in stream order
  }
  for (long blk = first/64 + blockIdx.x; blk*64 < end; blk += gridDim.x) {
  const long inst = blk*64 + lane;
  if (inst >= end || inst >= (long)nbase*P) continue;
  long b;
  int p;
  fd_bp(layout, nbase, inst, nv, &b, &p);
  Lane<64> d = lane_view(mr, (int)(inst >> 6), lane);
  for (int comp = wave; comp < ncomp; comp += waves) {
  if (comp < nv) {                       // qvel_k (+ eps on the qvel perturbation k)
    const double x = qvel[b*nv + comp];
    d.qvel[comp] = p - 1 - nv == comp ? x + eps : x;
    continue;
  }
  if (comp < 2*nv) {                     // qacc_k (+ eps on the qacc perturbation k)
    const int k = comp - nv;
    const double x = qacc[b*nv + k];
    d.qacc[k] = p - 1 == k ? x + eps : x;
    continue;
  }
  if (comp >= 2*nv + m.njnt + nctrl) {   // flg_actuation: the base state's activations
    const int k = comp - 2*nv - m.njnt - nctrl;
    d.act[k] = act[b*m.na + k];
    continue;
  }
  if (comp >= 2*nv + m.njnt) {           // flg_actuation: the base state's controls
    const int k = comp - 2*nv - m.njnt;
    d.ctrl[k] = ctrl[b*m.nu + k];
    continue;
  }
  // joint j's qpos: the base state's, or mj_integratePos(m, qpos, e_i, eps) for the qpos
  // perturbation of dof i (engine_support.c:1518-1550)
  const int j = comp - 2*nv, i = p > 2*nv ? p - 1 - 2*nv : -1;
  int padr = m.jnt_qposadr[j], vadr = m.jnt_dofadr[j], t = m.jnt_type[j];
  const long bq = b*nq;
  if (t == mjhipJNT_FREE) {
    for (int c = 0; c < 3; c++) {
      d.qpos[padr+c] = i < 0 ? qpos[bq + padr + c]
                             : qpos[bq + padr + c] + eps * (vadr + c == i ? 1.0 : 0.0);
    }
    padr += 3;
    vadr += 3;
    t = mjhipJNT_BALL;
  }
  if (t == mjhipJNT_BALL) {
    double q[4] = {qpos[bq + padr], qpos[bq + padr + 1], qpos[bq + padr + 2],
                   qpos[bq + padr + 3]};
    if (i >= 0) {
      const double vel[3] = {vadr == i ? 1.0 : 0.0, vadr + 1 == i ? 1.0 : 0.0,
                             vadr + 2 == i ? 1.0 : 0.0};
      mjh::quatIntegrate(q, vel, eps);
    }
    for (int c = 0; c < 4; c++) d.qpos[padr+c] = q[c];
  } else {
    d.qpos[padr] = i < 0 ? qpos[bq + padr] : qpos[bq + padr] + eps * (vadr == i ? 1.0 : 0.0);
  }
  }
  }
}

// diff(): DfD*[b][i][:] = (f(perturbed) - f(centre)) / eps  (engine_derivative_fd.c:48-53)
// Sensor rows follow the reference's stage skipping: a qacc perturbation runs
// mj_inverseSkip(mjSTAGE_VEL), so only acceleration-stage sensors change and the others keep
// the centre's values (their difference is exactly 0); a qvel perturbation runs
// mjSTAGE_POS, so position-stage sensors keep theirs (engine_derivative_fd.c:646-699).
// flg_actuation (inverseSkip, engine_derivative_fd.c:160-168): every evaluation's force is
// qfrc_inverse - qfrc_actuator, with mj_fwdActuation run after the inverse (k_fd_act)

__global__ void k_fd_act(mjhipModel m, Mirror mr, long ninst) {
  const long inst = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (inst >= ninst) return;
  Lane<64> d = lane_view(mr, (int)(inst >> 6), (int)(inst & 63));
  mjh::fwdActuation(m, d);
}

// DfDq/DfDv/DfDa (engine_derivative_fd.c:48-53) one thread per output element, the row's
// element k fastest, so a wave's stores are contiguous (the same difference and scaling as
// k_fd_diff, which keeps the sensor rows and DmDq; an LDS-tiled form, one block per 64
// instances, measured slower: 17.5 against 15.8 us at 1,024 base states)
__global__ void k_fd_dfd(mjhipModel m, Mirror mr, int nbase, double eps, int flg_actuation,
                         double* __restrict__ DfDq, double* __restrict__ DfDv,
                         double* __restrict__ DfDa, int layout) {
  const int nv = m.nv, P = 3*nv + 1;
  const long t = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= (long)nbase*(P-1)*nv) return;
  const int k = (int)(t % nv);
  const long r = t / nv;
  const long b = r / (P-1);
  const int p = (int)(r % (P-1)) + 1;
  double* out;
  int i;
  if (p <= nv) {
    out = DfDa; i = p - 1;
  } else if (p <= 2*nv) {
    out = DfDv; i = p - 1 - nv;
  } else {
    out = DfDq; i = p - 1 - 2*nv;
  }
  if (!out) return;
  const long ic = fd_inst(layout, nbase, b, 0, nv), ip = fd_inst(layout, nbase, b, p, nv);
  Lane<64> c = lane_view(mr, (int)(ic >> 6), (int)(ic & 63));
  Lane<64> q = lane_view(mr, (int)(ip >> 6), (int)(ip & 63));
  double fq = q.qfrc_inverse[k], fc = c.qfrc_inverse[k];
  if (flg_actuation) {
    fq -= q.qfrc_actuator[k];
    fc -= c.qfrc_actuator[k];
  }
  out[(b*nv + i)*nv + k] = (1/eps) * (fq - fc);
}

__global__ void k_fd_diff(mjhipModel m, Mirror mr, int nbase, double eps, int flg_actuation,
                          double* __restrict__ DfDq, double* __restrict__ DfDv,
                          double* __restrict__ DfDa, double* __restrict__ DsDq,
                          double* __restrict__ DsDv, double* __restrict__ DsDa,
                          double* __restrict__ DmDq, int layout) {
  const int nv = m.nv, P = 3*nv + 1;
  long t = (long)blockIdx.x*blockDim.x + threadIdx.x;   // one thread per (b, perturbation)
  if (t >= (long)nbase*(P-1)) return;
  long b = t / (P-1);
  int p = (int)(t % (P-1)) + 1;
  long ic = fd_inst(layout, nbase, b, 0, nv), ip = fd_inst(layout, nbase, b, p, nv);
  Lane<64> c = lane_view(mr, (int)(ic >> 6), (int)(ic & 63));
  Lane<64> q = lane_view(mr, (int)(ip >> 6), (int)(ip & 63));
  double inv_h = 1/eps;
  double *out, *sout;
  int i, minstage;
  if (p <= nv) {
    out = DfDa; sout = DsDa; i = p - 1; minstage = mjhipSTAGE_ACC;
  } else if (p <= 2*nv) {
    out = DfDv; sout = DsDv; i = p - 1 - nv; minstage = mjhipSTAGE_VEL;
  } else {
    out = DfDq; sout = DsDq; i = p - 1 - 2*nv; minstage = mjhipSTAGE_POS;
  }
  if (out) {
    for (int k = 0; k < nv; k++) {
      double fq = q.qfrc_inverse[k], fc = c.qfrc_inverse[k];
      if (flg_actuation) {
        fq -= q.qfrc_actuator[k];
        fc -= c.qfrc_actuator[k];
      }
      out[(b*nv + i)*nv + k] = inv_h * (fq - fc);
    }
  }
  if (sout) {
    const int ns = m.nsensordata;
    for (int s = 0; s < m.nsensor; s++) {
      const bool ran = m.sensor_needstage[s] >= minstage;
      for (int k = m.sensor_adr[s]; k < m.sensor_adr[s] + m.sensor_dim[s]; k++) {
        const double x1 = c.sensordata[k], x2 = ran ? q.sensordata[k] : x1;
        sout[(b*nv + i)*ns + k] = inv_h * (x2 - x1);
      }
    }
  }
  if (DmDq && p > 2*nv) {
    for (int k = 0; k < m.nM; k++) {
      DmDq[(b*nv + i)*m.nM + k] = inv_h * (q.qM[k] - c.qM[k]);
    }
  }
}

// Batched mj_fwdActuation (mjh::fwdActuation) over the actuator_length, actuator_velocity and
// actuator_moment already in the mirror: one lane per instance, 64-instance blocks, so a
// wave's read or write of one component of a mirror field is one 512-byte segment. Optional
// row-major ctrl / act are copied into the mirror first; optional row-major act_dot, act_next
// and qfrc_actuator are written at the end. mj_fwdActuation raises no per-instance condition
// on this path, so every status word is 0.
__global__ __launch_bounds__(64) void k_actuation(mjhipModel m, Mirror mr, int B,
                                                  const double* __restrict__ ctrl_in,
                                                  const double* __restrict__ act_in,
                                                  double* __restrict__ act_dot_out,
                                                  double* __restrict__ act_next_out,
                                                  double* __restrict__ qfrc_out,
                                                  int* __restrict__ status) {
  const int blk = blockIdx.x, lane = threadIdx.x;
  const long inst = (long)blk*64 + lane;
  if (inst >= B) return;
  Lane<64> d = lane_view(mr, blk, lane);
  if (ctrl_in) {
    for (int k = 0; k < m.nu; k++) d.ctrl[k] = ctrl_in[inst*m.nu + k];
  }
  if (act_in) {
    for (int k = 0; k < m.na; k++) d.act[k] = act_in[inst*m.na + k];
  }
  mjh::fwdActuation(m, d);
  if (act_dot_out) {
    for (int k = 0; k < m.na; k++) act_dot_out[inst*m.na + k] = d.act_dot[k];
  }
  if (act_next_out) {
    for (int k = 0; k < m.na; k++) act_next_out[inst*m.na + k] = d.act_next[k];
  }
  if (qfrc_out) {
    for (int k = 0; k < m.nv; k++) qfrc_out[inst*m.nv + k] = d.qfrc_actuator[k];
  }
  if (status) status[inst] = 0;
}

// Constraint-free mj_forward over a batch (mjh::forwardSkip). Optional row-major qpos, qvel,
// ctrl, act are copied into the mirror first; qfrc_applied / xfrc_applied are read from the
// mirror; optional row-major qacc is written at the end.
template <bool CONTACT>
__global__ __launch_bounds__(64) void k_forward(mjhipModel m, Mirror mr, int B,
                                                const double* __restrict__ qpos_in,
                                                const double* __restrict__ qvel_in,
                                                const double* __restrict__ ctrl_in,
                                                const double* __restrict__ act_in,
                                                double* __restrict__ qacc_out,
                                                double* __restrict__ act_dot_out,
                                                double* __restrict__ act_next_out,
                                                int* __restrict__ status) {
  const int blk = blockIdx.x, lane = threadIdx.x;
  const long inst = (long)blk*64 + lane;
  if (inst >= B) return;
  Lane<64> d = lane_view(mr, blk, lane);
  if (qpos_in) {
    for (int k = 0; k < m.nq; k++) d.qpos[k] = qpos_in[inst*m.nq + k];
  }
  if (qvel_in) {
    for (int k = 0; k < m.nv; k++) d.qvel[k] = qvel_in[inst*m.nv + k];
  }
  if (ctrl_in) {
    for (int k = 0; k < m.nu; k++) d.ctrl[k] = ctrl_in[inst*m.nu + k];
  }
  if (act_in) {
    for (int k = 0; k < m.na; k++) d.act[k] = act_in[inst*m.na + k];
  }
  int st = mjh::forwardSkip<64, CONTACT>(m, d, mjhipSTAGE_NONE);
  if (qacc_out) {
    for (int k = 0; k < m.nv; k++) qacc_out[inst*m.nv + k] = d.qacc[k];
  }
  if (act_dot_out) {
    for (int k = 0; k < m.na; k++) act_dot_out[inst*m.na + k] = d.act_dot[k];
  }
  if (act_next_out) {
    for (int k = 0; k < m.na; k++) act_next_out[inst*m.na + k] = d.act_next[k];
  }
  if (status) status[inst] = st;
}

//==================================== host side ==============================================

static thread_local std::string g_last_error;
static void (*g_error_cb)(const char*) = nullptr;

static void set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

#define HIPCHECK(expr)                                                              \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) {                                                         \
      set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,    \
                __LINE__);                                                          \
      return MJHIP_ERR_HIP;                                                         \
    }                                                                               \
  } while (0)

struct mjhipContext_ {
  int device = 0;
  int capacity = 0;         // instances (multiple of 64)
  int efc_cap = 0;
  int con_cap = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  mjhipModel hmodel{};      // host copy of sizes (pointers are host pointers of the caller)
  mjhipModel dmodel{};      // device pointers
  void* dmodel_buf = nullptr;
  Mirror mirror{};
  void* mirror_buf = nullptr;
  size_t mirror_bytes = 0;
  std::unordered_map<std::string, std::pair<double*, int>> fields;   // name -> (ptr, S)
  std::unordered_map<std::string, std::pair<int*, int>> ifields;   // int scratch fields
  std::unordered_set<std::string> contig;  // instance-contiguous fields (XSCC / XSIC)
  std::unordered_set<const void*> contig_ptr;   // and their device storage
  // staging for row-major host transfers
  double* stage = nullptr;
  size_t stage_bytes = 0;
  int* status = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  const FastKernelEntry* fast = nullptr;   // straight-line kernel for this model, if any
  int fast_lds = 0;                        // its k_all's static LDS (mjhip_contextFastKernelLds)
  int* worklist = nullptr;                 // capacity + 2 ints: [count0, count1, list...]
  int wl_parity = 0;                       // counter the next fast launch uses
  int wl_last = 0;                         // counter the last fast launch used
  int last_path = -1;                      // mjhip_contextLastPath
  const char* con_kernel = "none";         // mjhip_contextConstraintKernel
  // mjhip_inverseFDBatch's stage-skip fall-back, decided on the device: [0] a centre has limit
  // rows (k_vaskip), [1..2] the instance range {first, end} the gated k_fd_expand hands to
  // k_all
  int* fdflag = nullptr;
  CoopPair* pairs = nullptr;               // static geom-pair program (coop_program)
  mjh::ContactParam* cparams = nullptr;    // each program pair's mj_contactParam
  int* prog_ipair = nullptr;               // each program pair's predefined-pair index or -1
  unsigned long long* masks = nullptr;     // the cooperative kernel's chain masks (coop_masks)
  int npair = 0;
  bool boxpair = false;                    // a box-box pair is in the program (coop LDS)
  int coop = 16;                           // lanes per instance of k_constraint_coop (0: off)
  bool spatial = false;                    // spatial tendons: k_tendon_after runs (post_pass.h)
  // a straight-line kernel specialized for this model at run time (mjhip_contextLoadKernel):
  // a gfx950 code object holding extern "C" k_all_<name>; rt.launch stays null
  unsigned long long sig = 0;              // model_signature of the model at creation
  hipModule_t rt_module = nullptr;
  hipFunction_t rt_fn = nullptr;
  FastKernelEntry rt{};
  std::string rt_name;
  hipDeviceptr_t rt_tbuf = nullptr;        // the code object's mjh_tbuf (null: none)
  hipFunction_t rt_const_fn = nullptr;     // the code object's k_const_<name>
  int rt_nconst = 0;                       // and its k_const_count_<name>
  int rt_nhand = 0;                        // and its k_qm_handoff_<name> (0: none)
  int rt_nfwd = 0;                         // and its k_qm_forward_<name> (0: none)
  // the model-constant output slots the generated stage bodies leave to k_const may not hold
  // their values: set at creation, by mjhip_contextLoadKernel (another code object carries its
  // own constants) and by every mjhip_mirrorUpload; cleared by ensure_const
  bool const_stale = true;
  int const_launches = 0;                  // k_const launches so far (mjhip_contextConstLaunches)
  // per-stage timers (mjhip_contextTimers): the device accumulator the phase marks add to,
  // the reference's mjTimerStat table, and the events around each timed call
  unsigned long long* tbuf = nullptr;
  mjhipTimerStat timer[mjhipNTIMER]{};
  unsigned long long traw[MJH_TSLOTS]{};   // the raw mark sums (tools/exp_phases.py)
  hipEvent_t tev0 = nullptr, tev1 = nullptr;
  // mjhip_rolloutBatch's integrator scratch (csrc/step.h), [capacity/64][k][64]: allocated by
  // the context's first rollout, freed with the context
  double* rollout_scratch = nullptr;
  // mjhip_transitionFDBatch's next states (TransitionCall::Y), grown on demand
  double* transition_y = nullptr;
  size_t transition_y_n = 0;
  // mjhip_forwardSolveBatch's solver scratch (csrc/solver.h), [capacity/64][k][64], with the
  // kept qacc_warmstart: allocated and zeroed by the context's first solve, freed with it
  double* solver_scratch = nullptr;
};

// 1 when the model has activation states or a muscle gain / bias: only then are the arrays
// of MJHIP_MODEL_POINTERS_A read. They sit behind every older pointer of mjhipModel, so a
// caller compiled against a header without them passes a shorter struct, and for the models
// such a caller can describe the library never looks past its end.
static bool mjhip_modelUsesActivation(const mjhipModel* m) {
  if (m->na > 0) return true;
  for (int i = 0; i < m->nu; i++) {
    if (m->actuator_gaintype[i] == mjhipGAIN_MUSCLE || m->actuator_biastype[i] == mjhipBIAS_MUSCLE) {
      return true;
    }
  }
  return false;
}

// the model as the library reads it: *m, or its older prefix with the activation arrays absent
static mjhipModel model_read(const mjhipModel* m) {
  mjhipModel r;
  if (mjhip_modelUsesActivation(m)) {
    r = *m;
  } else {
    memcpy(&r, m, offsetof(mjhipModel, actuator_actadr));
#define X(type, name, d0, d1) r.name = nullptr;
    MJHIP_MODEL_POINTERS_A
#undef X
  }
  return r;
}

// FNV-1a 64 over sizes, options and every model array (= fields.model_signature in Python)
static unsigned long long model_signature(const mjhipModel* caller) {
  const mjhipModel rd = model_read(caller);
  const mjhipModel* m = &rd;
  unsigned long long h = 0xcbf29ce484222325ull;
  auto feed = [&](const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) {
      h ^= b[i];
      h *= 0x100000001b3ull;
    }
  };
#define XS(name) { int v = m->name; feed(&v, 4); }
  MJHIP_MODEL_SIZES
#undef XS
  feed(&m->opt.timestep, 8);
  feed(&m->opt.impratio, 8);
  feed(m->opt.gravity, 24);
  feed(m->opt.wind, 24);
  feed(m->opt.magnetic, 24);
  feed(&m->opt.density, 8);
  feed(&m->opt.viscosity, 8);
  feed(&m->opt.o_margin, 8);
  feed(m->opt.o_solref, 16);
  feed(m->opt.o_solimp, 40);
  feed(m->opt.o_friction, 40);
  feed(&m->opt.integrator, 4);
  feed(&m->opt.cone, 4);
  feed(&m->opt.jacobian, 4);
  feed(&m->opt.disableflags, 4);
  feed(&m->opt.enableflags, 4);
  feed(&m->opt.ccd_tolerance, 8);
  feed(&m->opt.ccd_iterations, 4);
#define MJ_M(n) m->n
#define X(type, name, d0, d1) if (m->name) feed(m->name, sizeof(type) * (size_t)(m->d0) * (d1));
  MJHIP_MODEL_POINTERS
#undef X
#undef MJ_M
  return h;
}

// model features outside the device path: rejected at context creation (fail loudly)
static const char* unsupported(const mjhipModel* m) {
  if ((m->opt.enableflags & mjhipENBL_INVDISCRETE) && m->opt.integrator == mjhipINT_RK4) {
    return "mjENBL_INVDISCRETE with the RK4 integrator (an error in the reference)";
  }
  for (int i = 0; i < m->ntendon; i++) {
    for (int w = m->tendon_adr[i]; w < m->tendon_adr[i] + m->tendon_num[i]; w++) {
      if (m->wrap_type[w] < mjhipWRAP_JOINT || m->wrap_type[w] > mjhipWRAP_CYLINDER) {
        return "unknown tendon wrap object type";
      }
    }
  }
  for (int i = 0; i < m->nu; i++) {
    int t = m->actuator_trntype[i];
    if (t != mjhipTRN_JOINT && t != mjhipTRN_JOINTINPARENT && t != mjhipTRN_TENDON &&
        t != mjhipTRN_SLIDERCRANK && t != mjhipTRN_SITE && t != mjhipTRN_BODY) {
      return "unknown transmission type";
    }
  }
  if (mjh_isSparse(m)) {
    for (int i = 0; i < m->nu; i++) {
      if (m->actuator_trntype[i] == mjhipTRN_TENDON &&
          m->wrap_type[m->tendon_adr[m->actuator_trnid[2*i]]] != mjhipWRAP_JOINT) {
        // the reference's moment row is the tendon's compressed ten_J row (:1060-1067), whose
        // pattern follows the wrapping state; actuator_moment's pattern is model-constant here
        return "a spatial-tendon transmission in a sparse-Jacobian model";
      }
    }
  }
  for (int i = 0; i < m->nsensor; i++) {
    const int t = m->sensor_type[i];
    if (t > mjhSENS_CLOCK) return "plugin/user sensors";
    if (t >= mjhSENS_GEOMDIST && t <= mjhSENS_GEOMFROMTO) {
      // mj_geomDistance's functions outside the subset: meshes, height fields, SDFs, and
      // libccd's MPR (convex and box-box pairs with the native solver disabled)
      const int o = m->sensor_objid[i], r = m->sensor_refid[i];
      const int n1 = m->sensor_objtype[i] == 1 ? m->body_geomnum[o] : 1;
      const int a1 = m->sensor_objtype[i] == 1 ? m->body_geomadr[o] : o;
      const int n2 = m->sensor_reftype[i] == 1 ? m->body_geomnum[r] : 1;
      const int a2 = m->sensor_reftype[i] == 1 ? m->body_geomadr[r] : r;
      const bool nccd = !(m->opt.disableflags & mjhipDSBL_NATIVECCD);
      for (int g1 = a1; g1 < a1 + n1; g1++) {
        for (int g2 = a2; g2 < a2 + n2; g2++) {
          int t1 = m->geom_type[g1], t2 = m->geom_type[g2];
          if (t1 > t2) std::swap(t1, t2);
          const bool ccd = mjhip_isConvexPair(t1, t2) ||
                           (t1 == mjhipGEOM_BOX && t2 == mjhipGEOM_BOX);
          if ((ccd && !nccd) || (!ccd && mjhip_pairMaxContacts(m, t1, t2) < 0)) {
            return "a geom-distance sensor on a height field or SDF geom, or on a "
                   "convex pair with the native CCD solver disabled";
          }
        }
      }
    }
    if (t == mjhSENS_RANGEFINDER) {   // mj_ray's SDF path is not built
      const int body = m->site_bodyid[m->sensor_objid[i]];
      for (int g = 0; g < m->ngeom; g++) {
        if (m->geom_type[g] == mjhipGEOM_SDF && !mjh::rayEliminate(*m, g, body)) {
          return "a rangefinder that can see an SDF geom";
        }
      }
    }
  }
  return nullptr;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" {

MJHIP_API const char* mjhip_version(void) { return "mjhip 0.1 (gfx950)"; }

#ifdef MJH_PHASE_TIMING
// experiment builds only (tools/exp_phases.py): the raw phase-mark sums of a timed context
extern "C" int mjhip_phaseRead(mjhipContext* c, unsigned long long* out) {
  if (!c) return 1;
  memcpy(out, c->traw, sizeof(c->traw));
  memset(c->traw, 0, sizeof(c->traw));
  return 0;
}
#endif

MJHIP_API const char* mjhip_lastError(void) { return g_last_error.c_str(); }

MJHIP_API void mjhip_setErrorCallback(void (*cb)(const char* msg)) { g_error_cb = cb; }

MJHIP_API int mjhip_deviceCount(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

MJHIP_API int mjhip_fieldSize(const mjhipModel* m, const char* name) {
#define MJ_M(n) m->n
#define XD(nm, d0, d1, stage) if (!strcmp(name, #nm)) return (m->d0) * (d1);
  MJHIP_DATA_FIELDS
  MJHIP_DATA_FORWARD
  MJHIP_DATA_ACTIVATION
#undef XD
#undef MJ_M
  return -1;
}

MJHIP_API int mjhip_outputDoubles(const mjhipModel* m) {
  int w = 0;
#define MJ_M(n) m->n
#define XD(nm, d0, d1, stage) if (stage > 0) w += (m->d0) * (d1);
  MJHIP_DATA_FIELDS
#undef XD
#undef MJ_M
  return w;
}

MJHIP_API int mjhip_contextCreate(const mjhipModel* m, int device, int capacity,
                                  mjhipContext** out) {
  return mjhip_contextCreateCapped(m, device, capacity, 0, 0, out);
}

MJHIP_API int mjhip_contextCreateCapped(const mjhipModel* caller, int device, int capacity,
                                        int max_contacts, int max_rows, mjhipContext** out) {
  if (!caller || !out || capacity <= 0 || max_contacts < 0 || max_rows < 0) {
    set_error("mjhip_contextCreate: bad argument");
    return MJHIP_ERR_ARG;
  }
  const mjhipModel rd = model_read(caller);
  const mjhipModel* m = &rd;
  *out = nullptr;
  int ndev = mjhip_deviceCount();
  if (ndev <= 0) {
    set_error("no HIP device available (the engine has no CPU fallback)");
    return MJHIP_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) {
    set_error("device %d out of range (%d devices)", device, ndev);
    return MJHIP_ERR_ARG;
  }
  if (const char* why = unsupported(m)) {
    set_error("model uses a feature the device path does not support: %s", why);
    return MJHIP_ERR_MODEL;
  }
  HIPCHECK(hipSetDevice(device));
  mjhipContext* c = new mjhipContext_();
  c->device = device;
  c->capacity = (capacity + 63) & ~63;
  c->efc_cap = mjhip_efcCapacity(m);
  c->con_cap = mjhip_contactCapacity(m, nullptr);
  // caller caps (the reference's <size nconmax njmax> / arena bound): an instance that needs
  // more is flagged MJHIP_INST_CNSTRFULL, as mjWARN_CONTACTFULL / mjWARN_CNSTRFULL
  if (max_contacts && max_contacts < c->con_cap) c->con_cap = max_contacts;
  if (max_rows && max_rows < c->efc_cap) c->efc_cap = max_rows;
  c->hmodel = *m;

  // ---- model upload: one buffer, 256-byte aligned arrays
  size_t total = 0;
#define MJ_M(n) m->n
#define X(type, name, d0, d1) total += align256(sizeof(type) * (size_t)(m->d0) * (d1));
  MJHIP_MODEL_POINTERS
#undef X
  std::vector<char> hbuf(total > 0 ? total : 1, 0);
  size_t off = 0;
  c->dmodel = *m;
  if (hipMalloc(&c->dmodel_buf, hbuf.size()) != hipSuccess) {
    set_error("hipMalloc(model) failed");
    delete c;
    return MJHIP_ERR_HIP;
  }
#define X(type, name, d0, d1)                                                       \
  {                                                                                 \
    size_t nb = sizeof(type) * (size_t)(m->d0) * (d1);                              \
    if (nb && m->name) memcpy(hbuf.data() + off, m->name, nb);                      \
    c->dmodel.name = (type*)((char*)c->dmodel_buf + off);                           \
    off += align256(nb);                                                            \
  }
  MJHIP_MODEL_POINTERS
#undef X
#undef MJ_M
  if (m->nu && (!m->actuator_actadr || !m->actuator_actnum)) {
    // a caller that does not fill the activation addresses gets the compiler's: consecutive
    // addresses, one activation per stateful actuator, -1 / 0 for dyntype none (the zeros an
    // absent array uploads as would alias every actuator to act[0])
    int* adr = (int*)(hbuf.data() + ((char*)c->dmodel.actuator_actadr - (char*)c->dmodel_buf));
    int* num = (int*)(hbuf.data() + ((char*)c->dmodel.actuator_actnum - (char*)c->dmodel_buf));
    for (int i = 0, k = 0; i < m->nu; i++) {
      const bool st = m->actuator_dyntype[i] != mjhipDYN_NONE;
      adr[i] = st ? k++ : -1;
      num[i] = st ? 1 : 0;
    }
  }
  if (hipMemcpy(c->dmodel_buf, hbuf.data(), hbuf.size(), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("model upload failed");
    hipFree(c->dmodel_buf);
    delete c;
    return MJHIP_ERR_HIP;
  }

  // ---- mirror: per-instance fields in 64-instance blocks
  const size_t nblk = c->capacity / 64;
  size_t mb = 0;
  const int nv = m->nv, nbody = m->nbody, efc_cap = c->efc_cap, con_cap = c->con_cap;
  (void)nbody;
#define MJ_M(n) m->n
#define XD(name, d0, d1, stage) c->mirror.name##_n = (m->d0) * (d1); \
  mb += align256(sizeof(double) * nblk * 64 * (size_t)c->mirror.name##_n);
  MJHIP_DATA_FIELDS
  MJHIP_DATA_FORWARD
#undef XD
#define XSC(name, n) { const int nbody = m->nbody; (void)nbody; c->mirror.name##_n = (n); \
  mb += align256(sizeof(double) * nblk * 64 * (size_t)c->mirror.name##_n); }
  MJHIP_SCRATCH_FIELDS
#undef XSC
#define XSI(name, n) { c->mirror.name##_n = (n); \
  mb += align256(sizeof(int) * nblk * 64 * (size_t)c->mirror.name##_n); }
  MJHIP_SCRATCH_INT_FIELDS
#undef XSI
#define XD(name, d0, d1, stage) c->mirror.name##_n = (m->d0) * (d1); \
  mb += align256(sizeof(double) * nblk * 64 * (size_t)c->mirror.name##_n);
  MJHIP_DATA_ACTIVATION
#undef XD
  (void)nv; (void)efc_cap; (void)con_cap;
  c->mirror.efc_cap = c->efc_cap;
  c->mirror.con_cap = c->con_cap;
  c->mirror.nj_cap = mjh_njCap(m, c->efc_cap);
  c->mirror_bytes = mb;
  if (hipMalloc(&c->mirror_buf, mb) != hipSuccess) {
    set_error("hipMalloc(mirror, %zu bytes) failed", mb);
    hipFree(c->dmodel_buf);
    delete c;
    return MJHIP_ERR_HIP;
  }
  hipMemset(c->mirror_buf, 0, mb);
  // the context's stream does not wait for the null stream: the zero fill is complete before
  // anything on it (k_const, the first launch's stores) touches the mirror
  hipStreamSynchronize(nullptr);
  char* p = (char*)c->mirror_buf;
#define XD(name, d0, d1, stage) c->mirror.name = (double*)p; \
  c->fields[#name] = {c->mirror.name, c->mirror.name##_n}; \
  p += align256(sizeof(double) * nblk * 64 * (size_t)c->mirror.name##_n);
  MJHIP_DATA_FIELDS
  MJHIP_DATA_FORWARD
#undef XD
#define XSC(name, n) c->mirror.name = (double*)p; \
  c->fields[#name] = {c->mirror.name, c->mirror.name##_n}; \
  p += align256(sizeof(double) * nblk * 64 * (size_t)c->mirror.name##_n);
#undef XSCC
#define XSCC(name, n) c->contig.insert(#name); \
  if (c->mirror.name##_n > 0) c->contig_ptr.insert(p); XSC(name, n)
  MJHIP_SCRATCH_FIELDS
#undef XSC
#define XSI(name, n) c->mirror.name = (int*)p; \
  c->ifields[#name] = {c->mirror.name, c->mirror.name##_n}; \
  p += align256(sizeof(int) * nblk * 64 * (size_t)c->mirror.name##_n);
#undef XSIC
#define XSIC(name, n) c->contig.insert(#name); \
  if (c->mirror.name##_n > 0) c->contig_ptr.insert(p); XSI(name, n)
  MJHIP_SCRATCH_INT_FIELDS
#undef XSI
#undef XSCC
#undef XSIC
#define XSCC(name, n) XSC(name, n)
#define XSIC(name, n) XSI(name, n)
  // the activation state, after every other field; act is zero from the fill above, as
  // mj_resetData leaves it
#define XD(name, d0, d1, stage) c->mirror.name = (double*)p; \
  c->fields[#name] = {c->mirror.name, c->mirror.name##_n}; \
  p += align256(sizeof(double) * nblk * 64 * (size_t)c->mirror.name##_n);
  MJHIP_DATA_ACTIVATION
#undef XD
#undef MJ_M
  // every failure below releases the partial context through mjhip_contextFree
  auto fail = [&](const char* what) {
    set_error("%s failed", what);
    mjhip_contextFree(c);
    return MJHIP_ERR_HIP;
  };
  // staging: row-major qpos, qvel, qacc, qfrc, ctrl, then act, act_dot, act_next for
  // `capacity` instances
  c->stage_bytes = sizeof(double) * (size_t)c->capacity *
                   (m->nq + 3*(size_t)m->nv + m->nu + 3*(size_t)m->na);
  if (hipMalloc((void**)&c->stage, c->stage_bytes) != hipSuccess ||
      hipMalloc((void**)&c->status, sizeof(int) * (size_t)c->capacity) != hipSuccess) {
    return fail("hipMalloc(staging)");
  }
  if (hipMalloc((void**)&c->worklist, sizeof(int) * ((size_t)c->capacity + 2)) != hipSuccess ||
      hipMemset(c->worklist, 0, 2 * sizeof(int)) != hipSuccess) {
    return fail("hipMalloc(worklist)");
  }
  if (hipMalloc((void**)&c->fdflag, 3 * sizeof(int)) != hipSuccess ||
      hipMemset(c->fdflag, 0, 3 * sizeof(int)) != hipSuccess) {
    return fail("hipMalloc(FD flag)");
  }
  const char* nofast = getenv("MJHIP_DISABLE_FAST");
  c->sig = model_signature(m);
  if (!(nofast && nofast[0] == '1')) {
    for (const FastKernelEntry* e = mjhip_fastKernels(); e->launch; e++) {
      if (e->sig == c->sig) c->fast = e;
    }
  }
  // the qM hand-off of the bundled k_all kernels (codegen.py QM_HANDOFF). Default: their HO
  // instantiation from the batch at which L2 no longer serves the re-read
  // (codegen.QM_HANDOFF_MIN_B); MJHIP_QM_HANDOFF=1: at every batch; =0: never (the fac stage
  // re-reads all of qM)
  const char* ho = getenv("MJHIP_QM_HANDOFF");
  c->mirror.qm_handoff = !ho ? 1 : ho[0] == '0' ? 0 : ho[0] == '1' ? 2 : 1;
  if (c->fast && c->fast->lds_bytes) {
    // four k_all workgroups share a CU's LDS (one wave per SIMD): a kernel compiled over the
    // budget would run on three SIMDs of each CU
    c->fast_lds = c->fast->lds_bytes();
    if (c->fast_lds < 0) return fail("hipFuncGetAttributes(k_all)");
    if (c->fast_lds > kFastLdsBudget) {
      set_error("kernel k_all_%s holds %d B of LDS, over the %d B that let four workgroups "
                "share a CU", c->fast->name, c->fast_lds, kFastLdsBudget);
      mjhip_contextFree(c);
      return MJHIP_ERR_MODEL;
    }
  }
  // the cooperative constraint kernel's pair program (16 lanes per instance: 8 and 32 were
  // slower, profiles/r02/bench_c4_L*.json; MJHIP_COOP_LANES=0 selects the one-lane
  // k_constraint)
  if (const char* lanes = getenv("MJHIP_COOP_LANES")) {
    const int n = atoi(lanes);             // 8 and 32: the contact path's lane-count variants
    c->coop = n == 0 ? 0 : (n == 8 || n == 32) ? n : 16;
  }
  if (c->con_cap > 0) {
    // the static collision program (csrc/pair_program.h): the cooperative kernel's pair
    // program, and collision()'s candidate list in every other kernel (Mirror::prog)
    std::vector<ProgItem> pairs = collision_pairs(m);
    c->npair = (int)pairs.size();
    for (const ProgItem& pr : pairs) {
      c->boxpair |= m->geom_type[pr.g1] == mjhipGEOM_BOX && m->geom_type[pr.g2] == mjhipGEOM_BOX;
    }
    if (c->npair) {
      const std::vector<CoopPair> prog = coop_program(m, pairs);
      // contact parameters are model constants: formed here once per pair, by the same
      // function (host arithmetic, as the reference's)
      const std::vector<mjh::ContactParam> cps = program_params(m, prog, pairs);
      std::vector<int> ipair(pairs.size());
      for (size_t i = 0; i < pairs.size(); i++) ipair[i] = pairs[i].ipair;
      if (hipMalloc((void**)&c->pairs, sizeof(CoopPair) * prog.size()) != hipSuccess ||
          hipMemcpy(c->pairs, prog.data(), sizeof(CoopPair) * prog.size(),
                    hipMemcpyHostToDevice) != hipSuccess ||
          hipMalloc((void**)&c->cparams, sizeof(mjh::ContactParam) * cps.size()) != hipSuccess ||
          hipMemcpy(c->cparams, cps.data(), sizeof(mjh::ContactParam) * cps.size(),
                    hipMemcpyHostToDevice) != hipSuccess ||
          hipMalloc((void**)&c->prog_ipair, sizeof(int) * ipair.size()) != hipSuccess ||
          hipMemcpy(c->prog_ipair, ipair.data(), sizeof(int) * ipair.size(),
                    hipMemcpyHostToDevice) != hipSuccess) {
        return fail("pair program upload");
      }
    }
  }
  c->mirror.prog = c->npair ? c->pairs : nullptr;
  c->mirror.prog_ipair = c->npair ? c->prog_ipair : nullptr;
  c->mirror.nprog = c->npair;
  // the native convex solver keeps its polytope in the instance's scratch: one lane per
  // instance (the cooperative kernel would run several pairs of an instance at once)
  if (mjh_needConvex(m) || m->nmesh || m->nhfield) c->coop = 0;
  c->spatial = mjh::hasSpatial(*m);
  // the cooperative kernel's per-dof chain masks are 64-bit
  if (m->nv > 64) c->coop = 0;
  if (c->coop) {
    // chain masks (mjh::chainMask per body: the body and its ancestors), then per body the
    // dofs of those bodies: model constants, formed here once
    std::vector<unsigned long long> mk(2 * (size_t)m->nbody, 0);
    for (int b = 0; b < m->nbody && b < 64; b++) mk[b] = mjh::chainMask(*m, b);
    for (int b = 0; b < m->nbody && b < 64; b++) {
      for (int j = 0; j < m->nv; j++) {
        if ((mk[b] >> m->dof_bodyid[j]) & 1) mk[m->nbody + b] |= 1ull << j;
      }
    }
    if (hipMalloc((void**)&c->masks, sizeof(unsigned long long) * mk.size()) != hipSuccess ||
        hipMemcpy(c->masks, mk.data(), sizeof(unsigned long long) * mk.size(),
                  hipMemcpyHostToDevice) != hipSuccess) {
      return fail("chain mask upload");
    }
  }
  if (c->coop) {
    // the cooperative kernel's dynamic LDS must fit one block: many box pairs (a large
    // efc_cap) or few lanes per instance can exceed it, and then the one-lane k_constraint
    // serves the model instead of every launch failing
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail("hipGetDeviceProperties");
    if (coopLdsBytes(*m, c->coop, c->efc_cap, c->boxpair, c->npair, c->con_cap) >
        (unsigned)prop.sharedMemPerBlock) {
      c->coop = 0;
    }
  }
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    return fail("hipStreamCreate");
  }
  c->own_stream = true;
  if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    return fail("hipEventCreate");
  }
  *out = c;
  return MJHIP_OK;
}

static int timers_detach(mjhipContext* c);
// the one context per process whose accumulator the phase marks may add into: mjh_tbuf is a
// process-wide device global per unit, so a second context's kernels would add into the
// first's accumulator
static mjhipContext* g_timed_ctx = nullptr;

MJHIP_API void mjhip_contextFree(mjhipContext* c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  // the timer pointers go back to null while the stream still exists (timers_attach
  // synchronizes it); an accumulator some unit may still point at is leaked, not freed
  const bool detached = !c->tbuf || timers_detach(c) == MJHIP_OK;
  if (g_timed_ctx == c) g_timed_ctx = nullptr;
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  if (c->ev0) hipEventDestroy(c->ev0);
  if (c->ev1) hipEventDestroy(c->ev1);
  if (c->tev0) hipEventDestroy(c->tev0);
  if (c->tev1) hipEventDestroy(c->tev1);
  if (detached) hipFree(c->tbuf);
  hipFree(c->stage);
  hipFree(c->status);
  hipFree(c->worklist);
  hipFree(c->fdflag);
  hipFree(c->pairs);
  hipFree(c->cparams);
  hipFree(c->prog_ipair);
  hipFree(c->masks);
  hipFree(c->rollout_scratch);
  hipFree(c->transition_y);
  hipFree(c->solver_scratch);
  hipFree(c->mirror_buf);
  hipFree(c->dmodel_buf);
  if (c->rt_module) hipModuleUnload(c->rt_module);
  delete c;
}

MJHIP_API int mjhip_contextLoadKernel(mjhipContext* c, const void* image, size_t size,
                                      const char* name, unsigned long long signature,
                                      int cmode) {
  if (!c || !image || !size || !name || cmode < 0 || cmode > 2) {
    set_error("mjhip_contextLoadKernel: bad arguments");
    return MJHIP_ERR_ARG;
  }
  if (signature != c->sig) {
    set_error("mjhip_contextLoadKernel: kernel '%s' was generated for another model "
              "(signature %016llx, context %016llx)", name, signature, c->sig);
    return MJHIP_ERR_MODEL;
  }
  if (mjh_isSparse(&c->hmodel)) {
    // the straight-line kernels and their constraint kernels keep dense rows
    set_error("mjhip_contextLoadKernel: sparse-Jacobian models run the generic kernel");
    return MJHIP_ERR_MODEL;
  }
  hipSetDevice(c->device);
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  const std::string kname = std::string("k_all_") + name;
  if (hipModuleLoadData(&mod, image) != hipSuccess) {
    set_error("mjhip_contextLoadKernel: hipModuleLoadData failed (not a gfx950 code object?)");
    return MJHIP_ERR_HIP;
  }
  if (hipModuleGetFunction(&fn, mod, kname.c_str()) != hipSuccess) {
    hipModuleUnload(mod);
    set_error("mjhip_contextLoadKernel: no kernel '%s' in the code object", kname.c_str());
    return MJHIP_ERR_HIP;
  }
  int lds = 0;
  if (hipFuncGetAttribute(&lds, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, fn) != hipSuccess) {
    hipModuleUnload(mod);
    set_error("mjhip_contextLoadKernel: hipFuncGetAttribute('%s') failed", kname.c_str());
    return MJHIP_ERR_HIP;
  }
  if (lds > kFastLdsBudget) {
    hipModuleUnload(mod);
    set_error("mjhip_contextLoadKernel: kernel '%s' holds %d B of LDS, over the %d B that let "
              "four workgroups share a CU", kname.c_str(), lds, kFastLdsBudget);
    return MJHIP_ERR_MODEL;
  }
  // its constant stores: the kernel and their count, both by name (the stage bodies of such
  // an object leave those slots to it, so one without it would leave them unwritten)
  hipFunction_t cfn = nullptr;
  hipDeviceptr_t ncp = nullptr;
  size_t ncbytes = 0;
  int nconst = 0;
  const std::string cname = std::string("k_const_") + name;
  const std::string nname = std::string("k_const_count_") + name;
  if (hipModuleGetFunction(&cfn, mod, cname.c_str()) != hipSuccess ||
      hipModuleGetGlobal(&ncp, &ncbytes, mod, nname.c_str()) != hipSuccess ||
      ncbytes != sizeof(int) ||
      hipMemcpy(&nconst, (const void*)ncp, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
      nconst < 0) {
    (void)hipGetLastError();
    hipModuleUnload(mod);
    set_error("mjhip_contextLoadKernel: no kernel '%s' (or its count '%s') in the code object",
              cname.c_str(), nname.c_str());
    return MJHIP_ERR_MODEL;
  }
  c->fast_lds = lds;
  if (c->rt_module) hipModuleUnload(c->rt_module);
  c->rt_module = mod;
  c->rt_fn = fn;
  c->rt_const_fn = cfn;
  c->rt_nconst = nconst;
  c->const_stale = true;
  // the entries its k_all hands on-chip (an object without the count hands none)
  const std::string hname = std::string("k_qm_handoff_") + name;
  hipDeviceptr_t nhp = nullptr;
  size_t nhbytes = 0;
  c->rt_nhand = 0;
  if (hipModuleGetGlobal(&nhp, &nhbytes, mod, hname.c_str()) != hipSuccess ||
      nhbytes != sizeof(int) ||
      hipMemcpy(&c->rt_nhand, (const void*)nhp, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
    c->rt_nhand = 0;
    (void)hipGetLastError();
  }
  const std::string fname = std::string("k_qm_forward_") + name;   // and forwards in registers
  c->rt_nfwd = 0;
  if (hipModuleGetGlobal(&nhp, &nhbytes, mod, fname.c_str()) != hipSuccess ||
      nhbytes != sizeof(int) ||
      hipMemcpy(&c->rt_nfwd, (const void*)nhp, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
    c->rt_nfwd = 0;
    (void)hipGetLastError();
  }
  size_t tbytes = 0;                       // its per-stage timer pointer (MJH_TBUF_EXTERN)
  if (hipModuleGetGlobal(&c->rt_tbuf, &tbytes, mod, "mjh_tbuf") != hipSuccess ||
      tbytes != sizeof(void*)) {
    c->rt_tbuf = nullptr;
    (void)hipGetLastError();
  }
  c->rt_name = name;
  c->rt = FastKernelEntry{signature, nullptr, c->rt_name.c_str(), cmode};
  c->fast = &c->rt;
  c->wl_parity = 0;                        // the run-time kernel zeroes the counters as the
  return hipMemset(c->worklist, 0, 2 * sizeof(int)) == hipSuccess ? MJHIP_OK : MJHIP_ERR_HIP;
}

MJHIP_API int mjhip_ccdBatch(mjhipContext* c, int n, const int* g1, const int* g2,
                             const mjtNum* pos1, const mjtNum* mat1, const mjtNum* pos2,
                             const mjtNum* mat2, const mjtNum* margin, int max_iterations,
                             mjtNum tolerance, int max_contacts, mjtNum dist_cutoff,
                             mjtNum* dist, int* nx, mjtNum* x1, mjtNum* x2) {
  if (!c || n < 0 || (n && (!g1 || !g2 || !pos1 || !mat1 || !pos2 || !mat2 || !dist || !nx ||
                            !x1 || !x2)) || max_iterations < 1 || max_contacts < 0) {
    set_error("mjhip_ccdBatch: bad argument");
    return MJHIP_ERR_ARG;
  }
  // witness points kept per pair: mjCCDStatus holds mjMAXCONPAIR
  const int xcap = max_contacts <= 1 ? 1 :
                   (max_contacts < mjh::CCD_MAXCON ? max_contacts : mjh::CCD_MAXCON);
  if (!n) return MJHIP_OK;
  const int ng = c->hmodel.ngeom;
  for (int i = 0; i < n; i++) {            // every index the kernel reads, checked here
    if (g1[i] < 0 || g1[i] >= ng || g2[i] < 0 || g2[i] >= ng) {
      set_error("mjhip_ccdBatch: geom id out of range at pair %d", i);
      return MJHIP_ERR_ARG;
    }
  }
  HIPCHECK(hipSetDevice(c->device));
  const long nd = mjh::ccdScratchDoubles(max_iterations), ni = mjh::ccdScratchInts(max_iterations);
  std::vector<double> in(24L*n), out(kCcdOut*n);
  for (int i = 0; i < n; i++) {
    memcpy(&in[24L*i], pos1 + 3L*i, 3*sizeof(double));
    memcpy(&in[24L*i + 3], mat1 + 9L*i, 9*sizeof(double));
    memcpy(&in[24L*i + 12], pos2 + 3L*i, 3*sizeof(double));
    memcpy(&in[24L*i + 15], mat2 + 9L*i, 9*sizeof(double));
  }
  // one allocation: inputs, margins, outputs, scratch, then the int arrays
  const size_t bytes = sizeof(double)*(24L*n + n + kCcdOut*n + nd*n) +
                       sizeof(int)*(2L*n + ni*n + n);
  char* buf = nullptr;
  HIPCHECK(hipMalloc((void**)&buf, bytes));
  double* d_in = (double*)buf;
  double* d_margin = d_in + 24L*n;
  double* d_out = d_margin + n;
  double* d_x = d_out + kCcdOut*n;
  int* d_g = (int*)(d_x + nd*n);
  int* d_xi = d_g + 2L*n;
  int* d_bad = d_xi + ni*n;
  std::vector<double> mg(n, 0.0);
  if (margin) memcpy(mg.data(), margin, n*sizeof(double));
  std::vector<int> bad(n);
  int rc = MJHIP_OK;
  auto run = [&]() -> int {
    HIPCHECK(hipMemcpy(d_in, in.data(), 24L*n*sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_margin, mg.data(), n*sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_g, g1, n*sizeof(int), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_g + n, g2, n*sizeof(int), hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(d_bad, 0, n*sizeof(int)));
    if (mjhip_launchCcd(c->stream, c->dmodel, n, d_g, d_g + n, d_in, d_margin, max_iterations,
                        tolerance, max_contacts, dist_cutoff, d_x, d_xi, d_out, d_bad)) {
      set_error("mjhip_ccdBatch: kernel launch failed");
      return MJHIP_ERR_HIP;
    }
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(hipMemcpy(out.data(), d_out, kCcdOut*n*sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(bad.data(), d_bad, n*sizeof(int), hipMemcpyDeviceToHost));
    return MJHIP_OK;
  };
  rc = run();
  hipFree(buf);
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    if (bad[i]) {
      set_error(bad[i] == 1 ? "mjhip_ccdBatch: pair %d outgrew the solver's polytope capacity"
                            : "mjhip_ccdBatch: pair %d needs multicontact outside the built "
                              "subset (a shape other than a box or mesh, or a mesh polygon "
                              "or vertex fan over 16)", i);
      return MJHIP_ERR_MODEL;
    }
    const double* o = &out[kCcdOut*i];
    dist[i] = o[0];
    nx[i] = (int)o[1];
    const int k = nx[i] < xcap ? (nx[i] > 1 ? nx[i] : 1) : xcap;
    memcpy(x1 + 3L*xcap*i, o + 2, 3*k*sizeof(double));
    memcpy(x2 + 3L*xcap*i, o + 2 + 3*mjh::CCD_MAXCON, 3*k*sizeof(double));
  }
  return MJHIP_OK;
}

MJHIP_API int mjhip_contextCapacity(const mjhipContext* c) { return c ? c->capacity : 0; }

MJHIP_API const char* mjhip_contextFastKernel(const mjhipContext* c) {
  return (c && c->fast) ? c->fast->name : nullptr;
}

MJHIP_API int mjhip_contextFastKernelLds(const mjhipContext* c) {
  return (c && c->fast) ? c->fast_lds : 0;
}

MJHIP_API int mjhip_contextLastPath(const mjhipContext* c) { return c ? c->last_path : -1; }

MJHIP_API int mjhip_contextConstStores(const mjhipContext* c) {
  if (!c || !c->fast) return 0;
  if (c->fast == &c->rt) return c->rt_nconst;
  return c->fast->const_stores ? c->fast->const_stores() : 0;
}

MJHIP_API int mjhip_contextQmHandoff(const mjhipContext* c) {
  if (!c || !c->fast) return 0;
  if (c->fast == &c->rt) return c->rt_nhand;
  return (c->mirror.qm_handoff && c->fast->qm_handoff) ? c->fast->qm_handoff() : 0;
}

MJHIP_API int mjhip_contextQmForward(const mjhipContext* c) {
  if (!c || !c->fast) return 0;
  if (c->fast == &c->rt) return c->rt_nfwd;
  return (c->mirror.qm_handoff && c->fast->qm_forward) ? c->fast->qm_forward() : 0;
}

MJHIP_API int mjhip_contextConstLaunches(const mjhipContext* c) {
  return c ? c->const_launches : 0;
}

// Before any launch that runs generated stage bodies: the model-constant slots they leave out
// (codegen.py CONST_ONCE) are written by k_const over the whole capacity when they may be
// stale, on the context's current stream, so ahead of the launch that follows. The generic
// kernel stores the same values in the same slots, so the two paths mix freely on a context.
static int ensure_const(mjhipContext* c) {
  if (!c->const_stale || !c->fast) return MJHIP_OK;
  if (mjhip_contextConstStores(c) > 0) {
    const int nblk = c->capacity / 64;
    if (c->fast == &c->rt) {
      void* args[] = {&c->mirror};
      HIPCHECK(hipModuleLaunchKernel(c->rt_const_fn, nblk, 1, 1, 64, 1, 1, 0, c->stream, args,
                                     nullptr));
    } else {
      c->fast->launch_const(c->stream, c->mirror, nblk);
      HIPCHECK(hipGetLastError());
    }
    c->const_launches++;
  }
  c->const_stale = false;
  return MJHIP_OK;
}

MJHIP_API const char* mjhip_contextConstraintKernel(const mjhipContext* c) {
  return c ? c->con_kernel : nullptr;
}

MJHIP_API int mjhip_worklistCount(mjhipContext* c) {
  if (!c) return -1;
  int n = 0;
  if (hipMemcpy(&n, c->worklist + c->wl_last, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return n;
}

MJHIP_API void* mjhip_contextStream(mjhipContext* c) { return c ? (void*)c->stream : nullptr; }

MJHIP_API int mjhip_contextSetStream(mjhipContext* c, void* stream) {
  if (!c) return MJHIP_ERR_ARG;
  if (c->own_stream && c->stream) {
    hipStreamSynchronize(c->stream);
    hipStreamDestroy(c->stream);
  }
  c->stream = (hipStream_t)stream;
  c->own_stream = false;
  return MJHIP_OK;
}

// the straight-line path's passes after the constraint part: sensors (and the transmission
// and energy terms they carry), INVDISCRETE's qacc restore, the status checks; then the
// work-list counters change hands
static int finish_fast(mjhipContext* c, int B, dim3 grid, dim3 block, int skipsensor,
                       int* status, bool discrete) {
  const int sensors = !skipsensor && c->hmodel.nsensor > 0 &&
                      !(c->hmodel.opt.disableflags & mjhipDSBL_SENSOR);
  const int trn = mjh_needTrnAfter(&c->hmodel) && !discrete;   // discrete: already formed
  if (sensors || trn || (c->hmodel.opt.enableflags & mjhipENBL_ENERGY)) {
    hipLaunchKernelGGL(k_sensors, grid, block, 0, c->stream, c->dmodel, c->mirror, B,
                       sensors, trn);
    HIPCHECK(hipGetLastError());
  }
  if (discrete) {                        // the caller's qacc back, after mj_sensorAcc
    hipLaunchKernelGGL(k_discrete_restore, grid, block, 0, c->stream, c->dmodel, c->mirror, B);
  }
  if (status) {
    hipLaunchKernelGGL(k_check, grid, block, 0, c->stream, c->dmodel, c->mirror, B, status,
                       (int)mjhipSTAGE_NONE);
    HIPCHECK(hipGetLastError());
  }
  c->wl_last = c->wl_parity;
  c->wl_parity ^= 1;
  return MJHIP_OK;
}

// internal launch_inverse flag (not a public MJHIP_FLAG_*): run the straight-line kernel of a
// work-list model without its constraint kernel; the next launch_inverse call continues the
// same work-list and serves both (the bare pipeline only: the FD stage-skip layout)
constexpr int kFlagDeferRows = 1 << 30;
// internal mjhip_inverseFDBatchEx flag: no stage-skip layout (every instance base-major, every
// field stored): the single-instance mjd_inverseFD reads back its last evaluation's fields
constexpr int kFlagFDFull = 1 << 29;

// range: null, or a device-side instance range {first, end} for the straight-line kernel (B
// then only sizes the grid: end - first <= B); only the FD fall-back uses it, on models whose
// whole pipeline is the straight-line and constraint kernels
static int launch_inverse(mjhipContext* c, int B, const double* qpos, const double* qvel,
                          const double* qacc, double* qfrc, int skipstage, int* status,
                          int flags = 0, int skipsensor = 0, const int* range = nullptr) {
  dim3 grid((B + 63) / 64), block(64);
  if (range && (skipstage != mjhipSTAGE_NONE || !c->fast || (flags & MJHIP_FLAG_GENERIC) ||
                status || qpos || qfrc || c->spatial || mjh::hasFluid(c->hmodel) ||
                mjh::hasDiscrete(c->hmodel) || mjh_needTrnAfter(&c->hmodel) || !skipsensor ||
                (c->hmodel.opt.enableflags & mjhipENBL_ENERGY))) {
    set_error("launch_inverse: a device-side range needs the bare straight-line pipeline");
    return MJHIP_ERR_ARG;
  }
  c->last_path = 0;
  if (skipstage == mjhipSTAGE_NONE && c->fast && !(flags & MJHIP_FLAG_GENERIC)) {
    c->last_path = 1;
    if (const int rc = ensure_const(c)) return rc;
    // two work-list counters alternate: this launch counts into `cnt` (zeroed by the
    // previous launch's k_pos, or at context creation) and zeroes `nxt` for the next one
    int* cnt = c->worklist + c->wl_parity;
    int* nxt = c->worklist + (c->wl_parity ^ 1);
    const bool discrete = mjh::hasDiscrete(c->hmodel);
    // fused rows whenever nbody allows, INVDISCRETE included (post_pass.h fastFusedOk)
    const bool fused = mjh::fastFusedOk(c->dmodel);
    if (c->fast->launch) {
      c->fast->launch(grid, block, c->stream, c->mirror, B, qpos, qvel, qacc, qfrc, status,
                      c->worklist + 2, cnt, nxt, c->mirror.efc_count, range);
      HIPCHECK(hipGetLastError());
    } else {                             // run-time specialized k_all_<name> (same arguments)
      int* wl = c->worklist + 2;
      int* efc = c->mirror.efc_count;
      void* args[] = {&c->mirror, &B, &qpos, &qvel, &qacc, &qfrc, &status, &wl, &cnt, &nxt,
                      &efc, (void*)&range};
      HIPCHECK(hipModuleLaunchKernel(c->rt_fn, grid.x, 1, 1, 64, 1, 1, 0, c->stream, args,
                                     nullptr));
    }
    if (flags & kFlagDeferRows) {
      // mjhip_inverseFDBatch: the work-list this launch filled is served after the next
      // launch, which appends to the same counter (the parity is not flipped)
      return MJHIP_OK;
    }
    if (c->spatial) {                    // spatial tendons and all of mj_passive
      hipLaunchKernelGGL(k_tendon_after, grid, block, 0, c->stream, c->dmodel, c->mirror, B);
    } else if (mjh::hasFluid(c->dmodel)) {   // fluid forces into qfrc_passive
      hipLaunchKernelGGL(k_fluid_after, grid, block, 0, c->stream, c->dmodel, c->mirror, B);
    }
    if (discrete) {                      // mj_discreteAcc and its RNE before the constraints
      hipLaunchKernelGGL(k_discrete_before, grid, block, 0, c->stream, c->dmodel, c->mirror, B,
                         mjh_needTrnAfter(&c->hmodel));
    }
    const int* wl = c->worklist + 2;
    if (fused && c->coop && c->fast->cmode) {   // cooperative lanes per instance
      const bool contact = c->con_cap > 0, list = c->fast->cmode == 1;
#define MJHIP_LAUNCH_COOP(G, C, L, X)                                                         \
      do {                                                                                    \
        c->con_kernel = "k_constraint_coop<" #G ", " #C ", " #L ", " #X ">";                \
        hipLaunchKernelGGL((k_constraint_coop<G, C, L, X>), dim3(coopGrid(B, G, L)),          \
                           dim3(64), coopLdsBytes(c->dmodel, G, c->efc_cap, c->boxpair,       \
                                                  c->npair, c->con_cap),                      \
                           c->stream,                                                         \
                           c->dmodel, c->mirror, B, wl,                                       \
                           (const int*)cnt, c->pairs, c->cparams, c->masks, c->npair, qfrc,  \
                           status);                                                           \
      } while (0)
      if (contact && c->boxpair) {       // the box-box path is compiled in only here
        if (list) MJHIP_LAUNCH_COOP(16, true, true, true);
        else MJHIP_LAUNCH_COOP(16, true, false, true);
      } else if (contact) {
        if (list) MJHIP_LAUNCH_COOP(16, true, true, false);
        else if (c->coop == 8) MJHIP_LAUNCH_COOP(8, true, false, false);
        else if (c->coop == 32) MJHIP_LAUNCH_COOP(32, true, false, false);
        else MJHIP_LAUNCH_COOP(16, true, false, false);
      } else {
        if (list) MJHIP_LAUNCH_COOP(16, false, true, false);
        else MJHIP_LAUNCH_COOP(16, false, false, false);
      }
#undef MJHIP_LAUNCH_COOP
    } else {
#define MJHIP_LAUNCH_CON(C, F, L)                                                             \
    do {                                                                                      \
      c->con_kernel = "k_constraint<" #C ", " #F ", " #L ">";                               \
      hipLaunchKernelGGL((k_constraint<C, F, L>), grid, block,                                \
                         ((C && F) ? mjh::gstageBytes(c->dmodel) : 0) +                       \
                         ((!L && qfrc) ? 64u*sizeof(double)*c->dmodel.nv : 0), c->stream,    \
                         c->dmodel, c->mirror, B, wl, (const int*)cnt, qfrc, status);         \
    } while (0)
    if (c->fast->cmode == 2) {          // contacts or friction loss: every instance
      if (c->con_cap > 0) {
        if (fused) MJHIP_LAUNCH_CON(true, true, false); else MJHIP_LAUNCH_CON(true, false, false);
      } else {
        if (fused) MJHIP_LAUNCH_CON(false, true, false);
        else MJHIP_LAUNCH_CON(false, false, false);
      }
    } else if (c->fast->cmode == 1) {   // limit-active instances (k_pos's work-list)
      if (fused) MJHIP_LAUNCH_CON(false, true, true); else MJHIP_LAUNCH_CON(false, false, true);
    }
#undef MJHIP_LAUNCH_CON
    }
    HIPCHECK(hipGetLastError());
    return finish_fast(c, B, grid, block, skipsensor, status, discrete);
  }
  // mj_inverseSkip(POS / VEL) on the straight-line kernels: the bare pipeline (no passes
  // after the generated kernels) of a model whose rows serve only limit-active instances
  const char* noskip = getenv("MJHIP_SKIP_GENERIC");
  if ((skipstage == mjhipSTAGE_POS || skipstage == mjhipSTAGE_VEL) && c->fast &&
      c->fast->launch_skip && !(flags & MJHIP_FLAG_GENERIC) && !c->spatial &&
      !mjh::hasFluid(c->hmodel) && !mjh::hasDiscrete(c->hmodel) &&
      !mjh_needTrnAfter(&c->hmodel) && !(c->hmodel.opt.enableflags & mjhipENBL_ENERGY) &&
      (skipsensor || !c->hmodel.nsensor || (c->hmodel.opt.disableflags & mjhipDSBL_SENSOR)) &&
      !(noskip && noskip[0] == '1')) {
    // row-major inputs into the mirror, as k_inverse copies them: the remaining stages read
    // qpos (springs) and qvel (mj_rne's cdof_dot * qvel) even when their own stage is skipped
    const int nq = c->hmodel.nq, nv = c->hmodel.nv;
    if (qpos) {
      hipLaunchKernelGGL(k_to_mirror, dim3(((long)B*nq + 255)/256), dim3(256), 0, c->stream,
                         qpos, c->mirror.qpos, B, nq);
    }
    if (qvel) {
      hipLaunchKernelGGL(k_to_mirror, dim3(((long)B*nv + 255)/256), dim3(256), 0, c->stream,
                         qvel, c->mirror.qvel, B, nv);
    }
    if (qacc) {
      hipLaunchKernelGGL(k_to_mirror, dim3(((long)B*nv + 255)/256), dim3(256), 0, c->stream,
                         qacc, c->mirror.qacc, B, nv);
    }
    c->last_path = 2;
    if (const int rc = ensure_const(c)) return rc;
    c->fast->launch_skip(c->stream, c->mirror, B, skipstage, qfrc, status, c->mirror.efc_count);
    HIPCHECK(hipGetLastError());
    if (c->fast->cmode) {                // work-list rows, or every instance (contacts)
      hipLaunchKernelGGL(k_skip_rows, grid, block, 0, c->stream, c->dmodel, c->mirror, B,
                         skipstage, qfrc, (int)(c->fast->cmode == 2));
      HIPCHECK(hipGetLastError());
    }
    if (status) {
      hipLaunchKernelGGL(k_check, grid, block, 0, c->stream, c->dmodel, c->mirror, B, status,
                         skipstage);
      HIPCHECK(hipGetLastError());
    }
    return MJHIP_OK;
  }
#define MJHIP_LAUNCH_K(SK, C, F)                                                              \
  hipLaunchKernelGGL((k_inverse<SK, C, F>), grid, block,                                      \
                     (C && F) ? mjh::gstageBytes(c->dmodel) : 0, c->stream, c->dmodel,        \
                     c->mirror, B, qpos, qvel, qacc, qfrc, status, skipsensor)
#define MJHIP_LAUNCH_GENERIC(SK)                                                              \
  if (c->con_cap > 0) {                                                                       \
    MJHIP_LAUNCH_K(SK, true, false);                                                          \
  } else {                                                                                    \
    MJHIP_LAUNCH_K(SK, false, false);                                                         \
  }
  switch (skipstage) {
  case mjhipSTAGE_NONE:
    if (mjh::fusedOk(c->dmodel, mjhipSTAGE_NONE)) {
      if (c->con_cap > 0) MJHIP_LAUNCH_K(0, true, true); else MJHIP_LAUNCH_K(0, false, true);
    } else {
      MJHIP_LAUNCH_GENERIC(0)
    }
    break;
  case mjhipSTAGE_POS:
    MJHIP_LAUNCH_GENERIC(1)
    break;
  case mjhipSTAGE_VEL:
    MJHIP_LAUNCH_GENERIC(2)
    break;
  default:
    set_error("skipstage must be mjSTAGE_NONE, mjSTAGE_POS or mjSTAGE_VEL");
    return MJHIP_ERR_ARG;
  }
#undef MJHIP_LAUNCH_GENERIC
#undef MJHIP_LAUNCH_K
  HIPCHECK(hipGetLastError());
  return MJHIP_OK;
}

//---------------------------------- per-stage timers ------------------------------------------

// point every copy of mjh_tbuf (this unit's, the generated kernels' and the run-time code
// object's) at p; blocking copies, after the stream's earlier work
static int timers_attach(mjhipContext* c, unsigned long long* p) {
  HIPCHECK(hipStreamSynchronize(c->stream));
  HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(mjh_tbuf), &p, sizeof(p)));
  if (mjhip_genSetTimerBuf(p) || mjhip_genExactSetTimerBuf(p) ||
      mjhip_setTimerBufConstraint(p) ||
      mjhip_setTimerBufInverse(p)) {
    set_error("setting the kernel units' timer pointers failed");
    return MJHIP_ERR_HIP;
  }
  if (c->rt_tbuf) HIPCHECK(hipMemcpyHtoD(c->rt_tbuf, &p, sizeof(p)));
  return MJHIP_OK;
}

// point every mjh_tbuf copy back at null (after the stream's earlier work), so that no kernel
// adds into an accumulator that is about to be freed; the caller frees it only on success
static int timers_detach(mjhipContext* c) {
  const int rc = timers_attach(c, nullptr);
  if (g_timed_ctx == c) g_timed_ctx = nullptr;
  return rc;
}

// fold one call's phase-mark sums (engine_device.h MJH_PHASE: slots and wave counts) into
// the reference's timer slots: mean wave time per stage, 100 MHz ticks -> milliseconds
static void timers_fold(mjhipContext* c, const unsigned long long* t, float call_ms) {
  auto span = [&](int a, int b, int n) {
    return t[n] ? (double)(long long)(t[b] - t[a]) / (double)t[n] / 1e5 : 0.0;
  };
  double kin = 0, inertia = 0, col = 0, make = 0, vel = 0, con = 0;
  if (t[24]) {                             // generic k_inverse, marks 0-9
    kin += span(0, 1, 24) + span(1, 2, 24) + span(5, 6, 24);
    inertia += span(2, 3, 24);
    col += span(3, 4, 24);
    make += span(4, 5, 24);
    vel += span(6, 7, 24);
    con += span(7, 8, 24);
  }
  if (t[27]) {                             // straight-line k_all, marks 19-22
    kin += span(19, 20, 27);
    inertia += span(20, 21, 27);
    vel += span(21, 22, 27);
  }
  if (t[25]) {                             // one-lane k_constraint, marks 10-13
    col += span(10, 11, 25);
    make += span(11, 12, 25);
    con += span(12, 13, 25);
  }
  if (t[26]) {                             // k_constraint_coop, marks 14, 15, (18,) 16, 17
    col += span(14, 15, 26);
    make += t[18] ? span(15, 18, 26) + span(18, 16, 26) : span(15, 16, 26);
    con += span(16, 17, 26);
  }
  auto add = [&](int slot, double ms) {
    c->timer[slot].duration += ms;
    c->timer[slot].number += 1;
  };
  add(mjhipTIMER_INVERSE, call_ms);
  add(mjhipTIMER_POSITION, kin + inertia + col + make);
  add(mjhipTIMER_POS_KINEMATICS, kin);
  add(mjhipTIMER_POS_INERTIA, inertia);
  add(mjhipTIMER_POS_COLLISION, col);
  add(mjhipTIMER_POS_MAKE, make);
  add(mjhipTIMER_VELOCITY, vel);
  add(mjhipTIMER_CONSTRAINT, con);
}

MJHIP_API int mjhip_contextTimers(mjhipContext* c, int enable) {
  if (!c) {
    set_error("mjhip_contextTimers: null context");
    return MJHIP_ERR_ARG;
  }
  HIPCHECK(hipSetDevice(c->device));
  if (!enable) {
    if (c->tbuf) {
      if (const int rc = timers_detach(c)) return rc;   // a unit may still point at it
      HIPCHECK(hipFree(c->tbuf));
      c->tbuf = nullptr;
    }
    if (g_timed_ctx == c) g_timed_ctx = nullptr;
    return MJHIP_OK;
  }
  if (g_timed_ctx && g_timed_ctx != c) {
    set_error("mjhip_contextTimers: another context of this process is being timed");
    return MJHIP_ERR_ARG;
  }
  if (!c->tbuf) {
    unsigned long long* buf = nullptr;
    HIPCHECK(hipMalloc((void**)&buf, MJH_TSLOTS * sizeof(unsigned long long)));
    if (hipMemset(buf, 0, MJH_TSLOTS * sizeof(unsigned long long)) != hipSuccess) {
      hipFree(buf);
      set_error("mjhip_contextTimers: hipMemset failed");
      return MJHIP_ERR_HIP;
    }
    c->tbuf = buf;
  }
  if (!c->tev0) HIPCHECK(hipEventCreate(&c->tev0));
  if (!c->tev1) HIPCHECK(hipEventCreate(&c->tev1));
  g_timed_ctx = c;                         // only once everything it needs exists
  return MJHIP_OK;
}

MJHIP_API int mjhip_timerRead(mjhipContext* c, mjhipTimerStat* out, int reset) {
  if (!c || !out) {
    set_error("mjhip_timerRead: bad argument");
    return MJHIP_ERR_ARG;
  }
  memcpy(out, c->timer, sizeof(c->timer));
  if (reset) memset(c->timer, 0, sizeof(c->timer));
  return MJHIP_OK;
}

MJHIP_API int mjhip_inverseBatch(mjhipContext* c, int B, const mjtNum* qpos,
                                 const mjtNum* qvel, const mjtNum* qacc, mjtNum* qfrc_inverse,
                                 int skipstage, int skipsensor, int flags, int* status) {
  if (!c || B < 0) {
    set_error("mjhip_inverseBatch: bad argument");
    return MJHIP_ERR_ARG;
  }
  if (B > c->capacity) {
    set_error("batch %d exceeds context capacity %d", B, c->capacity);
    return MJHIP_ERR_CAPACITY;
  }
  if (B == 0) return MJHIP_OK;
  HIPCHECK(hipSetDevice(c->device));
  const mjhipModel& m = c->hmodel;
  const bool dev = flags & MJHIP_FLAG_DEVICE_PTRS;
  const bool mirror_in = flags & MJHIP_FLAG_MIRROR_INPUT;
  const double *dq = nullptr, *dv = nullptr, *da = nullptr;
  double* dqfrc = nullptr;
  double* sq = c->stage;
  double* sv = sq + (size_t)c->capacity*m.nq;
  double* sa = sv + (size_t)c->capacity*m.nv;
  double* sf = sa + (size_t)c->capacity*m.nv;
  if (!mirror_in) {
    if (!qpos || !qvel || !qacc) {
      set_error("mjhip_inverseBatch: qpos/qvel/qacc required without MJHIP_FLAG_MIRROR_INPUT");
      return MJHIP_ERR_ARG;
    }
    if (dev) {
      dq = qpos; dv = qvel; da = qacc;
    } else {
      HIPCHECK(hipMemcpyAsync(sq, qpos, sizeof(double)*(size_t)B*m.nq, hipMemcpyHostToDevice,
                              c->stream));
      HIPCHECK(hipMemcpyAsync(sv, qvel, sizeof(double)*(size_t)B*m.nv, hipMemcpyHostToDevice,
                              c->stream));
      HIPCHECK(hipMemcpyAsync(sa, qacc, sizeof(double)*(size_t)B*m.nv, hipMemcpyHostToDevice,
                              c->stream));
      dq = sq; dv = sv; da = sa;
    }
  }
  if (qfrc_inverse) dqfrc = dev ? qfrc_inverse : sf;
  // per-instance statuses only when the caller can see them (status array, or the host path's
  // return code): a device-pointer call without them skips the input checks entirely
  const bool want_status = status || !dev;
  const bool timed = c->tbuf != nullptr;
  if (timed) {
    int trc = timers_attach(c, c->tbuf);
    if (trc) {
      timers_attach(c, nullptr);
      return trc;
    }
    HIPCHECK(hipEventRecord(c->tev0, c->stream));
  }
  int rc = launch_inverse(c, B, dq, dv, da, dqfrc, skipstage, want_status ? c->status : nullptr,
                          flags, skipsensor);
  if (timed) {
    HIPCHECK(hipEventRecord(c->tev1, c->stream));
    const int arc = timers_attach(c, nullptr);   // synchronizes the stream first
    if (rc) return rc;
    if (arc) return arc;
    unsigned long long t[MJH_TSLOTS];
    float call_ms = 0;
    HIPCHECK(hipMemcpy(t, c->tbuf, sizeof(t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemset(c->tbuf, 0, sizeof(t)));
    HIPCHECK(hipEventElapsedTime(&call_ms, c->tev0, c->tev1));
    for (int k = 0; k < MJH_TSLOTS; k++) c->traw[k] += t[k];
    timers_fold(c, t, call_ms);
  }
  if (rc) return rc;
  if (qfrc_inverse && !dev) {
    HIPCHECK(hipMemcpyAsync(qfrc_inverse, sf, sizeof(double)*(size_t)B*m.nv,
                            hipMemcpyDeviceToHost, c->stream));
  }
  int anybad = 0;
  if (want_status) {
    std::vector<int> st(B);
    HIPCHECK(hipMemcpyAsync(st.data(), c->status, sizeof(int)*(size_t)B, hipMemcpyDeviceToHost,
                            c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < B; i++) anybad |= st[i];
    if (status) memcpy(status, st.data(), sizeof(int)*(size_t)B);
  }
  return anybad ? MJHIP_ERR_INSTANCE : MJHIP_OK;
}

// the actuator subset of the entry points that take no activations (mjhip_forwardBatch,
// mjhip_inverseFDBatchEx): fixed/affine gain, none/affine bias, no activation dynamics
static const char* actuation_stateless(const mjhipModel& m) {
  for (int i = 0; i < m.nu; i++) {
    if ((m.actuator_gaintype[i] != mjhipGAIN_FIXED && m.actuator_gaintype[i] != mjhipGAIN_AFFINE) ||
        (m.actuator_biastype[i] != mjhipBIAS_NONE && m.actuator_biastype[i] != mjhipBIAS_AFFINE) ||
        m.actuator_dyntype[i] != mjhipDYN_NONE) {
      return "muscle/user gain or bias, or actuator dynamics (act)";
    }
  }
  return nullptr;
}

// the actuator subset of the device mj_fwdActuation (mjh::fwdActuation): every dynamics, gain
// and bias type but the user callbacks, one activation per stateful actuator
static const char* actuation_unsupported(const mjhipModel& m) {
  for (int i = 0; i < m.nu; i++) {
    if (m.actuator_dyntype[i] < mjhipDYN_NONE || m.actuator_dyntype[i] >= mjhipDYN_USER ||
        m.actuator_gaintype[i] < mjhipGAIN_FIXED || m.actuator_gaintype[i] >= mjhipGAIN_USER ||
        m.actuator_biastype[i] < mjhipBIAS_NONE || m.actuator_biastype[i] >= mjhipBIAS_USER) {
      return "user actuator dynamics, gain or bias";
    }
    if (m.actuator_actnum && m.actuator_actnum[i] > 1) return "an actuator with actdim > 1";
  }
  return nullptr;
}

// the staging slices behind qpos, qvel, qacc, qfrc (stage layout of mjhip_contextCreate)
struct StageAct {
  double *ctrl, *act, *act_dot, *act_next;
};
static StageAct stage_act(mjhipContext* c) {
  const mjhipModel& m = c->hmodel;
  StageAct s;
  s.ctrl = c->stage + (size_t)c->capacity*(m.nq + 3*(size_t)m.nv);
  s.act = s.ctrl + (size_t)c->capacity*m.nu;
  s.act_dot = s.act + (size_t)c->capacity*m.na;
  s.act_next = s.act_dot + (size_t)c->capacity*m.na;
  return s;
}

// the per-instance status words of the call that just ran, as every batch entry point
// returns them
static int collect_status(mjhipContext* c, int B, int* status, bool want) {
  int anybad = 0;
  if (want) {
    std::vector<int> st(B);
    HIPCHECK(hipMemcpyAsync(st.data(), c->status, sizeof(int)*(size_t)B, hipMemcpyDeviceToHost,
                            c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < B; i++) anybad |= st[i];
    if (status) memcpy(status, st.data(), sizeof(int)*(size_t)B);
  }
  return anybad ? MJHIP_ERR_INSTANCE : MJHIP_OK;
}

MJHIP_API int mjhip_forwardBatchEx(mjhipContext* c, int B, const mjtNum* qpos,
                                   const mjtNum* qvel, const mjtNum* ctrl, const mjtNum* act,
                                   mjtNum* qacc, mjtNum* act_dot, mjtNum* act_next, int flags,
                                   int* status) {
  if (!c || B < 0) {
    set_error("mjhip_forwardBatch: bad argument");
    return MJHIP_ERR_ARG;
  }
  if (B > c->capacity) {
    set_error("batch %d exceeds context capacity %d", B, c->capacity);
    return MJHIP_ERR_CAPACITY;
  }
  const mjhipModel& m = c->hmodel;
  if (const char* why = actuation_unsupported(m)) {
    set_error("mjhip_forwardBatch: %s is not supported", why);
    return MJHIP_ERR_MODEL;
  }
  if (B == 0) return MJHIP_OK;
  HIPCHECK(hipSetDevice(c->device));
  const bool dev = flags & MJHIP_FLAG_DEVICE_PTRS;
  const bool mirror_in = flags & MJHIP_FLAG_MIRROR_INPUT;
  const double *dq = nullptr, *dv = nullptr, *dc = nullptr, *dact = nullptr;
  double* sq = c->stage;
  double* sv = sq + (size_t)c->capacity*m.nq;
  double* sa = sv + (size_t)c->capacity*m.nv;
  const StageAct sx = stage_act(c);
  if (!mirror_in) {
    if (!qpos || !qvel) {
      set_error("mjhip_forwardBatch: qpos/qvel required without MJHIP_FLAG_MIRROR_INPUT");
      return MJHIP_ERR_ARG;
    }
    if (dev) {
      dq = qpos; dv = qvel; dc = ctrl; dact = m.na ? act : nullptr;
    } else {
      HIPCHECK(hipMemcpyAsync(sq, qpos, sizeof(double)*(size_t)B*m.nq, hipMemcpyHostToDevice,
                              c->stream));
      HIPCHECK(hipMemcpyAsync(sv, qvel, sizeof(double)*(size_t)B*m.nv, hipMemcpyHostToDevice,
                              c->stream));
      if (ctrl && m.nu) {
        HIPCHECK(hipMemcpyAsync(sx.ctrl, ctrl, sizeof(double)*(size_t)B*m.nu,
                                hipMemcpyHostToDevice, c->stream));
      }
      if (act && m.na) {
        HIPCHECK(hipMemcpyAsync(sx.act, act, sizeof(double)*(size_t)B*m.na,
                                hipMemcpyHostToDevice, c->stream));
      }
      dq = sq; dv = sv; dc = (ctrl && m.nu) ? sx.ctrl : nullptr;
      dact = (act && m.na) ? sx.act : nullptr;
    }
  }
  double* dqacc = qacc ? (dev ? qacc : sa) : nullptr;
  double* ddot = (act_dot && m.na) ? (dev ? act_dot : sx.act_dot) : nullptr;
  double* dnext = (act_next && m.na) ? (dev ? act_next : sx.act_next) : nullptr;
  dim3 grid((B + 63) / 64), block(64);
  if (c->con_cap > 0) {
    hipLaunchKernelGGL(k_forward<true>, grid, block, 0, c->stream, c->dmodel, c->mirror, B, dq,
                       dv, dc, dact, dqacc, ddot, dnext, c->status);
  } else {
    hipLaunchKernelGGL(k_forward<false>, grid, block, 0, c->stream, c->dmodel, c->mirror, B, dq,
                       dv, dc, dact, dqacc, ddot, dnext, c->status);
  }
  HIPCHECK(hipGetLastError());
  if (!dev) {
    if (qacc) {
      HIPCHECK(hipMemcpyAsync(qacc, sa, sizeof(double)*(size_t)B*m.nv, hipMemcpyDeviceToHost,
                              c->stream));
    }
    if (ddot) {
      HIPCHECK(hipMemcpyAsync(act_dot, ddot, sizeof(double)*(size_t)B*m.na,
                              hipMemcpyDeviceToHost, c->stream));
    }
    if (dnext) {
      HIPCHECK(hipMemcpyAsync(act_next, dnext, sizeof(double)*(size_t)B*m.na,
                              hipMemcpyDeviceToHost, c->stream));
    }
  }
  return collect_status(c, B, status, status || !dev);
}

MJHIP_API int mjhip_forwardBatch(mjhipContext* c, int B, const mjtNum* qpos, const mjtNum* qvel,
                                 const mjtNum* ctrl, mjtNum* qacc, int flags, int* status) {
  if (c) {
    if (const char* why = actuation_stateless(c->hmodel)) {
      set_error("mjhip_forwardBatch: %s is not supported (mjhip_forwardBatchEx takes act)", why);
      return MJHIP_ERR_MODEL;
    }
  }
  return mjhip_forwardBatchEx(c, B, qpos, qvel, ctrl, nullptr, qacc, nullptr, nullptr, flags,
                              status);
}

// Device buffers of one host-array rollout call, released when the call returns
struct RolloutTemps {
  std::vector<void*> bufs;
  ~RolloutTemps() { for (void* p : bufs) hipFree(p); }
  double* get(size_t doubles) {
    void* p = nullptr;
    if (hipMalloc(&p, sizeof(double)*(doubles ? doubles : 1)) != hipSuccess) return nullptr;
    bufs.push_back(p);
    return (double*)p;
  }
};

MJHIP_API int mjhip_rolloutBatch(mjhipContext* c, int B, int nstep, const mjhipRolloutIn* in,
                                 const mjhipRolloutOut* out, int flags, int* status,
                                 int* steps_done) {
  if (!in || in->size < (int)sizeof(mjhipRolloutIn)) {
    set_error("mjhip_rolloutBatch: mjhipRolloutIn is NULL or its size field (%d) is below %d",
              in ? in->size : 0, (int)sizeof(mjhipRolloutIn));
    return MJHIP_ERR_ARG;
  }
  if (!out || out->size < (int)sizeof(mjhipRolloutOut)) {
    set_error("mjhip_rolloutBatch: mjhipRolloutOut is NULL or its size field (%d) is below %d",
              out ? out->size : 0, (int)sizeof(mjhipRolloutOut));
    return MJHIP_ERR_ARG;
  }
  if (!c) {
    if (mjhip_deviceCount() <= 0) {
      set_error("mjhip_rolloutBatch: no HIP device (there is no CPU fallback)");
      return MJHIP_ERR_NO_DEVICE;
    }
    set_error("mjhip_rolloutBatch: NULL context");
    return MJHIP_ERR_ARG;
  }
  const int modes[3] = {in->ctrl_mode, in->qfrc_applied_mode, in->xfrc_applied_mode};
  const mjtNum* ptrs[3] = {in->ctrl, in->qfrc_applied, in->xfrc_applied};
  for (int k = 0; k < 3; k++) {
    if (modes[k] < MJHIP_ROLLOUT_ABSENT || modes[k] > MJHIP_ROLLOUT_PERSTEP ||
        (modes[k] != MJHIP_ROLLOUT_ABSENT && !ptrs[k])) {
      set_error("mjhip_rolloutBatch: input %d has mode %d and pointer %p", k, modes[k],
                (const void*)ptrs[k]);
      return MJHIP_ERR_ARG;
    }
  }
  if (B < 0 || nstep < 0) {
    set_error("mjhip_rolloutBatch: bad argument");
    return MJHIP_ERR_ARG;
  }
  if (B > c->capacity) {
    set_error("batch %d exceeds context capacity %d", B, c->capacity);
    return MJHIP_ERR_CAPACITY;
  }
  const mjhipModel& m = c->hmodel;
  if (const char* why = actuation_unsupported(m)) {
    set_error("mjhip_rolloutBatch: %s is not supported", why);
    return MJHIP_ERR_MODEL;
  }
  const bool dev = flags & MJHIP_FLAG_DEVICE_PTRS;
  const bool mirror_in = flags & MJHIP_FLAG_MIRROR_INPUT;
  if (!mirror_in && (!in->qpos || !in->qvel)) {
    set_error("mjhip_rolloutBatch: qpos/qvel required without MJHIP_FLAG_MIRROR_INPUT");
    return MJHIP_ERR_ARG;
  }
  if (B == 0) return MJHIP_OK;              // nstep = 0 still places the state in the mirror
  HIPCHECK(hipSetDevice(c->device));
  if (!c->rollout_scratch) {
    const size_t n = (size_t)mjhip_rolloutScratchDoubles(&m) * c->capacity;
    HIPCHECK(hipMalloc((void**)&c->rollout_scratch, sizeof(double)*(n ? n : 1)));
  }
  const size_t nB = (size_t)B, T = (size_t)nstep;
  const size_t nin[3] = {(size_t)m.nu, (size_t)m.nv, 6*(size_t)m.nbody};
  const size_t nstate = (size_t)m.nq + m.nv + m.na;
  RolloutCall call{};
  call.scratch = c->rollout_scratch;
  call.B = B;
  call.T = nstep;
  call.fwdinv_on = (flags & MJHIP_STEP_FWDINV) || (m.opt.enableflags & mjhipENBL_FWDINV);
  call.ctrl_mode = m.nu ? in->ctrl_mode : kRolloutAbsent;
  call.qfrc_mode = in->qfrc_applied_mode;
  call.xfrc_mode = in->xfrc_applied_mode;
  call.status = c->status;
  RolloutTemps tmp;
  int* dsteps = nullptr;
  if (dev) {
    if (!mirror_in) {
      call.qpos = in->qpos;
      call.qvel = in->qvel;
      call.act = m.na ? in->act : nullptr;
    }
    call.ctrl = in->ctrl;
    call.qfrc_applied = in->qfrc_applied;
    call.xfrc_applied = in->xfrc_applied;
    call.state = out->state;
    call.qacc = out->qacc;
    call.fwdinv = out->fwdinv;
    call.steps_done = steps_done;
  } else {
    auto up = [&](const mjtNum* src, size_t n) -> double* {
      double* p = tmp.get(n);
      if (p && hipMemcpyAsync(p, src, sizeof(double)*n, hipMemcpyHostToDevice, c->stream) !=
                   hipSuccess) {
        return nullptr;
      }
      return p;
    };
    bool ok = true;
    if (!mirror_in) {
      ok = ok && (call.qpos = up(in->qpos, nB*m.nq));
      ok = ok && (call.qvel = up(in->qvel, nB*m.nv));
      if (in->act && m.na) ok = ok && (call.act = up(in->act, nB*m.na));
    }
    const int cm[3] = {call.ctrl_mode, call.qfrc_mode, call.xfrc_mode};
    const double** dst[3] = {&call.ctrl, &call.qfrc_applied, &call.xfrc_applied};
    for (int k = 0; k < 3; k++) {
      if (cm[k] == kRolloutAbsent) continue;
      ok = ok && (*dst[k] = up(ptrs[k], nB*nin[k]*(cm[k] == kRolloutPerStep ? T : 1)));
    }
    if (out->state) ok = ok && (call.state = tmp.get(nB*T*nstate));
    if (out->qacc) ok = ok && (call.qacc = tmp.get(nB*T*m.nv));
    if (out->fwdinv) ok = ok && (call.fwdinv = tmp.get(nB*T));
    if (steps_done) ok = ok && (dsteps = (int*)tmp.get((nB + 1)/2));
    call.steps_done = dsteps;
    if (!ok) {
      set_error("mjhip_rolloutBatch: staging the host arrays on the device failed");
      return MJHIP_ERR_HIP;
    }
  }
  if (!call.fwdinv) call.fwdinv_on = 0;
  // measurement only (tools/rollout_bench.py, the byte-equality test): MJHIP_ROLLOUT_DIRECT=1
  // in the environment selects the per-lane row store instead of the LDS write-out
  const char* direct_env = getenv("MJHIP_ROLLOUT_DIRECT");
  if (mjhip_launchRollout(c->stream, c->dmodel, c->mirror, call, c->con_cap > 0,
                          direct_env && direct_env[0] == '1')) {
    set_error("mjhip_rolloutBatch: kernel launch failed");
    return MJHIP_ERR_HIP;
  }
  if (!dev) {
    if (out->state) {
      HIPCHECK(hipMemcpyAsync(out->state, call.state, sizeof(double)*nB*T*nstate,
                              hipMemcpyDeviceToHost, c->stream));
    }
    if (out->qacc) {
      HIPCHECK(hipMemcpyAsync(out->qacc, call.qacc, sizeof(double)*nB*T*m.nv,
                              hipMemcpyDeviceToHost, c->stream));
    }
    if (out->fwdinv) {
      HIPCHECK(hipMemcpyAsync(out->fwdinv, call.fwdinv, sizeof(double)*nB*T,
                              hipMemcpyDeviceToHost, c->stream));
    }
    if (steps_done) {
      HIPCHECK(hipMemcpyAsync(steps_done, dsteps, sizeof(int)*nB, hipMemcpyDeviceToHost,
                              c->stream));
    }
  }
  // host arrays: collect_status synchronizes the stream before the staging buffers go
  return collect_status(c, B, status, status || !dev);
}

MJHIP_API long mjhip_transitionFDSlots(const mjhipContext* c, int B, int want_A, int want_B,
                                       int flg_centered) {
  if (!c || B < 0) return -1;
  const long P = mjhip_transitionSlots(&c->hmodel, want_A, want_B, flg_centered);
  return 64L*((B + 63)/64)*(1 + P);
}

MJHIP_API int mjhip_transitionFDBatch(mjhipContext* c, int B, const mjhipTransitionIn* in,
                                      const mjhipTransitionOut* out, int flags, int* status) {
  if (!in || in->size < (int)sizeof(mjhipTransitionIn)) {
    set_error("mjhip_transitionFDBatch: mjhipTransitionIn is NULL or its size field (%d) is "
              "below %d", in ? in->size : 0, (int)sizeof(mjhipTransitionIn));
    return MJHIP_ERR_ARG;
  }
  if (!out || out->size < (int)sizeof(mjhipTransitionOut)) {
    set_error("mjhip_transitionFDBatch: mjhipTransitionOut is NULL or its size field (%d) is "
              "below %d", out ? out->size : 0, (int)sizeof(mjhipTransitionOut));
    return MJHIP_ERR_ARG;
  }
  if (out->C || out->D) {
    set_error("mjhip_transitionFDBatch: the sensor Jacobians C and D are not built (this path "
              "computes no sensors); pass NULL");
    return MJHIP_ERR_ARG;
  }
  if (!c) {
    if (mjhip_deviceCount() <= 0) {
      set_error("mjhip_transitionFDBatch: no HIP device (there is no CPU fallback)");
      return MJHIP_ERR_NO_DEVICE;
    }
    set_error("mjhip_transitionFDBatch: NULL context");
    return MJHIP_ERR_ARG;
  }
  if (B < 0 || !(in->eps > 0) || !in->qpos || !in->qvel) {
    set_error("mjhip_transitionFDBatch: bad argument (B %d, eps %g, qpos %p, qvel %p)", B,
              in->eps, (const void*)in->qpos, (const void*)in->qvel);
    return MJHIP_ERR_ARG;
  }
  const mjhipModel& m = c->hmodel;
  if (m.opt.integrator == mjhipINT_RK4) {
    set_error("mjhip_transitionFDBatch: RK4 integrator is not supported");
    return MJHIP_ERR_MODEL;
  }
  if (const char* why = actuation_unsupported(m)) {
    set_error("mjhip_transitionFDBatch: %s is not supported", why);
    return MJHIP_ERR_MODEL;
  }
  const int want_A = out->A != nullptr, want_B = out->B != nullptr && m.nu > 0;
  const int P = mjhip_transitionSlots(&m, want_A, want_B, in->flg_centered);
  const long nblk = (B + 63)/64, slots = 64*nblk*(1 + P);
  if (slots > c->capacity) {
    set_error("batch %d (%ld evaluation slots) exceeds context capacity %d", B, slots,
              c->capacity);
    return MJHIP_ERR_CAPACITY;
  }
  if (B == 0) return MJHIP_OK;
  HIPCHECK(hipSetDevice(c->device));
  if (!c->rollout_scratch) {
    const size_t n = (size_t)mjhip_rolloutScratchDoubles(&m) * c->capacity;
    HIPCHECK(hipMalloc((void**)&c->rollout_scratch, sizeof(double)*(n ? n : 1)));
  }
  const size_t nstate = (size_t)m.nq + m.nv + m.na, ndx = 2*(size_t)m.nv + m.na;
  const size_t ny = (size_t)slots*nstate;
  if (c->transition_y_n < ny) {
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(hipFree(c->transition_y));
    c->transition_y = nullptr;
    c->transition_y_n = 0;
    HIPCHECK(hipMalloc((void**)&c->transition_y, sizeof(double)*ny));
    c->transition_y_n = ny;
  }
  const bool dev = flags & MJHIP_FLAG_DEVICE_PTRS;
  const size_t nB = (size_t)B;
  TransitionCall call{};
  call.scratch = c->rollout_scratch;
  call.Y = c->transition_y;
  call.status = c->status;
  call.cstatus = P ? c->status + 64*nblk : nullptr;
  call.eps = in->eps;
  call.B = B;
  call.nblk = (int)nblk;
  call.centered = in->flg_centered != 0;
  call.want_A = want_A;
  call.want_B = want_B;
  RolloutTemps tmp;
  if (dev) {
    call.qpos = in->qpos;
    call.qvel = in->qvel;
    call.act = m.na ? in->act : nullptr;
    call.ctrl = m.nu ? in->ctrl : nullptr;
    call.qfrc_applied = in->qfrc_applied;
    call.xfrc_applied = in->xfrc_applied;
    call.A = out->A;
    call.Bm = want_B ? out->B : nullptr;
  } else {
    bool ok = true;
    auto up = [&](const mjtNum* src, size_t n) -> const double* {
      if (!src || !n) return nullptr;
      double* p = tmp.get(n);
      if (!p || hipMemcpyAsync(p, src, sizeof(double)*n, hipMemcpyHostToDevice, c->stream) !=
                    hipSuccess) {
        ok = false;
        return nullptr;
      }
      return p;
    };
    call.qpos = up(in->qpos, nB*m.nq);
    call.qvel = up(in->qvel, nB*m.nv);
    call.act = up(in->act, nB*m.na);
    call.ctrl = up(in->ctrl, nB*m.nu);
    call.qfrc_applied = up(in->qfrc_applied, nB*m.nv);
    call.xfrc_applied = up(in->xfrc_applied, nB*6*m.nbody);
    if (want_A) ok = (call.A = tmp.get(nB*ndx*ndx)) && ok;
    if (want_B) ok = (call.Bm = tmp.get(nB*ndx*m.nu)) && ok;
    if (!ok) {
      set_error("mjhip_transitionFDBatch: staging the host arrays on the device failed");
      return MJHIP_ERR_HIP;
    }
  }
  if (mjhip_launchTransition(c->stream, c->dmodel, c->mirror, call, P, c->con_cap > 0)) {
    set_error("mjhip_transitionFDBatch: kernel launch failed");
    return MJHIP_ERR_HIP;
  }
  if (!dev) {
    if (want_A) {
      HIPCHECK(hipMemcpyAsync(out->A, call.A, sizeof(double)*nB*ndx*ndx, hipMemcpyDeviceToHost,
                              c->stream));
    }
    if (want_B) {
      HIPCHECK(hipMemcpyAsync(out->B, call.Bm, sizeof(double)*nB*ndx*m.nu,
                              hipMemcpyDeviceToHost, c->stream));
    }
  }
  // host arrays: collect_status synchronizes the stream before the staging buffers go
  return collect_status(c, B, status, status || !dev);
}

// the part of mjhipSolveIn every caller has (solver and noslip_iterations came after it)
static constexpr int kSolveInMin = (int)offsetof(mjhipSolveIn, solver);

MJHIP_API int mjhip_forwardSolveCheck(const mjhipModel* m, const mjhipSolveIn* in,
                                      const mjhipSolveOut* out) {
  if (!in || in->size < kSolveInMin) {
    set_error("mjhip_forwardSolveBatch: mjhipSolveIn is NULL or its size field (%d) is below %d",
              in ? in->size : 0, kSolveInMin);
    return MJHIP_ERR_ARG;
  }
  if (!out || out->size < (int)sizeof(mjhipSolveOut)) {
    set_error("mjhip_forwardSolveBatch: mjhipSolveOut is NULL or its size field (%d) is below "
              "%d", out ? out->size : 0, (int)sizeof(mjhipSolveOut));
    return MJHIP_ERR_ARG;
  }
  if (in->iterations <= 0 || !(in->meaninertia > 0)) {
    set_error("mjhip_forwardSolveBatch: bad argument (iterations %d, meaninertia %g)",
              in->iterations, in->meaninertia);
    return MJHIP_ERR_ARG;
  }
  if (!m) return MJHIP_OK;
  const bool full = in->size >= (int)sizeof(mjhipSolveIn);
  const int solver = full ? in->solver : (int)mjhipSOL_NEWTON;
  const int noslip = full ? in->noslip_iterations : 0;
  const char* why = nullptr;
  if (m->opt.cone == mjhipCONE_ELLIPTIC) why = "the elliptic friction cone";
  else if (solver != mjhipSOL_NEWTON) why = "a solver other than Newton (CG, PGS)";
  else if (mjh_isSparse(m)) why = "a sparse constraint Jacobian";
  else if (noslip > 0) why = "the noslip pass (noslip_iterations > 0)";
  else why = actuation_unsupported(*m);
  if (why) {
    set_error("mjhip_forwardSolveBatch: %s is not supported", why);
    return MJHIP_ERR_MODEL;
  }
  return MJHIP_OK;
}

MJHIP_API int mjhip_forwardSolveBatch(mjhipContext* c, int B, const mjhipSolveIn* in,
                                      const mjhipSolveOut* out, int flags, int* status) {
  if (const int rc = mjhip_forwardSolveCheck(c ? &c->hmodel : nullptr, in, out)) return rc;
  if (!c) {
    if (mjhip_deviceCount() <= 0) {
      set_error("mjhip_forwardSolveBatch: no HIP device (there is no CPU fallback)");
      return MJHIP_ERR_NO_DEVICE;
    }
    set_error("mjhip_forwardSolveBatch: NULL context");
    return MJHIP_ERR_ARG;
  }
  const bool dev = flags & MJHIP_FLAG_DEVICE_PTRS;
  const bool mirror_in = flags & MJHIP_FLAG_MIRROR_INPUT;
  if (B < 0 || (!mirror_in && (!in->qpos || !in->qvel))) {
    set_error("mjhip_forwardSolveBatch: bad argument (B %d; qpos/qvel required without "
              "MJHIP_FLAG_MIRROR_INPUT)", B);
    return MJHIP_ERR_ARG;
  }
  if (B > c->capacity) {
    set_error("batch %d exceeds context capacity %d", B, c->capacity);
    return MJHIP_ERR_CAPACITY;
  }
  if (B == 0) return MJHIP_OK;
  const mjhipModel& m = c->hmodel;
  HIPCHECK(hipSetDevice(c->device));
  if (!c->solver_scratch) {
    const size_t n = (size_t)mjhip_solverScratchDoubles(&m, c->efc_cap) * c->capacity;
    HIPCHECK(hipMalloc((void**)&c->solver_scratch, sizeof(double)*(n ? n : 1)));
    HIPCHECK(hipMemsetAsync(c->solver_scratch, 0, sizeof(double)*(n ? n : 1), c->stream));
  }
  const size_t nB = (size_t)B;
  SolverCall call{};
  call.scratch = c->solver_scratch;
  call.status = c->status;
  call.tolerance = in->tolerance;
  call.ls_tolerance = in->ls_tolerance;
  call.meaninertia = in->meaninertia;
  call.iterations = in->iterations;
  call.ls_iterations = in->ls_iterations;
  call.B = B;
  RolloutTemps tmp;
  int* dniter = nullptr;
  if (dev) {
    if (!mirror_in) {
      call.qpos = in->qpos;
      call.qvel = in->qvel;
      call.ctrl = m.nu ? in->ctrl : nullptr;
      call.act = m.na ? in->act : nullptr;
    }
    call.qacc_warmstart = in->qacc_warmstart;
    call.qacc = out->qacc;
    call.qfrc_constraint = out->qfrc_constraint;
    call.act_dot = m.na ? out->act_dot : nullptr;
    call.act_next = m.na ? out->act_next : nullptr;
  } else {
    bool ok = true;
    auto up = [&](const mjtNum* src, size_t n) -> const double* {
      if (!src || !n) return nullptr;
      double* p = tmp.get(n);
      if (!p || hipMemcpyAsync(p, src, sizeof(double)*n, hipMemcpyHostToDevice, c->stream) !=
                    hipSuccess) {
        ok = false;
        return nullptr;
      }
      return p;
    };
    auto down = [&](const mjtNum* dst, size_t n) -> double* {
      if (!dst || !n) return nullptr;
      double* p = tmp.get(n);
      if (!p) ok = false;
      return p;
    };
    if (!mirror_in) {
      call.qpos = up(in->qpos, nB*m.nq);
      call.qvel = up(in->qvel, nB*m.nv);
      call.ctrl = up(in->ctrl, nB*m.nu);
      call.act = up(in->act, nB*m.na);
    }
    call.qacc_warmstart = up(in->qacc_warmstart, nB*m.nv);
    call.qacc = down(out->qacc, nB*m.nv);
    call.qfrc_constraint = down(out->qfrc_constraint, nB*m.nv);
    call.act_dot = down(out->act_dot, nB*m.na);
    call.act_next = down(out->act_next, nB*m.na);
    if (!ok) {
      set_error("mjhip_forwardSolveBatch: staging the host arrays on the device failed");
      return MJHIP_ERR_HIP;
    }
  }
  if (out->niter) {                         // a host array in either mode, as status is
    dniter = (int*)tmp.get((nB + 1)/2);
    if (!dniter) {
      set_error("mjhip_forwardSolveBatch: staging niter on the device failed");
      return MJHIP_ERR_HIP;
    }
    call.niter = dniter;
  }
  if (mjhip_launchForwardSolve(c->stream, c->dmodel, c->mirror, call, c->con_cap > 0)) {
    set_error("mjhip_forwardSolveBatch: kernel launch failed");
    return MJHIP_ERR_HIP;
  }
  if (!dev) {
    auto get = [&](mjtNum* dst, const double* src, size_t n) {
      return !dst || !src || !n ||
             hipMemcpyAsync(dst, src, sizeof(double)*n, hipMemcpyDeviceToHost, c->stream) ==
                 hipSuccess;
    };
    bool ok = get(out->qacc, call.qacc, nB*m.nv);
    ok = get(out->qfrc_constraint, call.qfrc_constraint, nB*m.nv) && ok;
    ok = get(out->act_dot, call.act_dot, nB*m.na) && ok;
    ok = get(out->act_next, call.act_next, nB*m.na) && ok;
    if (!ok) {
      set_error("mjhip_forwardSolveBatch: copying the results to the host failed");
      return MJHIP_ERR_HIP;
    }
  }
  if (dniter) {
    HIPCHECK(hipMemcpyAsync(out->niter, dniter, sizeof(int)*nB, hipMemcpyDeviceToHost,
                            c->stream));
  }
  // host arrays and niter: collect_status synchronizes the stream before the staging buffers go
  return collect_status(c, B, status, status || !dev || dniter);
}

MJHIP_API int mjhip_actuationBatch(mjhipContext* c, int B, const mjtNum* ctrl,
                                   const mjtNum* act, mjtNum* act_dot, mjtNum* act_next,
                                   mjtNum* qfrc_actuator, int flags, int* status) {
  if (!c || B < 0) {
    set_error("mjhip_actuationBatch: bad argument");
    return MJHIP_ERR_ARG;
  }
  if (B > c->capacity) {
    set_error("batch %d exceeds context capacity %d", B, c->capacity);
    return MJHIP_ERR_CAPACITY;
  }
  const mjhipModel& m = c->hmodel;
  if (const char* why = actuation_unsupported(m)) {
    set_error("mjhip_actuationBatch: %s is not supported", why);
    return MJHIP_ERR_MODEL;
  }
  if (B == 0) return MJHIP_OK;
  HIPCHECK(hipSetDevice(c->device));
  const bool dev = flags & MJHIP_FLAG_DEVICE_PTRS;
  const StageAct sx = stage_act(c);
  double* sf = c->stage + (size_t)c->capacity*(m.nq + 2*(size_t)m.nv);   // the qfrc slice
  const double* dc = (ctrl && m.nu) ? ctrl : nullptr;
  const double* dact = (act && m.na) ? act : nullptr;
  if (!dev) {
    if (dc) {
      HIPCHECK(hipMemcpyAsync(sx.ctrl, ctrl, sizeof(double)*(size_t)B*m.nu,
                              hipMemcpyHostToDevice, c->stream));
      dc = sx.ctrl;
    }
    if (dact) {
      HIPCHECK(hipMemcpyAsync(sx.act, act, sizeof(double)*(size_t)B*m.na, hipMemcpyHostToDevice,
                              c->stream));
      dact = sx.act;
    }
  }
  double* ddot = (act_dot && m.na) ? (dev ? act_dot : sx.act_dot) : nullptr;
  double* dnext = (act_next && m.na) ? (dev ? act_next : sx.act_next) : nullptr;
  double* dqf = qfrc_actuator ? (dev ? qfrc_actuator : sf) : nullptr;
  hipLaunchKernelGGL(k_actuation, dim3((B + 63) / 64), dim3(64), 0, c->stream, c->dmodel,
                     c->mirror, B, dc, dact, ddot, dnext, dqf, c->status);
  HIPCHECK(hipGetLastError());
  if (!dev) {
    if (ddot) {
      HIPCHECK(hipMemcpyAsync(act_dot, ddot, sizeof(double)*(size_t)B*m.na,
                              hipMemcpyDeviceToHost, c->stream));
    }
    if (dnext) {
      HIPCHECK(hipMemcpyAsync(act_next, dnext, sizeof(double)*(size_t)B*m.na,
                              hipMemcpyDeviceToHost, c->stream));
    }
    if (dqf) {
      HIPCHECK(hipMemcpyAsync(qfrc_actuator, dqf, sizeof(double)*(size_t)B*m.nv,
                              hipMemcpyDeviceToHost, c->stream));
    }
  }
  return collect_status(c, B, status, status || !dev);
}

MJHIP_API int mjhip_statusDownload(mjhipContext* c, int first, int count, int* dst) {
  if (!c || first < 0 || count < 0 || first + count > c->capacity || !dst) return MJHIP_ERR_ARG;
  HIPCHECK(hipSetDevice(c->device));
  HIPCHECK(hipMemcpyAsync(dst, c->status + first, sizeof(int)*(size_t)count,
                          hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return MJHIP_OK;
}

// element k of instance i (counted from the first fetched block) of an S-element field at
// tmp[base + k*step]: lane-interleaved (F[(blk*S + k)*64 + lane]) or instance-contiguous
// (F[(blk*64 + lane)*S + k], the XSCC / XSIC fields)
static void blockIndex(int i, int S, bool contig, size_t* base, size_t* step) {
  if (contig) {
    *base = (size_t)i * S;
    *step = 1;
  } else {
    *base = (size_t)(i / 64) * S * 64 + (i & 63);
    *step = 64;
  }
}

static int find_field(mjhipContext* c, const char* field, double** ptr, int* S) {
  auto it = c->fields.find(field);
  if (it == c->fields.end()) {
    set_error("unknown mirror field '%s'", field);
    return MJHIP_ERR_ARG;
  }
  *ptr = it->second.first;
  *S = it->second.second;
  return MJHIP_OK;
}

MJHIP_API void* mjhip_mirrorDevicePtr(mjhipContext* c, const char* field) {
  double* p;
  int S;
  if (!c || find_field(c, field, &p, &S)) return nullptr;
  return p;
}

// int scratch fields (constraint row types/ids/states, counts, contact geoms/dims), one
// instance-major row of `S` ints per instance
MJHIP_API int mjhip_mirrorDownloadInt(mjhipContext* c, const char* field, int first, int count,
                                      int* dst) {
  if (!c || !field || !dst || first < 0 || count < 0 || first + count > c->capacity) {
    return MJHIP_ERR_ARG;
  }
  auto it = c->ifields.find(field);
  if (it == c->ifields.end()) {
    set_error("unknown int mirror field '%s'", field);
    return MJHIP_ERR_ARG;
  }
  int* p = it->second.first;
  int S = it->second.second;
  if (!count || !S) return MJHIP_OK;
  HIPCHECK(hipSetDevice(c->device));
  int b0 = first / 64, b1 = (first + count + 63) / 64;
  std::vector<int> tmp((size_t)(b1 - b0) * S * 64);
  HIPCHECK(hipMemcpyAsync(tmp.data(), p + (size_t)b0*S*64, tmp.size()*sizeof(int),
                          hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  const bool ct = c->contig.count(field) > 0;
  for (int i = 0; i < count; i++) {
    int inst = first + i;
    size_t base, step;
    blockIndex(inst - b0*64, S, ct, &base, &step);
    for (int k = 0; k < S; k++) dst[(size_t)i*S + k] = tmp[base + (size_t)k*step];
  }
  return MJHIP_OK;
}

MJHIP_API int mjhip_mirrorFieldSize(const mjhipContext* c, const char* field) {
  if (!c || !field) return -1;
  auto it = c->fields.find(field);
  return it == c->fields.end() ? -1 : it->second.second;
}

MJHIP_API int mjhip_fieldSizeInt(const mjhipContext* c, const char* field) {
  if (!c || !field) return -1;
  auto it = c->ifields.find(field);
  return it == c->ifields.end() ? -1 : it->second.second;
}

// host transfers of whole 64-instance blocks, reordered on the host
MJHIP_API int mjhip_mirrorDownload(mjhipContext* c, const char* field, int first, int count,
                                   mjtNum* dst) {
  double* p;
  int S;
  if (!c || !dst || first < 0 || count < 0 || first + count > c->capacity) return MJHIP_ERR_ARG;
  if (int rc = find_field(c, field, &p, &S)) return rc;
  if (!count || !S) return MJHIP_OK;
  HIPCHECK(hipSetDevice(c->device));
  int b0 = first / 64, b1 = (first + count + 63) / 64;
  std::vector<double> tmp((size_t)(b1 - b0) * S * 64);
  HIPCHECK(hipMemcpyAsync(tmp.data(), p + (size_t)b0*S*64, tmp.size()*sizeof(double),
                          hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  const bool ct = c->contig.count(field) > 0;
  for (int i = 0; i < count; i++) {
    int inst = first + i;
    size_t base, step;
    blockIndex(inst - b0*64, S, ct, &base, &step);
    for (int k = 0; k < S; k++) dst[(size_t)i*S + k] = tmp[base + (size_t)k*step];
  }
  return MJHIP_OK;
}

MJHIP_API int mjhip_mirrorUpload(mjhipContext* c, const char* field, int first, int count,
                                 const mjtNum* src) {
  double* p;
  int S;
  if (!c || !src || first < 0 || count < 0 || first + count > c->capacity) return MJHIP_ERR_ARG;
  if (int rc = find_field(c, field, &p, &S)) return rc;
  if (!count || !S) return MJHIP_OK;
  HIPCHECK(hipSetDevice(c->device));
  int b0 = first / 64, b1 = (first + count + 63) / 64;
  std::vector<double> tmp((size_t)(b1 - b0) * S * 64);
  HIPCHECK(hipMemcpyAsync(tmp.data(), p + (size_t)b0*S*64, tmp.size()*sizeof(double),
                          hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  const bool ct = c->contig.count(field) > 0;
  for (int i = 0; i < count; i++) {
    int inst = first + i;
    size_t base, step;
    blockIndex(inst - b0*64, S, ct, &base, &step);
    for (int k = 0; k < S; k++) tmp[base + (size_t)k*step] = src[(size_t)i*S + k];
  }
  c->const_stale = true;                 // the rows may cover slots only k_const writes
  HIPCHECK(hipMemcpyAsync(p + (size_t)b0*S*64, tmp.data(), tmp.size()*sizeof(double),
                          hipMemcpyHostToDevice, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return MJHIP_OK;
}

MJHIP_API int mjhip_timeInverseKernel(mjhipContext* c, int B, int reps, int skipstage,
                                      int flags, float* ms) {
  if (!c || B <= 0 || B > c->capacity || reps <= 0 || !ms) return MJHIP_ERR_ARG;
  HIPCHECK(hipSetDevice(c->device));
  HIPCHECK(hipEventRecord(c->ev0, c->stream));
  for (int r = 0; r < reps; r++) {
    int rc = launch_inverse(c, B, nullptr, nullptr, nullptr, nullptr, skipstage, nullptr,
                            flags);
    if (rc) return rc;
  }
  HIPCHECK(hipEventRecord(c->ev1, c->stream));
  HIPCHECK(hipEventSynchronize(c->ev1));
  float t = 0;
  HIPCHECK(hipEventElapsedTime(&t, c->ev0, c->ev1));
  *ms = t / reps;
  return MJHIP_OK;
}

MJHIP_API int mjhip_inverseFDBatchAct(mjhipContext* c, int B, const mjtNum* qpos,
                                      const mjtNum* qvel, const mjtNum* qacc, const mjtNum* ctrl,
                                      const mjtNum* act, mjtNum eps, int flg_actuation,
                                      mjtNum* DfDq, mjtNum* DfDv, mjtNum* DfDa, mjtNum* DsDq,
                                      mjtNum* DsDv, mjtNum* DsDa, mjtNum* DmDq, int flags) {
  if (!c || B <= 0 || !qpos || !qvel || !qacc || (flg_actuation && c->hmodel.nu && !ctrl) ||
      (flg_actuation && c->hmodel.na && !act)) {
    set_error("mjhip_inverseFDBatch: bad argument");
    return MJHIP_ERR_ARG;
  }
  const mjhipModel& m = c->hmodel;
  const int nv = m.nv, P = 3*nv + 1;
  if (m.opt.integrator == mjhipINT_RK4) {       // engine_derivative_fd.c:619-621
    set_error("mjd_inverseFD: RK4 integrator is not supported");
    return MJHIP_ERR_MODEL;
  }
  if (m.nmocap) {
    set_error("mjhip_inverseFDBatch: mocap poses per base state are not an input of the "
              "batched FD API");
    return MJHIP_ERR_MODEL;
  }
  if (flg_actuation) {
    if (const char* why = actuation_unsupported(m)) {
      set_error("mjhip_inverseFDBatch(flg_actuation): %s is not supported", why);
      return MJHIP_ERR_MODEL;
    }
  }
  if ((long)B*P > c->capacity) {
    set_error("FD batch needs %ld instances, context capacity %d", (long)B*P, c->capacity);
    return MJHIP_ERR_CAPACITY;
  }
  HIPCHECK(hipSetDevice(c->device));
  const bool dev = flags & MJHIP_FLAG_DEVICE_PTRS;
  const double *dq = qpos, *dv = qvel, *da = qacc, *dc = flg_actuation ? ctrl : nullptr;
  // given activations reach every evaluation, with or without flg_actuation: the implicit
  // mj_discreteAcc of an mjENBL_INVDISCRETE model reads them too (mjd_actuator_vel)
  const double* dact = m.na ? act : nullptr;
  // per-call device buffers of the host-array form (ctrl, the Jacobians); freed on every
  // return path, after the stream has finished with them (the device-pointer form has none
  // and returns without waiting for the device)
  struct Scratch {
    mjhipContext* c;
    std::vector<double*> p;
    ~Scratch() {
      if (p.empty()) return;
      hipStreamSynchronize(c->stream);
      for (double* d : p) hipFree(d);
    }
    double* alloc(size_t n) {
      double* d = nullptr;
      if (hipMalloc((void**)&d, (n ? n : 1)*sizeof(double)) != hipSuccess) return nullptr;
      p.push_back(d);
      return d;
    }
  } tmp{c, {}};
#define FDCHECK(expr, what)                                                                   \
  do {                                                                                        \
    if ((expr) != hipSuccess) {                                                               \
      set_error("mjhip_inverseFDBatch: %s failed", what);                                    \
      return MJHIP_ERR_HIP;                                                                   \
    }                                                                                         \
  } while (0)
  if (!dev) {
    double* sq = c->stage;
    double* sv = sq + (size_t)c->capacity*m.nq;
    double* sa = sv + (size_t)c->capacity*m.nv;
    FDCHECK(hipMemcpyAsync(sq, qpos, sizeof(double)*(size_t)B*m.nq, hipMemcpyHostToDevice,
                           c->stream), "qpos upload");
    FDCHECK(hipMemcpyAsync(sv, qvel, sizeof(double)*(size_t)B*nv, hipMemcpyHostToDevice,
                           c->stream), "qvel upload");
    FDCHECK(hipMemcpyAsync(sa, qacc, sizeof(double)*(size_t)B*nv, hipMemcpyHostToDevice,
                           c->stream), "qacc upload");
    dq = sq; dv = sv; da = sa;
    if (dc && m.nu) {
      double* sc = tmp.alloc((size_t)B*m.nu);
      if (!sc) { set_error("hipMalloc(ctrl) failed"); return MJHIP_ERR_HIP; }
      FDCHECK(hipMemcpyAsync(sc, ctrl, sizeof(double)*(size_t)B*m.nu, hipMemcpyHostToDevice,
                             c->stream), "ctrl upload");
      dc = sc;
    }
    if (dact) {
      double* sact = tmp.alloc((size_t)B*m.na);
      if (!sact) { set_error("hipMalloc(act) failed"); return MJHIP_ERR_HIP; }
      FDCHECK(hipMemcpyAsync(sact, act, sizeof(double)*(size_t)B*m.na, hipMemcpyHostToDevice,
                             c->stream), "act upload");
      dact = sact;
    }
  }
  long ninst = (long)B*P;
  // sensors are skipped when no sensor derivative is asked for (derivative_fd.c:628)
  const int skipsensor = !DsDq && !DsDv && !DsDa;
  // Stage skipping after the reference's loop (engine_derivative_fd.c:646-699, which runs the
  // qvel perturbations through mj_inverseSkip(mjSTAGE_POS) and the qacc ones through
  // mjSTAGE_VEL): layout 1 runs both kinds on the generated va stage alone, over their
  // centre's position-stage outputs (k_vaskip). The skipped stages would see unchanged inputs,
  // so the operations are the full pipeline's; the perturbed instances' bodies leave out the
  // stores nobody reads (codegen.FD_KEEP), which lets the compiler contract a multiply-add
  // differently, so a term of qfrc_inverse can round differently by a few ulp (held to 16 ulp
  // of the largest |qfrc_inverse| over eps, test_inverse_fd_stage_skip_bit_exact). Taken only
  // where the straight-line kernel is the whole pipeline (no post passes, sensors or
  // actuation terms) and the position-stage block ends on a wave boundary.
  const long nA = (long)B*(nv + 1);
  const char* noskip = getenv("MJHIP_FD_NOSKIP");
  const int layout = c->fast && c->fast->launch_vaskip && !(flags & MJHIP_FLAG_GENERIC) &&
                     skipsensor && !flg_actuation && !c->spatial &&
                     !mjh::hasFluid(c->hmodel) && !mjh::hasDiscrete(c->hmodel) &&
                     !mjh_needTrnAfter(&c->hmodel) &&
                     !(m.opt.enableflags & mjhipENBL_ENERGY) && nA % 64 == 0 &&
                     !(noskip && noskip[0] == '1') && !(flags & kFlagFDFull);
  int rc = MJHIP_OK;
  // the skip layout's perturbed instances store only what a later kernel of this call reads
  // (codegen.FD_KEEP): instance blocks past the centres' drop the rest, as the launches below
  // see through the mirror; restored on every return path
  struct ElideGuard {
    Mirror* mr;
    ~ElideGuard() { mr->fd_elide = 0; mr->full_blk = 0; }
  } elide_guard{&c->mirror};
  if (layout) {
    c->mirror.fd_elide = 1;
    c->mirror.full_blk = (B + 63) / 64;
    // k_vaskip runs a generated stage body too
    if (const int rc2 = ensure_const(c)) return rc2;
  }
  // with the skip layout only the position-stage block is expanded: k_vaskip reads its
  // centre's inputs and perturbs them in registers (the fall-back expands the rest, below)
  const long nexp = layout ? nA : ninst;
  hipLaunchKernelGGL(k_fd_expand, dim3((unsigned)((nexp + 63)/64)), dim3(64*kExpandWaves), 0,
                     c->stream, c->dmodel, c->mirror, B, dq, dv, da, (m.nu ? dc : nullptr),
                     dact, eps, layout, layout ? c->fdflag : nullptr, (long)0, nexp, 0);
  FDCHECK(hipGetLastError(), "k_fd_expand launch");
  if (layout) {
    // the nv+1 position-stage instances of every base state: the full pipeline (a work-list
    // model's rows are served once, after the fall-back below has added its own)
    const bool defer = c->fast->cmode == 1 && c->fast->launch;
    rc = launch_inverse(c, (int)nA, nullptr, nullptr, nullptr, nullptr, mjhipSTAGE_NONE,
                        nullptr, defer ? kFlagDeferRows : 0, skipsensor);
    if (rc) return rc;
    // the 2nv qvel/qacc perturbations: the va stage over their centre's position stage
    c->fast->launch_vaskip(c->stream, c->mirror, (int)ninst, (int)nA, 2*nv, 1,
                           c->mirror.efc_count, c->fdflag, eps);
    FDCHECK(hipGetLastError(), "k_vaskip launch");
    if (c->fast->cmode == 1) {
      // a work-list model whose centre has limit rows: its perturbations need the rows'
      // velocity and acceleration terms, so every qvel/qacc perturbation then runs the full
      // pipeline over its own slot (the same layout; results as without skipping). Decided on
      // the device: the gated expansion below turns the flag into the range k_all reads,
      // empty when no centre has rows, so the call needs no host round trip.
      // the perturbations' own inputs, for the full pipeline over them (only when a centre
      // has rows)
      // gated: usually empty, so a few one-wave blocks striding over the range (an empty
      // launch of one 16-wave block per 64 instances took 5 us)
      const long gblk = (ninst - nA + 63)/64;
      hipLaunchKernelGGL(k_fd_expand, dim3((unsigned)(gblk < 256 ? gblk : 256)), dim3(64), 0,
                         c->stream, c->dmodel, c->mirror, B, dq, dv, da,
                         (m.nu ? dc : nullptr), dact, eps, layout, c->fdflag, nA, ninst, 1);
      FDCHECK(hipGetLastError(), "k_fd_expand (fall-back) launch");
      rc = launch_inverse(c, (int)(ninst - nA), nullptr, nullptr, nullptr, nullptr,
                          mjhipSTAGE_NONE, nullptr, 0, skipsensor, c->fdflag + 1);
      if (rc) return rc;
    }
  } else {
    rc = launch_inverse(c, (int)ninst, nullptr, nullptr, nullptr, nullptr, mjhipSTAGE_NONE,
                        nullptr, 0, skipsensor);
    if (rc) return rc;
  }
  if (flg_actuation) {
    hipLaunchKernelGGL(k_fd_act, dim3((ninst + 255)/256), dim3(256), 0, c->stream, c->dmodel,
                       c->mirror, ninst);
    FDCHECK(hipGetLastError(), "k_fd_act launch");
  }
  double *oq = DfDq, *ov = DfDv, *oa = DfDa, *om = DmDq;
  double *sq_ = DsDq, *sv_ = DsDv, *sa_ = DsDa;
  size_t nn = (size_t)B*nv*nv, nm = (size_t)B*nv*m.nM, ns = (size_t)B*nv*m.nsensordata;
  if (!dev) {
    bool ok = true;
    auto dalloc = [&](double* h, size_t n) -> double* {
      if (!h) return nullptr;
      double* d = tmp.alloc(n);
      ok = ok && d;
      return d;
    };
    oq = dalloc(DfDq, nn); ov = dalloc(DfDv, nn); oa = dalloc(DfDa, nn); om = dalloc(DmDq, nm);
    sq_ = dalloc(DsDq, ns); sv_ = dalloc(DsDv, ns); sa_ = dalloc(DsDa, ns);
    if (!ok) {
      set_error("hipMalloc(FD outputs) failed");
      return MJHIP_ERR_HIP;
    }
  }
  long nd = (long)B*(P-1);
  if (oq || ov || oa) {
    hipLaunchKernelGGL(k_fd_dfd, dim3((nd*nv + 255)/256), dim3(256), 0, c->stream, c->dmodel,
                       c->mirror, B, eps, flg_actuation, oq, ov, oa, layout);
  }
  if (sq_ || sv_ || sa_ || om) {
    hipLaunchKernelGGL(k_fd_diff, dim3((nd + 255)/256), dim3(256), 0, c->stream, c->dmodel,
                       c->mirror, B, eps, flg_actuation, nullptr, nullptr, nullptr, sq_, sv_,
                       sa_, om, layout);
  }
  FDCHECK(hipGetLastError(), "k_fd_diff launch");
  if (!dev) {
    auto get = [&](double* h, const double* d, size_t n) {
      return !h || hipMemcpyAsync(h, d, n*8, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    };
    bool ok = get(DfDq, oq, nn) && get(DfDv, ov, nn) && get(DfDa, oa, nn) && get(DmDq, om, nm) &&
              get(DsDq, sq_, ns) && get(DsDv, sv_, ns) && get(DsDa, sa_, ns);
    FDCHECK(ok ? hipStreamSynchronize(c->stream) : hipErrorUnknown, "FD output download");
  }
#undef FDCHECK
  return MJHIP_OK;
}

MJHIP_API int mjhip_inverseFDBatchEx(mjhipContext* c, int B, const mjtNum* qpos,
                                     const mjtNum* qvel, const mjtNum* qacc, const mjtNum* ctrl,
                                     mjtNum eps, int flg_actuation, mjtNum* DfDq, mjtNum* DfDv,
                                     mjtNum* DfDa, mjtNum* DsDq, mjtNum* DsDv, mjtNum* DsDa,
                                     mjtNum* DmDq, int flags) {
  if (c && flg_actuation) {
    if (const char* why = actuation_stateless(c->hmodel)) {
      set_error("mjhip_inverseFDBatch(flg_actuation): %s is not supported "
                "(mjhip_inverseFDBatchAct takes act)", why);
      return MJHIP_ERR_MODEL;
    }
  }
  return mjhip_inverseFDBatchAct(c, B, qpos, qvel, qacc, ctrl, nullptr, eps, flg_actuation,
                                 DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, DmDq, flags);
}

MJHIP_API int mjhip_inverseFDBatch(mjhipContext* c, int B, const mjtNum* qpos,
                                   const mjtNum* qvel, const mjtNum* qacc, mjtNum eps,
                                   mjtNum* DfDq, mjtNum* DfDv, mjtNum* DfDa, mjtNum* DsDq,
                                   mjtNum* DsDv, mjtNum* DsDa, mjtNum* DmDq, int flags) {
  return mjhip_inverseFDBatchEx(c, B, qpos, qvel, qacc, nullptr, eps, 0, DfDq, DfDv, DfDa,
                                DsDq, DsDv, DsDa, DmDq, flags);
}

//---------------------------------- single-instance drop-in ---------------------------------
// The reference's single-mjData entry points run as a batch of one on instance 0 of a
// per-model context: the fields a call reads are uploaded from the host mjhipData, one kernel
// runs the stages the reference function runs, and the fields it writes come back.

MJHIP_API int mjhip_modelCapacity(const mjhipModel* m, int* efc_rows, int* contacts) {
  if (!m) return MJHIP_ERR_ARG;
  if (efc_rows) *efc_rows = mjhip_efcCapacity(m);
  if (contacts) *contacts = mjhip_contactCapacity(m, nullptr);
  return MJHIP_OK;
}

// one stage of mj_inverseSkip (or a helper it calls) on instance 0 (the reference function
// is named in the comment); lane 0 of one 64-lane block runs it. ST_INV is the whole
// mj_inverseSkip on the unfused path, which leaves every constraint row in the mirror.
extern "C++" {
enum { ST_INV = 0, ST_POS, ST_VEL, ST_CON, ST_RNE0, ST_RNE1, ST_XFRC };
template <bool CONTACT>
__global__ __launch_bounds__(64) void k_stage(mjhipModel m, Mirror mr, int what, int skipstage,
                                              int skipsensor, int* __restrict__ status) {
  if (threadIdx.x) return;
  Lane<64> d = lane_view(mr, 0, 0);
  int st = 0;
  switch (what) {
    case ST_INV: st = mjh::inverseSkip<64, CONTACT, false>(m, d, skipstage, skipsensor); break;
    case ST_POS: mjh::invPosition<64, CONTACT, false>(m, d, &st); break;   // mj_invPosition
    case ST_VEL: mjh::invVelocity<64, false>(m, d); break;                 // mj_invVelocity
    case ST_CON: mjh::invConstraint(m, d); break;                          // mj_invConstraint
    case ST_RNE0: mjh::rne(m, d, 0, d.qfrc_tmp); break;                    // mj_rne(flg_acc=0)
    case ST_RNE1: mjh::rne(m, d, 1, d.qfrc_tmp); break;                    // mj_rne(flg_acc=1)
    case ST_XFRC: mjh::xfrcAccumulate(m, d, d.qfrc_tmp); break;            // mj_xfrcAccumulate
  }
  if (status) status[0] = st;
}
}  // extern "C++"

static int g_device = 0;
static std::mutex g_mu;
// contexts of the single-instance calls, keyed by the model's content signature (sizes,
// options, every array): a new or edited model at a reused address gets its own context.
// A call leases its entry for its whole upload/launch/download sequence: the lease holds a
// reference (an entry evicted or released meanwhile is freed when its last lease ends) and
// the entry's call lock (the calls share instance 0 and the stream of the context).
struct CtxEntry {
  unsigned long long sig = 0;
  mjhipContext* c = nullptr;
  std::mutex call_mu;
  ~CtxEntry() { if (c) mjhip_contextFree(c); }
};
using CtxRef = std::shared_ptr<CtxEntry>;
// most recently used last, at most kMaxCtx; never destroyed (contexts are not freed during
// static destruction, after the HIP runtime may have gone)
static std::vector<CtxRef>& g_ctx = *new std::vector<CtxRef>;
static const size_t kMaxCtx = 16;
// mjhip_inverseFD's context (capacity 3nv+1) is cached under the signature with this salt
static const unsigned long long kFDSalt = 0x9E3779B97F4A7C15ull;

struct CtxLease {
  CtxRef e;
  std::unique_lock<std::mutex> lk;
  mjhipContext* get() const { return e ? e->c : nullptr; }
};

static CtxLease lease_ctx(const mjhipModel* m, unsigned long long salt, int capacity) {
  const unsigned long long sig = model_signature(m) ^ salt;
  CtxRef e;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    for (size_t i = 0; i < g_ctx.size(); i++) {
      if (g_ctx[i]->sig == sig) {
        e = g_ctx[i];
        g_ctx.erase(g_ctx.begin() + i);
        g_ctx.push_back(e);
        break;
      }
    }
    if (!e) {
      mjhipContext* c = nullptr;
      if (mjhip_contextCreate(m, g_device, capacity, &c) != MJHIP_OK) return {};
      e = std::make_shared<CtxEntry>();
      e->sig = sig;
      e->c = c;
      if (g_ctx.size() >= kMaxCtx) g_ctx.erase(g_ctx.begin());   // least recently used
      g_ctx.push_back(e);
    }
  }
  CtxLease L;
  L.e = e;
  L.lk = std::unique_lock<std::mutex>(e->call_mu);
  return L;
}

static void report(const char* what) {
  std::string msg = std::string(what) + ": " + g_last_error;
  if (g_error_cb) {
    g_error_cb(msg.c_str());
  } else {
    fprintf(stderr, "mjhip error: %s\n", msg.c_str());
  }
}

MJHIP_API void mjhip_setDevice(int device) { g_device = device; }

MJHIP_API void mjhip_releaseModel(const mjhipModel* m) {
  const unsigned long long sig = model_signature(m);
  std::lock_guard<std::mutex> lk(g_mu);
  for (size_t i = g_ctx.size(); i-- > 0;) {
    if (g_ctx[i]->sig == sig || g_ctx[i]->sig == (sig ^ kFDSalt)) g_ctx.erase(g_ctx.begin() + i);
  }
}

extern "C++" {
// instance 0 of a mirror field: element k at F[k*64] (block 0, lane 0), or at F[k] for an
// instance-contiguous field (the XSCC / XSIC fields)
template <class T>
static int put0(mjhipContext* c, T* dev, const T* host, long n) {
  if (n <= 0 || !dev || !host) return MJHIP_OK;
  if (c->contig_ptr.count((const void*)dev)) {
    HIPCHECK(hipMemcpyAsync(dev, host, sizeof(T)*n, hipMemcpyHostToDevice, c->stream));
    return MJHIP_OK;
  }
  HIPCHECK(hipMemcpy2DAsync(dev, 64*sizeof(T), host, sizeof(T), sizeof(T), n,
                            hipMemcpyHostToDevice, c->stream));
  return MJHIP_OK;
}

template <class T>
static int get0(mjhipContext* c, T* host, const T* dev, long n) {
  if (n <= 0 || !dev || !host) return MJHIP_OK;
  if (c->contig_ptr.count((const void*)dev)) {
    HIPCHECK(hipMemcpyAsync(host, dev, sizeof(T)*n, hipMemcpyDeviceToHost, c->stream));
    return MJHIP_OK;
  }
  HIPCHECK(hipMemcpy2DAsync(host, sizeof(T), dev, 64*sizeof(T), sizeof(T), n,
                            hipMemcpyDeviceToHost, c->stream));
  return MJHIP_OK;
}
}  // extern "C++"

// data fields of stages lo..hi (MJHIP_DATA_FIELDS stage numbers) host -> instance 0
static int put_stages(mjhipContext* c, const mjhipModel* m, const mjhipData* d, int lo, int hi) {
  int rc = 0;
#define MJ_M(n) m->n
#define XD(name, d0, d1, stage)                                                          \
  if (!rc && stage >= lo && stage <= hi) rc = put0(c, c->mirror.name, (const double*)d->name, \
                                                   (long)(m->d0) * (d1));
  MJHIP_DATA_FIELDS
#undef XD
#undef MJ_M
  return rc;
}

static int get_stages(mjhipContext* c, const mjhipModel* m, mjhipData* d, int lo, int hi) {
  int rc = 0;
#define MJ_M(n) m->n
#define XD(name, d0, d1, stage)                                                          \
  if (!rc && stage >= lo && stage <= hi) rc = get0(c, d->name, (const double*)c->mirror.name, \
                                                   (long)(m->d0) * (d1));
  MJHIP_DATA_FIELDS
#undef XD
#undef MJ_M
  return rc;
}

// constraint rows (XE) and contacts (XC) written by stages lo..hi, host -> instance 0, with
// the counts. Rows beyond the context's capacity cannot come from a supported model.
static int put_rows(mjhipContext* c, const mjhipModel* m, const mjhipData* d, int lo, int hi) {
  if (d->nefc > c->efc_cap || d->ncon > c->con_cap || d->nefc < 0 || d->ncon < 0) {
    set_error("%d constraint rows / %d contacts exceed the model's device capacity (%d / %d)",
              d->nefc, d->ncon, c->efc_cap, c->con_cap);
    return MJHIP_ERR_CAPACITY;
  }
  if ((d->nefc && d->efc_capacity < d->nefc) || (d->ncon && d->con_capacity < d->ncon)) {
    set_error("mjhipData holds %d rows / %d contacts but capacities %d / %d",
              d->nefc, d->ncon, d->efc_capacity, d->con_capacity);
    return MJHIP_ERR_ARG;
  }
  // sparse-mode models: compressed rows (nJ values) and the tendon rows' structure
  const bool sparse = mjh_isSparse(m);
  if (sparse && lo <= 1 && hi >= 1) {
    if (d->nJ < 0 || d->nJ > c->mirror.nj_cap) {
      set_error("%d compressed Jacobian entries exceed the device capacity (%ld)", d->nJ,
                c->mirror.nj_cap);
      return MJHIP_ERR_CAPACITY;
    }
    if ((m->ntendon && (!d->ten_J_rownnz || !d->ten_J_rowadr || !d->ten_J_colind)) ||
        (d->nefc && (!d->efc_J_rownnz || !d->efc_J_rowadr || !d->efc_J_colind || !d->efc_JT ||
                     !d->efc_JT_rownnz || !d->efc_JT_rowadr || !d->efc_JT_colind))) {
      set_error("sparse-Jacobian model: mjhipData lacks the compressed Jacobian arrays");
      return MJHIP_ERR_ARG;
    }
  }
  const int cnt[4] = {d->nefc, d->ne, d->nf, d->nl};
  int rc = put0(c, c->mirror.efc_count, cnt, 4);
  if (!rc) rc = put0(c, c->mirror.con_count, &d->ncon, 1);
  const int nv = m->nv;
  (void)nv;
#define MJ_M(n) m->n
#define XE(type, name, w, stage) \
  if (!rc && stage >= lo && stage <= hi) \
    rc = put0(c, c->mirror.name, (const type*)d->name, \
              (sparse && !strcmp(#name, "efc_J")) ? (long)d->nJ : (long)d->nefc * (w));
  MJHIP_DATA_EFC
#undef XE
  if (!rc && sparse && lo <= 1 && hi >= 1) {
    const long nt = m->ntendon, nJ = d->nJ, ne = d->nefc;
    rc = put0(c, c->mirror.nJ, &d->nJ, 1);
    if (!rc) rc = put0(c, c->mirror.ten_J_rownnz, (const int*)d->ten_J_rownnz, nt);
    if (!rc) rc = put0(c, c->mirror.ten_J_rowadr, (const int*)d->ten_J_rowadr, nt);
    if (!rc) rc = put0(c, c->mirror.ten_J_colind, (const int*)d->ten_J_colind, nt*nv);
    if (!rc) rc = put0(c, c->mirror.efc_J_rownnz, (const int*)d->efc_J_rownnz, ne);
    if (!rc) rc = put0(c, c->mirror.efc_J_rowadr, (const int*)d->efc_J_rowadr, ne);
    if (!rc) rc = put0(c, c->mirror.efc_J_colind, (const int*)d->efc_J_colind, nJ);
    if (!rc) rc = put0(c, c->mirror.efc_JT, (const double*)d->efc_JT, nJ);
    if (!rc && ne) rc = put0(c, c->mirror.efc_JT_rownnz, (const int*)d->efc_JT_rownnz, (long)nv);
    if (!rc && ne) rc = put0(c, c->mirror.efc_JT_rowadr, (const int*)d->efc_JT_rowadr, (long)nv);
    if (!rc) rc = put0(c, c->mirror.efc_JT_colind, (const int*)d->efc_JT_colind, nJ);
  }
#define XC(type, name, w, stage) \
  if (!rc && stage >= lo && stage <= hi) rc = put0(c, c->mirror.name, (const type*)d->name, \
                                                   (long)d->ncon * (w));
  MJHIP_DATA_CONTACT
#undef XC
#undef MJ_M
  return rc;
}

// rows written by stages lo..hi, instance 0 -> host, and the counts (contacts when lo <= 1);
// the caller synchronizes. Reading the counts needs one blocking copy first.
static int get_rows(mjhipContext* c, const mjhipModel* m, mjhipData* d, int lo, int hi) {
  int cnt[4] = {0, 0, 0, 0}, ncon = 0, nJ = 0;
  const bool sparse = mjh_isSparse(m);
  int rc = get0(c, cnt, (const int*)c->mirror.efc_count, 4);
  if (!rc) rc = get0(c, &ncon, (const int*)c->mirror.con_count, 1);
  if (!rc && sparse) rc = get0(c, &nJ, (const int*)c->mirror.nJ, 1);
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) {
    set_error("hipStreamSynchronize failed");
    rc = MJHIP_ERR_HIP;
  }
  if (rc) return rc;
  d->nefc = cnt[0]; d->ne = cnt[1]; d->nf = cnt[2]; d->nl = cnt[3];
  if (lo <= 1) d->ncon = ncon;
  if (sparse && lo <= 1) d->nJ = nJ;
  if (sparse && lo <= 1 &&
      ((m->ntendon && (!d->ten_J_rownnz || !d->ten_J_rowadr || !d->ten_J_colind)) ||
       (cnt[0] && d->efc_capacity >= cnt[0] &&
        (!d->efc_J_rownnz || !d->efc_J_rowadr || !d->efc_J_colind || !d->efc_JT ||
         !d->efc_JT_rownnz || !d->efc_JT_rowadr || !d->efc_JT_colind)))) {
    set_error("sparse-Jacobian model: mjhipData lacks the compressed Jacobian arrays");
    return MJHIP_ERR_ARG;
  }
  // rows a caller's buffers cannot hold: mjWARN_CNSTRFULL analogue, nothing written
  if ((cnt[0] && d->efc_capacity < cnt[0]) || (lo <= 1 && ncon && d->con_capacity < ncon)) {
    if (d->efc_capacity > 0 || d->con_capacity > 0) d->status |= MJHIP_INST_CNSTRFULL;
    return MJHIP_OK;
  }
  const int nv = m->nv;
  (void)nv;
#define MJ_M(n) m->n
#define XE(type, name, w, stage) \
  if (!rc && stage >= lo && stage <= hi) \
    rc = get0(c, (type*)d->name, (const type*)c->mirror.name, \
              (sparse && !strcmp(#name, "efc_J")) ? (long)nJ : (long)cnt[0] * (w));
  MJHIP_DATA_EFC
#undef XE
  if (!rc && sparse && lo <= 1) {
    const long nt = m->ntendon, ne = cnt[0];
    rc = get0(c, (int*)d->ten_J_rownnz, (const int*)c->mirror.ten_J_rownnz, nt);
    if (!rc) rc = get0(c, (int*)d->ten_J_rowadr, (const int*)c->mirror.ten_J_rowadr, nt);
    if (!rc) rc = get0(c, (int*)d->ten_J_colind, (const int*)c->mirror.ten_J_colind, nt*nv);
    if (!rc) rc = get0(c, (int*)d->efc_J_rownnz, (const int*)c->mirror.efc_J_rownnz, ne);
    if (!rc) rc = get0(c, (int*)d->efc_J_rowadr, (const int*)c->mirror.efc_J_rowadr, ne);
    if (!rc) rc = get0(c, (int*)d->efc_J_colind, (const int*)c->mirror.efc_J_colind, (long)nJ);
    if (!rc) rc = get0(c, (double*)d->efc_JT, (const double*)c->mirror.efc_JT, (long)nJ);
    if (!rc && ne) rc = get0(c, (int*)d->efc_JT_rownnz, (const int*)c->mirror.efc_JT_rownnz, (long)nv);
    if (!rc && ne) rc = get0(c, (int*)d->efc_JT_rowadr, (const int*)c->mirror.efc_JT_rowadr, (long)nv);
    if (!rc) rc = get0(c, (int*)d->efc_JT_colind, (const int*)c->mirror.efc_JT_colind, (long)nJ);
  }
#define XC(type, name, w, stage) \
  if (!rc && lo <= 1 && stage >= lo && stage <= hi) \
    rc = get0(c, (type*)d->name, (const type*)c->mirror.name, (long)ncon * (w));
  MJHIP_DATA_CONTACT
#undef XC
#undef MJ_M
  return rc;
}

// 1 when mj_inverseSkip reads mjData.act: mj_discreteAcc under the implicit or implicitfast
// integrator forms qDeriv, and mjd_actuator_vel (engine_derivative.c:855-863) multiplies a
// stateful actuator's velocity gain (affine, or a muscle's) by act
static bool inverse_reads_act(const mjhipModel* m) {
  if (!(m->opt.enableflags & mjhipENBL_INVDISCRETE) || !m->na ||
      (m->opt.disableflags & mjhipDSBL_ACTUATION) ||
      (m->opt.integrator != mjhipINT_IMPLICIT && m->opt.integrator != mjhipINT_IMPLICITFAST)) {
    return false;
  }
  for (int i = 0; i < m->nu; i++) {
    if (m->actuator_dyntype[i] == mjhipDYN_NONE) continue;
    if (m->actuator_gaintype[i] == mjhipGAIN_MUSCLE ||
        (m->actuator_gaintype[i] == mjhipGAIN_AFFINE && m->actuator_gainprm[10*i+2] != 0)) {
      return true;
    }
  }
  return false;
}

static int sync_stream(mjhipContext* c) {
  HIPCHECK(hipStreamSynchronize(c->stream));
  return MJHIP_OK;
}

// run one k_stage on instance 0; status comes back into d->status
static int run_stage(mjhipContext* c, mjhipData* d, int what, int skipstage = 0,
                     int skipsensor = 1) {
  if (c->con_cap > 0) {
    hipLaunchKernelGGL(k_stage<true>, dim3(1), dim3(64), 0, c->stream, c->dmodel, c->mirror,
                       what, skipstage, skipsensor, c->status);
  } else {
    hipLaunchKernelGGL(k_stage<false>, dim3(1), dim3(64), 0, c->stream, c->dmodel, c->mirror,
                       what, skipstage, skipsensor, c->status);
  }
  HIPCHECK(hipGetLastError());
  int st = 0;
  if (int rc = get0(c, &st, (const int*)c->status, 1)) return rc;
  if (int rc = sync_stream(c)) return rc;
  d->status = st;
  return MJHIP_OK;
}

// upload the fields a skipped stage reads (data fields, constraint rows, contacts), run one
// instance, download every output field of the stages that ran
MJHIP_API void mjhip_inverseSkip(const mjhipModel* m, mjhipData* d, int skipstage,
                                 int skipsensor) {
  CtxLease lease = lease_ctx(m, 0, 64);
  mjhipContext* c = lease.get();
  if (!c) {
    report("mjhip_inverseSkip");
    return;
  }
  int rc = hipSetDevice(c->device) == hipSuccess ? 0 : MJHIP_ERR_HIP;
  if (!rc) rc = put_stages(c, m, d, 0, skipstage);
  // the constraint rows of the skipped stages: mj_makeConstraint's (skipstage >= POS) and
  // mj_referenceConstraint's efc_vel / efc_aref (skipstage >= VEL)
  if (!rc && skipstage >= mjhipSTAGE_POS) rc = put_rows(c, m, d, 1, skipstage);
  if (!rc && m->nsensor > 0) {
    // sensor inputs: the values of skipped stages' sensors are kept (sensordata), and the
    // mjData inputs some sensors read (clock: time; force/torque/accelerometer via
    // mj_rnePostConstraint: xfrc_applied; actuatorfrc/jointactuatorfrc)
    if (skipstage > mjhipSTAGE_NONE && d->sensordata)
      rc = put0(c, c->mirror.sensordata, (const double*)d->sensordata, m->nsensordata);
    if (!rc) rc = put0(c, c->mirror.time, &d->time, 1);
    if (!rc && d->xfrc_applied) rc = put0(c, c->mirror.xfrc_applied, (const double*)d->xfrc_applied,
                                          6L*m->nbody);
    if (!rc && d->actuator_force) rc = put0(c, c->mirror.actuator_force,
                                            (const double*)d->actuator_force, (long)m->nu);
    if (!rc && d->qfrc_actuator) rc = put0(c, c->mirror.qfrc_actuator,
                                           (const double*)d->qfrc_actuator, (long)m->nv);
  }
  if (!rc && inverse_reads_act(m)) {
    if (!d->act) {
      set_error("the model's implicit mj_discreteAcc reads mjData.act (na = %d), but "
                "mjhipData.act is NULL", m->na);
      rc = MJHIP_ERR_ARG;
    } else {
      rc = put0(c, c->mirror.act, (const double*)d->act, (long)m->na);
    }
  }
  if (!rc && (skipstage < mjhipSTAGE_NONE || skipstage > mjhipSTAGE_VEL)) {
    set_error("skipstage must be mjSTAGE_NONE, mjSTAGE_POS or mjSTAGE_VEL");
    rc = MJHIP_ERR_ARG;
  }
  if (!rc) rc = run_stage(c, d, ST_INV, skipstage, skipsensor);
  if (!rc) rc = get_stages(c, m, d, skipstage + 1, 3);
  if (!rc && m->nsensor > 0 && !skipsensor) {
    // mjData fields the sensor stages computed on demand (scratch sized 0 when unneeded)
#define MJ_M(n) m->n
#define XD(name, d0, d1, stage)                                                     \
    if (!rc && d->name && c->mirror.name##_n > 0)                                    \
      rc = get0(c, d->name, (const double*)c->mirror.name, (long)(m->d0) * (d1));
    MJHIP_DATA_SENSOR_AUX
#undef XD
#undef MJ_M
  }
  mjtNum e[2] = {0, 0};
  const bool energy = (m->opt.enableflags & mjhipENBL_ENERGY) && skipstage < mjhipSTAGE_VEL;
  if (!rc && energy) rc = get0(c, e, (const double*)c->mirror.energy, 2);
  // the rows of the stages that ran (and the counts); get_rows synchronizes the stream
  if (!rc) rc = get_rows(c, m, d, skipstage + 1, 3);
  if (!rc) rc = sync_stream(c);
  if (!rc && energy) {
    // mj_energyPos/Vel write the energy of the stages that ran (engine_inverse.c:207-223)
    if (skipstage < mjhipSTAGE_POS) d->energy[0] = e[0];
    d->energy[1] = e[1];
  }
  if (rc) report("mjhip_inverseSkip");
}

MJHIP_API void mjhip_inverse(const mjhipModel* m, mjhipData* d) {
  mjhip_inverseSkip(m, d, mjhipSTAGE_NONE, 0);
}

// mj_invPosition / mj_invVelocity / mj_invConstraint (engine_inverse.c:37-76, :169-192): only
// that stage runs, it reads the inputs and earlier stages' fields from d and writes only its
// own outputs into d
static void single_stage(const mjhipModel* m, mjhipData* d, int what, const char* name) {
  CtxLease lease = lease_ctx(m, 0, 64);
  mjhipContext* c = lease.get();
  int rc = c ? 0 : MJHIP_ERR_HIP;
  if (!rc && hipSetDevice(c->device) != hipSuccess) rc = MJHIP_ERR_HIP;
  const int stage = what;                  // ST_POS/VEL/CON = position/velocity/acceleration
  if (!rc) rc = put_stages(c, m, d, 0, stage - 1);
  if (!rc && stage > ST_POS) rc = put_rows(c, m, d, 1, stage - 1);
  if (!rc) rc = run_stage(c, d, what);
  if (!rc) {
    if (what == ST_CON) {                  // qfrc_constraint only (qfrc_inverse is not its output)
      rc = get0(c, d->qfrc_constraint, (const double*)c->mirror.qfrc_constraint, (long)m->nv);
    } else {
      rc = get_stages(c, m, d, stage, stage);
    }
  }
  if (!rc) rc = get_rows(c, m, d, stage, stage);
  if (!rc) rc = sync_stream(c);
  if (rc) report(name);
}

MJHIP_API void mjhip_invPosition(const mjhipModel* m, mjhipData* d) {
  single_stage(m, d, ST_POS, "mjhip_invPosition");
}

MJHIP_API void mjhip_invVelocity(const mjhipModel* m, mjhipData* d) {
  single_stage(m, d, ST_VEL, "mjhip_invVelocity");
}

MJHIP_API void mjhip_invConstraint(const mjhipModel* m, mjhipData* d) {
  single_stage(m, d, ST_CON, "mjhip_invConstraint");
}

// mj_rne (engine_core_smooth.c:1969-2023): reads the caller's cdof, cinert, cvel, cdof_dot,
// qvel (and qacc with flg_acc) and writes only `result`
MJHIP_API void mjhip_rne(const mjhipModel* m, mjhipData* d, int flg_acc, mjtNum* result) {
  CtxLease lease = lease_ctx(m, 0, 64);
  mjhipContext* c = lease.get();
  int rc = c ? 0 : MJHIP_ERR_HIP;
  if (!rc && hipSetDevice(c->device) != hipSuccess) rc = MJHIP_ERR_HIP;
  if (!rc) rc = put0(c, c->mirror.cdof, (const double*)d->cdof, 6L*m->nv);
  if (!rc) rc = put0(c, c->mirror.cinert, (const double*)d->cinert, 10L*m->nbody);
  if (!rc) rc = put0(c, c->mirror.cvel, (const double*)d->cvel, 6L*m->nbody);
  if (!rc) rc = put0(c, c->mirror.cdof_dot, (const double*)d->cdof_dot, 6L*m->nv);
  if (!rc) rc = put0(c, c->mirror.qvel, (const double*)d->qvel, (long)m->nv);
  if (!rc && flg_acc) rc = put0(c, c->mirror.qacc, (const double*)d->qacc, (long)m->nv);
  int st = d->status;
  if (!rc) rc = run_stage(c, d, flg_acc ? ST_RNE1 : ST_RNE0);
  d->status = st;                          // mj_rne leaves d alone
  if (!rc && result) rc = get0(c, result, (const double*)c->mirror.qfrc_tmp, (long)m->nv);
  if (!rc) rc = sync_stream(c);
  if (rc) report("mjhip_rne");
}

// mj_xfrcAccumulate (engine_support.c:1254-1261): qfrc += J' xfrc_applied over bodies 1..,
// through mj_applyFT (its mj_jac reads d's xipos, subtree_com and cdof)
MJHIP_API void mjhip_xfrcAccumulate(const mjhipModel* m, mjhipData* d, mjtNum* qfrc) {
  CtxLease lease = lease_ctx(m, 0, 64);
  mjhipContext* c = lease.get();
  int rc = c ? 0 : MJHIP_ERR_HIP;
  if (!rc && hipSetDevice(c->device) != hipSuccess) rc = MJHIP_ERR_HIP;
  if (!rc) rc = put0(c, c->mirror.xipos, (const double*)d->xipos, 3L*m->nbody);
  if (!rc) rc = put0(c, c->mirror.subtree_com, (const double*)d->subtree_com, 3L*m->nbody);
  if (!rc) rc = put0(c, c->mirror.cdof, (const double*)d->cdof, 6L*m->nv);
  if (!rc) rc = put0(c, c->mirror.xfrc_applied, (const double*)d->xfrc_applied, 6L*m->nbody);
  if (!rc) rc = put0(c, c->mirror.qfrc_tmp, (const double*)qfrc, (long)m->nv);
  int st = d->status;
  if (!rc) rc = run_stage(c, d, ST_XFRC);
  d->status = st;
  if (!rc) rc = get0(c, qfrc, (const double*)c->mirror.qfrc_tmp, (long)m->nv);
  if (!rc) rc = sync_stream(c);
  if (rc) report("mjhip_xfrcAccumulate");
}

// mju_dot (engine_util_blas.c:680-741, four partial sums) and mju_norm, for the two norms of
// mj_compareFwdInv
static double dot4(const double* a, const double* b, int n) {
  double r0 = 0, r1 = 0, r2 = 0, r3 = 0;
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    r0 += a[i]*b[i];
    r1 += a[i+1]*b[i+1];
    r2 += a[i+2]*b[i+2];
    r3 += a[i+3]*b[i+3];
  }
  double res = (r0 + r2) + (r1 + r3);
  const int left = n - i;           // the tail is one sum added to res, as mju_dot's
  if (left == 3) {
    res += a[i]*b[i] + a[i+1]*b[i+1] + a[i+2]*b[i+2];
  } else if (left == 2) {
    res += a[i]*b[i] + a[i+1]*b[i+1];
  } else if (left == 1) {
    res += a[i]*b[i];
  }
  return res;
}

// mj_compareFwdInv (engine_inverse.c:275-316): with constraint rows, qforce = qfrc_applied +
// qfrc_actuator + J'xfrc_applied (mj_xfrcAccumulate) is what inverse dynamics of the forward
// pass's qacc must return; mj_inverseSkip(VEL, 1) runs on the device with the forward pass's
// rows; solver_fwdinv = (|fwd - inv qfrc_constraint|, |qforce - qfrc_inverse|); the forward
// qfrc_constraint and efc_force are restored.
MJHIP_API void mjhip_compareFwdInv(const mjhipModel* m, mjhipData* d) {
  const int nv = m->nv, nefc = d->nefc;
  d->solver_fwdinv[0] = d->solver_fwdinv[1] = 0;
  if (!nefc) return;
  if (!d->efc_force || d->efc_capacity < nefc) {
    set_error("mj_compareFwdInv: the data holds no constraint rows (efc_capacity %d < nefc %d)",
              d->efc_capacity, nefc);
    report("mjhip_compareFwdInv");
    return;
  }
  std::vector<double> qforce(nv), dif(nv), save_qc(d->qfrc_constraint, d->qfrc_constraint + nv),
                      save_force(d->efc_force, d->efc_force + nefc);
  for (int i = 0; i < nv; i++) qforce[i] = d->qfrc_applied[i] + d->qfrc_actuator[i];
  mjhip_xfrcAccumulate(m, d, qforce.data());
  mjhip_inverseSkip(m, d, mjhipSTAGE_VEL, 1);
  for (int i = 0; i < nv; i++) dif[i] = save_qc[i] - d->qfrc_constraint[i];
  d->solver_fwdinv[0] = sqrt(dot4(dif.data(), dif.data(), nv));
  for (int i = 0; i < nv; i++) dif[i] = qforce[i] - d->qfrc_inverse[i];
  d->solver_fwdinv[1] = sqrt(dot4(dif.data(), dif.data(), nv));
  memcpy(d->qfrc_constraint, save_qc.data(), sizeof(double)*nv);
  memcpy(d->efc_force, save_force.data(), sizeof(double)*nefc);
}

// mjd_inverseFD (engine_derivative_fd.c:611-719, mujoco.h:1244-1247) for one mjData: the
// batched FD with one base state (d's qpos, qvel, qacc, ctrl, act). Like the reference, d is left
// with the outputs of the last evaluation (the last qpos perturbation) and its own qpos.
MJHIP_API void mjhip_inverseFD(const mjhipModel* m, mjhipData* d, mjtNum eps,
                               mjtByte flg_actuation, mjtNum* DfDq, mjtNum* DfDv, mjtNum* DfDa,
                               mjtNum* DsDq, mjtNum* DsDv, mjtNum* DsDa, mjtNum* DmDq) {
  const int P = 3*m->nv + 1;
  // an FD batch of one needs 3nv+1 instances: a context of that capacity, leased like the
  // single-instance ones under the salted signature
  CtxLease lease = lease_ctx(m, kFDSalt, P);
  mjhipContext* c = lease.get();
  int rc = c ? 0 : MJHIP_ERR_HIP;
  if (!rc && m->nsensor && (DsDq || DsDv || DsDa)) {
    std::vector<double> t(P, d->time);                    // clock sensors of every evaluation
    rc = mjhip_mirrorUpload(c, "time", 0, P, t.data());
  }
  if (!rc && m->na && !d->act && (flg_actuation || inverse_reads_act(m))) {
    set_error("mjd_inverseFD reads mjData.act (na = %d), but mjhipData.act is NULL", m->na);
    rc = MJHIP_ERR_ARG;
  }
  if (!rc) rc = mjhip_inverseFDBatchAct(c, 1, d->qpos, d->qvel, d->qacc, d->ctrl, d->act, eps,
                                        flg_actuation, DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, DmDq,
                                        kFlagFDFull);
  if (!rc) {
    // the reference's last evaluation (engine_derivative_fd.c:646-715): the last qpos
    // perturbation, else the last qvel one, else the last qacc one, else the centre
    const int nv = m->nv;
    const int last = (DfDq || DsDq || DmDq) ? P - 1 : (DfDv || DsDv) ? 2*nv
                     : (DfDa || DsDa) ? nv : 0;
    std::vector<double> keep(d->qpos, d->qpos + m->nq);
#define MJ_M(n) m->n
#define XD(name, d0, d1, stage)                                                     \
    if (!rc && d->name && stage > 0 && (m->d0) * (d1) > 0)                           \
      rc = mjhip_mirrorDownload(c, #name, last, 1, d->name);
    MJHIP_DATA_FIELDS
#undef XD
#undef MJ_M
    memcpy(d->qpos, keep.data(), sizeof(double)*m->nq);
  }
  if (rc) report("mjhip_inverseFD");
}

}  // extern "C"
