// transition_call.h -- what mjhip.hip (the C-ABI, mjhip_transitionFDBatch) and
// kern_transition.hip (k_transition, k_transition_diff) share: the kernels' own argument
// struct and their launcher. The lane functions (transition.h over step.h) are seen by
// kern_transition.hip alone.
#pragma once
#include <hip/hip_runtime.h>

#include "engine_device.h"

// the kernels' arguments beside mjhipModel and Mirror (device pointers, B x n row-major)
struct TransitionCall {
  double* scratch;                          // the integrator scratch, [blk][k][64]
  double* Y;                                // next states, [1 + P][nq+nv+na][nblk*64]
  const double *qpos, *qvel, *act, *ctrl;   // base states (act, ctrl null: zeros)
  const double *qfrc_applied, *xfrc_applied;  // held over a base state's evaluations (null: 0)
  double *A, *Bm;                           // B x ndx x ndx, B x ndx x nu (null: not wanted)
  int* status;                              // B words: the OR over a base state's evaluations
  int* cstatus;                             // B words: the centres' own (null when P == 0)
  double eps;
  int B, nblk;                              // base states, ceil(B/64)
  int centered, want_A, want_B;
};

// perturbation slots P of a call on this (host) model, as transition.h plans them
int mjhip_transitionSlots(const mjhipModel* hm, int want_A, int want_B, int centered);

// centres, perturbed evaluations, differencing: three launches in stream order. Nonzero when
// a launch failed.
int mjhip_launchTransition(hipStream_t s, const mjhipModel& dmodel, const Mirror& mr,
                           const TransitionCall& call, int P, bool contact);
