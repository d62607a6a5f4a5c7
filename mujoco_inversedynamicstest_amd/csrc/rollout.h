// rollout.h -- what mjhip.hip (the C-ABI, mjhip_rolloutBatch) and kern_step.hip (k_rollout)
// share: the kernel's own argument struct and its launcher. The integrators themselves
// (step.h) are seen by kern_step.hip alone.
#pragma once
#include <hip/hip_runtime.h>

#include "engine_device.h"

// how a per-step input reaches the kernel (mjhipRolloutIn's *_mode)
enum { kRolloutAbsent = 0, kRolloutHeld = 1, kRolloutPerStep = 2 };

// k_rollout's arguments beside mjhipModel and Mirror (device pointers; B x n row-major, the
// per-step arrays B x T x n). Kept out of Mirror and mjhipModel, which every other kernel
// takes by value.
struct RolloutCall {
  double* scratch;                          // the integrator scratch, [blk][k][64]
  const double *qpos, *qvel, *act;          // initial state (null: the mirror's)
  const double *ctrl, *qfrc_applied, *xfrc_applied;
  double *state, *qacc, *fwdinv;            // optional outputs
  int* steps_done;
  int* status;
  int ctrl_mode, qfrc_mode, xfrc_mode;
  int B, T;
  int fwdinv_on;                            // run the fwd/inv check (without `fwdinv`: unused)
};

// doubles of integrator scratch per instance for this (host) model
long mjhip_rolloutScratchDoubles(const mjhipModel* hm);

// one launch for all T steps; direct: the per-lane row store instead of the LDS write-out
// (measurement only). Nonzero when the launch failed.
int mjhip_launchRollout(hipStream_t s, const mjhipModel& dmodel, const Mirror& mr,
                        const RolloutCall& call, bool contact, bool direct);
