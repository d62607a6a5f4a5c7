// solver_call.h -- what mjhip.hip (the C-ABI, mjhip_forwardSolveBatch) and kern_solver.hip
// (k_forward_solve) share: the kernel's own argument struct and its launcher. The solver
// itself (solver.h) is seen by kern_solver.hip alone.
#pragma once
#include <hip/hip_runtime.h>

#include "engine_device.h"

// k_forward_solve's arguments beside mjhipModel and Mirror (device pointers, B x n row-major).
// Kept out of Mirror and mjhipModel, which every other kernel takes by value.
struct SolverCall {
  double* scratch;                          // the solver scratch, [blk][k][64]
  const double *qpos, *qvel, *ctrl, *act;   // inputs (null: the mirror's)
  const double* qacc_warmstart;             // null: the scratch's kept warmstart
  double *qacc, *qfrc_constraint, *act_dot, *act_next;   // optional outputs
  int* niter;                               // optional output, B ints
  int* status;                              // B words
  double tolerance, ls_tolerance, meaninertia;
  int iterations, ls_iterations;
  int B;
};

// doubles of solver scratch per instance for this (host) model and row capacity
long mjhip_solverScratchDoubles(const mjhipModel* hm, int efc_cap);

// one launch. Nonzero when the launch failed.
int mjhip_launchForwardSolve(hipStream_t s, const mjhipModel& dmodel, const Mirror& mr,
                             const SolverCall& call, bool contact);
