// fast_kernels.h — the registry entry of a straight-line (model-specialized) kernel, shared by
// mjhip.hip and gen_fast.hip (the bundled models' kernels, a translation unit of their own so
// the two compile in parallel).
#ifndef MJHIP_FAST_KERNELS_H_
#define MJHIP_FAST_KERNELS_H_

#include <hip/hip_runtime.h>

#include "engine_device.h"

struct FastKernelEntry {
  unsigned long long sig;
  void (*launch)(dim3, dim3, hipStream_t, const Mirror&, int, const double*, const double*,
                 const double*, double*, int*, int*, int*, int*, int*,
                 const int* /* device-side instance range {first, end}, or null */);
  const char* name;
  int cmode;   // codegen.constraint_mode: 0 none, 1 work-list, 2 every instance
  // mj_inverseSkip(mjSTAGE_POS) for mjd_inverseFD's qvel/qacc perturbations: the va stage of
  // instances [off, B), position-stage inputs from centre (t - off)/per*sstride (codegen.py
  // k_vaskip); null for run-time kernels and models whose rows serve every instance
  // (the last argument is eps: each skip instance reads its centre's qpos/qvel/qacc and adds
  // eps to the component it perturbs, so k_fd_expand writes only the position-stage block)
  void (*launch_vaskip)(hipStream_t, const Mirror&, int, int, int, int, int*, int*, double);
  // batched mj_inverseSkip(skipstage) for skipstage POS (k_va) or VEL (k_acc) over [0, B)
  // (qfrc_out row-major or null, status or null, efc_count)
  void (*launch_skip)(hipStream_t, const Mirror&, int, int, double*, int*, int*);
  // static LDS in bytes of the compiled k_all variants (hipFuncGetAttributes), -1 on a HIP
  // error; null for run-time kernels, whose code object mjhip_contextLoadKernel queries
  int (*lds_bytes)();
  // k_const (codegen.py CONST_ONCE): stores the model-constant output slots the stage bodies
  // leave out, over all nblk 64-instance blocks of the capacity; the library runs it before
  // the first generated-kernel launch of a context and again after anything that may have
  // overwritten the slots (mjhip.hip ensure_const). const_stores: their count per instance.
  // Both null when the kernels store everything themselves; a run-time kernel's are found in
  // its code object (mjhip_contextLoadKernel)
  void (*launch_const)(hipStream_t, const Mirror&, int);
  int (*const_stores)();
  // qM entries per instance that k_all's HO instantiation hands from its pos stage to its fac
  // stage in LDS (codegen.py qm_handoff_plan), launched when Mirror::qm_handoff is set; 0
  // where nothing fits. Null for run-time kernels: the count is a global of the code object
  int (*qm_handoff)();
  // and those it forwards in registers (codegen.py qm_forward_plan), under the same switch
  int (*qm_forward)();
};

// static LDS a k_all workgroup may hold while four of them share a CU's 160 KB
// (codegen.py LDS_BUDGET)
constexpr int kFastLdsBudget = 40960;

// the bundled models' kernels (gen_fast.hip), terminated by an entry with launch = nullptr
const FastKernelEntry* mjhip_fastKernels();
int mjhip_genSetTimerBuf(unsigned long long* p);   // gen_fast.hip's mjh_tbuf
int mjhip_genExactSetTimerBuf(unsigned long long* p);   // gen_fast_exact.hip's

#endif  // MJHIP_FAST_KERNELS_H_
