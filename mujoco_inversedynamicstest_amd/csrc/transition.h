// transition.h -- mjd_transitionFD (engine_derivative_fd.c:306-595) for constraint-free
// states: the lane functions of kern_transition.hip's kernels (one lane per evaluation of
// mj_stepSkip, then the differencing), shared with the host build tests/transition_harness.cpp.
//
// Evaluation slots. A call over B base states (padded to nblk = ceil(B/64) blocks) runs the
// nblk centre blocks, then P perturbation slots of nblk blocks each, kind-major in the order
// qpos, qvel, act (when A is wanted), ctrl (when B is wanted), perturbation-major within a
// kind, then the sign (+eps, and -eps when centred; ctrl always has both, because a forward
// difference at the upper end of ctrlrange is taken backward). Evaluation block g = (1 + slot)
// * nblk + cb uses mirror block g and step-scratch block g, and lane l of it belongs to base
// state cb*64 + l, the state of lane l of centre block cb.
//
// Skipped stages. A qvel evaluation skips the position stage, an act / ctrl evaluation the
// velocity stage too: the reference's mjData then still holds the centre's results, so the
// lane's view takes the pointers of those stages' outputs from the centre's lane view
// (aliasSkipped) and, where mj_stepSkip sets skipfactor, the factor from the centre's step
// scratch (aliasFactor). Both are read-only for the lane: everything it writes is a field its
// own slot keeps (DESIGN.md §Transition derivatives has the audit). The mocap poses of a base
// state are the centre slot's too, for every evaluation (aliasMocap).
#pragma once
#include "step.h"

namespace mjh {

enum { kTrQpos = 0, kTrQvel = 1, kTrAct = 2, kTrCtrl = 3 };

// what a call evaluates: perturbation slots per kind and each kind's first slot
struct TransitionPlan {
  int first[4], count[4], nsign[4];
  int P;                                    // perturbation slots in all
};

MJH_HD TransitionPlan transitionPlan(const mjhipModel& m, bool want_A, bool want_B,
                                     bool centered) {
  TransitionPlan p;
  const int n[4] = {want_A ? m.nv : 0, want_A ? m.nv : 0, want_A ? m.na : 0,
                    want_B ? m.nu : 0};
  int at = 0;
  for (int k = 0; k < 4; k++) {
    p.nsign[k] = (centered || k == kTrCtrl) ? 2 : 1;
    p.count[k] = n[k];
    p.first[k] = at;
    at += n[k] * p.nsign[k];
  }
  p.P = at;
  return p;
}

// slot of (kind, perturbation i, sign s: 0 = +eps, 1 = -eps)
MJH_HD int transitionSlot(const TransitionPlan& p, int kind, int i, int s) {
  return p.first[kind] + i*p.nsign[kind] + s;
}

// the inverse: kind, perturbation index and sign of a slot
MJH_HD void transitionDecode(const TransitionPlan& p, int slot, int* kind, int* i, int* s) {
  int k = 3;
  while (k > 0 && (p.count[k] == 0 || slot < p.first[k])) k--;
  *kind = k;
  *i = (slot - p.first[k]) / p.nsign[k];
  *s = (slot - p.first[k]) % p.nsign[k];
}

// mj_stepSkip's skipstage per kind (engine_derivative_fd.c:357, :400, :447, :496)
MJH_HD int transitionSkipstage(int kind) {
  return kind == kTrQpos ? mjhipSTAGE_NONE : kind == kTrQvel ? mjhipSTAGE_POS : mjhipSTAGE_VEL;
}

// inRange :112-115
MJH_HD int inRange(double x1, double x2, const double* range) {
  return x1 >= range[0] && x1 <= range[1] && x2 >= range[0] && x2 <= range[1];
}

// which nudges of ctrl[i] are taken (:349-366)
MJH_HD void ctrlNudge(const mjhipModel& m, int i, double ctrl, double eps, bool centered,
                      int* fwd, int* back) {
  const int limited = m.actuator_ctrllimited[i];
  const double* r = m.actuator_ctrlrange + 2*i;
  *fwd = !limited || inRange(ctrl, ctrl + eps, r);
  *back = (centered || !*fwd) && (!limited || inRange(ctrl - eps, ctrl, r));
}

// dpos = e_i as mj_integratePos reads it (:491-493)
struct UnitDof {
  int i, at;
  MJH_HD double operator[](long k) const { return at + k == i ? 1.0 : 0.0; }
  MJH_HD UnitDof operator+(long k) const { return UnitDof{i, at + (int)k}; }
};

// Apply the slot's perturbation to the base state in d (qpos, qvel, act, ctrl). Returns
// whether the evaluation takes place (a ctrl nudge out of range does not).
template <int S>
MJH_HD bool transitionPerturb(const mjhipModel& m, const Lane<S>& d, int kind, int i, int s,
                              double eps, bool centered) {
  const double e = s ? -eps : eps;
  switch (kind) {
  case kTrQpos:
    integratePos(m, d.qpos, UnitDof{i, 0}, e);
    return true;
  case kTrQvel:
    if (s) d.qvel[i] -= eps;
    else d.qvel[i] += eps;
    return true;
  case kTrAct:
    if (s) d.act[i] -= eps;
    else d.act[i] += eps;
    return true;
  default: {
    int fwd, back;
    ctrlNudge(m, i, d.ctrl[i], eps, centered, &fwd, &back);
    if (s ? !back : !fwd) return false;
    if (s) d.ctrl[i] -= eps;
    else d.ctrl[i] += eps;
    return true;
  }
  }
}

// The skipped stages' outputs are the centre's: every mjData field of the position stage
// (skipstage >= POS) and of the velocity stage (skipstage >= VEL), the row and contact counts
// mj_forwardSkip ends on, and a sparse model's tendon Jacobian structure. d keeps its own
// inputs, forward outputs, scratch and constraint rows (a lane runs only when its centre has
// no rows, so no row of either slot is touched).
template <int S>
MJH_HD void aliasSkipped(Lane<S>& d, const Lane<S>& c, int skipstage) {
  if (skipstage < mjhipSTAGE_POS) return;
#define XD(name, d0, d1, stage) d.name = c.name;
  MJHIP_DATA_POSITION
  if (skipstage >= mjhipSTAGE_VEL) {
    MJHIP_DATA_VELOCITY
  }
#undef XD
  d.efc_count = c.efc_count;
  d.con_count = c.con_count;
  d.ten_J_rownnz = c.ten_J_rownnz;
  d.ten_J_rowadr = c.ten_J_rowadr;
  d.ten_J_colind = c.ten_J_colind;
  d.gxpos = c.geom_xpos;
}

// Mocap poses are per-instance inputs the call does not take: they are what the caller put
// in the mirror slot of the base state (mjhip_mirrorUpload; the centre's slot), and every
// evaluation of that base state, whatever it skips, reads them from there (kinematics only
// reads them).
template <int S>
MJH_HD void aliasMocap(Lane<S>& d, const Lane<S>& c) {
  d.mocap_pos = c.mocap_pos;
  d.mocap_quat = c.mocap_quat;
}

// mj_EulerSkip's / mj_implicitSkip's skipfactor for this skipstage (:137, :147)
MJH_HD bool transitionSkipfactor(const mjhipModel& m, int skipstage) {
  return m.opt.integrator == mjhipINT_EULER ? skipstage >= mjhipSTAGE_POS
                                            : skipstage >= mjhipSTAGE_VEL;
}

// the factor a skipfactor step solves with is the centre's (read-only)
template <int S>
MJH_HD void aliasFactor(const mjhipModel& m, Lane<S>& d, StepScratch<S>& sc, const Lane<S>& c,
                        const StepScratch<S>& csc, int skipstage) {
  if (!transitionSkipfactor(m, skipstage)) return;
  sc.qH = csc.qH;
  sc.qHDiagInv = csc.qHDiagInv;
  if (m.opt.integrator == mjhipINT_IMPLICIT) d.qLU = c.qLU;
}

// a vector whose component k is p[k*stride]
struct Strided {
  const double* p;
  long stride;
  MJH_HD double operator[](long k) const { return p[k*stride]; }
  MJH_HD Strided operator+(long k) const { return Strided{p + k*stride, stride}; }
};

// One column of the transposed Jacobians, stateDiff :58-67: ds[r] for r < 2nv+na handed to
// put(r, value). s1, s2: states (qpos, qvel, act), h the step between them. nq == nv: plain
// differences times inv_h; else mj_differentiatePos (engine_support.c:1483-1513, which
// divides) for the qpos rows.
template <class Put>
MJH_HD void stateDiff(const mjhipModel& m, Strided s1, Strided s2, double h, Put put) {
  const int nq = m.nq, nv = m.nv, na = m.na;
  const double inv_h = 1/h;
  if (nq == nv) {
    for (int r = 0; r < nq + nv + na; r++) put(r, inv_h * (s2[r] - s1[r]));
    return;
  }
  for (int j = 0; j < m.njnt; j++) {
    int padr = m.jnt_qposadr[j], vadr = m.jnt_dofadr[j];
    switch (m.jnt_type[j]) {
    case mjhipJNT_FREE:
      for (int i = 0; i < 3; i++) put(vadr + i, (s2[padr+i] - s1[padr+i]) / h);
      vadr += 3;
      padr += 3;
      // fallthrough
    case mjhipJNT_BALL: {
      const double qa[4] = {s2[padr], s2[padr+1], s2[padr+2], s2[padr+3]};
      const double qb[4] = {s1[padr], s1[padr+1], s1[padr+2], s1[padr+3]};
      double v[3];
      subQuat(v, qa, qb);
      const double inv = 1/h;
      for (int i = 0; i < 3; i++) put(vadr + i, v[i] * inv);
      break;
    }
    default:
      put(vadr, (s2[padr] - s1[padr]) / h);
    }
  }
  for (int r = 0; r < nv + na; r++) put(nv + r, inv_h * (s2[nq + r] - s1[nq + r]));
}

// Column `col` of A (kinds qpos, qvel, act: col = i, nv + i, 2nv + i) or of B (ctrl: col = i)
// for one base state: the states of the evaluations it differences are at(slot) (slot -1: the
// centre), the clamped forms :72-107. ctrl: the base state's ctrl[i]. put(r, value) receives
// all 2nv+na rows.
template <class At, class Put>
MJH_HD void transitionColumn(const mjhipModel& m, const TransitionPlan& p, int kind, int i,
                             double eps, bool centered, double ctrl, At at, Put put) {
  int fwd = 1, back = centered;
  if (kind == kTrCtrl) ctrlNudge(m, i, ctrl, eps, centered, &fwd, &back);
  const int plus = transitionSlot(p, kind, i, 0), minus = transitionSlot(p, kind, i, 1);
  if (fwd && !back) stateDiff(m, at(-1), at(plus), eps, put);
  else if (!fwd && back) stateDiff(m, at(minus), at(-1), eps, put);
  else if (fwd && back) stateDiff(m, at(minus), at(plus), 2*eps, put);
  else for (int r = 0; r < 2*m.nv + m.na; r++) put(r, 0.0);
}

}  // namespace mjh
