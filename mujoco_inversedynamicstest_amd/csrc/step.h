// step.h -- mj_step for constraint-free states: the integrators of engine_forward.c on top of
// mjh::forwardSkip, restated in the reference's operation order (file:line as in
// engine_device.h). Included only by kern_step.hip (k_rollout), kern_transition.hip
// (k_transition, through transition.h) and, for the host, by the test harnesses;
// engine_device.h and the other hashed headers do not change.
//
// The integrators' scratch (qH, qHDiagInv, the RK4 stages, and the implicit integrator's
// qLU / qDeriv / mjd_rne_vel buffers when the mirror does not hold them) is not part of the
// mirror: it lives in one buffer of its own in the mirror's [blk][k][S] interleaving
// (StepLayout gives each array's first component, stepBind the per-lane views).
#pragma once
#include "engine_device.h"

namespace mjh {

// status bits that take an instance out of the constraint-free set
constexpr int kStepStop = MJHIP_INST_BADQPOS | MJHIP_INST_BADQVEL | MJHIP_INST_BADQACC |
                          MJHIP_INST_UNSUPPORTED;

// mjd_passive_vel's fluid terms enter qDeriv (mjh_fluidDeriv without its mjENBL_INVDISCRETE
// condition: here the integrator itself asks for them)
MJH_HD int stepFluidDeriv(const mjhipModel* m) {
  return (m->opt.integrator == mjhipINT_IMPLICIT || m->opt.integrator == mjhipINT_IMPLICITFAST) &&
         !(m->opt.disableflags & mjhipDSBL_PASSIVE) &&
         (m->opt.viscosity > 0 || m->opt.density > 0);
}

// first component of each scratch array (doubles per instance); -1: the array is not needed
// by the model's integrator, or (own == 0 arrays) the mirror already holds it
struct StepLayout {
  int qH = -1, qHDiagInv = -1, tmp = -1, X = -1, F = -1, dX = -1;
  int qLU = -1, qDeriv = -1, Dcvel = -1, Dcacc = -1, Dcfrc = -1, Dcdofdot = -1, Dtmp = -1;
  int rem = -1;                             // mju_factorLUSparse's int scratch (nv ints)
  int total = 0;
};

MJH_HD StepLayout stepLayout(const mjhipModel* m) {
  StepLayout L;
  const int nv = m->nv, nq = m->nq, na = m->na, integ = m->opt.integrator;
  int k = 0;
  auto take = [&](int n) { const int at = k; k += n; return at; };
  L.tmp = take(nv);                         // qfrc / qacc of the integrators, the fwd/inv force
  if (integ == mjhipINT_EULER || integ == mjhipINT_IMPLICITFAST) {
    L.qH = take(m->nC);
    L.qHDiagInv = take(nv);
  }
  if (integ == mjhipINT_RK4) {
    L.X = take(4*(nq + nv + na));
    L.F = take(4*(nv + na));
    L.dX = take(2*nv + na);
  }
  if (integ == mjhipINT_IMPLICIT) {
    L.rem = take((nv + 1) / 2);
    if (!mjh_implicit(m)) {
      L.qLU = take(m->nD);
      L.Dcvel = take(6*m->nB);
      L.Dcacc = take(6*m->nB);
      L.Dcfrc = take(6*m->nB);
      L.Dcdofdot = take(6*m->nD);
    }
  }
  if ((integ == mjhipINT_IMPLICIT || stepFluidDeriv(m)) && !mjh_qDerivStored(m)) {
    L.qDeriv = take(m->nD);
    L.Dtmp = take(6*nv);
  }
  L.total = k;
  return L;
}

template <int S>
struct StepScratch {
  SP<S> qH, qHDiagInv, tmp, X, F, dX;
  SP<S, int> rem;
};

// per-lane views of the scratch block `blk` (component k of lane l at blk[k*S + l]); the
// implicit integrator's arrays the mirror lacks are bound into the lane itself, where
// mjh::rneVel and mjh::fluidDeriv look for them
template <int S>
MJH_HD StepScratch<S> stepBind(const StepLayout& L, Lane<S>& d, double* blk, int lane) {
  StepScratch<S> sc{};
  auto at = [&](int off) { return SP<S>{off < 0 ? nullptr : blk + (long)off*S + lane}; };
  sc.qH = at(L.qH);
  sc.qHDiagInv = at(L.qHDiagInv);
  sc.tmp = at(L.tmp);
  sc.X = at(L.X);
  sc.F = at(L.F);
  sc.dX = at(L.dX);
  sc.rem.p = L.rem < 0 ? nullptr : reinterpret_cast<int*>(blk + (long)L.rem*S) + lane;
  if (L.qLU >= 0) {
    d.qLU = at(L.qLU);
    d.Dcvel = at(L.Dcvel);
    d.Dcacc = at(L.Dcacc);
    d.Dcfrc = at(L.Dcfrc);
    d.Dcdofdot = at(L.Dcdofdot);
  }
  if (L.qDeriv >= 0) {
    d.qDeriv = at(L.qDeriv);
    d.Dtmp = at(L.Dtmp);
  }
  return sc;
}

// mj_integratePos engine_support.c:1518-1548
template <class Q, class V>
MJH_HD void integratePos(const mjhipModel& m, Q qpos, V qvel, double dt) {
  for (int j = 0; j < m.njnt; j++) {
    int padr = m.jnt_qposadr[j], vadr = m.jnt_dofadr[j];
    switch (m.jnt_type[j]) {
    case mjhipJNT_FREE:
      for (int i = 0; i < 3; i++) qpos[padr+i] += dt * qvel[vadr+i];
      padr += 3;
      vadr += 3;
      // fallthrough
    case mjhipJNT_BALL:
      quatIntegrate(qpos + padr, qvel + vadr, dt);
      break;
    default:                                // hinge, slide
      qpos[padr] += dt * qvel[vadr];
    }
  }
}

// mj_advance engine_forward.c:738-776 (no plugins; time is not carried); qvel_given false:
// positions integrate with the updated d.qvel (semi-implicit)
template <int S, class A, class Q, class V>
MJH_HD void advance(const mjhipModel& m, const Lane<S>& d, A act_dot, Q qacc, V qvel,
                    bool qvel_given) {
  if (m.na && !(m.opt.disableflags & mjhipDSBL_ACTUATION)) {
    for (int i = 0; i < m.nu; i++) {
      const int actadr = m.actuator_actadr[i];
      const int actadr_end = actadr + m.actuator_actnum[i];
      for (int j = actadr; j < actadr_end; j++) {
        d.act[j] = nextActivation(m, i, d.act[j], act_dot[j]);
      }
    }
  }
  addToScl(d.qvel, qacc, m.opt.timestep, m.nv);
  if (qvel_given) integratePos(m, d.qpos, qvel, m.opt.timestep);
  else integratePos(m, d.qpos, d.qvel, m.opt.timestep);
}

// mj_factorI engine_core_smooth.c:1483-1511 on the C sparsity
template <int S>
MJH_HD void factorI(const mjhipModel& m, SP<S> mat, SP<S> diaginv) {
  const int *rownnz = m.C_rownnz, *rowadr = m.C_rowadr, *colind = m.C_colind;
  for (int k = m.nv-1; k >= 0; k--) {
    const int rowadr_k = rowadr[k];
    const int diag_k = rowadr_k + rownnz[k] - 1;
    const double invD = 1 / mat[diag_k];
    diaginv[k] = invD;
    if (m.dof_simplenum[k]) continue;
    for (int adr = diag_k - 1; adr >= rowadr_k; adr--) {
      const double tmp = mat[adr] * invD;
      const int i = colind[adr];
      addToScl(mat + rowadr[i], mat + rowadr_k, -tmp, rownnz[i]);
      mat[adr] = tmp;
    }
  }
}

// mj_solveLD engine_core_smooth.c:1629-1707, one right-hand side, in place
template <int S>
MJH_HD void solveLD(const mjhipModel& m, SP<S> x, SP<S> qLD, SP<S> diaginv) {
  const int nv = m.nv;
  for (int i = nv-1; i > 0; i--) {
    if (m.dof_simplenum[i]) continue;
    const double x_i = x[i];
    if (x_i) {
      const int start = m.C_rowadr[i], end = start + m.C_rownnz[i] - 1;
      for (int adr = start; adr < end; adr++) x[m.C_colind[adr]] -= qLD[adr] * x_i;
    }
  }
  for (int i = 0; i < nv; i++) x[i] *= diaginv[i];
  for (int i = 1; i < nv; i++) {
    if (m.dof_simplenum[i]) {
      i += m.dof_simplenum[i] - 1;
      continue;
    }
    const int dd = m.C_rownnz[i] - 1;
    if (dd > 0) {
      const int adr = m.C_rowadr[i];
      x[i] -= dotSparse(qLD + adr, x, dd, m.C_colind + adr);
    }
  }
}

// mju_factorLUSparse engine_util_solve.c:571-643 on the D sparsity (the structure checks are
// mjERRORs there; a diagonal below mjMINVAL, also an mjERROR, is reported as
// MJHIP_INST_INERTIA and the factorization goes on)
template <int S>
MJH_HD int factorLUSparse(const mjhipModel& m, SP<S> LU, SP<S, int> remaining) {
  const int n = m.nv;
  const int *rownnz = m.D_rownnz, *rowadr = m.D_rowadr, *colind = m.D_colind;
  int status = 0;
  for (int i = 0; i < n; i++) remaining[i] = rownnz[i];
  for (int i = n-1; i >= 0; i--) {
    const int ii = rowadr[i] + remaining[i] - 1;
    remaining[i]--;
    if (!(fabs(LU[ii]) >= MINVAL)) status |= MJHIP_INST_INERTIA;
    for (int j = i-1; j >= 0; j--) {
      const int ji = rowadr[j] + remaining[j] - 1;
      if (ji >= rowadr[j] && colind[ji] == i) {
        remaining[j]--;
        LU[ji] = LU[ji] / LU[ii];
        const double LUji = LU[ji];
        int icnt = rowadr[i], jcnt = rowadr[j];
        const int iend = rowadr[i] + remaining[i], jend = rowadr[j] + remaining[j];
        while (jcnt < jend && icnt < iend) {
          if (colind[icnt] == colind[jcnt]) {
            LU[jcnt] -= LU[icnt] * LUji;
            jcnt++;
            icnt++;
          } else if (colind[icnt] > colind[jcnt]) {
            jcnt++;
          } else {
            icnt++;                         // "requires fill-in": not reached on a tree
          }
        }
      }
    }
  }
  return status;
}

// mju_solveLUSparse engine_util_solve.c:648-675; D_diag (engine_io.c, a mjData field) is
// found per row as dAdr(m, i, i) does
template <int S, class R, class V>
MJH_HD void solveLUSparse(const mjhipModel& m, R res, SP<S> LU, V vec) {
  const int n = m.nv;
  const int *rownnz = m.D_rownnz, *rowadr = m.D_rowadr, *colind = m.D_colind;
  for (int i = n-1; i >= 0; i--) {
    res[i] = vec[i];
    const int d1 = dAdr(m, i, i) - rowadr[i] + 1;
    const int nnz = rownnz[i] - d1;
    if (nnz > 0) {
      const int adr = rowadr[i] + d1;
      res[i] -= dotSparse(LU + adr, res, nnz, colind + adr);
    }
  }
  for (int i = 0; i < n; i++) {
    const int dg = dAdr(m, i, i) - rowadr[i];
    const int adr = rowadr[i];
    if (dg > 0) res[i] -= dotSparse(LU + adr, res, dg, colind + adr);
    res[i] /= LU[adr + dg];
  }
}

// mj_EulerSkip engine_forward.c:779-830. skipfactor: qH / qHDiagInv are not formed; the
// solve reads the factor sc.qH / sc.qHDiagInv already hold (mj_stepSkip's reuse)
template <int S>
MJH_HD void eulerSkip(const mjhipModel& m, const Lane<S>& d, const StepScratch<S>& sc,
                      bool skipfactor = false) {
  const int nv = m.nv;
  SP<S> qacc = sc.tmp;
  int dof_damping = 0;
  if (!(m.opt.disableflags & mjhipDSBL_EULERDAMP)) {
    for (int i = 0; i < nv; i++) {
      if (m.dof_damping[i] > 0) {
        dof_damping = 1;
        break;
      }
    }
  }
  if (!dof_damping) {
    copy(qacc, d.qacc, nv);
  } else {
    if (!skipfactor) {
      for (int i = 0; i < m.nC; i++) sc.qH[i] = d.qM[m.mapM2C[i]];
      for (int i = 0; i < nv; i++) {
        sc.qH[m.C_rowadr[i] + m.C_rownnz[i] - 1] += m.opt.timestep * m.dof_damping[i];
      }
      factorI(m, sc.qH, sc.qHDiagInv);
    }
    for (int i = 0; i < nv; i++) qacc[i] = d.qfrc_smooth[i] + d.qfrc_constraint[i];
    solveLD(m, qacc, sc.qH, sc.qHDiagInv);
  }
  advance(m, d, d.act_dot, qacc, d.qvel, false);
}

// mjd_smooth_vel (engine_derivative.c:1522-1536) into d.qDeriv on the D sparsity: actuator
// and passive terms (qDerivAt, fluidDeriv), then mjd_rne_vel when flg_bias
template <int S>
MJH_HD void smoothVel(const mjhipModel& m, const Lane<S>& d, bool flg_bias) {
  for (int r = 0; r < m.nv; r++) {
    const int adr = m.D_rowadr[r];
    for (int k = 0; k < m.D_rownnz[r]; k++) {
      d.qDeriv[adr + k] = qDerivAt(m, d, r, m.D_colind[adr + k]);
    }
  }
  if (stepFluidDeriv(&m)) fluidDeriv(m, d);
  if (flg_bias) rneVel(m, d);
}

// mj_implicitSkip engine_forward.c:948-1021. skipfactor: neither qDeriv nor the factor is
// formed; the solve reads what d.qLU (implicit) or sc.qH / sc.qHDiagInv (implicitfast) hold
template <int S>
MJH_HD int implicitSkip(const mjhipModel& m, const Lane<S>& d, const StepScratch<S>& sc,
                        bool skipfactor = false) {
  const int nv = m.nv;
  const double h = m.opt.timestep;
  int status = 0;
  SP<S> qacc = sc.tmp;
  if (m.opt.integrator == mjhipINT_IMPLICIT) {
    if (!skipfactor) {
      smoothVel(m, d, true);
      for (int i = 0; i < m.nD; i++) d.qLU[i] = d.qM[m.mapM2D[i]];
      addToScl(d.qLU, d.qDeriv, -h, m.nD);
      status |= factorLUSparse(m, d.qLU, sc.rem);
    }
    // qfrc = qfrc_smooth + qfrc_constraint (held in qforce: res and vec are distinct arrays)
    for (int i = 0; i < nv; i++) d.qforce[i] = d.qfrc_smooth[i] + d.qfrc_constraint[i];
    solveLUSparse(m, qacc, d.qLU, d.qforce);
  } else {
    // MhB = qM - h*qDeriv[mapD2M], moved through mapM2C: entry (r, c) of the C sparsity is
    // M's entry of dof r and its ancestor c, and mapD2M's image of it is dAdr(m, r, c)
    const bool stored = stepFluidDeriv(&m);
    if (!skipfactor) {
      if (stored) smoothVel(m, d, false);
      for (int r = 0; r < nv; r++) {
        const int adr = m.C_rowadr[r];
        for (int k = 0; k < m.C_rownnz[r]; k++) {
          const int c = m.C_colind[adr + k];
          const double q = stored ? (double)d.qDeriv[dAdr(m, r, c)] : qDerivAt(m, d, r, c);
          sc.qH[adr + k] = d.qM[m.mapM2C[adr + k]] + q * -h;
        }
      }
      factorI(m, sc.qH, sc.qHDiagInv);
    }
    for (int i = 0; i < nv; i++) qacc[i] = d.qfrc_smooth[i] + d.qfrc_constraint[i];
    solveLD(m, qacc, sc.qH, sc.qHDiagInv);
  }
  advance(m, d, d.act_dot, qacc, d.qvel, false);
  return status;
}

// mj_RungeKutta(m, d, 4) engine_forward.c:855-943. X and F carry act and act_dot; the three
// inner evaluations are mj_forwardSkip(mjSTAGE_NONE, 1). An evaluation that leaves the
// constraint-free set ends the step: the state goes back to X[0] and the bits are returned.
template <int S, bool CONTACT>
MJH_HD int rungeKutta4(const mjhipModel& m, const Lane<S>& d, const StepScratch<S>& sc) {
  const double A[9] = {0.5, 0, 0, 0, 0.5, 0, 0, 0, 1};
  const double B[4] = {1.0/6.0, 1.0/3.0, 1.0/3.0, 1.0/6.0};
  const int nv = m.nv, nq = m.nq, na = m.na, N = 4;
  const int nx = nq + nv + na, nf = nv + na;
  const double h = m.opt.timestep;
  SP<S> dX = sc.dX, X0 = sc.X, F0 = sc.F;
  copy(X0, d.qpos, nq);
  copy(X0 + nq, d.qvel, nv);
  copy(F0, d.qacc, nv);
  if (na) {
    copy(X0 + nq + nv, d.act, na);
    copy(F0 + nv, d.act_dot, na);
  }
  for (int i = 1; i < N; i++) {
    SP<S> Xi = sc.X + (long)i*nx, Fi = sc.F + (long)i*nf;
    zero(dX, 2*nv + na);
    for (int j = 0; j < i; j++) {
      addToScl(dX, sc.X + (long)j*nx + nq, A[(i-1)*(N-1)+j], nv);
      addToScl(dX + nv, sc.F + (long)j*nf, A[(i-1)*(N-1)+j], nv + na);
    }
    copy(Xi, X0, nx);
    integratePos(m, Xi, dX, h);
    addToScl(Xi + nq, dX + nv, h, nv + na);
    copy(d.qpos, Xi, nq);
    copy(d.qvel, Xi + nq, nv);
    if (na) copy(d.act, Xi + nq + nv, na);
    const int st = forwardSkip<S, CONTACT>(m, d, mjhipSTAGE_NONE);
    if (st & kStepStop) {
      copy(d.qpos, X0, nq);
      copy(d.qvel, X0 + nq, nv);
      if (na) copy(d.act, X0 + nq + nv, na);
      return st;
    }
    copy(Fi, d.qacc, nv);
    if (na) copy(Fi + nv, d.act_dot, na);
  }
  zero(dX, 2*nv + na);
  for (int j = 0; j < N; j++) {
    addToScl(dX, sc.X + (long)j*nx + nq, B[j], nv);
    addToScl(dX + nv, sc.F + (long)j*nf, B[j], nv + na);
  }
  copy(d.qpos, X0, nq);
  copy(d.qvel, X0 + nq, nv);
  if (na) copy(d.act, X0 + nq + nv, na);
  advance(m, d, dX + 2*nv, dX + nv, dX, true);
  return 0;
}

// The driver's solver_fwdinv[1] (src/inverse/inverse_test.cpp:72-99; mj_compareFwdInv's
// second number for a constraint-free state, engine_inverse.c:297-301): the norm of
// qfrc_applied + qfrc_actuator + J'xfrc_applied - qfrc_inverse, the inverse run from
// mjSTAGE_VEL without sensors on forward's qacc. The inverse writes neither qacc nor
// qfrc_smooth, and its qfrc_constraint is forward's (0: no rows).
template <int S, bool CONTACT>
MJH_HD double compareFwdInv(const mjhipModel& m, const Lane<S>& d, const StepScratch<S>& sc) {
  const int nv = m.nv;
  SP<S> e = sc.tmp;
  for (int i = 0; i < nv; i++) e[i] = d.qfrc_applied[i] + d.qfrc_actuator[i];
  xfrcAccumulate(m, d, e);
  inverseSkip<S, CONTACT>(m, d, mjhipSTAGE_VEL, 1);
  for (int i = 0; i < nv; i++) e[i] = e[i] - d.qfrc_inverse[i];
  return sqrt(dot(e, e, nv));
}

// mj_step engine_forward.c:1134-1168 for a constraint-free state. The status bits of the
// step's forward are mj_checkPos / mj_checkVel / mj_checkAcc and the row count; a kStepStop
// bit returns before the integrator with the state as it came. *fwdinv (when asked for)
// receives compareFwdInv. After a completed step the first forward's qacc is firstQacc().
template <int S, bool CONTACT>
MJH_HD int step(const mjhipModel& m, const Lane<S>& d, const StepScratch<S>& sc,
                bool want_fwdinv, double* fwdinv) {
  int st = forwardSkip<S, CONTACT>(m, d, mjhipSTAGE_NONE);
  if (st & kStepStop) return st;
  if (want_fwdinv) *fwdinv = compareFwdInv<S, CONTACT>(m, d, sc);
  switch (m.opt.integrator) {
  case mjhipINT_EULER: eulerSkip(m, d, sc); break;
  case mjhipINT_RK4: st |= rungeKutta4<S, CONTACT>(m, d, sc); break;
  default: st |= implicitSkip(m, d, sc); break;
  }
  return st;
}

// mj_stepSkip engine_derivative_fd.c:120-155 for a constraint-free state (no fwd/inv check):
// forwardSkip(skipstage) with step's stop rule, then Euler with skipfactor = skipstage >= POS
// or implicit / implicitfast with skipfactor = skipstage >= VEL. The stages skipped and the
// factor reused are whatever d's and sc's pointers of those fields address (transition.h
// points them at the centre evaluation's). RK4 ignores skipstage in the reference and
// mjd_transitionFD refuses it; the entry point does too, and a lane that got here anyway is
// flagged and not advanced.
template <int S, bool CONTACT>
MJH_HD int stepSkip(const mjhipModel& m, const Lane<S>& d, const StepScratch<S>& sc,
                    int skipstage) {
  int st = forwardSkip<S, CONTACT>(m, d, skipstage);
  if (st & kStepStop) return st;
  switch (m.opt.integrator) {
  case mjhipINT_EULER: eulerSkip(m, d, sc, skipstage >= mjhipSTAGE_POS); break;
  case mjhipINT_RK4: st |= MJHIP_INST_UNSUPPORTED; break;
  default: st |= implicitSkip(m, d, sc, skipstage >= mjhipSTAGE_VEL); break;
  }
  return st;
}

// the first forward's qacc of the step that just completed: RK4 leaves its last evaluation's
// in d.qacc and the first in F[0]; the other integrators do not touch d.qacc
template <int S>
MJH_HD SP<S> firstQacc(const mjhipModel& m, const Lane<S>& d, const StepScratch<S>& sc) {
  return m.opt.integrator == mjhipINT_RK4 ? sc.F : d.qacc;
}

}  // namespace mjh
