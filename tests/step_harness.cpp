// step_harness.cpp — TEST ONLY: mj_step of the device path (mujoco_inversedynamicstest_amd/
// csrc/step.h over engine_device.h) compiled for the host with stride 1, so
// tests/test_step_cpu.py can compare the integrators bit for bit with the oracle and with the
// plain-Python restatement tests/step_ref.py without a GPU. Never part of the product library.
#include "cpu_kernel_harness.cpp"            // bind(): a Lane<1> over mjhipData and scratch
#include "../mujoco_inversedynamicstest_amd/csrc/step.h"

extern "C" long sh_scratchDoubles(const mjhipModel* m) { return mjh::stepLayout(m).total; }

// nstep calls of mj_step from the state in d (qpos, qvel; act / ctrl, na / nu doubles, may be
// null when the model has none). qfrc_applied / xfrc_applied: null (d's values), or
// nstep x nv / nstep x 6 nbody per-step rows. Outputs as mjhip_rolloutBatch's for one
// instance: state nstep x (nq+nv+na), qacc nstep x nv, fwdinv nstep (each may be null). The
// stop rule is the kernel's: returns the number of completed steps, *status the bits.
extern "C" int sh_rollout(const mjhipModel* m, mjhipData* d, double* scratch, int* iscratch,
                          int efc_cap, int con_cap, double* step_scratch, double* act,
                          double* ctrl, int nstep, const double* qfrc_applied,
                          const double* xfrc_applied, int want_fwdinv, double* state,
                          double* qacc, double* fwdinv, int* status) {
  mjh::Lane<1> L = bind(m, d, scratch, iscratch, efc_cap, con_cap);
  const int nq = m->nq, nv = m->nv, na = m->na, nx = 6*m->nbody;
  std::vector<double> act_dot(na + 1), act_next(na + 1), ctrl0(m->nu + 1, 0.0);
  L.act.p = act;
  L.act_dot.p = act_dot.data();
  L.act_next.p = act_next.data();
  if (!d->ctrl) L.ctrl.p = ctrl0.data();
  if (ctrl) L.ctrl.p = ctrl;
  const mjh::StepLayout lay = mjh::stepLayout(m);
  const mjh::StepScratch<1> sc = mjh::stepBind<1>(lay, L, step_scratch, 0);
  int done = 0, st_all = 0;
  bool active = true;
  for (int t = 0; t < nstep; t++) {
    bool stepped = false;
    double fi = 0;
    if (active) {
      if (qfrc_applied) for (int k = 0; k < nv; k++) L.qfrc_applied[k] = qfrc_applied[t*nv + k];
      if (xfrc_applied) for (int k = 0; k < nx; k++) L.xfrc_applied[k] = xfrc_applied[t*nx + k];
      const int st = mjh::step<1, true>(*m, L, sc, want_fwdinv != 0, &fi);
      st_all |= st;
      if (st & mjh::kStepStop) {
        active = false;
        fi = 0;
      } else {
        stepped = true;
        done++;
      }
    }
    if (state) {
      double* row = state + (long)t*(nq + nv + na);
      for (int k = 0; k < nq; k++) row[k] = L.qpos[k];
      for (int k = 0; k < nv; k++) row[nq + k] = L.qvel[k];
      for (int k = 0; k < na; k++) row[nq + nv + k] = L.act[k];
    }
    if (qacc) {
      const mjh::SP<1> q0 = mjh::firstQacc(*m, L, sc);
      for (int k = 0; k < nv; k++) qacc[(long)t*nv + k] = stepped ? (double)q0[k] : 0.0;
    }
    if (fwdinv) fwdinv[t] = fi;
  }
  d->nefc = L.efc_count[0];
  *status = st_all;
  return done;
}

// mj_forward alone, by the code that existed before the integrators (mjh::forwardSkip,
// qDerivAt, fluidDeriv, rneVel), for tests/step_ref.py's forward fields of a model whose
// actuators the oracle does not carry: qM, qfrc_smooth, qacc are left in d, act_dot (na) and
// mjd_smooth_vel(flg_bias) as a dense nv x nv matrix (entries of the D sparsity) are
// returned. flg_bias = 1 needs the implicit integrator's scratch, i.e. an implicit model.
extern "C" int sh_forward(const mjhipModel* m, mjhipData* d, double* scratch, int* iscratch,
                          int efc_cap, int con_cap, double* step_scratch, double* act,
                          double* ctrl, int flg_bias, double* act_dot, double* qderiv) {
  mjh::Lane<1> L = bind(m, d, scratch, iscratch, efc_cap, con_cap);
  std::vector<double> act_next(m->na + 1), ctrl0(m->nu + 1, 0.0);
  L.act.p = act;
  L.act_dot.p = act_dot;
  L.act_next.p = act_next.data();
  if (!d->ctrl) L.ctrl.p = ctrl0.data();
  if (ctrl) L.ctrl.p = ctrl;
  mjh::stepBind<1>(mjh::stepLayout(m), L, step_scratch, 0);
  const int st = mjh::forwardSkip(*m, L, mjhipSTAGE_NONE);
  const int nv = m->nv;
  for (int k = 0; k < nv*nv; k++) qderiv[k] = 0;
  if (flg_bias) {
    for (int r = 0; r < nv; r++) {
      for (int k = 0; k < m->D_rownnz[r]; k++) {
        L.qDeriv[m->D_rowadr[r] + k] = mjh::qDerivAt(*m, L, r, m->D_colind[m->D_rowadr[r] + k]);
      }
    }
    if (mjh::stepFluidDeriv(m)) mjh::fluidDeriv(*m, L);
    mjh::rneVel(*m, L);
  }
  for (int r = 0; r < nv; r++) {
    for (int k = 0; k < m->D_rownnz[r]; k++) {
      const int a = m->D_rowadr[r] + k, c = m->D_colind[a];
      qderiv[r*nv + c] = flg_bias ? (double)L.qDeriv[a] : mjh::qDerivAt(*m, L, r, c);
    }
  }
  d->nefc = L.efc_count[0];
  return st;
}
