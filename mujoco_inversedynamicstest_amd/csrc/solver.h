// solver.h -- mj_forward with constraint rows: mj_fwdConstraint, its warmstart and the Newton
// branch of mj_solCGNewton (dense Hessian, pyramidal or frictionless contacts), restated in the
// reference's operation order (file:line as in engine_device.h). Included only by
// kern_solver.hip (k_forward_solve) and, for the host, by the test harnesses; engine_device.h
// and the other hashed headers do not change.
//
// The solver's arrays are not part of the mirror: they live in one buffer of their own in the
// mirror's [blk][k][S] interleaving (SolverLayout gives each array's first component,
// solverBind the per-lane views). qacc_warmstart is the one array that carries a value from
// one call to the next.
//
// Out of scope (refused at the entry point): elliptic cones (HessianCone and the cone line
// search), the CG and PGS solvers, sparse Jacobians, the noslip pass. mjENBL_ISLAND is
// ignored, as the reference's Newton ignores it (engine_forward.c:679-682).
#pragma once
#include "engine_device.h"

namespace mjh {

// mjOption's solver settings and mjModel.stat.meaninertia (mjhipOption does not carry them)
struct SolverOpt {
  double tolerance, ls_tolerance, meaninertia;
  int iterations, ls_iterations;
};

// what the host tests read beside the mirror (null on the device)
struct SolverTrace {
  double cost;                              // ctx.cost after the last CGupdateConstraint
  double* alpha;                            // CGsearch's result per iteration (alpha_cap)
  int alpha_cap, nalpha;
  int nupdate, ndowndate, nrefactor;        // mju_cholUpdate calls (+, -), rank-loss refactors
  int warm;                                 // warmstart kept qacc_warmstart (1) or qacc_smooth (0)
};

// first component of each scratch array (doubles per instance)
struct SolverLayout {
  int L, Ma, Mv, grad, Mgrad, search, vec, qacc_warmstart, efc_b, Jaref, Jv, D, quad, oldstate;
  int total;
};

MJH_HD SolverLayout solverLayout(const mjhipModel* m, int efc_cap) {
  SolverLayout L;
  const int nv = m->nv;
  int k = 0;
  auto take = [&](int n) { const int at = k; k += n; return at; };
  L.qacc_warmstart = take(nv);
  L.L = take(nv*nv);
  L.Ma = take(nv);
  L.Mv = take(nv);
  L.grad = take(nv);
  L.Mgrad = take(nv);
  L.search = take(nv);
  L.vec = take(nv);
  L.efc_b = take(efc_cap);
  L.Jaref = take(efc_cap);
  L.Jv = take(efc_cap);
  L.D = take(efc_cap);
  L.quad = take(3*efc_cap);
  L.oldstate = take((efc_cap + 1)/2);
  L.total = k;
  return L;
}

template <int S>
struct SolverScratch {
  SP<S> L, Ma, Mv, grad, Mgrad, search, vec, qacc_warmstart, efc_b, Jaref, Jv, D, quad;
  SP<S, int> oldstate;
};

// per-lane views of the scratch block `blk` (component k of lane l at blk[k*S + l])
template <int S>
MJH_HD SolverScratch<S> solverBind(const SolverLayout& L, double* blk, int lane) {
  SolverScratch<S> sc;
  auto at = [&](int off) { return SP<S>{blk + (long)off*S + lane}; };
  sc.L = at(L.L);
  sc.Ma = at(L.Ma);
  sc.Mv = at(L.Mv);
  sc.grad = at(L.grad);
  sc.Mgrad = at(L.Mgrad);
  sc.search = at(L.search);
  sc.vec = at(L.vec);
  sc.qacc_warmstart = at(L.qacc_warmstart);
  sc.efc_b = at(L.efc_b);
  sc.Jaref = at(L.Jaref);
  sc.Jv = at(L.Jv);
  sc.D = at(L.D);
  sc.quad = at(L.quad);
  sc.oldstate.p = reinterpret_cast<int*>(blk + (long)L.oldstate*S) + lane;
  return sc;
}

//---------------------------------- engine_util_solve.c, engine_util_blas.c ------------------

// mju_cholFactor engine_util_solve.c:32-61
template <class M> MJH_HD int cholFactor(M mat, int n, double mindiag) {
  int rank = n;
  for (int j = 0; j < n; j++) {
    double tmp = mat[j*(n+1)];
    if (j) tmp -= dot(mat + j*n, mat + j*n, j);
    if (tmp < mindiag) {
      tmp = mindiag;
      rank--;
    }
    mat[j*(n+1)] = sqrt(tmp);
    tmp = 1/mat[j*(n+1)];
    for (int i = j+1; i < n; i++) {
      mat[i*n+j] = (mat[i*n+j] - dot(mat + i*n, mat + j*n, j)) * tmp;
    }
  }
  return rank;
}

// mju_cholSolve engine_util_solve.c:66-92
template <class R, class M, class V> MJH_HD void cholSolve(R res, M mat, V vec, int n) {
  copy(res, vec, n);
  for (int i = 0; i < n; i++) {
    if (i) res[i] -= dot(mat + i*n, res, i);
    res[i] /= mat[i*(n+1)];
  }
  for (int i = n-1; i >= 0; i--) {
    if (i < n-1) {
      for (int j = i+1; j < n; j++) res[i] -= mat[j*n+i] * res[j];
    }
    res[i] /= mat[i*(n+1)];
  }
}

// mju_cholUpdate engine_util_solve.c:97-137
template <class M, class V> MJH_HD int cholUpdate(M mat, V x, int n, int flg_plus) {
  int rank = n;
  for (int k = 0; k < n; k++) {
    if (x[k]) {
      const double Lkk = mat[k*(n+1)];
      double tmp = Lkk*Lkk + (flg_plus ? x[k]*x[k] : -x[k]*x[k]);
      if (tmp < MINVAL) {
        tmp = MINVAL;
        rank--;
      }
      const double r = sqrt(tmp);
      const double c = r / Lkk;
      const double cinv = 1 / c;
      const double s = x[k] / Lkk;
      mat[k*(n+1)] = r;
      if (flg_plus) {
        for (int i = k+1; i < n; i++) mat[i*n+k] = (mat[i*n+k] + s*x[i])*cinv;
      } else {
        for (int i = k+1; i < n; i++) mat[i*n+k] = (mat[i*n+k] - s*x[i])*cinv;
      }
      for (int i = k+1; i < n; i++) x[i] = c*x[i] - s*mat[i*n+k];
    }
  }
  return rank;
}

// mju_sqrMatTD engine_util_blas.c:848-879 (diag given)
template <class R, class M, class D>
MJH_HD void sqrMatTD(R res, M mat, D diag, int nr, int nc) {
  zero(res, nc*nc);
  for (int j = 0; j < nr; j++) {
    if (diag[j]) {
      for (int i = 0; i < nc; i++) {
        const double tmp = mat[j*nc+i];
        if (tmp) addToScl(res + i*nc, mat + j*nc, tmp*diag[j], i+1);
      }
    }
  }
  for (int i = 0; i < nc; i++) {
    for (int j = i+1; j < nc; j++) res[i*nc+j] = res[j*nc+i];
  }
}

// mj_addMDense engine_support.c:1164-1187
template <int S, class R> MJH_HD void addMDense(const mjhipModel& m, const Lane<S>& d, R dst) {
  const int nv = m.nv;
  for (int i = 0; i < nv; i++) {
    int adr = m.dof_Madr[i];
    int j = i;
    while (j >= 0) {
      dst[i*nv+j] += d.qM[adr];
      if (j < i) dst[j*nv+i] += d.qM[adr];
      if (m.dof_simplenum[i]) break;
      j = m.dof_parentid[j];
      adr++;
    }
  }
}

// mj_mulJacVec engine_core_constraint.c (dense: mju_mulMatVec engine_util_blas.c:747-751)
template <int S, class R, class V>
MJH_HD void mulJacVec(const mjhipModel& m, const Lane<S>& d, R res, V vec) {
  const int nv = m.nv, nefc = d.efc_count[0];
  for (int r = 0; r < nefc; r++) res[r] = dot(d.efc_J + r*nv, vec, nv);
}

//---------------------------------- engine_core_constraint.c ---------------------------------

// mj_constraintUpdate_island :2387-2549 (island < 0, with the cost, no cone Hessian). The
// force and state rules are invConstraint's; elliptic rows do not reach this function.
template <int S, class J>
MJH_HD void constraintUpdate(const mjhipModel& m, const Lane<S>& d, J jar, double* cost) {
  const int nv = m.nv, nefc = d.efc_count[0], ne = d.efc_count[1], nf = d.efc_count[2];
  double s = 0;
  if (!nefc) {
    zero(d.qfrc_constraint, nv);
    if (cost) *cost = 0;
    return;
  }
  for (int i = 0; i < nefc; i++) d.efc_force[i] = -d.efc_D[i]*jar[i];
  for (int i = 0; i < nefc; i++) {
    const double jr = jar[i], D = d.efc_D[i];
    if (i < ne) {
      if (cost) s += 0.5*D*jr*jr;
      d.efc_state[i] = CNSTRSTATE_QUADRATIC;
      continue;
    }
    if (i < ne + nf) {
      const double R = d.efc_R[i], floss = d.efc_frictionloss[i];
      if (jr <= -R*floss) {
        if (cost) s += -0.5*R*floss*floss - floss*jr;
        d.efc_force[i] = floss;
        d.efc_state[i] = CNSTRSTATE_LINEARNEG;
      } else if (jr >= R*floss) {
        if (cost) s += -0.5*R*floss*floss + floss*jr;
        d.efc_force[i] = -floss;
        d.efc_state[i] = CNSTRSTATE_LINEARPOS;
      } else {
        if (cost) s += 0.5*D*jr*jr;
        d.efc_state[i] = CNSTRSTATE_QUADRATIC;
      }
      continue;
    }
    if (jr >= 0) {
      d.efc_force[i] = 0;
      d.efc_state[i] = CNSTRSTATE_SATISFIED;
    } else {
      if (cost) s += 0.5*D*jr*jr;
      d.efc_state[i] = CNSTRSTATE_QUADRATIC;
    }
  }
  mulMatTVec(d.qfrc_constraint, d.efc_J, d.efc_force, nefc, nv);   // mj_mulJacTVec, dense
  if (cost) *cost = s;
}

//---------------------------------- engine_solver.c (Newton) ---------------------------------

// the scalar part of mjCGContext (:780-817); its arrays are SolverScratch
struct SolverCtx {
  double cost, quadGauss[3], scale;
  double gtol_scale;                        // opt.tolerance * opt.ls_tolerance
  int ls_iterations, LSiter;
  int nv, nefc, ne, nf;
};

// linesearch evaluation point :1021-1026
struct SolverPnt {
  double alpha, cost, deriv[2];
};

// CGupdateConstraint :869-895
template <int S>
MJH_HD void solverUpdateConstraint(const mjhipModel& m, const Lane<S>& d,
                                   const SolverScratch<S>& sc, SolverCtx& ctx) {
  constraintUpdate(m, d, sc.Jaref, &ctx.cost);
  double Gauss = 0;
  for (int i = 0; i < ctx.nv; i++) {
    Gauss += 0.5*(sc.Ma[i] - d.qfrc_smooth[i])*(d.qacc[i] - d.qacc_smooth[i]);
  }
  ctx.quadGauss[0] = Gauss;
  ctx.cost += Gauss;
}

// CGupdateGradient :900-926 (Newton, dense, no cones: Mgrad = H \ grad)
template <int S>
MJH_HD void solverUpdateGradient(const Lane<S>& d, const SolverScratch<S>& sc,
                                 const SolverCtx& ctx) {
  for (int i = 0; i < ctx.nv; i++) {
    sc.grad[i] = sc.Ma[i] - d.qfrc_smooth[i] - d.qfrc_constraint[i];
  }
  cholSolve(sc.Mgrad, sc.L, sc.grad, ctx.nv);
}

// CGprepare :931-1016 (no elliptic rows)
template <int S>
MJH_HD void solverPrepare(const Lane<S>& d, const SolverScratch<S>& sc, SolverCtx& ctx) {
  const int nv = ctx.nv;
  const double v_dot_smooth = dot(d.qfrc_smooth, sc.search, nv);
  ctx.quadGauss[1] = dot(sc.search, sc.Ma, nv) - v_dot_smooth;
  ctx.quadGauss[2] = 0.5*dot(sc.search, sc.Mv, nv);
  for (int i = 0; i < ctx.nefc; i++) {
    const double Jv = sc.Jv[i], Jaref = sc.Jaref[i], D = d.efc_D[i];
    const double DJ0 = D*Jaref;
    double q0 = Jaref*DJ0;
    const double q1 = Jv*DJ0;
    double q2 = Jv*D*Jv;
    q0 *= 0.5;
    q2 *= 0.5;
    sc.quad[3*i] = q0;
    sc.quad[3*i+1] = q1;
    sc.quad[3*i+2] = q2;
  }
}

// CGeval :1031-1170 (no elliptic rows)
template <int S>
MJH_HD void solverEval(const Lane<S>& d, const SolverScratch<S>& sc, SolverCtx& ctx,
                       SolverPnt* p) {
  const int ne = ctx.ne, nf = ctx.nf, nefc = ctx.nefc;
  double cost = 0;
  const double alpha = p->alpha;
  double deriv[2] = {0, 0};
  double quadTotal[3] = {ctx.quadGauss[0], ctx.quadGauss[1], ctx.quadGauss[2]};
  for (int i = 0; i < nefc; i++) {
    if (i < ne) {
      addTo3(quadTotal, sc.quad + 3*i);
      continue;
    }
    if (i < ne + nf) {
      const double start = sc.Jaref[i], dir = sc.Jv[i];
      const double x = start + alpha*dir;
      const double f = d.efc_frictionloss[i];
      const double Rf = d.efc_R[i]*f;
      if (-Rf < x && x < Rf) {
        addTo3(quadTotal, sc.quad + 3*i);
      } else if (x <= -Rf) {
        const double qf[3] = {f*(-0.5*Rf-start), -f*dir, 0};
        addTo3(quadTotal, qf);
      } else {
        const double qf[3] = {f*(-0.5*Rf+start), f*dir, 0};
        addTo3(quadTotal, qf);
      }
      continue;
    }
    const double x = sc.Jaref[i] + alpha*sc.Jv[i];
    if (x < 0) addTo3(quadTotal, sc.quad + 3*i);
  }
  cost += alpha*alpha*quadTotal[2] + alpha*quadTotal[1] + quadTotal[0];
  deriv[0] += 2*alpha*quadTotal[2] + quadTotal[1];
  deriv[1] += 2*quadTotal[2];
  if (deriv[1] <= 0) deriv[1] = MINVAL;     // not convex; SHOULD NOT OCCUR
  p->cost = cost;
  p->deriv[0] = deriv[0];
  p->deriv[1] = deriv[1];
  ctx.LSiter++;
}

// updateBracket :1173-1201
template <int S>
MJH_HD int solverUpdateBracket(const Lane<S>& d, const SolverScratch<S>& sc, SolverCtx& ctx,
                               SolverPnt* p, const SolverPnt candidates[3], SolverPnt* pnext) {
  int flag = 0;
  for (int i = 0; i < 3; i++) {
    if (p->deriv[0] < 0 && candidates[i].deriv[0] < 0 && p->deriv[0] < candidates[i].deriv[0]) {
      *p = candidates[i];
      flag = 1;
    } else if (p->deriv[0] > 0 && candidates[i].deriv[0] > 0 &&
               p->deriv[0] > candidates[i].deriv[0]) {
      *p = candidates[i];
      flag = 2;
    }
  }
  if (flag) {
    pnext->alpha = p->alpha - p->deriv[0]/p->deriv[1];
    solverEval(d, sc, ctx, pnext);
  }
  return flag;
}

// CGsearch :1204-1381 (LSresult and LSslope are statistics: not kept)
template <int S>
MJH_HD double solverSearch(const mjhipModel& m, const Lane<S>& d, const SolverScratch<S>& sc,
                           SolverCtx& ctx) {
  const int nv = ctx.nv;
  SolverPnt p0, p1, p2, pmid, p1next, p2next;
  ctx.LSiter = 0;
  const double snorm = sqrt(dot(sc.search, sc.search, nv));
  if (snorm < MINVAL) return 0;
  const double gtol = ctx.gtol_scale * snorm / ctx.scale;
  mulM(m, d, sc.Mv, sc.search);
  mulJacVec(m, d, sc.Jv, sc.search);
  solverPrepare(d, sc, ctx);
  p0.alpha = 0;
  solverEval(d, sc, ctx, &p0);
  p1.alpha = p0.alpha - p0.deriv[0]/p0.deriv[1];
  solverEval(d, sc, ctx, &p1);
  if (p0.cost < p1.cost) p1 = p0;
  if (fabs(p1.deriv[0]) < gtol) return p1.alpha;
  const int dir = (p1.deriv[0] < 0 ? +1 : -1);
  int p2update = 0;
  p2 = p1;
  while (p1.deriv[0]*dir <= -gtol && ctx.LSiter < ctx.ls_iterations) {
    p2 = p1;
    p2update = 1;
    p1.alpha -= p1.deriv[0]/p1.deriv[1];
    solverEval(d, sc, ctx, &p1);
    if (fabs(p1.deriv[0]) < gtol) return p1.alpha;
  }
  if (ctx.LSiter >= ctx.ls_iterations) return p1.alpha;
  if (!p2update) return p1.alpha;
  p2next = p1;
  p1next.alpha = p1.alpha - p1.deriv[0]/p1.deriv[1];
  solverEval(d, sc, ctx, &p1next);
  while (ctx.LSiter < ctx.ls_iterations) {
    pmid.alpha = 0.5*(p1.alpha + p2.alpha);
    solverEval(d, sc, ctx, &pmid);
    const SolverPnt candidates[3] = {p1next, p2next, pmid};
    double bestcost = 0;
    int bestind = -1;
    for (int i = 0; i < 3; i++) {
      if (fabs(candidates[i].deriv[0]) < gtol &&
          (bestind == -1 || candidates[i].cost < bestcost)) {
        bestcost = candidates[i].cost;
        bestind = i;
      }
    }
    if (bestind >= 0) return candidates[bestind].alpha;
    const int b1 = solverUpdateBracket(d, sc, ctx, &p1, candidates, &p1next);
    const int b2 = solverUpdateBracket(d, sc, ctx, &p2, candidates, &p2next);
    if (!b1 && !b2) return pmid.alpha;
  }
  if (p1.cost <= p2.cost && p1.cost < p0.cost) return p1.alpha;
  if (p2.cost <= p1.cost && p2.cost < p0.cost) return p2.alpha;
  return 0;
}

// MakeHessian :1480-1492 / FactorizeHessian :1501-1570, dense branches: D from efc_state,
// H = M + J'DJ in L, L = chol(H)
template <int S>
MJH_HD void solverFactorizeHessian(const mjhipModel& m, const Lane<S>& d,
                                   const SolverScratch<S>& sc, const SolverCtx& ctx) {
  for (int i = 0; i < ctx.nefc; i++) {
    sc.D[i] = d.efc_state[i] == CNSTRSTATE_QUADRATIC ? d.efc_D[i] : 0.0;
  }
  sqrMatTD(sc.L, d.efc_J, sc.D, ctx.nefc, ctx.nv);
  addMDense(m, d, sc.L);
  cholFactor(sc.L, ctx.nv, MINVAL);
}

// HessianIncremental :1654-1717, dense branch, no cones
template <int S>
MJH_HD void solverHessianIncremental(const mjhipModel& m, const Lane<S>& d,
                                     const SolverScratch<S>& sc, const SolverCtx& ctx,
                                     SolverTrace* tr) {
  const int nv = ctx.nv;
  for (int i = 0; i < ctx.nefc; i++) {
    int flag_update = -1;
    const int olds = sc.oldstate[i], news = d.efc_state[i];
    if (olds != CNSTRSTATE_QUADRATIC && news == CNSTRSTATE_QUADRATIC) {
      flag_update = 1;
    } else if (olds == CNSTRSTATE_QUADRATIC && news != CNSTRSTATE_QUADRATIC) {
      flag_update = 0;
    }
    if (flag_update != -1) {
      const double s = sqrt(d.efc_D[i]);
      for (int k = 0; k < nv; k++) sc.vec[k] = d.efc_J[i*nv + k]*s;
      const int rank = cholUpdate(sc.L, sc.vec, nv, flag_update);
      if (tr) {
        tr->nupdate++;
        tr->ndowndate += flag_update == 0;
      }
      if (rank < nv) {
        if (tr) tr->nrefactor++;
        solverFactorizeHessian(m, d, sc, ctx);
        return;
      }
    }
  }
}

// mj_solCGNewton :1722-1891 with flg_Newton = 1, island = -1; returns the iteration count
template <int S>
MJH_HD int solveNewton(const mjhipModel& m, const Lane<S>& d, const SolverScratch<S>& sc,
                       const SolverOpt& opt, SolverTrace* tr) {
  SolverCtx ctx;
  const int nv = m.nv, nefc = d.efc_count[0];
  ctx.nv = nv;
  ctx.nefc = nefc;
  ctx.ne = d.efc_count[1];
  ctx.nf = d.efc_count[2];
  ctx.ls_iterations = opt.ls_iterations;
  ctx.gtol_scale = opt.tolerance * opt.ls_tolerance;
  ctx.LSiter = 0;
  int iter = 0;
  mulM(m, d, sc.Ma, d.qacc);
  mulJacVec(m, d, sc.Jaref, d.qacc);
  subFrom(sc.Jaref, d.efc_aref, nefc);
  solverUpdateConstraint(m, d, sc, ctx);
  solverFactorizeHessian(m, d, sc, ctx);
  solverUpdateGradient(d, sc, ctx);
  scl(sc.search, sc.Mgrad, -1.0, nv);
  const double scale = 1 / (opt.meaninertia * max2(1, nv));
  ctx.scale = scale;
  while (iter < opt.iterations) {
    const double alpha = solverSearch(m, d, sc, ctx);
    if (tr && tr->nalpha < tr->alpha_cap) tr->alpha[tr->nalpha++] = alpha;
    if (alpha == 0) break;
    addToScl(d.qacc, sc.search, alpha, nv);
    addToScl(sc.Ma, sc.Mv, alpha, nv);
    addToScl(sc.Jaref, sc.Jv, alpha, nefc);
    for (int i = 0; i < nefc; i++) sc.oldstate[i] = d.efc_state[i];
    const double oldcost = ctx.cost;
    solverUpdateConstraint(m, d, sc, ctx);
    solverHessianIncremental(m, d, sc, ctx, tr);
    solverUpdateGradient(d, sc, ctx);
    const double improvement = scale * (oldcost - ctx.cost);
    const double gradient = scale * sqrt(dot(sc.grad, sc.grad, nv));
    iter++;
    if (improvement < opt.tolerance || gradient < opt.tolerance) break;
    scl(sc.search, sc.Mgrad, -1.0, nv);
  }
  if (tr) tr->cost = ctx.cost;
  return iter;
}

//---------------------------------- engine_forward.c -----------------------------------------

// warmstart :536-603, the non-PGS branch
template <int S>
MJH_HD void warmstart(const mjhipModel& m, const Lane<S>& d, const SolverScratch<S>& sc,
                      SolverTrace* tr) {
  const int nv = m.nv, nefc = d.efc_count[0];
  if (!(m.opt.disableflags & mjhipDSBL_WARMSTART)) {
    copy(d.qacc, sc.qacc_warmstart, nv);
    mulJacVec(m, d, d.jar, sc.qacc_warmstart);
    subFrom(d.jar, d.efc_aref, nefc);
    double cost_warmstart;
    constraintUpdate(m, d, d.jar, &cost_warmstart);
    mulM(m, d, sc.Ma, sc.qacc_warmstart);
    for (int i = 0; i < nv; i++) {
      cost_warmstart += 0.5*(sc.Ma[i] - d.qfrc_smooth[i])*(sc.qacc_warmstart[i] - d.qacc_smooth[i]);
    }
    double cost_smooth;
    constraintUpdate(m, d, sc.efc_b, &cost_smooth);
    const bool smooth = cost_warmstart > cost_smooth;
    if (smooth) copy(d.qacc, d.qacc_smooth, nv);
    if (tr) tr->warm = !smooth;
  } else {
    copy(d.qacc, d.qacc_smooth, nv);
    zero(d.efc_force, nefc);
    if (tr) tr->warm = 0;
  }
}

// mj_fwdConstraint :654-731 (Newton, no noslip); returns solver_niter[0]
template <int S>
MJH_HD int fwdConstraint(const mjhipModel& m, const Lane<S>& d, const SolverScratch<S>& sc,
                         const SolverOpt& opt, SolverTrace* tr = nullptr) {
  const int nv = m.nv, nefc = d.efc_count[0];
  zero(d.qfrc_constraint, nv);
  if (!nefc) {
    copy(d.qacc, d.qacc_smooth, nv);
    copy(sc.qacc_warmstart, d.qacc_smooth, nv);
    return 0;
  }
  mulJacVec(m, d, sc.efc_b, d.qacc_smooth);
  subFrom(sc.efc_b, d.efc_aref, nefc);
  warmstart(m, d, sc, tr);
  const int niter = solveNewton(m, d, sc, opt, tr);
  copy(sc.qacc_warmstart, d.qacc, nv);
  return niter;
}

// mj_forward :1054-1090 (skipsensor = 1): forwardSkip(mjhipSTAGE_NONE)'s stages up to
// qacc_smooth, then mj_fwdConstraint. An instance with a bad qpos / qvel / qacc_smooth or with
// a bit that collision or mj_makeConstraint raised (CNSTRFULL, an unsupported pair) is not
// solved: qacc = qacc_smooth. Constraint rows alone raise no bit.
template <int S, bool CONTACT = true>
MJH_HD int forward(const mjhipModel& m, const Lane<S>& d, const SolverScratch<S>& sc,
                   const SolverOpt& opt, int* niter, SolverTrace* tr = nullptr) {
  const int nv = m.nv;
  int status = 0;
  *niter = 0;
  for (int i = 0; i < m.nq; i++) status |= isBad(d.qpos[i]) ? MJHIP_INST_BADQPOS : 0;
  for (int i = 0; i < nv; i++) status |= isBad(d.qvel[i]) ? MJHIP_INST_BADQVEL : 0;
  invPosition<S, CONTACT>(m, d, &status);
  invVelocity(m, d);
  fwdActuation(m, d);
  for (int i = 0; i < nv; i++) d.qfrc_smooth[i] = d.qfrc_passive[i] - d.qfrc_bias[i];
  addTo(d.qfrc_smooth, d.qfrc_applied, nv);
  addTo(d.qfrc_smooth, d.qfrc_actuator, nv);
  xfrcAccumulate(m, d, d.qfrc_smooth);
  copy(d.qacc_smooth, d.qfrc_smooth, nv);
  solveM(m, d, d.qacc_smooth);
  for (int i = 0; i < nv; i++) status |= isBad(d.qacc_smooth[i]) ? MJHIP_INST_BADQACC : 0;
  if (status) {
    copy(d.qacc, d.qacc_smooth, nv);
    zero(d.qfrc_constraint, nv);
    return status;
  }
  *niter = fwdConstraint(m, d, sc, opt, tr);
  for (int i = 0; i < nv; i++) status |= isBad(d.qacc[i]) ? MJHIP_INST_BADQACC : 0;
  return status;
}

}  // namespace mjh
