"""mj_fwdConstraint with the Newton solver restated on Python floats in the reference's own
operation order, for tests/test_solver_cpu.py to compare the host build of csrc/solver.h with,
bit for bit (tests/step_ref.py does the same for the integrators).

The inputs are what the position and velocity stages leave: a `Problem` holds the rows
(efc_J, efc_D, efc_R, efc_aref, efc_frictionloss, ne, nf), qM with the model's dof tree,
qfrc_smooth and qacc_smooth. Everything the solver itself computes is computed here.
Pyramidal and frictionless rows only (no elliptic cone), dense Jacobian, island = -1."""
import math

MINVAL = 1e-15
SATISFIED, QUADRATIC, LINEARNEG, LINEARPOS = 0, 1, 2, 3
DSBL_WARMSTART = 1 << 8


def dot(a, b, n, ao=0, bo=0):                    # mju_dot engine_util_blas.c:680-741
  r0 = r1 = r2 = r3 = 0.0
  i = 0
  while i <= n - 4:
    r0 += a[ao+i]*b[bo+i]
    r1 += a[ao+i+1]*b[bo+i+1]
    r2 += a[ao+i+2]*b[bo+i+2]
    r3 += a[ao+i+3]*b[bo+i+3]
    i += 4
  res = (r0 + r2) + (r1 + r3)
  k = n - i
  if k == 3:
    res += a[ao+i]*b[bo+i] + a[ao+i+1]*b[bo+i+1] + a[ao+i+2]*b[bo+i+2]
  elif k == 2:
    res += a[ao+i]*b[bo+i] + a[ao+i+1]*b[bo+i+1]
  elif k == 1:
    res += a[ao+i]*b[bo+i]
  return res


def chol_factor(mat, n, mindiag):                # engine_util_solve.c:32-61
  rank = n
  for j in range(n):
    tmp = mat[j*(n+1)]
    if j:
      tmp -= dot(mat, mat, j, j*n, j*n)
    if tmp < mindiag:
      tmp = mindiag
      rank -= 1
    mat[j*(n+1)] = math.sqrt(tmp)
    tmp = 1/mat[j*(n+1)]
    for i in range(j+1, n):
      mat[i*n+j] = (mat[i*n+j] - dot(mat, mat, j, i*n, j*n)) * tmp
  return rank


def chol_solve(mat, vec, n):                     # engine_util_solve.c:66-92
  res = list(vec)
  for i in range(n):
    if i:
      res[i] -= dot(mat, res, i, i*n, 0)
    res[i] /= mat[i*(n+1)]
  for i in range(n-1, -1, -1):
    if i < n-1:
      for j in range(i+1, n):
        res[i] -= mat[j*n+i] * res[j]
    res[i] /= mat[i*(n+1)]
  return res


def chol_update(mat, x, n, flg_plus):            # engine_util_solve.c:97-137
  rank = n
  for k in range(n):
    if x[k]:
      Lkk = mat[k*(n+1)]
      tmp = Lkk*Lkk + (x[k]*x[k] if flg_plus else -x[k]*x[k])
      if tmp < MINVAL:
        tmp = MINVAL
        rank -= 1
      r = math.sqrt(tmp)
      c = r / Lkk
      cinv = 1 / c
      s = x[k] / Lkk
      mat[k*(n+1)] = r
      if flg_plus:
        for i in range(k+1, n):
          mat[i*n+k] = (mat[i*n+k] + s*x[i])*cinv
      else:
        for i in range(k+1, n):
          mat[i*n+k] = (mat[i*n+k] - s*x[i])*cinv
      for i in range(k+1, n):
        x[i] = c*x[i] - s*mat[i*n+k]
  return rank


def sqr_mat_td(mat, diag, nr, nc):               # engine_util_blas.c:848-879
  res = [0.0]*(nc*nc)
  for j in range(nr):
    if diag[j]:
      for i in range(nc):
        tmp = mat[j*nc+i]
        if tmp:
          s = tmp*diag[j]
          for k in range(i+1):
            res[i*nc+k] += mat[j*nc+k]*s
  for i in range(nc):
    for j in range(i+1, nc):
      res[i*nc+j] = res[j*nc+i]
  return res


class Problem:
  """One instance's convex problem. J: nefc x nv row-major list."""

  def __init__(self, m, qM, qfrc_smooth, qacc_smooth, J, D, R, aref, frictionloss, ne, nf):
    f = lambda a: [float(x) for x in a]
    self.nv = int(m.nv)
    self.dof_Madr = [int(x) for x in m.dof_Madr]
    self.dof_parentid = [int(x) for x in m.dof_parentid]
    self.dof_simplenum = [int(x) for x in m.dof_simplenum]
    self.disableflags = int(m.opt["disableflags"])
    self.qM, self.qfrc_smooth, self.qacc_smooth = f(qM), f(qfrc_smooth), f(qacc_smooth)
    self.J, self.D, self.R, self.aref = f(J), f(D), f(R), f(aref)
    self.floss = f(frictionloss)
    self.nefc, self.ne, self.nf = len(self.D), int(ne), int(nf)

  def mul_m(self, vec):                          # mj_mulM engine_support.c:966-1017
    nv = self.nv
    res = [0.0]*nv
    for i in range(nv):
      adr = self.dof_Madr[i]
      res[i] = self.qM[adr]*vec[i]
      if self.dof_simplenum[i]:
        continue
      j = self.dof_parentid[i]
      while j >= 0:
        adr += 1
        res[i] += self.qM[adr]*vec[j]
        res[j] += self.qM[adr]*vec[i]
        j = self.dof_parentid[j]
    return res

  def add_m_dense(self, dst):                    # mj_addMDense engine_support.c:1164-1187
    nv = self.nv
    for i in range(nv):
      adr = self.dof_Madr[i]
      j = i
      while j >= 0:
        dst[i*nv+j] += self.qM[adr]
        if j < i:
          dst[j*nv+i] += self.qM[adr]
        if self.dof_simplenum[i]:
          break
        j = self.dof_parentid[j]
        adr += 1

  def mul_jac_vec(self, vec):                    # mj_mulJacVec, dense
    return [dot(self.J, vec, self.nv, r*self.nv, 0) for r in range(self.nefc)]

  def mul_jac_t_vec(self, vec):                  # mju_mulMatTVec engine_util_blas.c:756-766
    nv = self.nv
    res = [0.0]*nv
    for r in range(self.nefc):
      tmp = vec[r]
      if tmp:
        for k in range(nv):
          res[k] += self.J[r*nv+k]*tmp
    return res


def constraint_update(p, jar):
  """mj_constraintUpdate_island engine_core_constraint.c:2387-2549 (island < 0, with the
  cost): (efc_force, efc_state, qfrc_constraint, cost)."""
  D, R, floss = p.D, p.R, p.floss
  force = [-D[i]*jar[i] for i in range(p.nefc)]
  state = [0]*p.nefc
  s = 0.0
  for i in range(p.nefc):
    if i < p.ne:
      s += 0.5*D[i]*jar[i]*jar[i]
      state[i] = QUADRATIC
      continue
    if i < p.ne + p.nf:
      if jar[i] <= -R[i]*floss[i]:
        s += -0.5*R[i]*floss[i]*floss[i] - floss[i]*jar[i]
        force[i] = floss[i]
        state[i] = LINEARNEG
      elif jar[i] >= R[i]*floss[i]:
        s += -0.5*R[i]*floss[i]*floss[i] + floss[i]*jar[i]
        force[i] = -floss[i]
        state[i] = LINEARPOS
      else:
        s += 0.5*D[i]*jar[i]*jar[i]
        state[i] = QUADRATIC
      continue
    if jar[i] >= 0:
      force[i] = 0.0
      state[i] = SATISFIED
    else:
      s += 0.5*D[i]*jar[i]*jar[i]
      state[i] = QUADRATIC
  return force, state, p.mul_jac_t_vec(force), s


class _Ctx:
  pass


def _update_constraint(p, c):                    # CGupdateConstraint engine_solver.c:869-895
  c.force, c.state, c.qfrc_constraint, c.cost = constraint_update(p, c.Jaref)
  gauss = 0.0
  for i in range(p.nv):
    gauss += 0.5*(c.Ma[i] - p.qfrc_smooth[i])*(c.qacc[i] - p.qacc_smooth[i])
  c.quadGauss = [gauss, 0.0, 0.0]
  c.cost += gauss


def _update_gradient(p, c):                      # CGupdateGradient :900-926 (Newton, dense)
  c.grad = [c.Ma[i] - p.qfrc_smooth[i] - c.qfrc_constraint[i] for i in range(p.nv)]
  c.Mgrad = chol_solve(c.L, c.grad, p.nv)


def _prepare(p, c):                              # CGprepare :931-1016
  nv, v = p.nv, c.search
  v_dot_smooth = dot(p.qfrc_smooth, v, nv)
  c.quadGauss[1] = dot(v, c.Ma, nv) - v_dot_smooth
  c.quadGauss[2] = 0.5*dot(v, c.Mv, nv)
  c.quad = []
  for i in range(p.nefc):
    Jv, Jaref, D = c.Jv[i], c.Jaref[i], p.D[i]
    DJ0 = D*Jaref
    q0 = Jaref*DJ0
    q1 = Jv*DJ0
    q2 = Jv*D*Jv
    q0 *= 0.5
    q2 *= 0.5
    c.quad.append((q0, q1, q2))


def _eval(p, c, alpha):                          # CGeval :1031-1170 -> (alpha, cost, d0, d1)
  qt = list(c.quadGauss)

  def add(q):
    qt[0] += q[0]; qt[1] += q[1]; qt[2] += q[2]

  for i in range(p.nefc):
    if i < p.ne:
      add(c.quad[i])
      continue
    if i < p.ne + p.nf:
      start, dr = c.Jaref[i], c.Jv[i]
      x = start + alpha*dr
      f = p.floss[i]
      Rf = p.R[i]*f
      if -Rf < x and x < Rf:
        add(c.quad[i])
      elif x <= -Rf:
        add((f*(-0.5*Rf-start), -f*dr, 0.0))
      else:
        add((f*(-0.5*Rf+start), f*dr, 0.0))
      continue
    x = c.Jaref[i] + alpha*c.Jv[i]
    if x < 0:
      add(c.quad[i])
  cost = 0.0
  cost += alpha*alpha*qt[2] + alpha*qt[1] + qt[0]
  d0 = 0.0
  d0 += 2*alpha*qt[2] + qt[1]
  d1 = 0.0
  d1 += 2*qt[2]
  if d1 <= 0:
    d1 = MINVAL
  c.LSiter += 1
  return [alpha, cost, d0, d1]


def _update_bracket(p, c, pt, cand):             # updateBracket :1173-1201
  flag = 0
  for i in range(3):
    if pt[2] < 0 and cand[i][2] < 0 and pt[2] < cand[i][2]:
      pt[:] = cand[i]
      flag = 1
    elif pt[2] > 0 and cand[i][2] > 0 and pt[2] > cand[i][2]:
      pt[:] = cand[i]
      flag = 2
  nxt = None
  if flag:
    nxt = _eval(p, c, pt[0] - pt[2]/pt[3])
  return flag, nxt


def _search(p, c, o):                            # CGsearch :1204-1381
  nv = p.nv
  c.LSiter = 0
  snorm = math.sqrt(dot(c.search, c.search, nv))
  if snorm < MINVAL:
    return 0.0
  gtol = o["tolerance"] * o["ls_tolerance"] * snorm / c.scale
  c.Mv = p.mul_m(c.search)
  c.Jv = p.mul_jac_vec(c.search)
  _prepare(p, c)
  p0 = _eval(p, c, 0.0)
  p1 = _eval(p, c, p0[0] - p0[2]/p0[3])
  if p0[1] < p1[1]:
    p1 = list(p0)
  if abs(p1[2]) < gtol:
    return p1[0]
  dr = 1 if p1[2] < 0 else -1
  p2update = 0
  p2 = list(p1)
  while p1[2]*dr <= -gtol and c.LSiter < o["ls_iterations"]:
    p2 = list(p1)
    p2update = 1
    p1 = _eval(p, c, p1[0] - p1[2]/p1[3])
    if abs(p1[2]) < gtol:
      return p1[0]
  if c.LSiter >= o["ls_iterations"]:
    return p1[0]
  if not p2update:
    return p1[0]
  p2next = list(p1)
  p1next = _eval(p, c, p1[0] - p1[2]/p1[3])
  while c.LSiter < o["ls_iterations"]:
    pmid = _eval(p, c, 0.5*(p1[0] + p2[0]))
    cand = [list(p1next), list(p2next), list(pmid)]
    bestcost, bestind = 0.0, -1
    for i in range(3):
      if abs(cand[i][2]) < gtol and (bestind == -1 or cand[i][1] < bestcost):
        bestcost, bestind = cand[i][1], i
    if bestind >= 0:
      return cand[bestind][0]
    b1, n1 = _update_bracket(p, c, p1, cand)
    if b1:
      p1next = n1
    b2, n2 = _update_bracket(p, c, p2, cand)
    if b2:
      p2next = n2
    if not b1 and not b2:
      return pmid[0]
  if p1[1] <= p2[1] and p1[1] < p0[1]:
    return p1[0]
  if p2[1] <= p1[1] and p2[1] < p0[1]:
    return p2[0]
  return 0.0


def _factorize(p, c):                            # MakeHessian / FactorizeHessian, dense
  Dq = [p.D[i] if c.state[i] == QUADRATIC else 0.0 for i in range(p.nefc)]
  c.L = sqr_mat_td(p.J, Dq, p.nefc, p.nv)
  p.add_m_dense(c.L)
  chol_factor(c.L, p.nv, MINVAL)


def _hessian_incremental(p, c, oldstate):        # HessianIncremental :1654-1717, dense
  nv = p.nv
  for i in range(p.nefc):
    flag = -1
    if oldstate[i] != QUADRATIC and c.state[i] == QUADRATIC:
      flag = 1
    elif oldstate[i] == QUADRATIC and c.state[i] != QUADRATIC:
      flag = 0
    if flag != -1:
      s = math.sqrt(p.D[i])
      vec = [p.J[i*nv+k]*s for k in range(nv)]
      rank = chol_update(c.L, vec, nv, flag)
      c.nupdate += 1
      c.ndowndate += flag == 0
      if rank < nv:
        c.nrefactor += 1
        _factorize(p, c)
        return


def solve_newton(p, qacc, o):
  """mj_solCGNewton engine_solver.c:1722-1891 (flg_Newton = 1, island = -1) from qacc."""
  c = _Ctx()
  nv, nefc = p.nv, p.nefc
  c.qacc = list(qacc)
  c.nupdate = c.ndowndate = c.nrefactor = 0
  c.LSiter = 0
  c.alpha = []
  c.Ma = p.mul_m(c.qacc)
  c.Jaref = p.mul_jac_vec(c.qacc)
  for i in range(nefc):
    c.Jaref[i] -= p.aref[i]
  _update_constraint(p, c)
  _factorize(p, c)
  _update_gradient(p, c)
  c.search = [x*-1.0 for x in c.Mgrad]
  scale = 1 / (o["meaninertia"] * max(1, nv))
  c.scale = scale
  it = 0
  while it < o["iterations"]:
    alpha = _search(p, c, o)
    c.alpha.append(alpha)
    if alpha == 0:
      break
    for i in range(nv):
      c.qacc[i] += c.search[i]*alpha
    for i in range(nv):
      c.Ma[i] += c.Mv[i]*alpha
    for i in range(nefc):
      c.Jaref[i] += c.Jv[i]*alpha
    oldstate = list(c.state)
    oldcost = c.cost
    _update_constraint(p, c)
    _hessian_incremental(p, c, oldstate)
    _update_gradient(p, c)
    improvement = scale * (oldcost - c.cost)
    gradient = scale * math.sqrt(dot(c.grad, c.grad, nv))
    it += 1
    if improvement < o["tolerance"] or gradient < o["tolerance"]:
      break
    c.search = [x*-1.0 for x in c.Mgrad]
  c.niter = it
  return c


def fwd_constraint(p, qacc_warmstart, o):
  """mj_fwdConstraint engine_forward.c:654-731 with warmstart :536-603 (non-PGS). Returns a
  dict shaped like SolverCPU.forward_solve's."""
  nv, nefc = p.nv, p.nefc
  if not nefc:
    return dict(qacc=list(p.qacc_smooth), qfrc_constraint=[0.0]*nv, efc_force=[], efc_state=[],
                niter=0, cost=0.0, alpha=[], qacc_warmstart=list(p.qacc_smooth), warm=0,
                nupdate=0, ndowndate=0, nrefactor=0, jar=[])
  efc_b = p.mul_jac_vec(p.qacc_smooth)
  for i in range(nefc):
    efc_b[i] -= p.aref[i]
  if not (p.disableflags & DSBL_WARMSTART):
    jar = p.mul_jac_vec(qacc_warmstart)
    for i in range(nefc):
      jar[i] -= p.aref[i]
    cost_warmstart = constraint_update(p, jar)[3]
    Ma = p.mul_m(qacc_warmstart)
    for i in range(nv):
      cost_warmstart += 0.5*(Ma[i]-p.qfrc_smooth[i])*(qacc_warmstart[i]-p.qacc_smooth[i])
    cost_smooth = constraint_update(p, efc_b)[3]
    warm = not cost_warmstart > cost_smooth
    qacc = list(qacc_warmstart) if warm else list(p.qacc_smooth)
  else:
    warm = False
    qacc = list(p.qacc_smooth)
  c = solve_newton(p, qacc, o)
  return dict(qacc=c.qacc, qfrc_constraint=c.qfrc_constraint, efc_force=c.force,
              efc_state=c.state, niter=c.niter, cost=c.cost, alpha=c.alpha,
              qacc_warmstart=list(c.qacc), warm=int(warm), nupdate=c.nupdate,
              ndowndate=c.ndowndate, nrefactor=c.nrefactor, jar=c.Jaref)
