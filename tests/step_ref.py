"""The reference's integrators restated on Python floats in its own operation order, for
tests/test_step_cpu.py to compare the host build of csrc/step.h with, bit for bit
(tests/actuation_ref.py does the same for the actuator models).

A `fwd` object supplies what mj_forward leaves in mjData for the current state: after
fwd.forward(qpos, qvel, act) it has qM, qfrc_smooth, qacc, act_dot (lists of floats) and
qderiv(flg_bias) -> {(row, col): value} on the D sparsity (mjd_smooth_vel). Everything the
integrators themselves compute is computed here."""
import math

from actuation_ref import next_activation

MINVAL = 1e-15
FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3
EULER, RK4, IMPLICIT, IMPLICITFAST = 0, 1, 2, 3
DSBL_ACTUATION, DSBL_EULERDAMP = 1 << 10, 1 << 14


def _flat(a):
  return [x for row in a for x in (row if hasattr(row, "__len__") else [row])]


def _ints(a):
  return [int(x) for x in a]


def normalize3(v):                               # engine_util_blas.c:123-140
  norm = math.sqrt(v[0]*v[0] + v[1]*v[1] + v[2]*v[2])
  if norm < MINVAL:
    v[:] = [1.0, 0.0, 0.0]
  else:
    inv = 1/norm
    v[0] *= inv; v[1] *= inv; v[2] *= inv
  return norm


def normalize4(v):                               # engine_util_blas.c:269-285
  norm = math.sqrt(v[0]*v[0] + v[1]*v[1] + v[2]*v[2] + v[3]*v[3])
  if norm < MINVAL:
    v[:] = [1.0, 0.0, 0.0, 0.0]
  elif abs(norm - 1) > MINVAL:
    inv = 1/norm
    v[0] *= inv; v[1] *= inv; v[2] *= inv; v[3] *= inv
  return norm


def quat_integrate(quat, vel, scale):            # engine_util_spatial.c:241-250
  tmp = [vel[0], vel[1], vel[2]]
  angle = scale * normalize3(tmp)
  if angle == 0:                                 # mju_axisAngle2Quat :97-114
    qr = [1.0, 0.0, 0.0, 0.0]
  else:
    s = math.sin(angle*0.5)
    qr = [math.cos(angle*0.5), tmp[0]*s, tmp[1]*s, tmp[2]*s]
  qa = list(quat)
  normalize4(qa)
  return [qa[0]*qr[0] - qa[1]*qr[1] - qa[2]*qr[2] - qa[3]*qr[3],   # mju_mulQuat :62-74
          qa[0]*qr[1] + qa[1]*qr[0] + qa[2]*qr[3] - qa[3]*qr[2],
          qa[0]*qr[2] - qa[1]*qr[3] + qa[2]*qr[0] + qa[3]*qr[1],
          qa[0]*qr[3] + qa[1]*qr[2] - qa[2]*qr[1] + qa[3]*qr[0]]


def integrate_pos(m, qpos, qvel, dt):            # engine_support.c:1518-1548, in place
  for j in range(int(m.njnt)):
    padr, vadr, t = int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j]), int(m.jnt_type[j])
    if t == FREE:
      for i in range(3):
        qpos[padr+i] += dt * qvel[vadr+i]
      padr += 3
      vadr += 3
    if t in (FREE, BALL):
      qpos[padr:padr+4] = quat_integrate(qpos[padr:padr+4], qvel[vadr:vadr+3], dt)
    else:
      qpos[padr] += dt * qvel[vadr]


def advance(m, qpos, qvel, act, act_dot, qacc, qvel_given=None):   # engine_forward.c:738-776
  h = float(m.opt["timestep"])
  if int(m.na) and not (int(m.opt["disableflags"]) & DSBL_ACTUATION):
    for i in range(int(m.nu)):
      adr = int(m.actuator_actadr[i])
      for j in range(adr, adr + int(m.actuator_actnum[i])):
        act[j] = next_activation(int(m.actuator_dyntype[i]),
                                 float(_flat(m.actuator_dynprm)[10*i]), h,
                                 int(m.actuator_actlimited[i]),
                                 [float(x) for x in _flat(m.actuator_actrange)[2*i:2*i+2]],
                                 act[j], act_dot[j])
  for i in range(int(m.nv)):                     # mju_addToScl
    qvel[i] += qacc[i]*h
  integrate_pos(m, qpos, qvel if qvel_given is None else qvel_given, h)


def dot_sparse(v1, a1, v2, nnz, ind, ai):        # engine_util_sparse.h:115-160
  i, r = 0, [0.0, 0.0, 0.0, 0.0]
  while i <= nnz - 4:
    for k in range(4):
      r[k] += v1[a1+i+k]*v2[ind[ai+i+k]]
    i += 4
  res = (r[0] + r[2]) + (r[1] + r[3])
  while i < nnz:
    res += v1[a1+i]*v2[ind[ai+i]]
    i += 1
  return res


def factor_i(m, mat):                            # engine_core_smooth.c:1483-1511, in place
  nv = int(m.nv)
  rownnz, rowadr, colind = _ints(m.C_rownnz), _ints(m.C_rowadr), _ints(m.C_colind)
  diaginv = [0.0]*nv
  for k in range(nv-1, -1, -1):
    ak = rowadr[k]
    dk = ak + rownnz[k] - 1
    inv = 1 / mat[dk]
    diaginv[k] = inv
    if int(m.dof_simplenum[k]):
      continue
    for adr in range(dk-1, ak-1, -1):
      tmp = mat[adr] * inv
      i = colind[adr]
      for c in range(rownnz[i]):                 # mju_addToScl(mat+rowadr[i], mat+rowadr_k, -tmp)
        mat[rowadr[i]+c] += mat[ak+c] * -tmp
      mat[adr] = tmp
  return diaginv


def solve_ld(m, x, ld, diaginv):                 # engine_core_smooth.c:1629-1707, n = 1
  nv = int(m.nv)
  rownnz, rowadr, colind = _ints(m.C_rownnz), _ints(m.C_rowadr), _ints(m.C_colind)
  simple = _ints(m.dof_simplenum)
  for i in range(nv-1, 0, -1):
    if simple[i]:
      continue
    xi = x[i]
    if xi:
      for adr in range(rowadr[i], rowadr[i] + rownnz[i] - 1):
        x[colind[adr]] -= ld[adr] * xi
  for i in range(nv):
    x[i] *= diaginv[i]
  i = 1
  while i < nv:
    if simple[i]:
      i += simple[i]                             # i += diagnum-1; continue; i++
      continue
    d = rownnz[i] - 1
    if d > 0:
      x[i] -= dot_sparse(ld, rowadr[i], x, d, colind, rowadr[i])
    i += 1


def factor_lu_sparse(m, lu):                     # engine_util_solve.c:571-643, in place
  n = int(m.nv)
  rownnz, rowadr, colind = _ints(m.D_rownnz), _ints(m.D_rowadr), _ints(m.D_colind)
  rem = list(rownnz)
  for i in range(n-1, -1, -1):
    ii = rowadr[i] + rem[i] - 1
    rem[i] -= 1
    assert colind[ii] == i
    for j in range(i-1, -1, -1):
      ji = rowadr[j] + rem[j] - 1
      if colind[ji] == i:
        rem[j] -= 1
        lu[ji] = lu[ji] / lu[ii]
        luji = lu[ji]
        ic, jc = rowadr[i], rowadr[j]
        while jc < rowadr[j] + rem[j]:
          if colind[ic] == colind[jc]:
            lu[jc] -= lu[ic] * luji
            jc += 1
            ic += 1
          elif colind[ic] > colind[jc]:
            jc += 1
          else:
            raise AssertionError("requires fill-in")


def solve_lu_sparse(m, lu, vec):                 # engine_util_solve.c:648-675
  n = int(m.nv)
  rownnz, rowadr, colind = _ints(m.D_rownnz), _ints(m.D_rowadr), _ints(m.D_colind)
  diag = [colind[rowadr[i]:rowadr[i]+rownnz[i]].index(i) for i in range(n)]   # D_diag
  res = [0.0]*n
  for i in range(n-1, -1, -1):
    res[i] = vec[i]
    d1 = diag[i] + 1
    nnz = rownnz[i] - d1
    if nnz > 0:
      res[i] -= dot_sparse(lu, rowadr[i]+d1, res, nnz, colind, rowadr[i]+d1)
  for i in range(n):
    d = diag[i]
    if d > 0:
      res[i] -= dot_sparse(lu, rowadr[i], res, d, colind, rowadr[i])
    res[i] /= lu[rowadr[i] + d]
  return res


def _qfrc(fwd, nv):                              # qfrc_smooth + qfrc_constraint (0: no rows)
  return [fwd.qfrc_smooth[i] + 0.0 for i in range(nv)]


def euler(m, fwd, qpos, qvel, act):              # mj_EulerSkip engine_forward.c:779-830
  nv, h = int(m.nv), float(m.opt["timestep"])
  damp = [float(x) for x in m.dof_damping]
  damping = (not (int(m.opt["disableflags"]) & DSBL_EULERDAMP)) and any(d > 0 for d in damp)
  if not damping:
    qacc = list(fwd.qacc)
  else:
    qh = [fwd.qM[int(k)] for k in m.mapM2C]
    for i in range(nv):
      qh[int(m.C_rowadr[i]) + int(m.C_rownnz[i]) - 1] += h * damp[i]
    dinv = factor_i(m, qh)
    qacc = _qfrc(fwd, nv)
    solve_ld(m, qacc, qh, dinv)
  advance(m, qpos, qvel, act, fwd.act_dot, qacc)


def implicit(m, fwd, qpos, qvel, act):           # mj_implicitSkip engine_forward.c:948-1021
  nv, h = int(m.nv), float(m.opt["timestep"])
  qfrc = _qfrc(fwd, nv)
  rowadr, rownnz, colind = _ints(m.D_rowadr), _ints(m.D_rownnz), _ints(m.D_colind)
  if int(m.opt["integrator"]) == IMPLICIT:
    qd = fwd.qderiv(1)
    lu = [fwd.qM[int(k)] for k in m.mapM2D]
    for r in range(nv):                          # mju_addToScl(qLU, qDeriv, -h, nD)
      for a in range(rowadr[r], rowadr[r] + rownnz[r]):
        lu[a] += qd[(r, colind[a])] * -h
    factor_lu_sparse(m, lu)
    qacc = solve_lu_sparse(m, lu, qfrc)
  else:
    qd = fwd.qderiv(0)
    # MhB[i] = qM[i] + qDeriv[mapD2M[i]] * -h over M's layout: dof r, then its ancestors
    mhb = [0.0]*int(m.nM)
    for r in range(nv):
      adr, c = int(m.dof_Madr[r]), r
      while c >= 0:
        mhb[adr] = fwd.qM[adr] + qd[(r, c)] * -h
        adr += 1
        c = int(m.dof_parentid[c])
    qh = [mhb[int(k)] for k in m.mapM2C]
    dinv = factor_i(m, qh)
    qacc = list(qfrc)
    solve_ld(m, qacc, qh, dinv)
  advance(m, qpos, qvel, act, fwd.act_dot, qacc)


def rk4(m, fwd, qpos, qvel, act):                # mj_RungeKutta engine_forward.c:855-943, N = 4
  A = [0.5, 0, 0, 0, 0.5, 0, 0, 0, 1]
  B = [1.0/6.0, 1.0/3.0, 1.0/3.0, 1.0/6.0]
  nq, nv, na, N = int(m.nq), int(m.nv), int(m.na), 4
  h = float(m.opt["timestep"])
  X = [list(qpos) + list(qvel) + list(act)]
  F = [list(fwd.qacc) + list(fwd.act_dot)]
  for i in range(1, N):
    dX = [0.0]*(2*nv + na)
    for j in range(i):
      a = A[(i-1)*(N-1)+j]
      for k in range(nv):
        dX[k] += X[j][nq+k]*a
      for k in range(nv + na):
        dX[nv+k] += F[j][k]*a
    Xi = list(X[0])
    pos = Xi[:nq]
    integrate_pos(m, pos, dX, h)
    Xi[:nq] = pos
    for k in range(nv + na):
      Xi[nq+k] += dX[nv+k]*h
    X.append(Xi)
    fwd.forward(Xi[:nq], Xi[nq:nq+nv], Xi[nq+nv:])
    F.append(list(fwd.qacc) + list(fwd.act_dot))
  dX = [0.0]*(2*nv + na)
  for j in range(N):
    for k in range(nv):
      dX[k] += X[j][nq+k]*B[j]
    for k in range(nv + na):
      dX[nv+k] += F[j][k]*B[j]
  qpos[:], qvel[:], act[:] = X[0][:nq], X[0][nq:nq+nv], X[0][nq+nv:]
  advance(m, qpos, qvel, act, dX[2*nv:], dX[nv:2*nv], qvel_given=dX[:nv])


def step(m, fwd, qpos, qvel, act):
  """mj_step (engine_forward.c:1134-1168) on lists of floats, in place."""
  fwd.forward(qpos, qvel, act)
  integ = int(m.opt["integrator"])
  {EULER: euler, RK4: rk4, IMPLICIT: implicit, IMPLICITFAST: implicit}[integ](m, fwd, qpos, qvel,
                                                                              act)
