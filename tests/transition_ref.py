"""mjd_stepFD / mjd_transitionFD (engine_derivative_fd.c:306-595) restated on Python floats in
the reference's own order, on top of tests/step_ref.py, for tests/test_transition_cpu.py to
compare the host build of csrc/transition.h with, bit for bit.

A `fwd` object supplies what mj_forward leaves in mjData: after fwd.forward(qpos, qvel, act,
ctrl) it has qM, qfrc_smooth, qacc, act_dot and qderiv(flg_bias), as step_ref's does (its
forward() returns the status bits of the state, 0 for a constraint-free one). A skipped
stage recomputes nothing that differs: the position stage reads qpos alone and the velocity
stage qpos and qvel, which the evaluations that skip them leave as the centre's, so the whole
forward on the perturbed state gives the bits mj_forwardSkip gives. What skipping does change
is skipfactor: the factor of the Euler / implicit solve is the one the last unskipped
factorization left, which in mjd_stepFD's order (ctrl, act, qvel, then qpos) is always the
centre's. `refactor=True` restates the routine without that reuse."""
import math

import step_ref
from step_ref import EULER, IMPLICIT, IMPLICITFAST, RK4, FREE, BALL, DSBL_EULERDAMP

STAGE_NONE, STAGE_POS, STAGE_VEL = 0, 1, 2
PI = 3.14159265358979323846


def _euler_skip(m, fwd, qpos, qvel, act, skipfactor, fac):   # engine_forward.c:779-830
  nv, h = int(m.nv), float(m.opt["timestep"])
  damp = [float(x) for x in m.dof_damping]
  damping = (not (int(m.opt["disableflags"]) & DSBL_EULERDAMP)) and any(d > 0 for d in damp)
  if not damping:
    qacc = list(fwd.qacc)
  else:
    if not skipfactor:
      qh = [fwd.qM[int(k)] for k in m.mapM2C]
      for i in range(nv):
        qh[int(m.C_rowadr[i]) + int(m.C_rownnz[i]) - 1] += h * damp[i]
      fac["qH"], fac["qHDiagInv"] = qh, step_ref.factor_i(m, qh)
    qacc = step_ref._qfrc(fwd, nv)
    step_ref.solve_ld(m, qacc, fac["qH"], fac["qHDiagInv"])
  step_ref.advance(m, qpos, qvel, act, fwd.act_dot, qacc)


def _implicit_skip(m, fwd, qpos, qvel, act, skipfactor, fac):   # engine_forward.c:948-1021
  nv, h = int(m.nv), float(m.opt["timestep"])
  qfrc = step_ref._qfrc(fwd, nv)
  rowadr, rownnz, colind = (step_ref._ints(m.D_rowadr), step_ref._ints(m.D_rownnz),
                            step_ref._ints(m.D_colind))
  if int(m.opt["integrator"]) == IMPLICIT:
    if not skipfactor:
      qd = fwd.qderiv(1)
      lu = [fwd.qM[int(k)] for k in m.mapM2D]
      for r in range(nv):
        for a in range(rowadr[r], rowadr[r] + rownnz[r]):
          lu[a] += qd[(r, colind[a])] * -h
      step_ref.factor_lu_sparse(m, lu)
      fac["qLU"] = lu
    qacc = step_ref.solve_lu_sparse(m, fac["qLU"], qfrc)
  else:
    if not skipfactor:
      qd = fwd.qderiv(0)
      mhb = [0.0]*int(m.nM)
      for r in range(nv):
        adr, c = int(m.dof_Madr[r]), r
        while c >= 0:
          mhb[adr] = fwd.qM[adr] + qd[(r, c)] * -h
          adr += 1
          c = int(m.dof_parentid[c])
      qh = [mhb[int(k)] for k in m.mapM2C]
      fac["qH"], fac["qHDiagInv"] = qh, step_ref.factor_i(m, qh)
    qacc = list(qfrc)
    step_ref.solve_ld(m, qacc, fac["qH"], fac["qHDiagInv"])
  step_ref.advance(m, qpos, qvel, act, fwd.act_dot, qacc)


def step_skip(m, fwd, qpos, qvel, act, ctrl, skipstage, fac, refactor=False):
  """mj_stepSkip :120-155 in place; returns the forward's status bits (nonzero: no step)."""
  st = fwd.forward(qpos, qvel, act, ctrl)
  if st:
    return st
  integ = int(m.opt["integrator"])
  if integ == EULER:
    _euler_skip(m, fwd, qpos, qvel, act, skipstage >= STAGE_POS and not refactor, fac)
  elif integ in (IMPLICIT, IMPLICITFAST):
    _implicit_skip(m, fwd, qpos, qvel, act, skipstage >= STAGE_VEL and not refactor, fac)
  else:
    raise ValueError("RK4 integrator is not supported")
  return 0


def mul_quat(a, b):                              # engine_util_spatial.c:62-74
  return [a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3],
          a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
          a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1],
          a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]]


def quat2vel(quat, dt):                          # engine_util_spatial.c:118-135
  axis = [quat[1], quat[2], quat[3]]
  sin_a_2 = step_ref.normalize3(axis)
  speed = 2 * math.atan2(sin_a_2, quat[0])
  if speed > PI:
    speed -= 2*PI
  speed /= dt
  return [axis[0]*speed, axis[1]*speed, axis[2]*speed]


def sub_quat(qa, qb):                            # engine_util_spatial.c:138-146
  qneg = [qb[0], -qb[1], -qb[2], -qb[3]]
  return quat2vel(mul_quat(qneg, qa), 1)


def differentiate_pos(m, dt, qpos1, qpos2):      # engine_support.c:1483-1513
  qvel = [0.0]*int(m.nv)
  for j in range(int(m.njnt)):
    padr, vadr, t = int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j]), int(m.jnt_type[j])
    if t == FREE:
      for i in range(3):
        qvel[vadr+i] = (qpos2[padr+i] - qpos1[padr+i]) / dt
      vadr += 3
      padr += 3
    if t in (FREE, BALL):
      v = sub_quat(qpos2[padr:padr+4], qpos1[padr:padr+4])
      inv = 1/dt
      qvel[vadr:vadr+3] = [v[0]*inv, v[1]*inv, v[2]*inv]
    else:
      qvel[vadr] = (qpos2[padr] - qpos1[padr]) / dt
  return qvel


def state_diff(m, s1, s2, h):                    # :48-67
  nq, nv, na = int(m.nq), int(m.nv), int(m.na)
  inv_h = 1/h
  if nq == nv:
    return [inv_h * (s2[i] - s1[i]) for i in range(nq + nv + na)]
  return differentiate_pos(m, h, s1[:nq], s2[:nq]) + \
      [inv_h * (s2[nq+i] - s1[nq+i]) for i in range(nv + na)]


def clamped_state_diff(m, s, s_plus, s_minus, h):   # :92-107
  if s_plus is not None and s_minus is None:
    return state_diff(m, s, s_plus, h)
  if s_plus is None and s_minus is not None:
    return state_diff(m, s_minus, s, h)
  if s_plus is not None and s_minus is not None:
    return state_diff(m, s_minus, s_plus, 2*h)
  return [0.0]*(2*int(m.nv) + int(m.na))


def in_range(x1, x2, r):                         # :112-115
  return r[0] <= x1 <= r[1] and r[0] <= x2 <= r[1]


def transition_fd(m, fwd, qpos, qvel, act, ctrl, eps, centered, want_A=True, want_B=True,
                  refactor=False):
  """mjd_transitionFD: (A, B, status) as lists of rows (None for one not wanted). A nonzero
  status of any evaluation gives zero matrices, as mjhip_transitionFDBatch reports."""
  nq, nv, na, nu = int(m.nq), int(m.nv), int(m.na), int(m.nu)
  ndx = 2*nv + na
  q0, v0 = [float(x) for x in qpos], [float(x) for x in qvel]
  a0, u0 = [float(x) for x in act], [float(x) for x in ctrl]
  fac, status = {}, [0]

  def run(q, v, a, u, skipstage):
    q, v, a = list(q), list(v), list(a)
    status[0] |= step_skip(m, fwd, q, v, a, u, skipstage, fac, refactor)
    return q + v + a

  nxt = run(q0, v0, a0, u0, STAGE_NONE)
  DyDq, DyDv, DyDa, DyDu = [], [], [], []
  if status[0]:
    want_rows = False
  else:
    want_rows = True
  if want_rows and want_B:
    rng = [float(x) for row in m.actuator_ctrlrange for x in row] if nu else []
    for i in range(nu):
      limited = int(m.actuator_ctrllimited[i])
      r = rng[2*i:2*i+2]
      plus = minus = None
      fwd_ok = (not limited) or in_range(u0[i], u0[i] + eps, r)
      if fwd_ok:
        u = list(u0)
        u[i] += eps
        plus = run(q0, v0, a0, u, STAGE_VEL)
      back_ok = (centered or not fwd_ok) and ((not limited) or in_range(u0[i] - eps, u0[i], r))
      if back_ok:
        u = list(u0)
        u[i] -= eps
        minus = run(q0, v0, a0, u, STAGE_VEL)
      DyDu.append(clamped_state_diff(m, nxt, plus, minus, eps))

  def two_sided(perturb, skipstage, n, out):
    for i in range(n):
      plus = run(*perturb(i, eps), skipstage)
      if centered:
        minus = run(*perturb(i, -eps), skipstage)
        out.append(state_diff(m, minus, plus, 2*eps))
      else:
        out.append(state_diff(m, nxt, plus, eps))

  def p_act(i, e):
    a = list(a0)
    if e > 0:
      a[i] += eps
    else:
      a[i] -= eps
    return q0, v0, a, u0

  def p_vel(i, e):
    v = list(v0)
    if e > 0:
      v[i] += eps
    else:
      v[i] -= eps
    return q0, v, a0, u0

  def p_pos(i, e):
    q = list(q0)
    step_ref.integrate_pos(m, q, [1.0 if k == i else 0.0 for k in range(nv)], e)
    return q, v0, a0, u0

  if want_rows and want_A:
    two_sided(p_act, STAGE_VEL, na, DyDa)
    two_sided(p_vel, STAGE_POS, nv, DyDv)
    two_sided(p_pos, STAGE_NONE, nv, DyDq)
  A = B = None
  if want_A:
    AT = DyDq + DyDv + DyDa                      # AT is ndx x ndx; A = AT' (:589)
    A = [[AT[c][r] if not status[0] and want_rows else 0.0 for c in range(ndx)]
         for r in range(ndx)]
  if want_B:
    B = [[DyDu[c][r] if not status[0] and want_rows else 0.0 for c in range(nu)]
         for r in range(ndx)]
  return A, B, status[0]
