"""The reference's actuation functions restated on scalar IEEE doubles (Python floats), one
operation per operation and in the reference's order: the yardstick of the activation-state
tests (the C oracle has no actuator dynamics).

Restated, with the reference's file:line:
  mju_sigmoid                  engine_util_misc.c:1470-1483
  mju_muscleGainLength         engine_util_misc.c:503-525
  mju_muscleGain               engine_util_misc.c:529-571
  mju_muscleBias               engine_util_misc.c:575-607
  mju_muscleDynamicsTimescale  engine_util_misc.c:611-627
  mju_muscleDynamics           engine_util_misc.c:631-649
  mjd_muscleGain_vel           engine_derivative.c:762-807
  nextActivation               engine_forward.c:236-259
  mj_fwdActuation              engine_forward.c:276-515
  mj_advance's activation loop engine_forward.c:738-750 (act_next)

Every function takes an optional `cov` dict and counts the branch it took there, so a test
can assert that its states reach every branch.
"""
import math

MINVAL = 1e-15                                   # mjMINVAL, mjmodel.h

DYN_NONE, DYN_INTEGRATOR, DYN_FILTER, DYN_FILTEREXACT, DYN_MUSCLE = range(5)
GAIN_FIXED, GAIN_AFFINE, GAIN_MUSCLE = range(3)
BIAS_NONE, BIAS_AFFINE, BIAS_MUSCLE = range(3)


def _hit(cov, key):
  if cov is not None:
    cov[key] = cov.get(key, 0) + 1


def mjmax(a, b):                                 # mjMAX, mjmacro.h
  return a if a > b else b


def clip(x, lo, hi):                             # mju_clip, engine_util_misc.c
  return lo if x < lo else (hi if x > hi else x)


def sigmoid(x):                                  # engine_util_misc.c:1470-1483
  if x <= 0:
    return 0.0
  if x >= 1:
    return 1.0
  return x*x*x * (3*x * (2*x - 5) + 10)


def muscle_gain_length(length, lmin, lmax, cov=None):   # engine_util_misc.c:503-525
  if lmin <= length and length <= lmax:
    a = 0.5*(lmin+1)
    b = 0.5*(1+lmax)
    if length <= a:
      _hit(cov, "FL_rise_low")
      x = (length-lmin) / mjmax(MINVAL, a-lmin)
      return 0.5*x*x
    elif length <= 1:
      _hit(cov, "FL_rise_high")
      x = (1-length) / mjmax(MINVAL, 1-a)
      return 1 - 0.5*x*x
    elif length <= b:
      _hit(cov, "FL_fall_high")
      x = (length-1) / mjmax(MINVAL, b-1)
      return 1 - 0.5*x*x
    else:
      _hit(cov, "FL_fall_low")
      x = (lmax-length) / mjmax(MINVAL, lmax-b)
      return 0.5*x*x
  _hit(cov, "FL_outside")
  return 0.0


def _muscle_norm(length, vel, lengthrange, acc0, prm):
  """force, L, V and the velocity scale, as :533-551 / :765-783 / :579-594 derive them."""
  rng0, rng1 = prm[0], prm[1]
  force, scale, vmax = prm[2], prm[3], prm[6]
  if force < 0:
    force = scale / mjmax(MINVAL, acc0)
  L0 = (lengthrange[1]-lengthrange[0]) / mjmax(MINVAL, rng1-rng0)
  L = rng0 + (length-lengthrange[0]) / mjmax(MINVAL, L0)
  vscale = mjmax(MINVAL, L0*vmax)
  V = vel / vscale
  return force, L, V, vscale


def muscle_gain(length, vel, lengthrange, acc0, prm, cov=None):   # engine_util_misc.c:529-571
  force, L, V, _ = _muscle_norm(length, vel, lengthrange, acc0, prm)
  lmin, lmax, fvmax = prm[4], prm[5], prm[8]
  FL = muscle_gain_length(L, lmin, lmax, cov)
  y = fvmax-1
  if V <= -1:
    _hit(cov, "FV_zero")
    FV = 0.0
  elif V <= 0:
    _hit(cov, "FV_shortening")
    FV = (V+1)*(V+1)
  elif V <= y:
    _hit(cov, "FV_lengthening")
    FV = fvmax - (y-V)*(y-V) / mjmax(MINVAL, y)
  else:
    _hit(cov, "FV_max")
    FV = fvmax
  return -force*FL*FV


def muscle_gain_vel(length, vel, lengthrange, acc0, prm):   # engine_derivative.c:762-807
  force, L, V, vscale = _muscle_norm(length, vel, lengthrange, acc0, prm)
  FL = muscle_gain_length(L, prm[4], prm[5])
  y = prm[8]-1
  if V <= -1:
    dFV = 0.0
  elif V <= 0:
    dFV = 2*V + 2
  elif V <= y:
    dFV = (-2*V + 2*y) / mjmax(MINVAL, y)
  else:
    dFV = 0.0
  return -force*FL*dFV/vscale


def muscle_bias(length, lengthrange, acc0, prm, cov=None):   # engine_util_misc.c:575-607
  force, L, _, _ = _muscle_norm(length, 0.0, lengthrange, acc0, prm)
  lmax, fpmax = prm[5], prm[7]
  b = 0.5*(1+lmax)
  if L <= 1:
    _hit(cov, "FP_zero")
    return 0.0
  elif L <= b:
    _hit(cov, "FP_quadratic")
    x = (L-1) / mjmax(MINVAL, b-1)
    return -force*fpmax*0.5*x*x
  else:
    _hit(cov, "FP_linear")
    x = (L-b) / mjmax(MINVAL, b-1)
    return -force*fpmax*(0.5 + x)


def muscle_dynamics_timescale(dctrl, tau_act, tau_deact, smoothing_width, cov=None):
  """engine_util_misc.c:611-627"""
  if smoothing_width < MINVAL:
    _hit(cov, "switch_hard")
    return tau_act if dctrl > 0 else tau_deact
  _hit(cov, "switch_smooth")
  return tau_deact + (tau_act-tau_deact)*sigmoid(dctrl/smoothing_width + 0.5)


def muscle_dynamics(ctrl, act, prm, cov=None):   # engine_util_misc.c:631-649
  ctrlclamp = clip(ctrl, 0.0, 1.0)
  actclamp = clip(act, 0.0, 1.0)
  tau_act = prm[0] * (0.5 + 1.5*actclamp)
  tau_deact = prm[1] / (0.5 + 1.5*actclamp)
  smoothing_width = prm[2]
  dctrl = ctrlclamp - act
  _hit(cov, "dctrl_pos" if dctrl > 0 else "dctrl_nonpos")
  tau = muscle_dynamics_timescale(dctrl, tau_act, tau_deact, smoothing_width, cov)
  return dctrl / mjmax(MINVAL, tau)


def muscle_dynamics_millard(ctrl, act, prm):
  """The closed form the reference's test compares with (engine_util_misc_test.cc:150-161)."""
  ctrlclamp = clip(ctrl, 0.0, 1.0)
  actclamp = clip(act, 0.0, 1.0)
  if ctrlclamp > act:
    tau = prm[0] * (0.5 + 1.5*actclamp)
  else:
    tau = prm[1] / (0.5 + 1.5*actclamp)
  return (ctrlclamp - act) / mjmax(MINVAL, tau)


def next_activation(dyntype, dynprm0, timestep, actlimited, actrange, act, act_dot, cov=None):
  """engine_forward.c:236-259"""
  if dyntype == DYN_FILTEREXACT:
    tau = mjmax(MINVAL, dynprm0)
    act = act + act_dot * tau * (1 - math.exp(-timestep / tau))
  else:
    act = act + act_dot * timestep
  if actlimited:
    c = clip(act, actrange[0], actrange[1])
    _hit(cov, "actclamp_on" if c != act else "actclamp_off")
    act = c
  return act


def fwd_actuation(m, length, velocity, moment, ctrl, act, cov=None):
  """mj_fwdActuation (engine_forward.c:276-515) of one instance of model m over its
  actuator_length, actuator_velocity and sparse actuator_moment; act_next is the activation
  mj_advance's loop (:738-750) writes over act. Returns (act_dot, act_next, actuator_force,
  qfrc_actuator) as lists of floats; `act` is not modified."""
  nu, nv, na = int(m.nu), int(m.nv), int(m.na)
  h = float(m.opt["timestep"])
  disable = int(m.opt["disableflags"])
  force = [0.0]*nu
  qfrc = [0.0]*nv
  act_dot = [0.0]*na
  act_next = [0.0]*na
  if nu == 0 or (disable & (1 << 10)):           # mjDSBL_ACTUATION
    return act_dot, act_next, force, qfrc
  c = [float(x) for x in ctrl]
  if not (disable & (1 << 7)):                   # mjDSBL_CLAMPCTRL; clampVec :264-272
    for i in range(nu):
      if m.actuator_ctrllimited[i]:
        r = m.actuator_ctrlrange[i]
        cl = clip(c[i], float(r[0]), float(r[1]))
        _hit(cov, "ctrlclamp_on" if cl != c[i] else "ctrlclamp_off")
        c[i] = cl
  for i in range(nu):                            # act_dot :309-355
    first = int(m.actuator_actadr[i])
    if first < 0:
      continue
    last = first + int(m.actuator_actnum[i]) - 1
    prm = [float(x) for x in m.actuator_dynprm[i]]
    dyn = int(m.actuator_dyntype[i])
    a = float(act[last])
    if dyn == DYN_INTEGRATOR:
      act_dot[last] = c[i]
    elif dyn in (DYN_FILTER, DYN_FILTEREXACT):
      tau = mjmax(MINVAL, prm[0])
      act_dot[last] = (c[i] - a) / tau
    elif dyn == DYN_MUSCLE:
      act_dot[last] = muscle_dynamics(c[i], a, prm, cov)
    # mj_advance :738-750
    act_next[last] = next_activation(dyn, prm[0], h, int(m.actuator_actlimited[i]),
                                     [float(x) for x in m.actuator_actrange[i]], a,
                                     act_dot[last], cov)
  for i in range(nu):                            # force = gain * [ctrl | act] + bias :375-465
    prm = [float(x) for x in m.actuator_gainprm[i]]
    ln, vl = float(length[i]), float(velocity[i])
    lr = [float(x) for x in m.actuator_lengthrange[i]]
    acc0 = float(m.actuator_acc0[i])
    gt = int(m.actuator_gaintype[i])
    if gt == GAIN_FIXED:
      gain = prm[0]
    elif gt == GAIN_AFFINE:
      gain = prm[0] + prm[1]*ln + prm[2]*vl
    else:
      gain = muscle_gain(ln, vl, lr, acc0, prm, cov)
    if int(m.actuator_actadr[i]) == -1:
      force[i] = gain * c[i]
    else:
      adr = int(m.actuator_actadr[i]) + int(m.actuator_actnum[i]) - 1
      if m.actuator_actearly[i]:
        a = next_activation(int(m.actuator_dyntype[i]), float(m.actuator_dynprm[i][0]), h,
                            int(m.actuator_actlimited[i]),
                            [float(x) for x in m.actuator_actrange[i]], float(act[adr]),
                            act_dot[adr])
      else:
        a = float(act[adr])
      force[i] = gain * a
    prm = [float(x) for x in m.actuator_biasprm[i]]
    bt = int(m.actuator_biastype[i])
    if bt == BIAS_NONE:
      bias = 0.0
    elif bt == BIAS_AFFINE:
      bias = prm[0] + prm[1]*ln + prm[2]*vl
    else:
      bias = muscle_bias(ln, lr, acc0, prm, cov)
    force[i] += bias
  for i in range(nu):                            # clampVec(force) :486
    if m.actuator_forcelimited[i]:
      r = m.actuator_forcerange[i]
      cl = clip(force[i], float(r[0]), float(r[1]))
      _hit(cov, "forceclamp_on" if cl != force[i] else "forceclamp_off")
      force[i] = cl
  for i in range(nu):                            # mju_mulMatTVecSparse :489
    f = force[i]
    if not f:
      continue
    adr = int(m.moment_rowadr[i])
    for j in range(int(m.moment_rownnz[i])):
      qfrc[int(m.moment_colind[adr+j])] += float(moment[adr+j])*f
  return act_dot, act_next, force, qfrc
