"""Rate of mjhip_transitionFDBatch: Jacobian sets (A and B) per second on the contact-disabled
humanoid, forward and centred differences, beside the composition it replaces: the
1 + s (2 nv + na + nu) perturbed states per base state expanded on the host, one
rollout(nstep = 1) launch over them on device-resident data, and numpy differences. The
rollout launch alone is what the new call has to beat: it runs the same steps without
skipping a stage. The host expansion and the differencing are reported beside it.

  python tools/transition_bench.py [B ...]        (default 1024 4096)

Timed with events on the context's stream, warm, 5 runs: median and spread. One JSON line."""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mujoco_inversedynamicstest_amd import engine, models  # noqa: E402
from mujoco_inversedynamicstest_amd.sampler import sample_states  # noqa: E402

RUNS = 5
EPS = 1e-6
FREE, BALL = 0, 1


def timed(eng, fn):
  import torch
  s = torch.cuda.ExternalStream(eng.stream, device=eng.device)
  ms = []
  for r in range(RUNS + 1):                 # the first run warms up
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    if r:
      ms.append(e0.elapsed_time(e1))
  return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def quat_mul(a, b):
  return np.stack([a[:, 0]*b[0] - a[:, 1]*b[1] - a[:, 2]*b[2] - a[:, 3]*b[3],
                   a[:, 0]*b[1] + a[:, 1]*b[0] + a[:, 2]*b[3] - a[:, 3]*b[2],
                   a[:, 0]*b[2] - a[:, 1]*b[3] + a[:, 2]*b[0] + a[:, 3]*b[1],
                   a[:, 0]*b[3] + a[:, 1]*b[2] - a[:, 2]*b[1] + a[:, 3]*b[0]], axis=1)


def nudge_pos(m, q, i, e):
  """mj_integratePos(qpos, e_i, e) for a batch."""
  q = q.copy()
  for j in range(m.njnt):
    padr, vadr, t = int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j]), int(m.jnt_type[j])
    n = 6 if t == FREE else 3 if t == BALL else 1
    if not vadr <= i < vadr + n:
      continue
    k = i - vadr
    if t == FREE and k < 3:
      q[:, padr + k] += e
    elif t in (FREE, BALL):
      if t == FREE:
        padr, k = padr + 3, k - 3
      r = np.zeros(4)
      r[0], r[1 + k] = np.cos(abs(e)*0.5), np.sin(abs(e)*0.5)*np.sign(e)
      q[:, padr:padr + 4] = quat_mul(q[:, padr:padr + 4], r)
    else:
      q[:, padr] += e
  return q


def expand(m, q, v, u, centered):
  """The composition's host expansion: every state mjd_stepFD evaluates, [1 + P', B, n]."""
  signs = (EPS, -EPS) if centered else (EPS,)
  Q, V, U = [q], [v], [u]
  for i in range(m.nv):
    for e in signs:
      Q.append(nudge_pos(m, q, i, e)); V.append(v); U.append(u)
  for i in range(m.nv):
    for e in signs:
      vv = v.copy()
      vv[:, i] += e
      Q.append(q); V.append(vv); U.append(u)
  for i in range(m.nu):
    for e in signs:
      uu = u.copy()
      uu[:, i] += e
      Q.append(q); V.append(v); U.append(uu)
  return np.concatenate(Q), np.concatenate(V), np.concatenate(U)


def bench(B, centered):
  import torch
  m = models.load("humanoid", disable_contact=True)
  assert m.na == 0
  ndx, nstate = 2*m.nv, m.nq + m.nv
  q, v, _ = sample_states(m, B, margin=0.05)
  u = np.random.default_rng(1).uniform(-0.9, 0.9, (B, m.nu))
  ns = 2 if centered else 1
  P = ns*ndx + 2*m.nu
  eng = engine.InverseEngine(m, capacity=64*((B + 63)//64)*(1 + P), device=0)
  L = engine.lib()
  dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0").contiguous()
  dq, dv, du = dev(q), dev(v), dev(u)
  A = torch.empty((B, ndx, ndx), dtype=torch.float64, device="cuda:0")
  Bm = torch.empty((B, ndx, m.nu), dtype=torch.float64, device="cuda:0")
  tin, tout = engine.TransitionIn(), engine.TransitionOut()
  tin.size, tout.size = ctypes.sizeof(tin), ctypes.sizeof(tout)
  tin.eps, tin.flg_centered = EPS, int(centered)
  tin.qpos, tin.qvel, tin.ctrl = dq.data_ptr(), dv.data_ptr(), du.data_ptr()
  tout.A, tout.B = A.data_ptr(), Bm.data_ptr()

  def run_new():
    rc = L.mjhip_transitionFDBatch(eng.ctx, B, ctypes.byref(tin), ctypes.byref(tout),
                                   engine.FLAG_DEVICE_PTRS, None)
    assert rc >= 0, L.mjhip_lastError()

  res = {"B": B, "centered": centered, "evaluations": B*(1 + P), "new": timed(eng, run_new)}
  st = np.zeros(B, dtype=np.int32)
  rc = L.mjhip_transitionFDBatch(eng.ctx, B, ctypes.byref(tin), ctypes.byref(tout),
                                 engine.FLAG_DEVICE_PTRS, st.ctypes.data)
  assert rc >= 0, L.mjhip_lastError()
  res["status_zero"] = float((st == 0).mean())
  res["new"]["sets_per_s"] = B / (res["new"]["ms"] * 1e-3)

  t0 = time.perf_counter()
  Q, V, U = expand(m, q, v, u, centered)
  res["host_expand_ms"] = (time.perf_counter() - t0) * 1e3
  n = len(Q)
  assert n <= eng.capacity
  eq, ev, eu = dev(Q), dev(V), dev(U)
  state = torch.empty((n, 1, nstate), dtype=torch.float64, device="cuda:0")
  rin, rout = engine.RolloutIn(), engine.RolloutOut()
  rin.size, rout.size = ctypes.sizeof(rin), ctypes.sizeof(rout)
  rin.qpos, rin.qvel, rin.ctrl = eq.data_ptr(), ev.data_ptr(), eu.data_ptr()
  rin.ctrl_mode = engine.ROLLOUT_HELD
  rout.state = state.data_ptr()

  def run_old():
    rc = L.mjhip_rolloutBatch(eng.ctx, n, 1, ctypes.byref(rin), ctypes.byref(rout),
                              engine.FLAG_DEVICE_PTRS, None, None)
    assert rc >= 0, L.mjhip_lastError()

  res["rollout"] = timed(eng, run_old)
  res["rollout"]["states"] = n
  s = state.cpu().numpy().reshape(-1, B, nstate)
  t0 = time.perf_counter()
  inv_h = 1/(2*EPS) if centered else 1/EPS
  J = np.stack([inv_h * (s[1 + c*ns] - (s[2 + c*ns] if centered else s[0]))
                for c in range(ndx + m.nu)], axis=2)
  res["host_diff_ms"] = (time.perf_counter() - t0) * 1e3
  res["new_over_rollout"] = res["new"]["ms"] / res["rollout"]["ms"]
  del J
  eng.close()
  return res


def main():
  Bs = [int(a) for a in sys.argv[1:]] or [1024, 4096]
  out = [bench(B, c) for B in Bs for c in (False, True)]
  print(json.dumps(out))


if __name__ == "__main__":
  main()
