"""Rollout rate of mjhip_rolloutBatch: steps x instances per second on the contact-disabled
humanoid, states sampled with every limit inactive, for Euler and RK4, with the LDS write-out
and with the direct store; beside it the two things it replaces: T separate forward launches
with the state left on the device (no integration: the parent's best), and the oracle's
forward + rk4 chain on one CPU core.

  python tools/rollout_bench.py [B] [T]        (default 65536 32)

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


def timed(eng, fn, reset):
  import torch
  s = torch.cuda.ExternalStream(eng.stream, device=eng.device)
  ms = []
  for r in range(RUNS + 1):                 # the first run warms up
    reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    if r:
      ms.append(e0.elapsed_time(e1))
  return float(np.median(ms)), float(min(ms)), float(max(ms))


def gpu(integrator, B, T, q, v):
  import torch
  m = models.load("humanoid", disable_contact=True)
  m.opt["integrator"] = integrator
  eng = engine.InverseEngine(m, capacity=B, device=0)
  L = engine.lib()
  nstate = m.nq + m.nv + m.na
  state = torch.empty((B, T, nstate), dtype=torch.float64, device="cuda:0")
  done = torch.empty(B, dtype=torch.int32, device="cuda:0")
  rin, rout = engine.RolloutIn(), engine.RolloutOut()
  rin.size, rout.size = ctypes.sizeof(rin), ctypes.sizeof(rout)
  rout.state = state.data_ptr()

  def reset():
    eng.set_field("qpos", q)
    eng.set_field("qvel", v)

  res = {}
  for name, direct in (("lds", "0"), ("direct", "1")):
    os.environ["MJHIP_ROLLOUT_DIRECT"] = direct          # read by the library at every call
    flags = engine.FLAG_DEVICE_PTRS | engine.FLAG_MIRROR_INPUT

    def run():
      rc = L.mjhip_rolloutBatch(eng.ctx, B, T, ctypes.byref(rin), ctypes.byref(rout), flags,
                                None, done.data_ptr())
      assert rc >= 0, L.mjhip_lastError()

    med, lo, hi = timed(eng, run, reset)
    res[name] = {"ms": med, "ms_min": lo, "ms_max": hi, "steps_per_s": B * T / (med * 1e-3),
                 "completed": float((done.cpu().numpy() == T).mean())}

  os.environ.pop("MJHIP_ROLLOUT_DIRECT", None)

  def forwards():
    for _ in range(T):
      rc = L.mjhip_forwardBatchEx(eng.ctx, B, None, None, None, None, None, None, None,
                                  engine.FLAG_DEVICE_PTRS | engine.FLAG_MIRROR_INPUT, None)
      assert rc >= 0, L.mjhip_lastError()

  med, lo, hi = timed(eng, forwards, reset)
  res["forward_launches"] = {"ms": med, "ms_min": lo, "ms_max": hi,
                             "evals_per_s": B * T / (med * 1e-3)}
  eng.close()
  return res


def cpu_chain(q, v, steps=200):
  from oracle.oracle import Oracle
  m = models.load("humanoid", disable_contact=True)
  m.opt["integrator"] = 1
  o = Oracle(m)
  o.d.qpos[:], o.d.qvel[:] = q[0], v[0]
  t0 = time.perf_counter()
  for _ in range(steps):
    o.forward()
    o.rk4()
  return steps / (time.perf_counter() - t0)


def main():
  B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
  T = int(sys.argv[2]) if len(sys.argv) > 2 else 32
  m = models.load("humanoid", disable_contact=True)
  q, v, _ = sample_states(m, B)
  out = {"B": B, "T": T, "euler": gpu(0, B, T, q, v), "rk4": gpu(1, B, T, q, v),
         "oracle_rk4_steps_per_s_per_core": cpu_chain(q, v)}
  print(json.dumps(out))


if __name__ == "__main__":
  main()
