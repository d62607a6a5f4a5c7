"""The va stage's cdof stack in LDS (codegen.VA_LDS_SLOTS) on the GPU: every kernel that runs
the va body with the stack -- k_all in both of its store instantiations, k_vaskip, and the
run-time code object of a chain deeper than the stack -- against the oracle, and the reuse of
the trig region from one call to the next.
"""
import os
import sys

import numpy as np
import pytest

from mujoco_inversedynamicstest_amd import codegen, engine, fields
from mujoco_inversedynamicstest_amd.sampler import sample_states
from oracle.oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
  sys.path.insert(0, HERE)
import va_lds_chain  # noqa: E402
from test_gpu import OUTPUTS, RTOL, _assert_fd_contraction_close, assert_close, oracle_batch  # noqa: E402

pytestmark = pytest.mark.gpu


def test_humanoid_b65_every_output(humanoid):
  """One full block and a block of a single lane: every mj_inverse output field."""
  B = 65
  q, v, a = sample_states(humanoid, B, first=1234)
  e = engine.InverseEngine(humanoid, capacity=B)
  try:
    assert e.fast_kernel == "humanoid"
    assert e.fast_kernel_lds == codegen.k_all_lds_bytes(humanoid) <= codegen.LDS_BUDGET
    f, st = e.inverse(q, v, a, status=True)
    got = {n: e.field(n, 0, B) for n in OUTPUTS if fields.DATA_FIELD[n].size(humanoid.sizes)}
  finally:
    e.close()
  assert (st == 0).all()
  ref, _ = oracle_batch(humanoid, q, v, a, OUTPUTS)
  assert_close(f, ref["qfrc_inverse"], "qfrc_inverse (row-major)")
  for n, x in got.items():
    assert_close(x, ref[n], n)


def test_humanoid_streaming_instantiation_partial_block(humanoid):
  """B = 49,153 >= NT_SV_MIN_B runs k_all<SV = true>, the headline's instantiation, with one
  lane in its last block: qfrc_inverse of 256 seeded rows, the last row among them."""
  B = 49153
  assert B >= codegen.NT_SV_MIN_B and B % 64 == 1
  q, v, a = sample_states(humanoid, B, first=7)
  rows = np.random.default_rng(49153).choice(B - 1, 255, replace=False)
  rows = np.sort(np.append(rows, B - 1))
  e = engine.InverseEngine(humanoid, capacity=B)
  try:
    f, st = e.inverse(q, v, a, status=True)
  finally:
    e.close()
  assert (st == 0).all()
  ref, _ = oracle_batch(humanoid, q[rows], v[rows], a[rows])
  assert_close(f[rows], ref["qfrc_inverse"], "qfrc_inverse")


def test_back_to_back_calls_identical(humanoid):
  """The next call's pos stage writes its sin/cos over the stack the last va stage left in the
  shared region: two calls on one context give identical results."""
  B = 4096 + 65
  q, v, a = sample_states(humanoid, B, first=99)
  e = engine.InverseEngine(humanoid, capacity=B)
  try:
    f1 = e.inverse(q, v, a).copy()
    bias1 = e.field("qfrc_bias", 0, B)
    f2 = e.inverse(q, v, a)
    bias2 = e.field("qfrc_bias", 0, B)
  finally:
    e.close()
  assert np.array_equal(f1, f2) and np.array_equal(bias1, bias2)


@pytest.mark.parametrize("NB", [2, 16])
def test_inverse_fd_vaskip(humanoid, NB, monkeypatch):
  """mjd_inverseFD at 2 base states, and at 16, the fewest whose position-stage block
  (NB x (nv + 1) instances) ends on a wave boundary so that the qvel/qacc perturbations run
  k_vaskip (2 base states go through k_all alone): against the full pipeline within the
  existing contraction bound, and against the oracle's serial mjd_inverseFD."""
  q, v, a = sample_states(humanoid, NB, first=640)
  e = engine.InverseEngine(humanoid, capacity=NB * (3 * humanoid.nv + 1))
  try:
    got = e.inverse_fd(q, v, a, eps=1e-6)
    monkeypatch.setenv("MJHIP_FD_NOSKIP", "1")
    ref = e.inverse_fd(q, v, a, eps=1e-6)
  finally:
    e.close()
  for g, r in zip(got[:3], ref[:3]):
    _assert_fd_contraction_close(g, r)
  o = Oracle(humanoid)
  for i in range(0, NB, 8):
    o.set_state(q[i], v[i], a[i])
    rq, rv, ra, _ = o.inverse_fd(1e-6)
    np.testing.assert_allclose(got[2][i], ra, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[1][i], rv, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[0][i], rq, rtol=1e-5, atol=1e-4)


def test_chain_runtime_kernel_b65():
  """The synthetic chain (free, ball, slide, more hinges in series than slots) as a run-time
  code object: the slot branch and the re-read branch of one tree pass, every output field."""
  m = va_lds_chain.load()
  B = 65
  q, v, a = sample_states(m, B, first=21)
  e = engine.InverseEngine(m, capacity=B, specialize=True)
  try:
    assert e.fast_kernel and e.fast_kernel.startswith("rt_")
    assert e.fast_kernel_lds == codegen.k_all_lds_bytes(m) <= codegen.LDS_BUDGET
    f, st = e.inverse(q, v, a, status=True)
    got = {n: e.field(n, 0, B) for n in OUTPUTS if fields.DATA_FIELD[n].size(m.sizes)}
  finally:
    e.close()
  assert (st == 0).all()
  ref, _ = oracle_batch(m, q, v, a, OUTPUTS)
  assert_close(f, ref["qfrc_inverse"], "qfrc_inverse (row-major)")
  for n, x in got.items():
    assert_close(x, ref[n], n)
