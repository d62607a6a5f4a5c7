"""The qM hand-off of k_all (codegen.QM_HANDOFF) on the GPU: a context that launches the HO
instantiation against one created with MJHIP_QM_HANDOFF=0, in one process, bit for bit; and
against the oracle.

B = 1 and B = 65 (a lone lane, a partial second block) run k_all<SV = false>, with the hand-off
forced (MJHIP_QM_HANDOFF=1: by default it starts at batch 49,152); B = 49,152 is the smallest
batch that runs the SV = true instantiation the benchmark runs, and the smallest that hands by
default, so that case runs the library as shipped. Limit-active states keep the work-list
path covered. At 49,152 the fields are compared where they are, as raw
device bytes (the mirror of such a batch is close to a gigabyte per context).
"""
import os
import sys

import numpy as np
import pytest

from mujoco_inversedynamicstest_amd import codegen, engine, fields
from mujoco_inversedynamicstest_amd.sampler import sample_states

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
  sys.path.insert(0, HERE)
from test_gpu import OUTPUTS, assert_close, oracle_batch  # noqa: E402

pytestmark = pytest.mark.gpu
BIG = 49152


def _states(m, B, first):
  q, v, a = sample_states(m, B, first=first)
  # some instances past a joint range: k_pos appends them to the constraint kernel's work-list
  j = int(np.flatnonzero(np.asarray(m.jnt_limited))[3])
  q[::7, m.jnt_qposadr[j]] = m.jnt_range[j][1] + 0.2
  return q, v, a


@pytest.fixture(scope="module")
def big_states(humanoid):
  return _states(humanoid, BIG, 11)


def _pair(m, B, monkeypatch, force):
  """Two contexts of capacity B: the hand-off on (forced at every batch, or the default) and
  off."""
  monkeypatch.delenv("MJHIP_QM_HANDOFF", raising=False)
  if force:
    monkeypatch.setenv("MJHIP_QM_HANDOFF", "1")
  on = engine.InverseEngine(m, capacity=B)
  monkeypatch.setenv("MJHIP_QM_HANDOFF", "0")
  off = engine.InverseEngine(m, capacity=B)
  monkeypatch.delenv("MJHIP_QM_HANDOFF")
  assert on.fast_kernel == off.fast_kernel == "humanoid"
  # the switch is read when the context is created, and the test cannot pass on the old path
  assert on.qm_handoff == len(codegen.qm_handoff_plan(m)) > 0
  assert off.qm_handoff == 0
  assert on.fast_kernel_lds == off.fast_kernel_lds == codegen.k_all_lds_bytes(m) == 38400
  return on, off


@pytest.mark.parametrize("B", [1, 65])
def test_on_off_bit_identical_small(humanoid, B, monkeypatch):
  assert B < codegen.NT_SV_MIN_B
  q, v, a = _states(humanoid, B, 300 + B)
  on, off = _pair(humanoid, B, monkeypatch, force=True)
  try:
    got = {}
    for key, e in (("on", on), ("off", off)):
      f, st = e.inverse(q, v, a, status=True)
      assert e.last_path == 1
      got[key] = (f.copy(), st.copy(), e.field_int("efc_count", 0, B),
                  {n: e.field(n, 0, B) for n in OUTPUTS
                   if fields.DATA_FIELD[n].size(humanoid.sizes)})
  finally:
    on.close()
    off.close()
  (f1, st1, c1, d1), (f0, st0, c0, d0) = got["on"], got["off"]
  assert (st1 == 0).all() and np.array_equal(st1, st0) and np.array_equal(c1, c0)
  assert c1[0, 0] > 0                                  # instance 0 has limit rows
  assert np.array_equal(f1.view(np.uint64), f0.view(np.uint64)), "qfrc_inverse (row-major)"
  assert d1["qM"].any() and d1["qLD"].any() and d1["qLDiagInv"].all()
  for n in d1:
    assert np.array_equal(d1[n].view(np.uint64), d0[n].view(np.uint64)), n
  if B == 65:
    ref, nefc = oracle_batch(humanoid, q, v, a, ("qM", "qLD", "qLDiagInv", "qfrc_inverse"))
    assert (nefc > 0).any() and (nefc == 0).any()
    assert_close(f1, ref["qfrc_inverse"], "qfrc_inverse (row-major)")
    for n in ref:
      assert_close(d1[n], ref[n], n)


class _DevArray:
  """A mirror field's whole device buffer as int64 words (torch reads the interface)."""

  def __init__(self, ptr, n):
    self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (int(ptr), False),
                                     "version": 2}


def test_on_off_bit_identical_streaming_instantiation(humanoid, big_states, monkeypatch):
  import torch
  assert BIG == codegen.NT_SV_MIN_B == codegen.QM_HANDOFF_MIN_B and BIG % 64 == 0
  q, v, a = big_states
  on, off = _pair(humanoid, BIG, monkeypatch, force=False)
  try:
    L = engine.lib()
    out = {}
    for key, e in (("on", on), ("off", off)):
      f, st = e.inverse(q, v, a, status=True)
      assert e.last_path == 1 and (st == 0).all()
      out[key] = f.copy()
    assert np.array_equal(out["on"].view(np.uint64), out["off"].view(np.uint64))
    assert np.array_equal(on.field_int("efc_count", 0, BIG), off.field_int("efc_count", 0, BIG))
    assert on.field_int("efc_count", 0, 1)[0, 0] > 0
    for n in OUTPUTS:
      S = L.mjhip_mirrorFieldSize(on.ctx, n.encode())
      if S <= 0:
        continue
      x, y = (torch.as_tensor(_DevArray(L.mjhip_mirrorDevicePtr(e.ctx, n.encode()), BIG * S),
                              device="cuda:0") for e in (on, off))
      assert torch.equal(x, y), n
      if n in ("qM", "qLD", "qLDiagInv"):
        assert bool((x != 0).any()), n
  finally:
    on.close()
    off.close()
