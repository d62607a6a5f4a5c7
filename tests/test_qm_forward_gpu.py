"""The register forwarding of qM rows (codegen.QM_FORWARD) on the GPU, on models other than the
humanoid (tests/test_qm_handoff_gpu.py runs that one at 1, 65 and 49,152 with the library as
shipped): a context whose k_all forwards against one created with MJHIP_QM_HANDOFF=0, in one
process, bit for bit.

Both models run as run-time code objects, whose one k_all has the HO = true bodies compiled
in: the synthetic chain (free, ball, slide, hinges; its rows outnumber the LDS pool and the
register budget, so it uses both and still re-reads some), and the bundled connect model
(free joints only, nM = 63, no bundled kernel) generated with the LDS pool withheld
(codegen.QM_LDS), so that every row is forwarded and nothing goes through LDS. Neither model
has joint limits.
B = 1 is a lone lane, B = 65 a full block and a partial second one.
"""
import os
import sys

import numpy as np
import pytest

from mujoco_inversedynamicstest_amd import codegen, engine, fields, models
from mujoco_inversedynamicstest_amd.sampler import sample_states

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
  sys.path.insert(0, HERE)
import va_lds_chain  # noqa: E402
from test_gpu import OUTPUTS, assert_close, oracle_batch  # noqa: E402

pytestmark = pytest.mark.gpu


def _model(name):
  return va_lds_chain.load() if name == "va_lds_chain" else \
      models.load(name, disable_contact=True)


def _pair(m, B, monkeypatch):
  """Two specialized contexts of capacity B: forwarding on and, with MJHIP_QM_HANDOFF=0 read
  as the code object is generated, off."""
  monkeypatch.setenv("MJHIP_QM_HANDOFF", "1")
  on = engine.InverseEngine(m, capacity=B, specialize=True)
  monkeypatch.setenv("MJHIP_QM_HANDOFF", "0")
  off = engine.InverseEngine(m, capacity=B, specialize=True)
  monkeypatch.delenv("MJHIP_QM_HANDOFF")
  assert on.fast_kernel.startswith("rt_") and off.fast_kernel.startswith("rt_")
  # the test cannot pass on the old path
  assert on.qm_forward == len(codegen.qm_forward_plan(m)) > 0
  assert on.qm_handoff == len(codegen.qm_handoff_plan(m))
  assert off.qm_forward == 0 and off.qm_handoff == 0
  return on, off


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("name", ["va_lds_chain", "connect"])
def test_on_off_bit_identical(name, B, monkeypatch):
  m = _model(name)
  if name == "connect":
    monkeypatch.setattr(codegen, "QM_LDS", False)
    assert codegen.qm_handoff_plan(m) == {} and len(codegen.qm_forward_plan(m)) == m.nM
  else:
    assert codegen.qm_handoff_plan(m) and \
        len(codegen.qm_handoff_plan(m)) + len(codegen.qm_forward_plan(m)) < m.nM
  q, v, a = sample_states(m, B, first=700 + B)
  on, off = _pair(m, B, monkeypatch)
  try:
    got = {}
    for key, e in (("on", on), ("off", off)):
      f, st = e.inverse(q, v, a, status=True)
      assert e.last_path == 1
      got[key] = (f.copy(), st.copy(),
                  {n: e.field(n, 0, B) for n in OUTPUTS if fields.DATA_FIELD[n].size(m.sizes)})
  finally:
    on.close()
    off.close()
  (f1, st1, d1), (f0, st0, d0) = got["on"], got["off"]
  assert (st1 == 0).all() and np.array_equal(st1, st0)
  assert np.array_equal(f1.view(np.uint64), f0.view(np.uint64)), "qfrc_inverse (row-major)"
  assert d1["qM"].any() and d1["qLD"].any() and d1["qLDiagInv"].all()
  for n in d1:
    assert np.array_equal(d1[n].view(np.uint64), d0[n].view(np.uint64)), n
  if B == 65:
    ref, _ = oracle_batch(m, q, v, a, ("qM", "qLD", "qLDiagInv", "qfrc_inverse"))
    assert_close(f1, ref["qfrc_inverse"], "qfrc_inverse (row-major)")
    for n in ref:
      assert_close(d1[n], ref[n], n)
