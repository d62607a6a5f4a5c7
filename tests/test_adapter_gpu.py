"""The reference-side adapter (integration/engine_inverse_mjhip.c) driving the real
libmjhip.so on the GPU: mj_inverseSkip (NONE, POS, VEL), the stage functions and
mj_compareFwdInv on real mjModel/mjData structs with a real arena (SURVEY.md §8 row b).

The adapter is compiled by __graft_entry__.build() against the reference's public headers
(mjModel/mjData layout) together with the test harness's struct builder
(tests/adapter_harness.c) and linked to libmjhip.so: oracle/_ref/libadapter_gpu.so. A
machine without the reference's headers runs the file built where they exist (oracle/_ref
travels with the tree); a missing file is a failure. Checked against the CPU
oracle on the same states: counts exact, qfrc_inverse and the constraint rows to the
north-star 1e-10, contacts to 1e-12, solver_fwdinv of mj_compareFwdInv to 1e-10; the
position-skipping calls read and update the rows the adapter left in the arena.
"""
import os

import numpy as np
import pytest

from mujoco_inversedynamicstest_amd import engine, models
from mujoco_inversedynamicstest_amd.sampler import sample_contact_states, sample_states
from oracle.oracle import Oracle

import adapter_common
from adapter_common import Adapter

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_ref", "libadapter_gpu.so")
RTOL = 1e-10


@pytest.fixture(scope="module")
def lib():
  if not os.path.exists(LIB):
    pytest.fail(f"{LIB} not built: run __graft_entry__.build() where the reference headers "
                "exist (the adapter compiles against them)")
  engine.lib()             # libmjhip.so first, bound to torch's HIP runtime (engine.lib)
  return adapter_common.load(LIB)


def _close(a, b, tol, what):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  assert a.shape == b.shape, what
  scale = max(1.0, float(np.abs(b).max(initial=0)))
  err = float(np.abs(a - b).max(initial=0)) / scale
  assert err <= tol, f"{what}: {err:.3e}"


def _rows(A, o, m):
  assert (A.s("nefc"), A.s("ne"), A.s("nf"), A.s("nl")) == \
      (o.efc.nefc, o.efc.ne, o.efc.nf, o.efc.nl)
  for name in ("efc_type", "efc_id", "efc_state"):
    np.testing.assert_array_equal(A.efc(name, 1, np.int32), o.efc_field(name), err_msg=name)
  for name, w in (("efc_J", m.nv), ("efc_pos", 1), ("efc_aref", 1), ("efc_force", 1)):
    _close(A.efc(name, w), o.efc_field(name), RTOL, name)


def _states():
  mc = models.load("humanoid")
  qc, vc, ac = sample_contact_states(mc, 6)
  ml = models.load("humanoid", disable_contact=True)
  ql, vl, al = sample_states(ml, 48, margin=-0.15, resample_tendons=False)
  return [(mc, qc[i], vc[i], ac[i]) for i in range(6)] + \
         [(ml, ql[i], vl[i], al[i]) for i in range(0, 48, 8)]


def test_inverse_skip_through_adapter(lib):
  rng = np.random.default_rng(8)
  ncon = 0
  for m, q, v, a in _states():
    A, o = Adapter(lib, m), Oracle(m)
    try:
      A.set_state(q, v, a)
      assert A.call(0, 0) == (0, "")
      ref = o.inverse(q, v, a)
      _close(A.field("qfrc_inverse"), ref, RTOL, "qfrc_inverse")
      _rows(A, o, m)
      assert A.s("ncon") == o.efc.ncon
      if o.efc.ncon:
        dv, iv = A.contacts()
        np.testing.assert_array_equal(iv[:, 1:3], o.contact_field("con_geom"))
        _close(dv[:, 0], o.contact_field("con_dist"), 1e-12, "con_dist")
        _close(dv[:, 4:13], o.contact_field("con_frame"), 1e-12, "con_frame")
      ncon += A.s("ncon")
      for skip in (1, 2):                 # rows read and updated in the arena in place
        v2 = v if skip == 2 else v + rng.normal(size=m.nv)
        a2 = a + rng.normal(size=m.nv)
        A.field("qvel")[:] = v2
        A.field("qacc")[:] = a2
        assert A.call(0, skip) == (0, "")
        o.set_state(None, v2, a2)
        _close(A.field("qfrc_inverse"), o.inverse(skipstage=skip), RTOL, f"skip {skip}")
        _rows(A, o, m)
    finally:
      A.close()
  assert ncon >= 6


def test_stage_functions_and_compare_fwd_inv_through_adapter(lib):
  for m, q, v, a in _states()[:3] + _states()[6:8]:
    A, o = Adapter(lib, m), Oracle(m)
    try:
      A.set_state(q, v, a)
      assert A.call(2) == (0, "")          # mj_invPosition
      assert A.call(3) == (0, "")          # mj_invVelocity
      assert A.call(4) == (0, "")          # mj_invConstraint
      o.inverse(q, v, a)
      for name in ("qM", "qLD", "cvel", "qfrc_bias", "qfrc_passive", "qfrc_constraint"):
        _close(A.field(name), getattr(o.d, name), RTOL, name)
      _rows(A, o, m)
      A.field("qfrc_applied")[:] = np.linspace(-1, 1, m.nv)
      o.d.qfrc_applied[:] = np.linspace(-1, 1, m.nv)
      assert A.call(5) == (0, "")          # mj_compareFwdInv
      fw = np.ctypeslib.as_array(lib.hx_solver_fwdinv(A.h), (2,)).copy()
      ref = o.compare_fwd_inv()
      np.testing.assert_allclose(fw, ref, rtol=1e-8, atol=1e-10)
    finally:
      A.close()


def test_humanoid100_through_adapter(lib):
  """The reference's 627-dof humanoid100 (sparse Jacobians, mj_isSparse) through
  mj_inverseSkip(NONE, POS, VEL) into the real libmjhip.so: the adapter lays out the
  reference's compressed arena (efc_J/efc_JT over nJ entries, their rownnz/rowadr/colind,
  ten_J's structure); counts and structure exact, qfrc_inverse and the rows to 1e-10, and
  the position-skipping calls read and update the compressed rows in place."""
  import humanoid100_states as H
  m = H.model()
  q, v, a = H.states(m, 3, seed=9)
  rng = np.random.default_rng(9)
  for i in range(3):
    A, o = Adapter(lib, m, narena=256 << 20), Oracle(m)
    try:
      A.set_state(q[i], v[i], a[i])
      assert A.call(0, 0) == (0, "")
      ref = o.inverse(q[i], v[i], a[i])
      _close(A.field("qfrc_inverse"), ref, RTOL, "qfrc_inverse")
      sp, nefc, nJ = o.efc_sparse(), o.efc.nefc, o.efc.nJ
      assert (A.s("nefc"), A.s("nJ"), A.s("ncon")) == (nefc, nJ, o.efc.ncon)
      assert nJ < nefc * m.nv // 20
      for name in ("efc_type", "efc_id", "efc_state"):
        np.testing.assert_array_equal(A.efc(name, 1, np.int32), o.efc_field(name))
      for name in ("efc_J_rownnz", "efc_J_rowadr"):
        np.testing.assert_array_equal(A.arr(name, nefc, np.int32), sp[name])
      for name in ("efc_J_colind", "efc_JT_colind"):
        np.testing.assert_array_equal(A.arr(name, nJ, np.int32), sp[name])
      _close(A.arr("efc_J", nJ), sp["efc_J"], RTOL, "efc_J")
      _close(A.arr("efc_JT", nJ), sp["efc_JT"], RTOL, "efc_JT")
      for name in ("efc_force", "efc_aref"):
        _close(A.efc(name), o.efc_field(name), RTOL, name)
      for skip in (1, 2):
        v2 = v[i] if skip == 2 else v[i] + rng.normal(size=m.nv)
        a2 = a[i] + rng.normal(size=m.nv)
        A.field("qvel")[:] = v2
        A.field("qacc")[:] = a2
        assert A.call(0, skip) == (0, "")
        o.set_state(None, v2, a2)
        _close(A.field("qfrc_inverse"), o.inverse(skipstage=skip), RTOL, f"skip {skip}")
        _close(A.efc("efc_force"), o.efc_field("efc_force"), RTOL, "efc_force")
        assert A.s("nJ") == nJ
    finally:
      A.close()
