"""Model-constant stores written once per context (codegen.CONST_ONCE) -- GPU.

k_const_<name> writes the generator-constant output slots over the whole capacity before the
context's first launch of generated code, and again after mjhip_mirrorUpload or
mjhip_contextLoadKernel; the stage bodies no longer store them. Context capacity 192 with
batches of 65 and 130: one full block, one partial block, and one block no call ever serves.
The generic reference runs on a context of its own, so that it cannot fill the slots in.
"""
import ctypes

import numpy as np
import pytest

from mujoco_inversedynamicstest_amd import codegen, engine, fields, specialize
from mujoco_inversedynamicstest_amd.sampler import sample_states

pytestmark = pytest.mark.gpu
RTOL = 1e-10                      # tests/test_gpu.py's parity bar
CAP, B1, B2 = 192, 65, 130
OUTPUTS = [f.name for f in fields.DATA_FIELDS if f.stage > 0]


def assert_close(gpu, cpu, what):
  gpu = np.asarray(gpu).reshape(len(gpu), -1)
  cpu = np.asarray(cpu).reshape(len(cpu), -1)
  scale = np.maximum(1.0, np.abs(cpu).max(axis=1))
  err = (np.abs(gpu - cpu).max(axis=1) / scale).max()
  assert err <= RTOL, f"{what}: normwise relative error {err:.3e} > {RTOL}"


def _fields(e, m, n):
  return {f: e.field(f, 0, n) for f in OUTPUTS if fields.DATA_FIELD[f].size(m.sizes)}


def _counts(e, n):
  return e.field_int("efc_count", 0, n)


@pytest.fixture(scope="module")
def states(humanoid):
  # some instances past a joint range: the work-list's constraint kernel serves them
  q, v, a = sample_states(humanoid, B2, first=40)
  j = int(np.flatnonzero(np.asarray(humanoid.jnt_limited))[3])
  q[::7, humanoid.jnt_qposadr[j]] = humanoid.jnt_range[j][1] + 0.2
  return q, v, a


@pytest.fixture(scope="module")
def generic(humanoid, states):
  """The generic kernel's fields and counts on the states, computed once on its own context."""
  q, v, a = states
  e = engine.InverseEngine(humanoid, capacity=CAP, specialize=False)
  try:
    f = e.inverse(q, v, a, generic=True)
    assert e.last_path == 0 and e.const_launches == 0
    return f, _fields(e, humanoid, B2), _counts(e, B2)
  finally:
    e.close()


def _check_constants(e, m, ref_fields, what):
  """Every constant slot of every instance of the capacity, served or not, holds the value the
  generic kernel stored for its first instance."""
  const = codegen.const_slots(m)
  assert const
  for f in sorted({f for f, _ in const}):
    ks = [k for g, k in const if g == f]
    got = e.field(f, 0, e.capacity)[:, ks]
    assert_close(got, np.broadcast_to(ref_fields[f][0, ks], got.shape), f"{what}: constant {f}")


def test_parity_count_upload_and_second_call(humanoid, states, generic):
  q, v, a = states
  gf, gfields, gcounts = generic
  const = codegen.const_slots(humanoid)
  e = engine.InverseEngine(humanoid, capacity=CAP)
  try:
    assert e.fast_kernel == "humanoid" and e.capacity == CAP
    # count: the library's equals the generator's
    assert e.const_stores == len(const) > 0
    assert e.const_launches == 0
    # parity after ONE fast-path call, a full and a partial block served
    f = e.inverse(q[:B1], v[:B1], a[:B1])
    assert e.last_path == 1 and e.const_launches == 1
    assert_close(f, gf[:B1], "qfrc_inverse")
    got = _fields(e, humanoid, B1)
    for name in got:
      assert_close(got[name], gfields[name][:B1], name)
    np.testing.assert_array_equal(_counts(e, B1), gcounts[:B1])
    assert (gcounts[:B1, 0] > 0).any()
    # the partial block's idle lanes and the block no call touches hold the constants too
    _check_constants(e, humanoid, gfields, "first call")
    # upload: garbage over a world-body field and ten_J of every instance, then one call
    for name in ("xmat", "ten_J"):
      S = fields.DATA_FIELD[name].size(humanoid.sizes)
      e.set_field(name, np.full((CAP, S), 12345.678))
      assert (e.field(name, 0, CAP) == 12345.678).all()
    f = e.inverse(q, v, a)
    assert e.const_launches == 2
    assert_close(f, gf, "qfrc_inverse after the upload")
    got = _fields(e, humanoid, B2)
    for name in ("xmat", "ten_J"):
      assert_close(got[name], gfields[name], f"{name} after the upload")
    _check_constants(e, humanoid, gfields, "after the upload")
    # second call: nothing is stale, no k_const
    f = e.inverse(q, v, a)
    assert e.const_launches == 2 and e.last_path == 1
    assert_close(f, gf, "qfrc_inverse, second call")
    np.testing.assert_array_equal(_counts(e, B2), gcounts)
  finally:
    e.close()


def test_interleaved_paths(humanoid, states, generic):
  """A skip stage, mjd_inverseFD with 2 base states, then a plain call: each path runs k_const
  when the slots are stale, and the last call's fields are a fresh context's bit for bit."""
  q, v, a = states
  fresh = engine.InverseEngine(humanoid, capacity=CAP)
  try:
    ff = fresh.inverse(q, v, a)
    want = _fields(fresh, humanoid, B2)
    want_counts = _counts(fresh, B2)
  finally:
    fresh.close()
  e = engine.InverseEngine(humanoid, capacity=CAP)
  try:
    e.inverse(q, v, a)
    assert e.const_launches == 1
    S = fields.DATA_FIELD["ten_J"].size(humanoid.sizes)
    e.set_field("ten_J", np.full((CAP, S), -7.5))
    e.inverse(q, v * 0.9, a, skipstage=engine.mjSTAGE_POS)
    assert e.last_path == 2 and e.const_launches == 2
    assert_close(e.field("ten_J", 0, CAP), np.broadcast_to(generic[1]["ten_J"][0], (CAP, S)),
                 "ten_J after the skip call")
    S = fields.DATA_FIELD["xmat"].size(humanoid.sizes)
    e.set_field("xmat", np.full((CAP, S), -7.5))
    assert 2 * (3 * humanoid.nv + 1) <= CAP
    e.inverse_fd(q[:2], v[:2], a[:2])
    assert e.const_launches == 3
    f = e.inverse(q, v, a)
    assert e.last_path == 1 and e.const_launches == 3
    np.testing.assert_array_equal(f, ff)
    got = _fields(e, humanoid, B2)
    for name in got:
      np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    np.testing.assert_array_equal(_counts(e, B2), want_counts)
    _check_constants(e, humanoid, generic[1], "after the interleaved calls")
  finally:
    e.close()


def test_runtime_kernel(inertia):
  """A run-time code object (specialize.py, mjhip_contextLoadKernel) carries its own k_const:
  loading it makes the slots stale, and its results match the generic kernel's. The model is
  the bundled contact-free `inertia` (constraint mode none, so qfrc_constraint is among the
  constants); its context first selects the bundled kernel, which the loaded one replaces."""
  m = inertia
  assert codegen.fast_path_supported(m) is None and codegen.constraint_mode(m) == "none"
  const = codegen.const_slots(m)
  assert sum(f == "qfrc_constraint" for f, _ in const) == m.nv
  q, v, a = sample_states(m, B2, first=3)
  g = engine.InverseEngine(m, capacity=CAP, specialize=False)
  try:
    gf = g.inverse(q, v, a, generic=True)
    assert g.last_path == 0 and g.const_launches == 0
    gfields, gcounts = _fields(g, m, B2), _counts(g, B2)
  finally:
    g.close()
  e = engine.InverseEngine(m, capacity=CAP, specialize=False)
  try:
    assert e.fast_kernel == "inertia" and e.const_stores == len(const)
    e.inverse(q[:B1], v[:B1], a[:B1])
    assert e.last_path == 1 and e.const_launches == 1
    name = specialize.load(e)
    assert e.fast_kernel == name and name.startswith("rt_")
    assert e.const_stores == len(const) > 0
    # garbage where only k_const writes: the loaded object's own k_const must restore it
    S = fields.DATA_FIELD["qfrc_constraint"].size(m.sizes)
    raw = engine.lib().mjhip_mirrorDevicePtr(e.ctx, b"qfrc_constraint")
    assert raw
    junk = np.full(CAP * S, 99.5)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(raw, junk.ctypes.data, junk.nbytes, 1) == 0
    assert (e.field("qfrc_constraint", 0, CAP) == 99.5).all()
    f = e.inverse(q[:B1], v[:B1], a[:B1])
    assert e.last_path == 1 and e.const_launches == 2       # loading set the flag
    assert_close(f, gf[:B1], "qfrc_inverse")
    got = _fields(e, m, B1)
    for fname in got:
      assert_close(got[fname], gfields[fname][:B1], fname)
    np.testing.assert_array_equal(_counts(e, B1), gcounts[:B1])
    _check_constants(e, m, gfields, "run-time kernel")
    f = e.inverse(q, v, a)
    assert e.const_launches == 2
    assert_close(f, gf, "qfrc_inverse, second call")
  finally:
    e.close()
