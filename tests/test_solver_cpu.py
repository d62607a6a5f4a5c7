"""mj_forward with the Newton constraint solver of the device path (csrc/solver.h) compiled for
the host (tests/solver_harness.cpp): bit for bit against the plain-Python restatement
tests/solver_ref.py, the reference's forward/inverse identity (ForwardInverseMatch,
test/engine/engine_inverse_test.cc:35-56), the KKT conditions by hand, the options, and a
stand-alone AddressSanitizer program on exact-size arrays."""
import os
import struct
import subprocess

import numpy as np
import pytest

import solver_cases as sc
import solver_ref
from kernel_harness import BUILD, HERE
from mujoco_inversedynamicstest_amd import fields, host
from solver_harness import FLAGS, SRC, SolverCPU, solver_options

DSBL_WARMSTART = 1 << 8
CNSTRFULL = 1 << 4
QUADRATIC, LINEARNEG, LINEARPOS = 1, 2, 3

CASES = {
    "two_hinge": (sc.two_hinge, lambda m: sc.two_hinge_states(12)),
    "connect": (sc.connect_model, lambda m: sc.equality_states(m, 4)),
    "weld": (sc.weld_model, lambda m: sc.equality_states(m, 4)),
    "humanoid": (sc.humanoid, lambda m: sc.humanoid_states(m, 8)),
    "reference": (sc.reference_model, lambda m: sc.reference_states(m, 3)),
}

_cache = {}


def _case(name):
  """(model, qpos, qvel, host build, oracle problem source), made once per module run."""
  if name not in _cache:
    m = CASES[name][0]()
    q, v = CASES[name][1](m)
    _cache[name] = (m, q, v, SolverCPU(m), sc.OracleProblem(m))
  return _cache[name]


def _same(a, b):
  """Bit-for-bit equality of two float sequences (NaN-safe, signed zeros told apart)."""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  return a.shape == b.shape and a.tobytes() == b.tobytes()


def _compare(got, ref, what):
  for k in ("qacc", "efc_force", "cost", "alpha", "qfrc_constraint"):
    assert _same(got[k], ref[k]), f"{what}: {k}\n{got[k]}\n{ref[k]}"
  assert list(got["efc_state"]) == list(ref["efc_state"]), f"{what}: efc_state"
  for k in ("niter", "warm", "nupdate", "ndowndate", "nrefactor"):
    assert got[k] == ref[k], f"{what}: {k} {got[k]} != {ref[k]}"


@pytest.mark.parametrize("name", list(CASES))
def test_host_build_equals_restatement_bitwise(name):
  """Cold (qacc_warmstart = 0), warm (a second call from the first call's result: at most one
  iteration) and with mjDSBL_WARMSTART, on every state of the case."""
  m, Q, V, s, op = _case(name)
  o = solver_options(m)
  rows = 0
  for i in range(len(Q)):
    p = op.problem(Q[i], V[i])
    # the rows the device pipeline makes are the oracle's (its own tests): the solver's inputs
    cold = s.forward_solve(Q[i], V[i], qacc_warmstart=np.zeros(m.nv))
    assert cold["status"] == 0 and cold["nefc"] == p.nefc
    assert _same(s.field("efc_aref")[:p.nefc], p.aref)
    assert _same(s.d.qacc_smooth, p.qacc_smooth)
    rcold = solver_ref.fwd_constraint(p, [0.0] * m.nv, o)
    _compare(cold, rcold, f"{name}[{i}] cold")
    assert _same(s.qacc_warmstart, rcold["qacc_warmstart"])
    warm = s.forward_solve(Q[i], V[i])               # the kept warmstart
    rwarm = solver_ref.fwd_constraint(p, rcold["qacc_warmstart"], o)
    _compare(warm, rwarm, f"{name}[{i}] warm")
    assert warm["niter"] <= 1
    if p.nefc:
      assert warm["warm"] == 1
    rows += p.nefc > 0
    m.opt["disableflags"] |= DSBL_WARMSTART
    try:
      s2 = SolverCPU(m)
      s2.qacc_warmstart[:] = 1.0                     # must not be looked at
      nows = s2.forward_solve(Q[i], V[i])
      p.disableflags |= DSBL_WARMSTART
      _compare(nows, solver_ref.fwd_constraint(p, [1.0] * m.nv, o), f"{name}[{i}] nowarm")
      assert nows["warm"] == 0
    finally:
      m.opt["disableflags"] &= ~DSBL_WARMSTART
  assert rows > 0


@pytest.mark.parametrize("name", ["connect", "weld"])
def test_friction_rows_reach_every_state(name):
  """What the connect and weld cases are for: over the case's states the friction-loss row
  ends QUADRATIC, LINEARNEG and LINEARPOS, so the friction branches of constraintUpdate and
  of the line search's evaluation are among what the bit-for-bit comparison covers; and a
  LINEAR row carries exactly -/+ frictionloss."""
  m, Q, V, s, op = _case(name)
  seen = set()
  for i in range(len(Q)):
    r = s.forward_solve(Q[i], V[i], qacc_warmstart=np.zeros(m.nv))
    ne, nf = int(s.field("efc_count")[1]), int(s.field("efc_count")[2])
    assert nf >= 1 and len(r["alpha"]) >= 1       # the line search ran with friction rows
    for k in range(ne, ne + nf):
      st, floss = int(r["efc_state"][k]), s.field("efc_frictionloss")[k]
      seen.add(st)
      if st == LINEARNEG:
        assert r["efc_force"][k] == floss > 0
      if st == LINEARPOS:
        assert r["efc_force"][k] == -floss < 0
  assert seen == {QUADRATIC, LINEARNEG, LINEARPOS}


def test_two_hinge_covers_none_one_and_two_rows():
  m, Q, V, s, op = _case("two_hinge")
  counts = {op.problem(Q[i], V[i]).nefc for i in range(len(Q))}
  assert counts == {0, 1, 2}


def test_no_rows_takes_the_early_exit():
  """nefc == 0 (engine_forward.c:662-668): qacc = qacc_warmstart = qacc_smooth's bytes."""
  m = sc.two_hinge()
  s = SolverCPU(m)
  s.qacc_warmstart[:] = 7.0
  s.d.qfrc_applied[:] = [0.3, -0.2]
  r = s.forward_solve([0.01, -0.02], [0.5, 0.1])
  assert r["nefc"] == 0 and r["niter"] == 0 and r["status"] == 0
  assert _same(r["qacc"], s.d.qacc_smooth) and _same(s.qacc_warmstart, s.d.qacc_smooth)
  assert not r["qfrc_constraint"].any()


def _downdate_state():
  """Joint 1 beyond its lower limit, joint 2 just beyond its upper one and moving back: the
  force on joint 1 accelerates joint 2 out of its limit (the off-diagonal of M^-1 is
  negative), so its row is QUADRATIC at qacc_smooth and SATISFIED at the solution."""
  return np.array([-0.07584151, 0.05061259]), np.array([0.1921268, -0.00826382])


def test_row_leaves_quadratic_between_iterations():
  """HessianIncremental's downdate (mju_cholUpdate with flg_plus = 0) runs, in the host build
  and in the restatement alike."""
  m = sc.two_hinge()
  s, op = SolverCPU(m), sc.OracleProblem(m)
  q, v = _downdate_state()
  p = op.problem(q, v)
  r = s.forward_solve(q, v, qacc_warmstart=np.zeros(2))
  ref = solver_ref.fwd_constraint(p, [0.0, 0.0], solver_options(m))
  _compare(r, ref, "downdate")
  assert r["ndowndate"] >= 1
  jar0 = np.asarray(p.mul_jac_vec(p.qacc_smooth)) - np.asarray(p.aref)
  assert (jar0 < 0).all()                            # both rows QUADRATIC at the start
  assert list(r["efc_state"]).count(QUADRATIC) == 1  # one left


@pytest.mark.parametrize("name", list(CASES))
def test_forward_inverse_identity(name):
  """tolerance = 0, iterations = 100: the oracle's mj_inverse of the solved qacc returns the
  applied forces and the same constraint force. The bounds are solver_cases.fwdinv_bound's."""
  m, Q, V, s, op = _case(name)
  o = solver_options(m, tolerance=0.0, iterations=100)
  ref_vals, got = [], []
  for i in range(len(Q)):
    p = op.problem(Q[i], V[i])
    if not p.nefc:
      continue
    r = solver_ref.fwd_constraint(p, [0.0] * m.nv, o)
    ref_vals.append(op.fwdinv(Q[i], V[i], r["qacc"], r["qfrc_constraint"]))
    h = s.forward_solve(Q[i], V[i], qacc_warmstart=np.zeros(m.nv), tolerance=0.0,
                        iterations=100)
    got.append(op.fwdinv(Q[i], V[i], h["qacc"], h["qfrc_constraint"]))
  ref_vals, got = np.array(ref_vals), np.array(got)
  print(f"{name}: restatement fwdinv max {ref_vals.max(axis=0)}, host build {got.max(axis=0)}")
  if name == "reference":
    assert ref_vals.max() < sc.FWDINV_REFERENCE_BOUND   # else: replace the state, not the bound
  for k in range(2):
    bound = sc.fwdinv_bound(ref_vals[:, k], reference_model=name == "reference")
    assert got[:, k].max() <= bound if name != "reference" else got[:, k].max() < bound


def test_kkt_by_hand():
  """Two hinges, one active limit: force >= 0, complementarity to round-off, and qacc is the
  closed form qacc_smooth + M^-1 J' f with f from the scalar problem
  f = -D (J qacc_smooth - aref + A f), A = J M^-1 J'. The rows are soft: the slack that is
  complementary to the force is jar + R force (the dual's A f + b + R f), which is 0 on an
  active row, where jar itself is -R force < 0; force * jar = 0 holds on an inactive row."""
  m = sc.two_hinge()
  s, op = SolverCPU(m), sc.OracleProblem(m)
  q, v = np.array([-0.08, 0.01]), np.array([-0.3, 0.2])
  s.d.qfrc_applied[:] = [-0.05, 0.02]
  op.o.d.qfrc_applied[:] = [-0.05, 0.02]
  r = s.forward_solve(q, v, qacc_warmstart=np.zeros(2), tolerance=0.0)
  p = op.problem(q, v)
  assert p.nefc == 1 and r["status"] == 0
  f = r["efc_force"][0]
  J = np.array(p.J)
  jar = J @ r["qacc"] - p.aref[0]
  assert f > 0
  assert abs(f * (jar + p.R[0] * f)) <= 1e-12 * p.R[0] * f * f
  M = op.o.fullM()
  Minv = np.linalg.inv(M)
  A = J @ Minv @ J
  b = J @ np.array(p.qacc_smooth) - p.aref[0]
  f_closed = -b / (A + 1 / p.D[0])
  qacc_closed = np.array(p.qacc_smooth) + Minv @ J * f_closed
  assert abs(f - f_closed) <= 1e-12 * abs(f_closed)
  assert np.abs(r["qacc"] - qacc_closed).max() <= 1e-12 * np.abs(qacc_closed).max()
  # an inactive row: zero force, jar >= 0 (force * jar = 0 exactly)
  r0 = s.forward_solve([0.051, 0.0], [-5.0, 0.0], qacc_warmstart=np.zeros(2))
  assert r0["nefc"] == 1 and r0["efc_force"][0] == 0.0 and r0["efc_state"][0] == 0
  p0 = op.problem([0.051, 0.0], [-5.0, 0.0])
  jar0 = np.array(p0.J) @ r0["qacc"] - p0.aref[0]
  assert jar0 >= 0 and r0["efc_force"][0] * jar0 == 0.0


def test_options():
  m, Q, V, s, _ = _case("humanoid")
  z = np.zeros(m.nv)
  one = s.forward_solve(Q[0], V[0], qacc_warmstart=z, iterations=1)
  assert one["niter"] == 1 and len(one["alpha"]) == 1
  dflt = s.forward_solve(Q[0], V[0], qacc_warmstart=z)
  full = s.forward_solve(Q[0], V[0], qacc_warmstart=z, tolerance=0.0)
  assert 1 < dflt["niter"] <= full["niter"]
  assert solver_options(m)["tolerance"] == 1e-8


def test_meaninertia_and_solver_options_are_read():
  """setconst computes stat.meaninertia as mj_setConst does; <option> carries the solver's
  settings, and only those it names enter m.opt."""
  from mujoco_inversedynamicstest_amd import mjcf
  from oracle.oracle import Oracle
  m = sc.two_hinge()
  o = Oracle(m)
  o.inverse(m.qpos0, np.zeros(2), np.zeros(2))
  M = o.fullM()
  assert abs(m.stat["meaninertia"] - np.trace(M) / 2) <= 1e-15 * np.trace(M)
  assert m.solver_opt == {} and mjcf.solver_options(m) == mjcf.SOLVER_DEFAULTS
  x = sc.TWO_HINGE_LIMIT.replace('<option gravity="0 0 0"/>',
                                 '<option gravity="0 0 0" solver="CG" iterations="7" '
                                 'tolerance="1e-6" ls_iterations="9" ls_tolerance="0.1" '
                                 'noslip_iterations="2"/>')
  m2 = mjcf.load_xml_string(x)
  assert mjcf.solver_options(m2) == {"solver": 1, "iterations": 7, "tolerance": 1e-6,
                                     "ls_iterations": 9, "ls_tolerance": 0.1,
                                     "noslip_iterations": 2}
  # no existing hash or struct sees them: not opt, so neither the signature nor the name of
  # the model's run-time kernel (codegen.model_hash)
  from mujoco_inversedynamicstest_amd import codegen
  assert m2.opt == m.opt
  assert fields.model_signature(m2) == fields.model_signature(m)
  assert codegen.model_hash(m2) == codegen.model_hash(m)


def test_solver_options_survive_the_model_file(tmp_path):
  """Model.save / Model.load keep solver_opt beside opt."""
  from mujoco_inversedynamicstest_amd import codegen, mjcf
  m = sc.two_hinge()
  h = codegen.model_hash(m)
  m.solver_opt.update(iterations=7, tolerance=1e-6)
  path = str(tmp_path / "m.npz")
  m.save(path)
  r = mjcf.Model.load(path)
  assert r.solver_opt == {"iterations": 7, "tolerance": 1e-6}
  assert mjcf.solver_options(r)["iterations"] == 7 and codegen.model_hash(r) == h


def test_solve_options_does_not_write_the_model():
  """A model file carries no statistics: meaninertia is computed as mj_setConst does, once,
  and the caller's model stays as it was."""
  from mujoco_inversedynamicstest_amd import engine, setconst
  m = sc.connect_model()
  before = dict(m.stat)
  sin = engine.solve_options(m)
  assert m.stat == before == {}
  assert sin.meaninertia == setconst.mean_inertia(m) > 0
  assert engine.solve_options(m, iterations=3).iterations == 3


def test_mjb_meaninertia_is_read_from_the_files_statistics():
  """mjStatistic follows mjOption and mjVisual in the file and meaninertia is its first
  member (mjmodel.h): a buffer written with a known value reads back with it; one written
  without statistics (0) leaves the model's stat empty and the value is computed."""
  from mujoco_inversedynamicstest_amd import engine, mjb, setconst
  m = sc.two_hinge()
  buf = bytearray(mjb.write(m))
  base = mjb.NHEADER * 4 + 4 * len(mjb.INTS) + 8 * len(mjb.SIZES)
  at = base + mjb.SIZEOF_OPTION + mjb.SIZEOF_VISUAL
  assert struct.unpack_from("<7d", buf, at) == (0.0,) * 7      # the statistics block, empty
  assert struct.unpack_from("<d", buf, base)[0] == m.opt["timestep"]   # mjOption starts here
  ints, sizes, opt, arrays, stat = mjb.read_raw(bytes(buf))
  assert stat == {"meaninertia": 0.0}
  r = mjb.read(bytes(buf))
  assert r.stat == {} and engine.mean_inertia(r) == setconst.mean_inertia(r)
  struct.pack_into("<d", buf, at, 0.4375)
  r = mjb.read(bytes(buf))
  assert r.stat == {"meaninertia": 0.4375} and engine.solve_options(r).meaninertia == 0.4375
  assert mjb.read_raw(bytes(buf))[4] == {"meaninertia": 0.4375}
  for f in fields.MODEL_FIELDS:                                # nothing else moved
    assert np.array_equal(getattr(r, f.name), getattr(m, f.name)), f.name


def _dump_model(m, path):
  """The model as tests/solver_san_main.cpp reads it (transition_san_main.cpp's format)."""
  cm = host.model_struct(m)
  with open(path, "wb") as f:
    for k in fields.MODEL_SIZES:
      f.write(struct.pack("<i", int(getattr(cm, k))))
    f.write(bytes(cm.opt))
    for fl in fields.MODEL_FIELDS:
      a = np.ascontiguousarray(getattr(m, fl.name), dtype=fields.NPTYPE[fl.ctype])
      f.write(struct.pack("<q", a.size))
      f.write(a.tobytes())


@pytest.fixture(scope="module")
def san_program():
  exe = os.path.join(BUILD, "solver_san")
  src = os.path.join(HERE, "solver_san_main.cpp")
  os.makedirs(BUILD, exist_ok=True)
  deps = [src] + SRC
  if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
    tmp = f"{exe}.{os.getpid()}"
    subprocess.run(["g++", *FLAGS, "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", tmp, src], check=True)
    os.replace(tmp, exe)
  return exe


@pytest.mark.parametrize("name", ["two_hinge", "connect", "humanoid"])
def test_sanitized_program_on_exact_size_arrays(name, san_program, tmp_path):
  """Every model, data, row and solver-scratch array is a heap block of its exact size, with
  efc_cap equal to the rows the state makes: the program's qacc is the harness's, bit for bit.
  One row less is MJHIP_INST_CNSTRFULL, and that instance is not solved."""
  m, Q, V, s, op = _case(name)
  i = max(range(len(Q)), key=lambda k: op.problem(Q[k], V[k]).nefc)
  nefc = op.problem(Q[i], V[i]).nefc
  assert nefc > 0
  want = s.forward_solve(Q[i], V[i], qacc_warmstart=np.zeros(m.nv))
  path = str(tmp_path / "model.bin")
  _dump_model(m, path)
  o = solver_options(m)
  args = [repr(float(x)) for x in list(Q[i]) + list(V[i])]
  for cap in (nefc, nefc - 1):
    run = subprocess.run([san_program, path, str(cap), str(s.con_cap), str(o["iterations"]),
                          str(o["ls_iterations"]), repr(o["tolerance"]),
                          repr(o["ls_tolerance"]), repr(o["meaninertia"]), *args],
                         capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stderr[-3000:]
    out = run.stdout.split()
    status, niter = int(out[0]), int(out[1])
    qacc = np.array([float.fromhex(x) for x in out[2:2 + m.nv]])
    smooth = np.array([float.fromhex(x) for x in out[2 + m.nv:2 + 2 * m.nv]])
    if cap == nefc:
      assert status == 0 and niter == want["niter"]
      assert _same(qacc, want["qacc"])
    else:
      assert status & CNSTRFULL and niter == 0
      assert _same(qacc, smooth)
