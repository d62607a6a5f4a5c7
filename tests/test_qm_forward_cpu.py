"""The register forwarding of qM rows in the fused straight-line kernel (codegen.QM_FORWARD):
the plan, the generated text and the host build.

k_all's pos stage produces qM rows at pass-2 post-visits in descending dof order. The last of
them appear while the traversal unwinds and registers fall idle, and the fac stage updates
exactly those rows from its first elimination step, so the HO instantiation passes them on in
a local array (registers once the stage bodies are inlined) instead of through the mirror.
The LDS hand-off (test_qm_handoff_cpu.py) takes the rows before them. A forwarded entry keeps
its plain mirror store, and no output may change by a bit.
"""
import os
import re
import sys

import numpy as np
import pytest

from mujoco_inversedynamicstest_amd import codegen, models
from mujoco_inversedynamicstest_amd.sampler import sample_states
from oracle.oracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
  sys.path.insert(0, HERE)
import va_lds_chain  # noqa: E402
from kernel_harness import KernelCPU  # noqa: E402
from test_codegen_cpu import run_and_compare  # noqa: E402

# the headline model; a chain whose rows outnumber both pools; one without hinges. (A model
# whose rows all fit the LDS pool keeps them there and forwards nothing: inertia, below.)
NAMES = ("humanoid", "va_lds_chain", "connect")


def _load(name):
  m = va_lds_chain.load() if name == "va_lds_chain" else models.load(name, disable_contact=True)
  assert codegen.fast_path_supported(m) is None
  return m


@pytest.fixture(scope="module", params=NAMES)
def model(request):
  return request.param, _load(request.param)


def _rows(m):
  """{dof: its qM entries} and {dof: position in the production order}: pass 2's post-visits
  run in descending body order, a body's dofs in ascending order."""
  rows = {}
  for k in range(m.nv):
    n, j = 0, k
    while j >= 0:
      n, j = n + 1, int(m.dof_parentid[j])
    rows[k] = list(range(int(m.dof_Madr[k]), int(m.dof_Madr[k]) + n))
  order = sorted(range(m.nv), key=lambda k: (-int(m.dof_bodyid[k]), k))
  return rows, {k: t for t, k in enumerate(order)}


def test_plan(model):
  name, m = model
  fwd, lds = codegen.qm_forward_plan(m), codegen.qm_handoff_plan(m)
  rows, produced = _rows(m)
  assert 0 < len(fwd) <= codegen.QM_FORWARD
  assert sorted(fwd.values()) == list(range(len(fwd)))          # one register each
  assert not set(fwd) & set(lds)
  assert len(fwd) + len(lds) <= m.nM
  state = {}
  for k, entries in rows.items():
    f, h = [a in fwd for a in entries], [a in lds for a in entries]
    assert all(f) or not any(f), (name, k)                      # whole rows
    assert all(h) or not any(h), (name, k)
    if int(m.dof_simplenum[k]):
      assert not any(f) and not any(h), (name, k)               # never a row of constants
    else:
      state[k] = "fwd" if f[0] else "lds" if h[0] else "mirror"
  # every row left to the mirror is produced before every forwarded one
  last_mirror = max([produced[k] for k, s in state.items() if s == "mirror"], default=-1)
  assert all(produced[k] > last_mirror for k, s in state.items() if s == "fwd"), name
  # the other order of the LDS plan is what it was: nothing forwarded beside it
  assert codegen._qm_plans(m, None, "early")[1] == {}
  assert codegen.qm_handoff_plan(m) == codegen.qm_handoff_plan(m, None, codegen.QM_ORDER)


def test_humanoid_plan_figures():
  """The last-produced rows (root, waist, right leg, the left leg's first) go in registers up
  to the budget, and the LDS pool stays full: the pairs of the right leg's hinges, free only
  after its pre-visits, hold a right-leg row, the rest the left leg's. 203 of 243 doubles
  stay on-chip; only the arms' rows and one more are re-read."""
  m = _load("humanoid")
  fwd, lds = codegen.qm_forward_plan(m), codegen.qm_handoff_plan(m)
  rows, _ = _rows(m)
  assert all(a in fwd for k in range(1, 9) for a in rows[k])
  assert len(fwd) == codegen.QM_FORWARD == 128
  assert len(lds) == len(codegen.qm_handoff_plan(m, None, "early")) == 75
  assert codegen.k_all_lds_bytes(m) == 38400


def test_small_model_forwards_every_row_without_the_lds_pool(monkeypatch):
  """inertia (nM = 38, three rows of constants): the LDS pool holds every other row, so by
  default nothing is forwarded (test_qm_handoff_cpu.py pins its LDS hand-off); with the pool
  withheld (QM_LDS) all of them are, and the LDS plan is empty."""
  m = _load("inertia")
  rows, _ = _rows(m)
  want = {a for k in range(m.nv) if not int(m.dof_simplenum[k]) for a in rows[k]}
  assert m.nM <= codegen.QM_FORWARD and any(int(x) for x in m.dof_simplenum)
  assert codegen.qm_forward_plan(m) == {} and set(codegen.qm_handoff_plan(m)) == want
  monkeypatch.setattr(codegen, "QM_LDS", False)
  assert set(codegen.qm_forward_plan(m)) == want
  assert codegen.qm_handoff_plan(m) == {}


@pytest.mark.parametrize("switch", ["QM_HANDOFF", "FUSE", "QM_FORWARD"])
def test_switches_empty_the_plan(switch, monkeypatch):
  m = _load("humanoid")
  monkeypatch.setattr(codegen, switch, 0 if switch == "QM_FORWARD" else False)
  assert codegen.qm_forward_plan(m) == {}
  if switch == "QM_FORWARD":      # the LDS plan alone, as before there was forwarding
    assert len(codegen.qm_handoff_plan(m)) == 75


def _body(text, fn, name):
  return text[text.index(f"void {fn}_{name}("):].split("\n}\n")[0]


def test_generated_text(model):
  name, m = model
  fwd = codegen.qm_forward_plan(m)
  text = codegen.generate(m, name)
  pos, fac = _body(text, "fast_pos", name), _body(text, "fast_fac", name)
  for a, i in fwd.items():
    # one assignment beside the entry's plain (temporal) store, one take
    assert pos.count(f"if constexpr (HO) fw[{i}] = v_; }}") == 1
    assert len(re.findall(rf"^\s*P_qM\[{a}\*64\] = v_;$", pos, re.M)) == 1
    assert fac.count(f"const double M_{a} = HO ? fw[{i}] : P_qM[{a}*64];") == 1
  assert len(re.findall(r"\bfw\[", pos)) == len(re.findall(r"\bfw\[", fac)) == len(fwd)
  # the store-rewriting passes leave the assignments alone
  for line in text.split("\n"):
    if re.search(r"\bfw\[", line):
      assert "MJH_NT_" not in line and "!FD" not in line, line
  # the array is declared where both stages run (k_all, the host entry) and nowhere else
  decl = f"double fw[{len(fwd)}];"
  assert text.count(decl) == 2
  assert decl in _body(text, "k_all", name) and decl in _body(text, "fast_body", name)
  for kern in ("k_pos", "k_fac", "k_va", "k_vaskip", "fast_vaskip", "fast_va", "k_acc"):
    if f"void {kern}_{name}(" in text:
      assert not re.search(r"\bfw\b", _body(text, kern, name)), kern
  # every instantiation of k_all exists with and without it, behind the hand-off's switch
  launch = _body(text, "launch_fast", name)
  assert len(re.findall(rf"k_all_{name}<\w+, \w+, true>", launch)) == \
      len(re.findall(rf"k_all_{name}<\w+, \w+, false>", launch)) > 0
  assert f"int qm_forward_{name}() {{ return {len(fwd)}; }}" in text


def test_fd_elision_unchanged(model, monkeypatch):
  """The fields mjd_inverseFD's perturbed blocks leave unstored are the same with and without
  forwarding: its assignments are no mirror stores."""
  name, m = model
  on = [codegen._GEN[st](codegen._Model(m), None) for st in codegen.STAGES]
  monkeypatch.setattr(codegen, "QM_FORWARD", 0)
  off = [codegen._GEN[st](codegen._Model(m), None) for st in codegen.STAGES]
  assert any("fw[" in b for b in on) and not any("fw[" in b for b in off)
  assert codegen.fd_elided(on) == codegen.fd_elided(off)


def test_handoff_false_leaves_no_trace(model):
  name, m = model
  off = codegen.generate(m, name, handoff=False)
  assert not re.search(r"\bfw\b", off) and "HO ?" not in off
  assert f"int qm_forward_{name}() {{ return 0; }}" in off
  assert not re.search(rf"k_all_{name}<\w+, \w+, true>", off)


def test_runtime_code_object_text():
  m = _load("va_lds_chain")
  rt = codegen.generate(m, "rt_x", extern_c=True)
  n = len(codegen.qm_forward_plan(m))
  assert f"int k_qm_forward_rt_x = {n};" in rt and f"double fw[{n}];" in _body(rt, "k_all", "rt_x")
  assert "fast_pos_rt_x<true, false, true>" in rt and "fast_fac_rt_x<true, false, true>" in rt
  off = codegen.generate(m, "rt_x", extern_c=True, handoff=False)
  assert "int k_qm_forward_rt_x = 0;" in off and not re.search(r"\bfw\b", off)


@pytest.mark.parametrize("name,B,limits", [("humanoid", 130, True), ("va_lds_chain", 40, False),
                                           ("inertia", 40, False), ("connect", 40, False)])
def test_host_build_bit_exact(name, B, limits, monkeypatch):
  """fast_body_<name> on the host runs the HO = true bodies with the forwarded entries in its
  local array: every output equals the oracle's bit for bit (130 humanoid states: two full
  blocks and a partial one, limit-active ones among them), and the generic pipeline gives the
  same bits. inertia and connect run with the LDS pool withheld: every non-constant row
  forwarded, no LDS hand-off beside it."""
  m = _load(name)
  if name in ("inertia", "connect"):
    monkeypatch.setattr(codegen, "QM_LDS", False)
    assert "handQM" not in codegen.generate(m, f"{name}_fw")
  assert "fw[" in _body(codegen.generate(m, f"{name}_fw"), "fast_body", f"{name}_fw")
  if limits:
    q, v, a = sample_states(m, B, first=5000, margin=-0.1, resample_tendons=False)
  else:
    q, v, a = sample_states(m, B, first=21)
  nwl = run_and_compare(m, f"{name}_fw", q, v, a)
  assert nwl > 10 or not limits      # the work-list path among the humanoid's states
  o, k = Oracle(m), KernelCPU(m)
  for i in range(0, B, 13):
    ref = o.inverse(q[i], v[i], a[i])
    got, st = k.inverse(q[i], v[i], a[i])
    assert st == 0
    np.testing.assert_array_equal(got, ref)
