"""The va stage's cdof stack in LDS (codegen.VA_LDS_SLOTS): the slot plan, the LDS budget and
the generated code on the host, bit for bit against the oracle and the generic pipeline.

The projections at a body's post-visit take the cdof of its dofs from a per-lane stack the
pre-visit filled (slot = index among the non-constant dofs of the root-to-body path), a free
joint's translational cdof are literals, and qfrc_passive stays in registers. None of it may
change a bit of any output.
"""
import os
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

# every bundled model with a straight-line kernel: (name, model, contacts off, sensors off)
BUNDLED = (("humanoid", "humanoid", True, False), ("humanoid_contact", "humanoid", False, False),
           ("inverse_test", "inverse_test", True, False), ("linear", "linear", True, True),
           ("inertia", "inertia", True, False), ("slider_crank", "slider_crank", False, False))


def test_bundled_list_matches_the_build():
  import __graft_entry__
  assert tuple(__graft_entry__.FAST_MODELS) == BUNDLED


def _paths(m):
  """Root-to-leaf paths as lists of dofs."""
  kids = {b: [] for b in range(m.nbody)}
  for b in range(1, m.nbody):
    kids[int(m.body_parentid[b])].append(b)
  out = []

  def walk(b, dofs):
    dofs = dofs + list(range(int(m.body_dofadr[b]), int(m.body_dofadr[b]) + int(m.body_dofnum[b]))) \
        if b else dofs
    if not kids[b]:
      out.append(dofs)
    for c in kids[b]:
      walk(c, dofs)
  walk(0, [])
  return out


@pytest.mark.parametrize("name,src,dc,ds", BUNDLED)
def test_slot_plan_and_budget(name, src, dc, ds):
  m = models.load(src, disable_contact=dc, disable_sensor=ds)
  cap = codegen.va_lds_capacity(m)
  slot, depth = codegen.va_slot_plan(m, cap)
  assert 0 <= cap <= depth
  for path in _paths(m):
    used = [slot[k] for k in path if k in slot]
    assert len(used) == len(set(used)), (name, path)
    assert all(0 <= s < cap for s in used)
    # a dof without a slot is a literal or lies past the capacity, never a hole below it
    free = [k for k in path if codegen.const_cdof(m, k) is None]
    assert [k in slot for k in free] == [i < cap for i in range(len(free))]
  assert codegen.k_all_lds_bytes(m) <= codegen.LDS_BUDGET == 40960
  # one more slot would not fit (or no path needs one)
  assert cap == depth or codegen.k_all_lds_bytes(m, cap + 1) > codegen.LDS_BUDGET
  # the arrays the generated kernel declares are the ones counted
  src_text = codegen.generate(m, name)
  k_all = src_text[src_text.index(f"void k_all_{name}("):]
  import re
  n = [int(x) for x in re.findall(r"__shared__ double (?:trig|qo_lds)\[(\d+)\];", k_all)[:2]]
  assert 8 * sum(n) == codegen.k_all_lds_bytes(m)


def test_humanoid_plan_figures():
  """The headline model: 8 slots, 24,576 B + 13,824 B, 16 of 27 dofs in a slot and 3 literals."""
  m = models.load("humanoid", disable_contact=True)
  assert codegen.va_lds_capacity(m) == 8
  assert codegen.k_all_lds_bytes(m) == 24576 + 13824
  slot, depth = codegen.va_slot_plan(m, 8)
  assert len(slot) == 16 and depth > 8
  assert sum(codegen.const_cdof(m, k) is not None for k in range(m.nv)) == 3


@pytest.fixture(scope="module")
def chain():
  m = va_lds_chain.load()
  assert codegen.fast_path_supported(m) is None
  types = set(int(t) for t in m.jnt_type)
  assert types == {codegen.FREE, codegen.BALL, codegen.SLIDE, codegen.HINGE}
  cap = codegen.va_lds_capacity(m)
  slot, depth = codegen.va_slot_plan(m, cap)
  assert va_lds_chain.NHINGE > cap and depth > cap >= 1     # both branches are emitted
  q, v, a = sample_states(m, 40, first=21)
  return m, q, v, a


def _branches(m, va_slots=None):
  va = codegen._gen_va(codegen._Model(m, va_slots))
  return va.count("mjh::get6("), va.count("= P_cdof["), va.count("= P_qfrc_passive[")


def test_chain_default_capacity_bitexact(chain):
  m, q, v, a = chain
  gets, rereads, qfp = _branches(m)
  cap = codegen.va_lds_capacity(m)
  free = sum(codegen.const_cdof(m, k) is None for k in range(m.nv))
  assert gets == len(codegen.va_slot_plan(m, cap)[0]) > 0
  assert rereads == 6 * free + 6 * (free - gets) and free - gets > 0   # pre-visits + re-reads
  assert qfp == 0
  run_and_compare(m, "va_chain", q, v, a)
  # the generic pipeline on the host gives the same bits as the oracle, so as the generated code
  o, k = Oracle(m), KernelCPU(m)
  for i in range(0, len(q), 5):
    ref = o.inverse(q[i], v[i], a[i])
    got, st = k.inverse(q[i], v[i], a[i])
    assert st == 0
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("cap", [0, 1])
def test_chain_forced_capacity_bitexact(chain, cap, monkeypatch):
  m, q, v, a = chain
  monkeypatch.setattr(codegen, "VA_LDS_SLOTS", cap)
  text = codegen.generate(m, f"va_chain_cap{cap}")
  monkeypatch.setattr(codegen, "VA_LDS_SLOTS", None)
  assert text == codegen.generate(m, f"va_chain_cap{cap}", va_slots=cap)   # the argument
  assert text != codegen.generate(m, f"va_chain_cap{cap}")
  gets = _branches(m, cap)[0]
  assert gets == (0 if cap == 0 else len(codegen.va_slot_plan(m, 1)[0]))
  assert ("cstk" in codegen._gen_va(codegen._Model(m, cap))) == bool(cap)
  monkeypatch.setattr(codegen, "VA_LDS_SLOTS", cap)
  run_and_compare(m, f"va_chain_cap{cap}", q, v, a)


def test_lds_writes_are_not_mirror_stores(chain):
  """The stack's writes are invisible to the passes that rewrite mirror stores: the fields
  elided for mjd_inverseFD and the fields k_vaskip keeps its own are what they were with the
  stack off, and no stack access is turned into a streaming store or a perturbed load."""
  for m, name in ((models.load("humanoid", disable_contact=True), "humanoid"), (chain[0], "c")):
    on, off = codegen._Model(m), codegen._Model(m, 0)
    b_on = [codegen._GEN[st](on, None) for st in codegen.STAGES]
    va_stored_on = set(on.va_stored)
    b_off = [codegen._GEN[st](off, None) for st in codegen.STAGES]
    assert codegen.fd_elided(b_on) == codegen.fd_elided(b_off)
    assert va_stored_on == set(off.va_stored)
    text = codegen.generate(m, name)
    for line in text.split("\n"):
      if "cstk" in line:
        assert "MJH_NT_" not in line and "P_" not in line and "eps" not in line, line
