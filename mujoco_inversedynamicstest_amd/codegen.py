"""Model-specialized HIP kernel generator: the fast path of mj_inverse for one model.

The generic kernel (csrc/engine_device.h) walks the model's arrays at run time and keeps
every intermediate in the device mirror. This generator instead unrolls the reference's
loops over the model's bodies, joints and dofs at build time. Model constants become exact
literals, and every mjData output is stored to the mirror exactly once per call -- except the
outputs that are themselves model constants, which k_const_<name> stores once per context
(CONST_ONCE below). Arithmetic goes
through the same helper templates as the generic kernel (mjh::mulQuat, mjh::inertCom,
mjh::dot6, ...) in the same order, so the outputs are bit-identical to the generic kernel's
and the oracle's (tests/test_codegen_cpu.py).

Schedule (why it is not one fused kernel): one lane owns one instance and a 65,536 batch is
one wave per SIMD, so nothing hides a stall. Every load on CDNA waits for all of the wave's
older stores (one vmcnt counter). Any value that spills to scratch and is reloaded after
mirror stores therefore waits for those stores to reach memory. The generator keeps the live
set small enough for the register file and puts all of a kernel's loads ahead of its stores:

  k_pos  qpos -> tree pass 1 (kinematics, subtree COM), tree pass 2 (kinematics again, stores,
         cinert, cdof, crb, qM). Pass 2 recomputes instead of keeping pass 1's frames live.
  k_fac  qM -> mj_factorM (qLD, qLDiagInv)
  k_vel  qvel, cinert, cdof -> fwdVelocity, passive, comVel + mj_rne(flg_acc=0)
  k_acc  qvel, qacc, cinert, cdof, cvel, cdof_dot -> mj_rne(flg_acc=1) + mj_inverse assembly

The tree passes are depth-first, with children in DESCENDING body index. The post-order of
that traversal is exactly the descending body order of the reference's backward loops
(subtree_com, crb, cfrc accumulation), so every sum is formed in the reference's order while
only the current root-to-body path is live.

Constraint rows are left to the generic constraint kernel (k_constraint, mjhip.hip:
collision, mj_makeConstraint and its velocity/acceleration-stage parts, final assembly),
which reads the constraint-free stages from the mirror. constraint_mode(m) says which
instances it serves: 'list' -- joint/tendon limits only; k_pos evaluates the predicates of
mj_instantiateLimit (engine_core_constraint.c:824-959) and appends limit-active instances to
a device work-list, marked in efc_count[0] (-1); 'all' -- contacts or always-active friction
loss, every instance; 'none' -- no rows possible. For a served instance k_va stores the raw
mj_rne(flg_acc = 1) result as qfrc_inverse, so the assembly rne + ((armature*qacc - passive)
- constraint) happens once, in the reference's order, in k_constraint.

Reference functions restated (engine_core_smooth.c unless noted): mj_kinematics :38-178,
mj_comPos :183-270, mj_camlight :275-392, mj_tendon :651-723 (fixed), mj_transmission
:865-916 (joint), mj_crb :1353-1401, mj_factorM/mj_factorI :1470-1511, mj_fwdVelocity
engine_forward.c:193-231, mj_comVel :1833-1896, mj_passive engine_passive.c:436-493,
mj_rne :1969-2023, mj_inverseSkip engine_inverse.c:197-261.
"""
from __future__ import annotations

import hashlib
import re

import numpy as np

from . import fields

FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3
STAGES = ("pos", "fac", "va")
FRAMES_IN_PASS1 = True   # k_pos: pass 1 stores the frames, pass 2 cinert/cdof/crb/qM
MAX_LDS_HINGES = 32
PREFETCH = 1      # tree-pass events between a body's mirror loads and their first use
FUSE = True       # one launch running the three stage bodies back to back per wave
# k_va recomputes each body's frame, cinert and pre-visit cdof along its tree pass (from
# qpos, the root's subtree_com and k_pos's hinge sin/cos in LDS) instead of re-reading them
# from the mirror (332 fewer doubles read per humanoid instance; needs the fused kernel's LDS
# trig). Off: the frames kept along the path make k_all spill 844 B/lane (1,228 B when cdof
# is kept for the projections too), far worse than the reads it saves
# (tools/kernel_resources.py). Bit-exact either way (tests/test_codegen_cpu.py).
VA_RECOMPUTE = False
# lanes per workgroup of each stage kernel: 64 = one instance block per wave; 32 = a block
# split over two half-filled waves (twice the waves per SIMD, same mirror layout)
# k_all hands the qM rows of qm_handoff_plan from the pos stage to the fac stage in LDS that
# is dead at that point (qo_lds, the tail of the trig/stack region, and each hinge's sin/cos
# pair once its body's pass-2 pre-visit has read it) instead of fac re-reading them from the
# mirror: the HO = true instantiation of the pos and fac bodies, which only k_all and the
# host entry select. A handed entry is never re-read, so its mirror store streams there.
# (Round 2 handed all of qM in registers instead: exact, but the 243 values live across
# pos's post-order pushed k_all from 20 B to 1,968 B of scratch per lane.)
# QM_ORDER: "early" hands the first-produced rows (the longest store-to-load distance),
# "late" the last-produced ones, both under the same liveness rule. Both fill the pool (75
# doubles for the humanoid); late measured 0.4% faster on the bench step in an alternated A/B
# (DESIGN.md §Measurements, round 9).
QM_HANDOFF = True
QM_ORDER = "late"
# QM_FORWARD: the doubles per lane that k_all's pos stage may forward to its fac stage in
# registers on top of the LDS pool (qm_forward_plan): whole rows from the last-produced one
# backwards, which appear while pass 2 unwinds and its register demand falls, and which the
# fac stage's eliminations update from their first step. k_all is allocated the fac stage's
# registers anyway, so the pos stage leaves that many idle. The budget is the largest for which
# no HO instantiation of k_all_humanoid has scratch (tools/kernel_resources.py): the humanoid
# forwards 128 doubles with 0 B; the next whole row (136) brings 20 B, all rows (243) 860 B.
# 0: none forwarded, the LDS plan alone.
QM_FORWARD = 128
# experiment knob: False withholds the LDS pool, so that forwarding works alone (the A/B of
# the two mechanisms; a model whose every row fits QM_FORWARD then forwards all of them)
QM_LDS = True
# batches from which the launch functions pick the HO instantiation by default: the same
# threshold as SV, for the same reason. Below it L2 is not oversubscribed, the fac stage's
# re-read of qM is served there, and the hand-off only adds LDS traffic to a latency-bound
# wave (batch 4,096 with contacts: 0.3% slower with it in a 12-run A/B; 65,536: 1.3% faster).
# Mirror::qm_handoff = 2 (MJHIP_QM_HANDOFF=1) hands at every batch, 0 at none.
QM_HANDOFF_MIN_B = 49152      # = NT_SV_MIN_B (below)
# The va stage's tree pass keeps the cdof of the dofs on the current root-to-body path in an
# LDS stack (written at a body's pre-visit, read back for the projections at its post-visit)
# instead of re-reading them from the mirror. The stack shares k_all's trig region, which is
# dead once the pos stage ends. None: as many slots as keep k_all's static LDS within
# LDS_BUDGET (va_lds_capacity); an int forces the capacity (0: every projection re-reads, the
# earlier behaviour). generate()'s va_slots argument overrides it per call.
VA_LDS_SLOTS = None
# the va stage keeps the qfrc_passive values it stores in registers for the assembly at the
# post-visits instead of re-reading them from the mirror
VA_KEEP_QFP = True
# static LDS a k_all workgroup may hold while four of them share a CU's 160 KB
LDS_BUDGET = 40960
LANES = {"pos": 64, "fac": 64, "va": 64}
# k_all's workgroup: ALL_LANES lanes (64 = one instance block per wave; 32 = each block split
# over two half-filled waves, so batch 65,536 is 2,048 waves) and the waves per SIMD it is
# compiled for (__launch_bounds__'s second argument: 2 caps the kernel at 256 registers so
# two waves share a SIMD)
ALL_LANES = 64
ALL_WAVES = 1
# stores of mirror fields go out as streaming (non-temporal) stores, MJH_NT_STORE in
# engine_device.h, except those the fac stage re-reads right after the pos stage stored them
# (qM): those stay in L2 for it. The va stage's re-reads (cinert, cdof) come long after their
# stores, by which time 32 waves per XCD have written far more than its 4 MB L2 holds, so
# keeping them temporal only displaced qM (round 4 A/B, tools/exp_variants.py: 347.6 us with
# every re-read field temporal, 317.4 us with qM alone, 338.4 us with none; bit-identical
# outputs). -DMJHIP_NO_NT compiles them as plain stores (the A/B build)
NT_STORES = True
# experiment knobs (tools/exp_variants.py): NT_TEMPORAL None = the rule above, else the set
# of fields whose stores stay temporal (all others stream); NT_STAGES: the stages whose
# stores may stream
NT_TEMPORAL = None
NT_STAGES = ("pos", "fac", "va")
# batches from which k_all also streams the stores the va stage re-reads (SV = true): below
# it, L2 is not oversubscribed and keeping them pays (mjd_inverseFD's position-stage launch,
# whose centres' fields k_vaskip re-reads)
NT_SV_MIN_B = 49152
# experiment knob: stages whose re-reads of the mirror load as streaming (non-temporal)
# loads (MJH_NT_LOAD), so they do not displace the lines a later stage re-reads
NT_LOAD_STAGES = ()
# stages whose mirror loads stream in the SV instantiation only (batches >= NT_SV_MIN_B, where
# the va stage's re-read fields stream as well): 319.7 against 324.2 us per 65,536 in the A/B
# (profiles/r04/experiments/nt_variants_3.log); below it, and in k_vaskip (whose loads of the
# centre's fields are shared by 54 perturbations), they stay temporal
NT_LOAD_SV_STAGES = ("va",)
# Stores whose value is a model constant -- a number this generator holds and prints as a
# literal, the same in every instance and every call -- leave the stage bodies for
# fast_const_<name>, which k_const_<name> runs once per context over the whole capacity (and
# again after anything that may have overwritten the slots: mjhip.hip const_stale). Only
# _Stage.st_const sites qualify, and only fields no other kernel of the context may write
# with another value (_Model.const_ok). Off: the parent's text.
CONST_ONCE = True


# mjd_inverseFD's perturbed instances (mjhip_inverseFDBatch with a stage-skip layout, whose
# centres come first): a mirror field the straight-line stages store but never load is read
# by no later kernel of that call either -- the finite differences read qfrc_inverse (and qM
# for DmDq), a work-list model's limit rows the fields below -- so in instance blocks at or
# past Mirror::full_blk (Mirror::fd_elide set) its stores are compiled out: the FD = true
# instantiation of the stage bodies drops them (if constexpr), and the k_all kernel launched
# when Mirror::fd_elide is set runs it on those blocks and the plain bodies on the centres'
# (one wave-uniform branch at the top); k_vaskip has the FD bodies only. Every other launch is
# the plain kernel. The operations are the plain kernel's, but without the stores the compiler
# contracts a few multiply-adds differently, so a result can differ from the full pipeline's
# by a few ulp of qfrc_inverse (test_inverse_fd_stage_skip_bit_exact holds the Jacobians to 16
# ulp of the largest |qfrc_inverse| over eps). Measured (28,672 instances of
# the humanoid, mjd_inverseFD's position stage): 134.6 us storing everything, 126.6 us with
# streaming stores into a shared sink (a streaming store reaches memory wherever it points),
# 125.4 us with temporal stores into it, 148 us skipping each store behind a wave-uniform
# branch (which also moved results by an ulp: the branches split the blocks the
# multiply-adds are formed in); selecting the sink in every instantiation cost the headline
# kernel 4%.
FD_KEEP = frozenset({"qpos", "qvel", "qacc", "qfrc_inverse", "qfrc_passive", "qfrc_constraint",
                     "qfrc_actuator", "ten_length", "ten_J", "ten_velocity", "actuator_length",
                     "actuator_moment", "actuator_velocity", "qM", "sensordata"})


def fd_elided(bodies) -> set:
  """The mirror fields the stage bodies store and never load, less FD_KEEP."""
  import re
  text = re.sub(r"double\* __restrict__ P_\w+ = [^;]*;", "", "\n".join(bodies))
  store_nt = re.compile(r"MJH_NT_STORE(?:_IF)?\((?:\w+, )?P_(\w+)\[")
  store_eq = re.compile(r"^\s*P_(\w+)\[[^\]]+\] = ", re.M)
  stores = set(store_nt.findall(text)) | set(store_eq.findall(text))
  loads = set(re.findall(r"P_(\w+)\[", store_eq.sub("", store_nt.sub("", text))))
  return stores - loads - FD_KEEP


def _elide_stores(body: str, elided) -> str:
  """FD instantiation: the elided fields' stores are compiled out (if constexpr); k_all runs
  it on the instance blocks past Mirror::full_blk and the plain body on the others."""
  import re
  store = re.compile(r"^(\s*)((?:MJH_NT_STORE(?:_IF)?\((?:\w+, )?P_(\w+)\[|P_(\w+)\[[^\]]+\] = ).*;)$")

  def one(line):
    mt = store.match(line)
    if not mt or (mt.group(3) or mt.group(4)) not in elided:
      return line
    return f"{mt.group(1)}if constexpr (!FD) {{ {mt.group(2)} }}"
  return "\n".join(one(x) for x in body.split("\n"))


def _ll(st):
  """LDS lane index and stride of stage st (LDS arrays are per workgroup)."""
  n = LANES[st]
  return ("lane", 64) if n == 64 else (f"(lane & {n - 1})", n)


def lit(x) -> str:
  """Exact C literal for a double (hex float keeps every bit)."""
  x = float(x)
  if x == 0:
    return "-0.0" if np.signbit(x) else "0.0"
  if x == int(x) and abs(x) < 2**53:
    return f"{int(x)}.0"
  return x.hex()


def arr_lit(vals) -> str:
  return "{" + ", ".join(lit(v) for v in np.ravel(vals)) + "}"


class _Emitter:
  def __init__(self):
    self.lines = []
    self.ind = 1

  def __call__(self, s=""):
    self.lines.append("  " * self.ind + s if s else "")

  def open(self, s="{"):
    self(s)
    self.ind += 1

  def close(self, s="}"):
    self.ind -= 1
    self(s)

  def text(self):
    return "\n".join(self.lines)


def fast_path_supported(m) -> str | None:
  """Return why the model cannot use the straight-line kernels, or None."""
  if m.nv == 0:
    # nothing to unroll (and zero-length arrays are not valid device code)
    return "no degrees of freedom"
  if m.nv >= 60:
    # straight-line code grows with the tree; large models (the reference's sparse-Jacobian
    # range) run the generic kernel
    return "large model (nv >= 60)"
  if fields.is_sparse(m):
    # compressed constraint rows (mj_isSparse) are built by the generic kernel only
    return "sparse-Jacobian model (jacobian=\"sparse\")"
  if m.opt["enableflags"] & (1 << 3):
    if int(m.opt["integrator"]) == 1:
      return "INVDISCRETE with RK4 (an error in the reference)"
    if any(int(t) == 5 for t in m.actuator_trntype[:m.nu]):
      # mj_discreteAcc's implicit damping reads actuator_moment before the constraint kernel
      # (k_discrete_before forms the slider-crank and site ones first), but a body
      # transmission needs the contacts that kernel makes
      return "INVDISCRETE with body (adhesion) transmissions"
  for a in range(m.nu):
    if m.actuator_trntype[a] not in (0, 1, 2, 3, 4, 5):
      return "unknown transmission"
  if 8 * sum(_lds_doubles(m, 0)) > LDS_BUDGET:
    # hinge sin/cos and the row-major output block: a fourth workgroup would not fit the CU
    return "k_all's LDS over budget (hinges and dofs)"
  return None


# transmissions the generated kernels leave to the pass after the constraint kernel
# (mjh::transmissionAfter in k_sensors): slider-crank, site and body. Inverse dynamics does not
# read actuators, so their actuator_length/moment/velocity can come last; a body transmission
# needs the instance's contacts, which only the constraint kernel makes.
TRN_AFTER = (2, 4, 5)


def _pair_uses_ccd(t1, t2) -> bool:
  """mjhip_pairUsesCcd (include/mjhip_contact.h) for type-ordered t1 <= t2: the pair runs
  the iterative native solver (mjc_Convex, mjc_ConvexHField)."""
  if t1 == 1:                                           # height field
    return 2 <= t2 <= 7
  if t1 == 0:
    return False
  if t2 in (4, 7):                                      # ellipsoid, mesh
    return True
  if t2 == 5:                                           # cylinder
    return t1 in (3, 4, 5)
  if t2 == 6:                                           # box
    return t1 in (4, 5)
  return False


def exact_fp(m) -> bool:
  """True when some collidable geom pair runs the iterative native solver. Its result moves
  by up to ccd_tolerance under a last-bit change of the geom frames, so the generated
  kernels of such a model compute the frames without multiply-add contraction, rounding
  each operation as the reference does (the solver itself is compiled that way too,
  csrc/engine_device.h)."""
  if int(m.opt["disableflags"]) & ((1 << 4) | 1):       # contact or constraint disabled
    return False
  ng = m.sizes["ngeom"]
  t = np.asarray(m.geom_type)[:ng]
  ct = np.asarray(m.geom_contype)[:ng]
  ca = np.asarray(m.geom_conaffinity)[:ng]
  wb = np.asarray(m.body_weldid)[np.asarray(m.geom_bodyid)[:ng]]
  for i in range(ng):
    for j in range(i + 1, ng):
      if wb[i] == wb[j] or not ((ct[i] & ca[j]) or (ct[j] & ca[i])):
        continue
      if _pair_uses_ccd(min(t[i], t[j]), max(t[i], t[j])):
        return True
  return False


def spatial_tendons(m) -> list:
  """Tendons whose path is spatial (their first wrap is not a joint, engine_core_smooth.c
  mj_tendon): their length, Jacobian and velocity, the tendon transmissions on them and
  mj_passive are left to the pass before the constraint kernel (csrc/post_pass.h)."""
  return [t for t in range(m.ntendon) if int(m.wrap_type[int(m.tendon_adr[t])]) != 1]


def constraint_mode(m) -> str:
  """Which instances the constraint kernel serves: 'all', 'list' or 'none' (module doc)."""
  dsbl = int(m.opt["disableflags"])
  if spatial_tendons(m):
    return "all"          # the tendon pass (csrc/post_pass.h) forms ten_J and qfrc_passive
  if int(m.opt["enableflags"]) & (1 << 3):
    return "all"          # the discrete pass (csrc/post_pass.h) changes qacc before the
                          # constraint kernel, which assembles qfrc_inverse from it
  if (m.opt["density"] > 0 or m.opt["viscosity"] > 0) and not dsbl & (1 << 5):
    return "all"          # fluid: the post pass (csrc/post_pass.h) updates qfrc_passive, and
                          # the constraint kernel assembles qfrc_inverse for every instance
  if dsbl & 1:                                             # mjDSBL_CONSTRAINT
    return "none"
  contacts = not (dsbl & (1 << 4)) and m.nbody >= 2 and \
      bool(np.any((m.geom_contype != 0) | (m.geom_conaffinity != 0)))
  friction = (bool(np.any(m.dof_frictionloss > 0)) or
              bool(np.any(np.asarray(m.tendon_frictionloss)[:m.ntendon] > 0))) and \
      not (dsbl & (1 << 2))
  equality = m.sizes.get("neq", 0) > 0 and bool(np.any(m.eq_active0)) and not (dsbl & (1 << 1))
  if contacts or friction or equality:
    return "all"
  limits = not (dsbl & (1 << 3)) and (bool(np.any(m.jnt_limited)) or
                                      bool(np.any(m.tendon_limited[:m.ntendon])))
  return "list" if limits else "none"


CONSTRAINT_MODES = {"none": 0, "list": 1, "all": 2}


def const_cdof(m, k):
  """cdof of dof k where it is a model constant -- a free joint's translational dofs,
  [0, 0, 0, e_k] (mj_comPos, engine_core_smooth.c:230-234) -- else None."""
  j = int(m.dof_jntid[k])
  c = k - int(m.jnt_dofadr[j])
  if int(m.jnt_type[j]) != FREE or c >= 3:
    return None
  return [0.0] * 3 + [1.0 if r == c else 0.0 for r in range(3)]


def va_slot_plan(m, capacity):
  """The va stage's cdof stack: ({dof: slot}, deepest path's slot count). A dof's slot is its
  index among the non-constant dofs (const_cdof) on its root-to-body path, so two dofs live
  on one path at the same time never share one; dofs at or past `capacity` get none and keep
  the re-read from the mirror."""
  slot, depth = {}, {0: 0}
  for b in range(1, m.nbody):
    n = depth[int(m.body_parentid[b])]
    for k in range(int(m.body_dofadr[b]), int(m.body_dofadr[b]) + int(m.body_dofnum[b])):
      if const_cdof(m, k) is not None:
        continue
      if n < capacity:
        slot[k] = n
      n += 1
    depth[b] = n
  return slot, max(depth.values())


def _lds_doubles(m, slots, nl=None):
  """(trig region, qo_lds) doubles per k_all workgroup of nl lanes with a cdof stack of
  `slots` slots: trig and the stack share one region sized the larger of the two."""
  nl = ALL_LANES if nl is None else nl
  hinges = sum(1 for j in range(m.njnt) if int(m.jnt_type[j]) == HINGE)
  ntrig = 2 * hinges if 0 < hinges <= MAX_LDS_HINGES else 0
  return max(1, max(ntrig, 6 * slots) * nl), nl * max(m.nv, 1)


def va_lds_capacity(m) -> int:
  """The largest slot count (no more than the deepest path needs) for which k_all's static
  LDS stays within LDS_BUDGET. The humanoid: (40,960 - 13,824 B of qo_lds) / 3,072 B per
  slot = 8, a region of 24,576 B where trig alone took 21,504 B."""
  depth = va_slot_plan(m, 0)[1]
  n = depth
  while n > 0 and 8 * sum(_lds_doubles(m, n)) > LDS_BUDGET:
    n -= 1
  return n


def k_all_lds_bytes(m, va_slots=None) -> int:
  """Static LDS of k_all_<name> (trig/stack region + qo_lds), as generate() declares it."""
  M = _Model(m, va_slots)
  return 8 * sum(_lds_doubles(m, M.va_nslot))


def qm_row(M, k) -> list:
  """The qM entries of dof k's row (mj_crb: the dof, then its ancestors), in stored order."""
  n, j = 0, k
  while j >= 0:
    n += 1
    j = M.dparent[j]
  return list(range(M.Madr[k], M.Madr[k] + n))


def qm_handoff_plan(m, va_slots=None, order=None) -> dict:
  """{qM index -> LDS slot} of the entries k_all's pos stage hands to its fac stage on-chip.

  A slot is one double per lane at [slot*64 + lane] of the trig/stack region (slots below
  its rows, _lds_doubles(m, slots, 64)[0] / 64) or of qo_lds (the slots from there on). Three
  pools, none of which adds a byte to k_all's static LDS:
    qo_lds              written by the va stage only, so free during all of pos and fac;
    the region's tail   the rows past the hinges' sin/cos pairs, the va stage's as well;
    a hinge's pair      free once its body's pass-2 pre-visit has read it (_emit_frame), and
                        qM rows are produced at post-visits only.
  A handed value stays in its slot until the fac stage, so slots are never reused. A row is
  handed whole or not at all, and a row of constants (dof_simplenum) never. order "early":
  rows in production order, each taken when enough slots are free at its post-visit; "late":
  from the last-produced row backwards, each preferring the slots released last, and leaving
  out the rows that are forwarded in registers instead (qm_forward_plan; the two are planned
  together, _qm_plans). Empty when the switch is off or less than one row fits."""
  return _qm_plans(m, va_slots, order)[0]


def qm_forward_plan(m, va_slots=None) -> dict:
  """{qM index -> index into the fw array} of the entries k_all's pos stage forwards to its
  fac stage in registers (QM_FORWARD): whole rows from the last-produced one backwards, never
  a row of constants, disjoint from qm_handoff_plan(m) -- the two are planned together
  (_qm_plans). Empty with the hand-off off."""
  return _qm_plans(m, va_slots, None)[1]


def _qm_plans(m, va_slots=None, order=None) -> tuple:
  """(LDS plan, forward plan) of qm_handoff_plan / qm_forward_plan.

  Order "early" forwards nothing. Otherwise the forwarded set is a suffix of the production
  order (the rows whose values appear as pass 2 unwinds), and the LDS pool goes to the rows
  before it. A hinge pair is free only after its body's pre-visit, so pairs of the bodies
  visited last can hold only rows of the suffix: where rows before the suffix are left
  without a slot while such slots stay empty, suffix rows move back to them, the
  earliest-produced (the one that would live in registers longest) first. Of all suffixes
  whose forwarded doubles stay within QM_FORWARD the one handing the most doubles in total is
  taken, the shortest among equals: what the LDS pool holds anyway stays there, and registers
  (whose overflow is scratch, which costs far more than either) take only what it cannot."""
  order = QM_ORDER if order is None else order
  assert order in ("early", "late"), order
  M = m if isinstance(m, _Model) else _Model(m, va_slots, handoff=False)
  if not QM_HANDOFF or not FUSE or ALL_LANES > 64:
    return {}, {}
  if order == "early" or QM_FORWARD <= 0:
    return _qm_lds_plan(M, order, ()), {}
  last_first = [k for _, k in sorted(_qm_produced(M), reverse=True)]
  best = None
  for n in range(len(last_first) + 1):
    suffix = last_first[:n]
    lds = _qm_lds_plan(M, order, suffix)
    fwd = [k for k in suffix if M.Madr[k] not in lds]
    nfwd = sum(len(qm_row(M, k)) for k in fwd)
    if nfwd <= QM_FORWARD and (best is None or len(lds) + nfwd > best[0]):
      best = (len(lds) + nfwd, lds, fwd)
  _, lds, fwd = best
  entries = sorted(a for k in fwd for a in qm_row(M, k))
  return lds, {a: i for i, a in enumerate(entries)}


def _qm_events(M) -> dict:
  """{("pre" | "post", body): position} in the pos stage's pass-2 traversal."""
  events = []
  M.dfs(lambda b: events.append(("pre", b)), lambda b: events.append(("post", b)))
  return {ev: t for t, ev in enumerate(events)}


def _qm_produced(M) -> list:
  """[(post-visit that produces it, dof)] of the qM rows that are not rows of constants."""
  when = _qm_events(M)
  return [(when[("post", M.dbody[k])], k) for k in range(M.nv) if not M.simplenum[k]]


def _qm_lds_plan(M, order, suffix) -> dict:
  """qm_handoff_plan's slot assignment with the rows of the dofs in `suffix` held back for
  forwarding: they are offered slots only where a row outside it went without, and after
  all of those, in production order."""
  m = M.m
  if not QM_LDS:
    return {}
  nreg, nqo = _lds_doubles(m, M.va_nslot, 64)
  rows = nreg // 64                     # of the trig/stack region (max(1, ...) // 64 = 0: none)
  when = _qm_events(M)
  # slot -> the event after which it is free (-1: from the start of the pos stage)
  free_from = {s: -1 for s in range(2 * len(M.trig), rows)}
  if m.nv > 0:
    free_from.update({rows + k: -1 for k in range(nqo // 64)})
  if not (VA_RECOMPUTE and FUSE):       # that experiment reads trig throughout the va stage
    for j, h in M.trig.items():
      t = when[("pre", int(m.jnt_bodyid[j]))]
      free_from[2 * h] = free_from[2 * h + 1] = t
  held = set(suffix)
  produced = [x for x in _qm_produced(M) if x[1] not in held]
  produced.sort(reverse=order == "late")
  plan, taken = {}, set()

  def offer(t, k):
    entries = qm_row(M, k)
    free = sorted((s for s in free_from if free_from[s] < t and s not in taken),
                  key=lambda s: (free_from[s], s), reverse=order == "late")
    if len(free) < len(entries):
      return False
    for a, s in zip(entries, free):
      plan[a] = s
      taken.add(s)
    return True
  left_out = [offer(t, k) for t, k in produced].count(False)
  if left_out:
    for t, k in sorted(x for x in _qm_produced(M) if x[1] in held):
      offer(t, k)
  return plan


def _ho_ref(M, slot, st) -> str:
  """The arguments (array, row, stride, lane) of handQM / takeQM for a plan slot in stage st:
  each LDS array is reached through its own __restrict__ pointer only."""
  rows = _lds_doubles(M.m, M.va_nslot, 64)[0] // 64
  li, ls = _ll(st)
  return f"trig, {slot}, {ls}, {li}" if slot < rows else f"qo_lds, {slot - rows}, {ls}, {li}"


class _Model:
  """Model constants the emitters share."""

  def __init__(self, m, va_slots=None, handoff=None):
    self.m = m
    self.nbody, self.nv, self.nq, self.njnt = m.nbody, m.nv, m.nq, m.njnt
    self.parent = [int(x) for x in m.body_parentid]
    self.rootid = [int(x) for x in m.body_rootid]
    self.children = {b: [] for b in range(m.nbody)}
    for b in range(1, m.nbody):
      self.children[self.parent[b]].append(b)
    for b in self.children:
      self.children[b].sort(reverse=True)
    self.mass = [float(x) for x in m.body_mass]
    self.dsbl = int(m.opt["disableflags"])
    self.cmode = constraint_mode(m)
    self.bdofadr = [int(x) for x in m.body_dofadr]
    self.bdofnum = [int(x) for x in m.body_dofnum]
    self.djnt = [int(x) for x in m.dof_jntid]
    self.dbody = [int(x) for x in m.dof_bodyid]
    self.Madr = [int(x) for x in m.dof_Madr]
    self.dparent = [int(x) for x in m.dof_parentid]
    self.simplenum = [int(x) for x in m.dof_simplenum]
    S = {f.name: f.size(m.sizes) for f in fields.DATA_FIELDS}
    self.S = S
    # subtree masses are model constants (mj_comPos accumulates them in descending order)
    ms = [0.0] * m.nbody
    for i in range(m.nbody - 1, -1, -1):
      ms[i] = ms[i] + self.mass[i]
      if i:
        ms[self.parent[i]] = ms[self.parent[i]] + ms[i]
    self.subtree_mass = ms
    # hinge joints whose sin/cos k_pos evaluates once, into LDS (2 doubles per lane each;
    # 4 waves per CU must fit in 160 KB)
    hinges = [j for j in range(m.njnt) if int(m.jnt_type[j]) == HINGE]
    self.trig = {j: h for h, j in enumerate(hinges)} if 0 < len(hinges) <= MAX_LDS_HINGES else {}
    # the va stage's cdof stack (VA_LDS_SLOTS): dof -> slot, and the slots the region holds
    if va_slots is None:
      va_slots = VA_LDS_SLOTS
    if va_slots is None:
      va_slots = va_lds_capacity(m)
    if VA_RECOMPUTE and FUSE:
      va_slots = 0          # that experiment reads trig throughout the va stage
    self.va_slot, depth = va_slot_plan(m, va_slots)
    self.va_nslot = min(va_slots, depth)
    self.spatial = set(spatial_tendons(m))
    # QM_HANDOFF: {qM index: LDS slot} of the entries the HO instantiation hands on-chip
    # QM_FORWARD: {qM index: fw index} of those it forwards in registers instead
    self.handoff, self.forward = _qm_plans(self) if handoff is None or handoff else ({}, {})
    # CONST_ONCE: {(field, index): expression} in emission order, and the declarations the
    # expressions name
    self.consts, self.const_decls = {}, []
    g = np.asarray(m.opt["gravity"], dtype=float)
    self.has_gravcomp = bool(m.ngravcomp and not (self.dsbl & (1 << 5)) and
                             not (self.dsbl & (1 << 6)) and np.sqrt(g @ g) != 0)
    self.has_fluid = (m.opt["density"] > 0 or m.opt["viscosity"] > 0) and \
        not self.dsbl & (1 << 5)
    self.ten_terms = []
    for t in range(m.ntendon):
      adr, num = int(m.tendon_adr[t]), int(m.tendon_num[t])
      if t in self.spatial:
        self.ten_terms.append(None)      # formed by the tendon pass, never emitted here
        continue
      self.ten_terms.append([(float(m.wrap_prm[w]), int(m.jnt_qposadr[m.wrap_objid[w]]),
                              int(m.jnt_dofadr[m.wrap_objid[w]]))
                             for w in range(adr, adr + num)])

  def const_ok(self, field) -> bool:
    """Whether a generator-constant store of `field` may leave the stage bodies: no other
    kernel of the context writes the field's slots with another value. The tendon pass
    (post_pass.h tendonAfter) re-forms tendons, their transmissions and all of mj_passive,
    the fluid pass qfrc_fluid; the constraint kernels write qfrc_constraint for the instances
    they serve (and every efc_*/con_* field, which no st_const site names)."""
    if not CONST_ONCE:
      return False
    if field in ("ten_J", "actuator_moment"):
      return not self.spatial
    if field in ("qfrc_fluid", "qfrc_gravcomp"):
      return not self.spatial and not self.has_fluid
    if field == "qfrc_constraint":
      return self.cmode == "none"
    return field in ("xpos", "xquat", "xmat", "xipos", "ximat", "geom_xpos", "geom_xmat",
                     "site_xpos", "site_xmat", "cinert", "crb", "cdof", "cvel", "cdof_dot")

  def ten_row(self, t):
    assert t not in self.spatial, "spatial tendon rows are formed at run time"
    J = np.zeros(self.nv)
    for prm, _, da in self.ten_terms[t]:
      J[da] = prm
    return J

  def jnt_ndof(self, j):
    return {FREE: 6, BALL: 3}.get(int(self.m.jnt_type[j]), 1)

  def preorder(self):
    out = []
    self.dfs(lambda b: out.append(b) if b else None, lambda b: None)
    return out

  def dfs(self, pre, post, root=0):
    """Depth-first over the tree, children in descending index (post-order = descending)."""
    pre(root)
    for c in self.children[root]:
      self.dfs(pre, post, c)
    post(root)


class _Stage:
  """Code of one stage body: pointer setup + emission helpers."""

  def __init__(self, M: _Model, store_fields=None):
    self.M = M
    self.E = _Emitter()
    self.store_fields = store_fields
    self.stored = set()      # mirror fields this stage stores through (k_vaskip's own set)

  def st(self, field, k, expr):
    self.stored.add(field)
    if field == "qM" and k in self.M.handoff:
      # a handed entry: the mirror store (qM is an output; generate() makes it a streaming
      # store in the HO instantiation) and the LDS slot the fac stage takes it from
      self.E(f"{{ const double v_ = {expr};")
      if self.store_fields is None or field in self.store_fields:
        self.E(f"P_qM[{k}*64] = v_;")
      self.E(f"mjh::handQM<HO>({_ho_ref(self.M, self.M.handoff[k], 'pos')}, v_); }}")
      return
    if field == "qM" and k in self.M.forward:
      # a forwarded entry: the plain mirror store (the kernels whose fac stage re-reads it,
      # and every reader after the call) and the register the fac stage takes it from
      self.E(f"{{ const double v_ = {expr};")
      if self.store_fields is None or field in self.store_fields:
        self.E(f"P_qM[{k}*64] = v_;")
      self.E(f"if constexpr (HO) fw[{self.M.forward[k]}] = v_; }}")
      return
    if self.store_fields is None or field in self.store_fields:
      self.E(f"P_{field}[{k}*64] = {expr};")

  def stv(self, field, k0, arr, n):
    for c in range(n):
      self.st(field, k0 + c, f"{arr}[{c}]")

  def st_const(self, field, k, expr, decl=None):
    """A store whose value the generator holds as a Python number: `expr` is its literal, or
    names an array that `decl` declares from literals and nothing assigns afterwards. With
    CONST_ONCE it goes to fast_const_<name> (same expression text) instead of this stage."""
    if not self.M.const_ok(field):
      self.st(field, k, expr)
      return
    if self.store_fields is not None and field not in self.store_fields:
      return
    M = self.M
    assert M.consts.setdefault((field, k), expr) == expr, (field, k, expr)
    if decl and decl not in M.const_decls:
      M.const_decls.append(decl)

  def stv_const(self, field, k0, arr, n, decl):
    for c in range(n):
      self.st_const(field, k0 + c, f"{arr}[{c}]", decl)

  def pointers(self, names):
    for nm in names:
      n = self.M.S[nm]
      if n:
        self.E(f"double* __restrict__ P_{nm} = mr.{nm} + ((long)blk*{n})*64 + lane;")

  def prologue(self):
    E = self.E
    E("const long inst = (long)blk*64 + lane;")
    E("if (inst >= B) return;")
    E("int* __restrict__ ec = efc_count + (long)blk*4*64 + lane;")

  def load(self, arr, field, n, off=0):
    self.E(f"double {arr}[{max(n, 1)}];")
    for k in range(n):
      self.E(f"{arr}[{k}] = P_{field}[{off + k}*64];")


def _prefetched_dfs(G: _Stage, loads, pre, post, dist):
  """Tree pass whose mirror loads are issued `dist` visit events ahead of their use.

  The events are the pre- and post-visits of the depth-first pass (world excluded).
  loads(kind, i) -> (decls, [(dst, field, idx)]): declarations (emitted at function scope)
  and scalar loads `dst = P_field[idx]` the event needs. A scheduling fence at each event
  keeps the loads where they are emitted, so at most `dist` events' worth is in flight.
  """
  M, E = G.M, G.E
  events = []
  M.dfs(lambda b: events.append(("pre", b)) if b else None,
        lambda b: events.append(("post", b)) if b else None)
  for ev in events:
    for d in loads(*ev)[0]:
      E(d)

  def emit_loads(ev):
    for dst, field, idx in loads(*ev)[1]:
      E(f"{dst} = P_{field}[{idx}*64];")

  for ev in events[:dist]:
    emit_loads(ev)
  pos = {ev: k for k, ev in enumerate(events)}

  def visit(kind, fn):
    def f(i):
      if i:
        E("MJH_SCHED_FENCE();")
        k = pos[(kind, i)] + dist
        if k < len(events):
          emit_loads(events[k])
      fn(i)
    return f

  M.dfs(visit("pre", pre), visit("post", post))


def _vec_loads(name, field, first, n):
  return [(f"{name}[{c}]", field, first + c) for c in range(n)]


# ------------------------------------------------------------------------------ kinematics
def _emit_frame(G: _Stage, i, store):
  """Frame of body i from its parent's frame (mj_kinematics, engine_core_smooth.c:56-160).

  Declares xpos_i, xquat_i, xmat_i and xanchor_j, xaxis_j for the body's joints.
  """
  M, E, m = G.M, G.E, G.M.m
  ja, jn = int(m.body_jntadr[i]), int(m.body_jntnum[i])
  E(f"double xpos_{i}[3], xquat_{i}[4], xmat_{i}[9];")
  if jn == 1 and m.jnt_type[ja] == FREE:
    qa = int(m.jnt_qposadr[ja])
    E(f"mjh::copy3(xpos_{i}, qpos + {qa});")
    E(f"mjh::copy4(xquat_{i}, qpos + {qa + 3});")
    E(f"mjh::normalize4s(xquat_{i});")
    E(f"double xanchor_{ja}[3], xaxis_{ja}[3] = {arr_lit(m.jnt_axis[ja])};")
    E(f"mjh::copy3(xanchor_{ja}, xpos_{i});")
  else:
    pid = M.parent[i]
    E.open()
    mid = int(m.body_mocapid[i]) if m.nmocap else -1
    if mid >= 0:                       # :72-82 mocap body: the per-instance input pose
      E(f"double bpos[3], bquat[4];")
      E(f"for (int k = 0; k < 3; k++) bpos[k] = P_mocap_pos[({3 * mid} + k)*64];")
      E(f"for (int k = 0; k < 4; k++) bquat[k] = P_mocap_quat[({4 * mid} + k)*64];")
      E("mjh::normalize4s(bquat);")
    else:
      E(f"const double bpos[3] = {arr_lit(m.body_pos[i])};")
      E(f"const double bquat[4] = {arr_lit(m.body_quat[i])};")
    if pid:
      E(f"mjh::mulMatVec3(xpos_{i}, xmat_{pid}, bpos);")
      E(f"mjh::addTo3(xpos_{i}, xpos_{pid});")
      E(f"mjh::mulQuat(xquat_{i}, xquat_{pid}, bquat);")
    else:
      E(f"mjh::copy3(xpos_{i}, bpos);")
      E(f"mjh::copy4(xquat_{i}, bquat);")
    E.close()
    for j in range(ja, ja + jn):
      t = int(m.jnt_type[j])
      qa = int(m.jnt_qposadr[j])
      E(f"double xanchor_{j}[3], xaxis_{j}[3];")
      E.open()
      E(f"const double jaxis[3] = {arr_lit(m.jnt_axis[j])};")
      E(f"const double jpos[3] = {arr_lit(m.jnt_pos[j])};")
      E(f"mjh::rotVecQuat(xaxis_{j}, jaxis, xquat_{i});")
      E(f"mjh::rotVecQuat(xanchor_{j}, jpos, xquat_{i});")
      E(f"mjh::addTo3(xanchor_{j}, xpos_{i});")
      if t == SLIDE:
        E(f"mjh::addToScl3(xpos_{i}, xaxis_{j}, qpos[{qa}] - {lit(m.qpos0[qa])});")
      else:
        E("double qloc[4];")
        if t == BALL:
          E(f"mjh::copy4(qloc, qpos + {qa});")
          E("mjh::normalize4s(qloc);")
        else:
          if j in M.trig:
            h = M.trig[j]
            E(f"mjh::axisAngle2QuatSC(qloc, jaxis, qpos[{qa}] - {lit(m.qpos0[qa])}, "
              f"trig[{2 * h}*{_ll('pos')[1]} + {_ll('pos')[0]}], "
              f"trig[{2 * h + 1}*{_ll('pos')[1]} + {_ll('pos')[0]}]);")
          else:
            E(f"mjh::axisAngle2Quat(qloc, jaxis, qpos[{qa}] - {lit(m.qpos0[qa])});")
        E(f"mjh::mulQuat(xquat_{i}, xquat_{i}, qloc);")
        E("double vec[3];")
        E(f"mjh::rotVecQuat(vec, jpos, xquat_{i});")
        E(f"mjh::sub3(xpos_{i}, xanchor_{j}, vec);")
      E.close()
  E(f"mjh::normalize4s(xquat_{i});")
  E(f"mjh::quat2Mats(xmat_{i}, xquat_{i});")
  if store:
    G.stv("xquat", 4 * i, f"xquat_{i}", 4)
    G.stv("xpos", 3 * i, f"xpos_{i}", 3)
    G.stv("xmat", 9 * i, f"xmat_{i}", 9)
    for j in range(ja, ja + jn):
      G.stv("xanchor", 3 * j, f"xanchor_{j}", 3)
      G.stv("xaxis", 3 * j, f"xaxis_{j}", 3)


def _emit_local2global(G: _Stage, dst_pos, dst_mat, pos, quat, body, sf, with_mat=True):
  """mj_local2Global (engine_support.c:1565-1606) into local arrays."""
  E = G.E
  E(f"double {dst_pos}[3]" + (f", {dst_mat}[9];" if with_mat else ";"))
  E.open()
  E(f"const double lp[3] = {arr_lit(pos)};")
  if sf in (0, 3, 4):
    E(f"mjh::mulMatVec3({dst_pos}, xmat_{body}, lp);")
    E(f"mjh::addTo3({dst_pos}, xpos_{body});")
  elif sf == 1:
    E(f"mjh::copy3({dst_pos}, xpos_{body});")
  else:
    E(f"mjh::copy3({dst_pos}, xipos_{body});")
  if with_mat:
    if sf == 0:
      E(f"const double lq[4] = {arr_lit(quat)};")
      E("double tmp[4];")
      E(f"mjh::mulQuat(tmp, xquat_{body}, lq);")
      E(f"mjh::quat2Mats({dst_mat}, tmp);")
    elif sf in (1, 3):
      E(f"mjh::copy({dst_mat}, xmat_{body}, 9);")
    else:
      E(f"mjh::copy({dst_mat}, ximat_{body}, 9);")
  E.close()


_WORLD_FRAME = ("double xpos_0[3] = {0.0, 0.0, 0.0}, xquat_0[4] = {1.0, 0.0, 0.0, 0.0};",
                "double xmat_0[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};",
                "double xipos_0[3] = {0.0, 0.0, 0.0};",
                "double ximat_0[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};")
# the world body's frame is these literals and nothing assigns them (the declaration each
# st_const of a world-body store names)
_WORLD_DECL = "\n".join(_WORLD_FRAME)
_CRB0_DECL = "double crb_0[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};"
_CVEL0_DECL = "double cvel_0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};"


def _world_frame(E):
  for line in _WORLD_FRAME:
    E(line)


def _camlight_needs(m):
  """Bodies whose subtree COM / position the camera and light modes need in pass 2."""
  stc, xpos = set(), set()
  for mode, b, tgt in ([(int(m.cam_mode[c]), int(m.cam_bodyid[c]), int(m.cam_targetbodyid[c]))
                        for c in range(m.ncam)] +
                       [(int(m.light_mode[l]), int(m.light_bodyid[l]),
                         int(m.light_targetbodyid[l])) for l in range(m.nlight)]):
    if mode == 2:
      stc.add(b)
    elif mode == 4 and tgt >= 0:
      stc.add(tgt)
    elif mode == 3 and tgt >= 0:
      xpos.add(tgt)
  return stc, xpos


# ------------------------------------------------------------------------------ k_pos
def _gen_pos(M: _Model, store_fields=None) -> str:
  G = _Stage(M, store_fields)
  E, m = G.E, M.m
  nq, nv, dsbl = M.nq, M.nv, M.dsbl
  # the next call's work-list counter (two alternate; stream order makes this safe)
  E("if (worklist_next && blk == 0 && lane == 0) *worklist_next = 0;")
  G.prologue()
  G.pointers([f.name for f in fields.DATA_FIELDS if f.stage <= 1])
  E(f"double qpos[{max(nq, 1)}];")
  E("if (qpos_in) {")
  E(f"  for (int k = 0; k < {nq}; k++) {{ qpos[k] = qpos_in[inst*{nq} + k]; "
    f"P_qpos[k*64] = qpos[k]; }}")
  E(f"  for (int k = 0; k < {nv}; k++) P_qvel[k*64] = qvel_in[inst*{nv} + k];")
  E(f"  for (int k = 0; k < {nv}; k++) P_qacc[k*64] = qacc_in[inst*{nv} + k];")
  E("} else {")
  E(f"  for (int k = 0; k < {nq}; k++) qpos[k] = P_qpos[k*64];")
  E("}")

  # limits predicate: mj_instantiateLimit (engine_core_constraint.c:824-959)
  E("// ---- constraint detection (mj_instantiateLimit predicates)")
  E("bool active = false;")
  limits_on = M.cmode == "list"
  if limits_on:
    for j in range(M.njnt):
      if not m.jnt_limited[j]:
        continue
      t = int(m.jnt_type[j])
      qa = int(m.jnt_qposadr[j])
      mg = lit(m.jnt_margin[j])
      if t in (SLIDE, HINGE):
        lo, hi = m.jnt_range[j]
        E(f"active |= (-1.0*({lit(lo)} - qpos[{qa}]) < {mg}) | "
          f"(1.0*({lit(hi)} - qpos[{qa}]) < {mg});")
      elif t == BALL:
        E.open()
        E(f"double q4[4] = {{qpos[{qa}], qpos[{qa+1}], qpos[{qa+2}], qpos[{qa+3}]}}, aa[3];")
        E("mjh::normalize4s(q4); mjh::quat2Vel(aa, q4, 1);")
        E("double val = mjh::normalize3s(aa);")
        E(f"active |= (mjh::dmax({lit(m.jnt_range[j][0])}, {lit(m.jnt_range[j][1])}) - val"
          f" < {mg});")
        E.close()
  if m.ntendon:
    E(f"double ten_length[{m.ntendon}];")
    for t, terms in enumerate(M.ten_terms):
      if terms is None:
        continue
      E(f"ten_length[{t}] = 0.0;")
      for prm, qa, _ in terms:
        E(f"ten_length[{t}] += {lit(prm)} * qpos[{qa}];")
    if limits_on:
      for t in range(m.ntendon):
        if m.tendon_limited[t] and t not in M.spatial:
          lo, hi = m.tendon_range[t]
          mg = lit(m.tendon_margin[t])
          E(f"active |= (-1.0*({lit(lo)} - ten_length[{t}]) < {mg}) | "
            f"(1.0*({lit(hi)} - ten_length[{t}]) < {mg});")
  if M.cmode == "list":
    E("if (active) {   // k_constraint's work-list; the stages below still run")
    E("  int slot = MJH_ATOMIC_ADD(worklist_count, 1);")
    E("  worklist[slot] = (int)inst;")
    E("}")
    E("ec[0] = active ? -1 : 0;")
  else:
    E("(void)active;")

  # tendons and transmission depend on qpos only
  if m.ntendon:
    E("// ---- mj_tendon (fixed, dense ten_J)")   # spatial ones: the tendon pass
    for t in range(m.ntendon):
      if t in M.spatial:
        continue
      G.st("ten_length", t, f"ten_length[{t}]")
      J = M.ten_row(t)
      for k in range(nv):
        G.st_const("ten_J", t * nv + k, lit(J[k]))
  if m.nu:
    E("// ---- mj_transmission (hinge/slide/ball/free joint, fixed tendon)")
    for a in range(m.nu):
      if int(m.actuator_trntype[a]) in TRN_AFTER:
        continue                       # k_sensors' mjh::transmissionAfter
      jid = int(m.actuator_trnid[a, 0])
      if m.actuator_trntype[a] == 3 and jid in M.spatial:
        continue                       # the tendon pass (csrc/post_pass.h)
      g = float(m.actuator_gear[a, 0])
      adr = int(m.moment_rowadr[a])
      if m.actuator_trntype[a] == 3:   # :1053-1081: gear * ten_J over the row's nonzeros
        G.st("actuator_length", a, f"ten_length[{jid}]*{lit(g)}")
        J = M.ten_row(jid)
        for k in range(int(m.moment_rownnz[a])):
          G.st_const("actuator_moment", adr + k,
                     lit(float(J[int(m.moment_colind[adr + k])]) * g))
        continue
      jt, qa = int(m.jnt_type[jid]), int(m.jnt_qposadr[jid])
      inparent = m.actuator_trntype[a] == 1
      gear = [float(x) for x in m.actuator_gear[a]]
      if jt == BALL:                   # :912-942 expmap axis . gear axis
        E.open()
        E("double axis[3], quat[4], ga[3];")
        E(f"mjh::copy4(quat, qpos + {qa});")
        E("mjh::normalize4(quat);")
        E("mjh::quat2Vel(axis, quat, 1);")
        E(f"const double g3[3] = {arr_lit(gear[:3])};")
        if inparent:
          E("quat[1] = -quat[1]; quat[2] = -quat[2]; quat[3] = -quat[3];")
          E("mjh::rotVecQuat(ga, g3, quat);")
        else:
          E("mjh::copy3(ga, g3);")
        G.st("actuator_length", a, "axis[0]*ga[0] + axis[1]*ga[1] + axis[2]*ga[2]")
        G.stv("actuator_moment", adr, "ga", 3)
        E.close()
        continue
      if jt == FREE:                   # :944-971 length 0, moment = (gear, gear axis)
        E.open()
        E("double ga[3];")
        E(f"const double g3[3] = {arr_lit(gear[3:6])};")
        if inparent:
          E("double quat[4];")
          E(f"mjh::copy4(quat, qpos + {qa + 3});")
          E("mjh::normalize4(quat);")
          E("quat[1] = -quat[1]; quat[2] = -quat[2]; quat[3] = -quat[3];")
          E("mjh::rotVecQuat(ga, g3, quat);")
        else:
          E("mjh::copy3(ga, g3);")
        G.st("actuator_length", a, "0.0")
        for k in range(3):
          G.st_const("actuator_moment", adr + k, lit(gear[k]))
        G.stv("actuator_moment", adr + 3, "ga", 3)
        E.close()
        continue
      G.st("actuator_length", a, f"qpos[{qa}]*{lit(g)}")
      G.st_const("actuator_moment", adr, lit(g))

  cams = {}
  for c in range(m.ncam):
    cams.setdefault(int(m.cam_bodyid[c]), []).append(("cam", c))
  for l in range(m.nlight):
    cams.setdefault(int(m.light_bodyid[l]), []).append(("light", l))
  geoms, sites = {}, {}
  for g in range(m.ngeom):
    geoms.setdefault(int(m.geom_bodyid[g]), []).append(g)
  for s in range(m.nsite):
    sites.setdefault(int(m.site_bodyid[s]), []).append(s)
  if M.trig:
    # every hinge's sin/cos once, into LDS: both tree passes read them, so neither carries
    # the branches of the trig functions' argument reduction
    E("// ---- hinge half-angle sin/cos (mju_axisAngle2Quat, engine_util_spatial.c:78-90)")
    for j, h in M.trig.items():
      qa = int(m.jnt_qposadr[j])
      E.open()
      E(f"double s, c, a = (qpos[{qa}] - {lit(m.qpos0[qa])})*0.5;")
      E("MJH_SINCOS(a, s, c);")
      li, ls = _ll("pos")
      E(f"trig[{2 * h}*{ls} + {li}] = s; trig[{2 * h + 1}*{ls} + {li}] = c;")
      E.close()
    E("MJH_MEM_BARRIER();")
  # ---- pass 1: kinematics -> subtree centers of mass (mj_comPos :183-208)
  E("// ---- tree pass 1: mj_kinematics -> mj_comPos subtree_com (post-order = descending)")
  need_stc, need_xpos = _camlight_needs(m)
  roots = sorted(set(M.rootid[1:]))
  need_stc |= set(roots)
  for b in sorted(need_stc):
    E(f"double keep_stc_{b}[3];")
  for b in sorted(need_xpos):
    E(f"double keep_xpos_{b}[3];")
  _world_frame(E)

  def world_attached(kind, k, sf):
    """A geom or site of the world body whose frame is a copy of the world's (sameframe 1:
    the body frame, 2: the inertial frame): the literals themselves, stored as constants."""
    if sf not in (1, 2) or not (M.const_ok(f"{kind}_xpos") and M.const_ok(f"{kind}_xmat")):
      return False
    G.stv_const(f"{kind}_xpos", 3 * k, "xpos_0" if sf == 1 else "xipos_0", 3, _WORLD_DECL)
    G.stv_const(f"{kind}_xmat", 9 * k, "xmat_0" if sf == 1 else "ximat_0", 9, _WORLD_DECL)
    return True

  def frame_outputs(i):
    """xipos/ximat, geom and site frames of body i (stored by whichever pass owns them)."""
    if i:
      G.stv("xipos", 3 * i, f"xipos_{i}", 3)
      G.stv("ximat", 9 * i, f"ximat_{i}", 9)
    else:
      G.stv_const("xipos", 0, "xipos_0", 3, _WORLD_DECL)
      G.stv_const("ximat", 0, "ximat_0", 9, _WORLD_DECL)
    for g in geoms.get(i, []):
      if not i and world_attached("geom", g, int(m.geom_sameframe[g])):
        continue
      E.open()
      _emit_local2global(G, "gp", "gm", m.geom_pos[g], m.geom_quat[g], i,
                         int(m.geom_sameframe[g]))
      G.stv("geom_xpos", 3 * g, "gp", 3)
      G.stv("geom_xmat", 9 * g, "gm", 9)
      E.close()
    for s in sites.get(i, []):
      if not i and world_attached("site", s, int(m.site_sameframe[s])):
        continue
      E.open()
      _emit_local2global(G, "sp", "sm", m.site_pos[s], m.site_quat[s], i,
                         int(m.site_sameframe[s]))
      G.stv("site_xpos", 3 * s, "sp", 3)
      G.stv("site_xmat", 9 * s, "sm", 9)
      E.close()

  def pre1(i):
    E.open(f"{{  // body {i}")
    if i:
      _emit_frame(G, i, store=FRAMES_IN_PASS1)
      _emit_local2global(G, f"xipos_{i}", f"ximat_{i}", m.body_ipos[i], m.body_iquat[i], i,
                         int(m.body_sameframe[i]), with_mat=FRAMES_IN_PASS1)
    elif FRAMES_IN_PASS1:
      G.stv_const("xpos", 0, "xpos_0", 3, _WORLD_DECL)
      G.stv_const("xquat", 0, "xquat_0", 4, _WORLD_DECL)
      G.stv_const("xmat", 0, "xmat_0", 9, _WORLD_DECL)
    if FRAMES_IN_PASS1:
      frame_outputs(i)
    if i in need_xpos:
      E(f"mjh::copy3(keep_xpos_{i}, xpos_{i});")
    E(f"double stc_{i}[3] = {{0.0, 0.0, 0.0}};")

  def post1(i):
    E(f"mjh::addToScl3(stc_{i}, xipos_{i}, {lit(M.mass[i])});")
    if i:
      E(f"mjh::addTo3(stc_{M.parent[i]}, stc_{i});")
    if M.subtree_mass[i] < 1e-15:
      E(f"mjh::copy3(stc_{i}, xipos_{i});")
    else:
      E(f"mjh::scl3(stc_{i}, stc_{i}, 1.0/{lit(max(1e-15, M.subtree_mass[i]))});")
    G.stv("subtree_com", 3 * i, f"stc_{i}", 3)
    if i in need_stc:
      E(f"mjh::copy3(keep_stc_{i}, stc_{i});")
    E.close()

  M.dfs(pre1, post1)

  # pass 2 recomputes the frames: make qpos opaque so the compiler cannot reuse pass 1's
  # (which would keep every frame live across the passes)
  E("// ---- tree pass 2: kinematics (stored), cinert, cdof, camlight, crb, qM")
  E(f"for (int k = 0; k < {nq}; k++) MJH_OPAQUE(qpos[k]);")
  if M.trig:
    E("MJH_MEM_BARRIER();")


  def pre2(i):
    E.open(f"{{  // body {i}")
    if i:
      _emit_frame(G, i, store=not FRAMES_IN_PASS1)
      _emit_local2global(G, f"xipos_{i}", f"ximat_{i}", m.body_ipos[i], m.body_iquat[i], i,
                         int(m.body_sameframe[i]))
    else:
      _world_frame(E)
      if not FRAMES_IN_PASS1:
        G.stv_const("xpos", 0, "xpos_0", 3, _WORLD_DECL)
        G.stv_const("xquat", 0, "xquat_0", 4, _WORLD_DECL)
        G.stv_const("xmat", 0, "xmat_0", 9, _WORLD_DECL)
    if not FRAMES_IN_PASS1:
      frame_outputs(i)
    for kind, c in cams.get(i, []):
      _emit_camlight(G, kind, c)
    # cinert (mj_comPos :211-222), crb starts as a copy (mj_crb :1360)
    if i:
      E(f"double crb_{i}[10];")
      E.open()
      E("double off[3];")
      E(f"mjh::sub3(off, xipos_{i}, keep_stc_{M.rootid[i]});")
      E(f"const double inert[3] = {arr_lit(m.body_inertia[i])};")
      E(f"mjh::inertCom(crb_{i}, inert, ximat_{i}, off, {lit(M.mass[i])});")
      E.close()
      G.stv("cinert", 10 * i, f"crb_{i}", 10)
    else:
      E(_CRB0_DECL)
      G.stv_const("cinert", 0, "crb_0", 10, _CRB0_DECL)
    # cdof (mj_comPos :225-268)
    ja, jn = int(m.body_jntadr[i]), int(m.body_jntnum[i])
    for j in range(ja, ja + jn):
      da = int(m.jnt_dofadr[j])
      t = int(m.jnt_type[j])
      ndof = M.jnt_ndof(j)
      for k in range(ndof):
        E(f"double cdof_{da + k}[6];")
      E.open()
      E("double off[3], axis[3];")
      E(f"mjh::sub3(off, keep_stc_{M.rootid[i]}, xanchor_{j});")
      skip = 0
      if t == FREE:
        for k in range(3):
          E(f"mjh::zero(cdof_{da + k}, 6); cdof_{da + k}[{3 + k}] = 1.0;")
        skip = 3
      if t in (FREE, BALL):
        for k in range(3):
          E(f"axis[0] = xmat_{i}[{k}]; axis[1] = xmat_{i}[{k + 3}]; axis[2] = xmat_{i}[{k + 6}];")
          E(f"mjh::dofComHinge(cdof_{da + skip + k}, axis, off);")
      elif t == SLIDE:
        E(f"mjh::zero3(cdof_{da}); mjh::copy3(cdof_{da} + 3, xaxis_{j});")
      else:
        E(f"mjh::dofComHinge(cdof_{da}, xaxis_{j}, off);")
      E.close()
      for k in range(ndof):
        cc = const_cdof(m, da + k)
        if cc is None:
          G.stv("cdof", 6 * (da + k), f"cdof_{da + k}", 6)
        else:       # the literals mjh::zero and the 1.0 above leave in cdof_<k>
          G.stv_const("cdof", 6 * (da + k), f"cdof_{da + k}", 6,
                      f"const double cdof_{da + k}[6] = {arr_lit(cc)};")

  def post2(i):
    # crb_i is final: every child (higher index) has been added, in descending order
    if i:
      G.stv("crb", 10 * i, f"crb_{i}", 10)
    else:           # nothing is added to the world's (the parent > 0 test below)
      G.stv_const("crb", 0, "crb_0", 10, _CRB0_DECL)
    # qM rows of this body's dofs (mj_crb :1370-1399); qM starts zeroed (mju_zero)
    for k in range(M.bdofadr[i], M.bdofadr[i] + M.bdofnum[i]):
      adr = M.Madr[k]
      rowlen = len(qm_row(M, k))
      if M.simplenum[k]:
        G.st("qM", adr, lit(m.dof_M0[k]))
        for a in range(adr + 1, adr + rowlen):
          G.st("qM", a, "0.0")
        continue
      E.open()
      E("double buf[6];")
      E(f"mjh::mulInertVec(buf, crb_{i}, cdof_{k});")
      j, a, first = k, adr, True
      while j >= 0:
        expr = (f"{lit(m.dof_armature[k])} + mjh::dot6(cdof_{j}, buf)" if first
                else f"0.0 + mjh::dot6(cdof_{j}, buf)")
        G.st("qM", a, expr)
        first = False
        a += 1
        j = M.dparent[j]
      E.close()
    if i and M.parent[i] > 0:
      E(f"mjh::addTo(crb_{M.parent[i]}, crb_{i}, 10);")
    E.close()

  M.dfs(pre2, post2)
  return E.text()


def _emit_camlight(G: _Stage, kind, c):
  """mj_camlight (engine_core_smooth.c:275-392) for one camera or light on the current body."""
  E, m = G.E, G.M.m
  E.open()
  if kind == "cam":
    b = int(m.cam_bodyid[c])
    mode = int(m.cam_mode[c])
    tgt = int(m.cam_targetbodyid[c])
    _emit_local2global(G, "cp", "cm", m.cam_pos[c], m.cam_quat[c], b, 0)
    if mode in (1, 2):
      E(f"const double mat0[9] = {arr_lit(m.cam_mat0[c])};")
      E("mjh::copy(cm, mat0, 9);")
      if mode == 1:
        E(f"const double p0[3] = {arr_lit(m.cam_pos0[c])};")
        E(f"mjh::add3(cp, xpos_{b}, p0);")
      else:
        E(f"const double p0[3] = {arr_lit(m.cam_poscom0[c])};")
        E(f"mjh::add3(cp, keep_stc_{b}, p0);")
    elif mode in (3, 4) and tgt >= 0:
      src = f"keep_xpos_{tgt}" if mode == 3 else f"keep_stc_{tgt}"
      E("double matT[9];")
      E(f"mjh::sub3(matT + 6, cp, {src});")
      E("mjh::normalize3s(matT + 6);")
      E("matT[3] = 0; matT[4] = 0; matT[5] = 1;")
      E("mjh::cross(matT, matT + 3, matT + 6);")
      E("mjh::normalize3s(matT);")
      E("mjh::cross(matT + 3, matT + 6, matT);")
      E("mjh::normalize3s(matT + 3);")
      E("for (int r = 0; r < 3; r++) for (int q = 0; q < 3; q++) cm[3*q + r] = matT[3*r + q];")
    G.stv("cam_xpos", 3 * c, "cp", 3)
    G.stv("cam_xmat", 9 * c, "cm", 9)
  else:
    l = c
    b = int(m.light_bodyid[l])
    mode = int(m.light_mode[l])
    tgt = int(m.light_targetbodyid[l])
    E(f"const double lp[3] = {arr_lit(m.light_pos[l])};")
    E(f"const double ld[3] = {arr_lit(m.light_dir[l])};")
    E("double lx[3], dx[3];")
    E(f"mjh::mulMatVec3(lx, xmat_{b}, lp);")
    E(f"mjh::addTo3(lx, xpos_{b});")
    E(f"mjh::rotVecQuat(dx, ld, xquat_{b});")
    if mode in (1, 2):
      E(f"const double d0[3] = {arr_lit(m.light_dir0[l])};")
      E("mjh::copy3(dx, d0);")
      if mode == 1:
        E(f"const double p0[3] = {arr_lit(m.light_pos0[l])};")
        E(f"mjh::add3(lx, xpos_{b}, p0);")
      else:
        E(f"const double p0[3] = {arr_lit(m.light_poscom0[l])};")
        E(f"mjh::add3(lx, keep_stc_{b}, p0);")
    elif mode in (3, 4) and tgt >= 0:
      src = f"keep_xpos_{tgt}" if mode == 3 else f"keep_stc_{tgt}"
      E(f"mjh::sub3(dx, {src}, lx);")
    E("mjh::normalize3s(dx);")
    G.stv("light_xpos", 3 * l, "lx", 3)
    G.stv("light_xdir", 3 * l, "dx", 3)
  E.close()


# ------------------------------------------------------------------------------ k_fac
def _gen_fac(M: _Model, store_fields=None) -> str:
  """mj_factorM / mj_factorI (engine_core_smooth.c:1470-1511) on qM loaded from the mirror."""
  G = _Stage(M, store_fields)
  E, m = G.E, M.m
  nv = M.nv
  G.prologue()
  G.pointers(["qM", "qLD", "qLDiagInv"])
  rownnz = [int(x) for x in m.C_rownnz]
  rowadr = [int(x) for x in m.C_rowadr]
  colind = [int(x) for x in m.C_colind]
  mapM2C = [int(x) for x in m.mapM2C]
  for a in range(m.nM):
    E(f"const double M_{a} = mjh::takeQM<HO>({_ho_ref(M, M.handoff[a], 'fac')}, P_qM + {a}*64);"
      if a in M.handoff else f"const double M_{a} = HO ? fw[{M.forward[a]}] : P_qM[{a}*64];"
      if a in M.forward else f"const double M_{a} = P_qM[{a}*64];")
  E(f"double {', '.join(f'L_{c} = M_{mapM2C[c]}' for c in range(m.nC))};")
  for k in range(nv - 1, -1, -1):
    ra = rowadr[k]
    dk = ra + rownnz[k] - 1
    E(f"const double diaginv_{k} = 1 / L_{dk};")
    G.st("qLDiagInv", k, f"diaginv_{k}")
    if not M.simplenum[k]:
      for a in range(dk - 1, ra - 1, -1):
        ii = colind[a]
        E.open()
        E(f"double tmp = L_{a} * diaginv_{k};")
        for t in range(rownnz[ii]):
          E(f"L_{rowadr[ii] + t} += L_{ra + t} * -tmp;")
        E(f"L_{a} = tmp;")
        E.close()
    # row k is final once its own update is done (later rows only update rows < k)
    for c in range(ra, ra + rownnz[k]):
      G.st("qLD", c, f"L_{c}")
  return E.text()


# ------------------------------------------------------------------------------ k_vel / k_acc
def _emit_muldofvec(E, res, arrname, bda, n, vec):
  """mju_mulDofVec (engine_util_spatial.c:481-489) with dof arrays named arrname_<k>."""
  if n == 1:
    E(f"mjh::scl({res}, {arrname}_{bda}, {vec}[{bda}], 6);")
  elif n <= 0:
    E(f"mjh::zero({res}, 6);")
  else:
    E(f"mjh::zero({res}, 6);")
    for r in range(n):
      E(f"mjh::addToSclIf({res}, {arrname}_{bda + r}, {vec}[{bda + r}], 6);")


def _gravity_acc(M, E):
  m = M.m
  E("double cacc_0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};")
  if not (M.dsbl & (1 << 6)):
    g = m.opt["gravity"]
    E(f"cacc_0[3] = {lit(g[0])}*-1; cacc_0[4] = {lit(g[1])}*-1; cacc_0[5] = {lit(g[2])}*-1;")


def _gen_va(M: _Model, store_fields=None) -> str:
  """Velocity and acceleration stages in one kernel: fwdVelocity, passive, then one tree
  pass with mj_comVel and both mj_rne calls (flg_acc = 0 -> qfrc_bias, 1 -> qfrc_inverse).
  The two RNE recursions share cdof_dot*qvel and the gyroscopic term cvel x (cinert*cvel),
  which the reference computes identically in each call."""
  G = _Stage(M, store_fields)
  M.va_stored = G.stored     # filled as the body is emitted; read by generate (k_vaskip)
  E, m = G.E, M.m
  nv, nq, dsbl = M.nv, M.nq, M.dsbl
  recompute = VA_RECOMPUTE and FUSE
  G.prologue()
  if M.cmode == "list":   # k_pos's work-list flag: k_constraint assembles this instance
    E("const bool cflag = ec[0] != 0;")
  G.pointers(["qpos", "qvel", "qacc", "cinert", "cdof", "xipos", "subtree_com", "ten_length",
              "ten_velocity", "actuator_velocity", "actuator_moment", "cvel", "cdof_dot",
              "qfrc_spring",
              "qfrc_damper", "qfrc_gravcomp", "qfrc_fluid", "qfrc_passive", "qfrc_bias",
              "qfrc_constraint", "qfrc_inverse"])
  G.load("qpos", "qpos", nq)
  G.load("qvel", "qvel", nv)
  if m.ntendon:
    G.load("ten_length", "ten_length", m.ntendon)
  E(f"double qfg[{nv}];")
  E(f"mjh::zero(qfg, {nv});")
  has_gravcomp = M.has_gravcomp
  if has_gravcomp:
    E("// ---- mj_gravcomp (engine_passive.c:381-399), bodies in ascending order")
    for b in range(1, M.nbody):
      if m.body_gravcomp[b]:
        _emit_applyforce(E, M, b)

  E("// ---- mj_fwdVelocity (engine_forward.c:193-231)")
  for t in range(m.ntendon):
    if t in M.spatial:
      continue
    E(f"double ten_velocity_{t};")
    E.open()
    E(f"const double J[{nv}] = {arr_lit(M.ten_row(t))};")
    E(f"ten_velocity_{t} = mjh::dot(J, qvel, {nv});")
    E.close()
    G.st("ten_velocity", t, f"ten_velocity_{t}")
  if m.nu and not (dsbl & (1 << 10)):
    for a in range(m.nu):
      adr, n = int(m.moment_rowadr[a]), int(m.moment_rownnz[a])
      g = float(m.actuator_gear[a, 0])
      if int(m.actuator_trntype[a]) in TRN_AFTER:
        continue                       # with its transmission, after the constraint kernel
      if m.actuator_trntype[a] == 3 and int(m.actuator_trnid[a, 0]) in M.spatial:
        continue                       # the tendon pass (csrc/post_pass.h)
      if m.actuator_trntype[a] == 3:   # mju_dotSparse over the tendon row's nonzeros
        if not n:
          G.st("actuator_velocity", a, "0.0")
          continue
        J = M.ten_row(int(m.actuator_trnid[a, 0]))
        cols = [int(c) for c in m.moment_colind[adr:adr + n]]
        E.open()
        E(f"const double mom[{n}] = {arr_lit([float(J[c]) * g for c in cols])};")
        E(f"const int ind[{n}] = {{{', '.join(str(c) for c in cols)}}};")
        G.st("actuator_velocity", a, f"mjh::dotSparse(mom, qvel, {n}, ind)")
        E.close()
        continue
      if int(m.jnt_type[int(m.actuator_trnid[a, 0])]) in (BALL, FREE):
        cols = [int(c) for c in m.moment_colind[adr:adr + n]]
        E.open()                       # the row k_pos stored, over its 3 or 6 columns
        E(f"double mom[{n}];")
        for k in range(n):
          E(f"mom[{k}] = P_actuator_moment[{adr + k}*64];")
        E(f"const int ind[{n}] = {{{', '.join(str(c) for c in cols)}}};")
        G.st("actuator_velocity", a, f"mjh::dotSparse(mom, qvel, {n}, ind)")
        E.close()
        continue
      col = int(m.moment_colind[adr])
      G.st("actuator_velocity", a, f"((0.0 + 0.0) + (0.0 + 0.0)) + {lit(g)}*qvel[{col}]")

  # mj_passive: springs, dampers, tendon spring-dampers (engine_passive.c:436-493)
  E("// ---- mj_passive (engine_passive.c:436-493)")
  E(f"double qfs[{nv}], qfd[{nv}];")
  E(f"mjh::zero(qfs, {nv}); mjh::zero(qfd, {nv});")
  if not (dsbl & (1 << 5)):
    for j in range(M.njnt):
      k = float(m.jnt_stiffness[j])
      if k == 0:
        continue
      pa, da, t = int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j]), int(m.jnt_type[j])
      if t == FREE:
        for c in range(3):
          E(f"qfs[{da + c}] = -{lit(k)}*(qpos[{pa + c}] - {lit(m.qpos_spring[pa + c])});")
        pa += 3
        da += 3
        t = BALL
      if t == BALL:
        E.open()
        E(f"double dif[3], quat[4]; mjh::copy4(quat, qpos + {pa}); mjh::normalize4s(quat);")
        E(f"const double qs[4] = {arr_lit(m.qpos_spring[pa:pa + 4])};")
        E("mjh::subQuat(dif, quat, qs);")
        for c in range(3):
          E(f"qfs[{da + c}] = -{lit(k)}*dif[{c}];")
        E.close()
      else:
        E(f"qfs[{da}] = -{lit(k)}*(qpos[{pa}] - {lit(m.qpos_spring[pa])});")
    for dof in range(nv):
      b = float(m.dof_damping[dof])
      if b != 0:
        E(f"qfd[{dof}] = -{lit(b)}*qvel[{dof}];")
    for t in range(m.ntendon):
      k, b = float(m.tendon_stiffness[t]), float(m.tendon_damping[t])
      if (k == 0 and b == 0) or t in M.spatial:
        continue                       # spatial: the tendon pass re-forms mj_passive
      lo, hi = m.tendon_lengthspring[t]
      E.open()
      E(f"const double J[{nv}] = {arr_lit(M.ten_row(t))};")
      E(f"double L = ten_length[{t}], fs = 0;")
      E(f"if (L > {lit(hi)}) fs = {lit(k)} * ({lit(hi)} - L);")
      E(f"else if (L < {lit(lo)}) fs = {lit(k)} * ({lit(lo)} - L);")
      E(f"double fd = -{lit(b)} * ten_velocity_{t};")
      E(f"if (fs) mjh::addToScl(qfs, J, fs, {nv});")
      E(f"if (fd) mjh::addToScl(qfd, J, fd, {nv});")
      E.close()
  actgc = set()
  for j in range(M.njnt):
    if m.jnt_actgravcomp[j]:
      actgc.update(range(int(m.jnt_dofadr[j]), int(m.jnt_dofadr[j]) + M.jnt_ndof(j)))
  # the value stored as qfrc_passive stays in qfp[] for the assembly at the dof's body's
  # post-visit (raw-RNE models, cmode 'all', never read it there)
  keep_qfp = VA_KEEP_QFP and M.cmode != "all"
  if keep_qfp:
    E(f"double qfp[{nv}];")
  for dof in range(nv):
    G.st("qfrc_spring", dof, f"qfs[{dof}]")
    G.st("qfrc_damper", dof, f"qfd[{dof}]")
    if has_gravcomp:
      G.st("qfrc_gravcomp", dof, f"qfg[{dof}]")
    else:           # mjh::zero's 0.0, never added to
      G.st_const("qfrc_gravcomp", dof, f"qfg[{dof}]", f"const double qfg[{nv}] = {{0.0}};")
    G.st_const("qfrc_fluid", dof, "0.0")
    if dsbl & (1 << 5):
      passive = "0.0"
    elif has_gravcomp and dof not in actgc:
      passive = f"(qfs[{dof}] + qfd[{dof}]) + qfg[{dof}]"
    else:
      passive = f"qfs[{dof}] + qfd[{dof}]"
    if keep_qfp:
      E(f"qfp[{dof}] = {passive};")
      passive = f"qfp[{dof}]"
    G.st("qfrc_passive", dof, passive)

  # mj_comVel (:1833-1896) and both mj_rne calls (:1969-2023) in one tree pass
  E("// ---- tree pass: mj_comVel + mj_rne(flg_acc=0) + mj_rne(flg_acc=1)")
  if recompute:
    # frames, cinert and cdof recomputed along the pass as k_pos's pass 2 computes them (the
    # same operations on the same inputs: bit-identical values)
    roots = sorted(set(M.rootid[1:]))
    for r in roots:
      E(f"double keep_stc_{r}[3];")
      for c in range(3):
        E(f"keep_stc_{r}[{c}] = P_subtree_com[{3 * r + c}*64];")
    _world_frame(E)
  E(_CVEL0_DECL)
  G.stv_const("cvel", 0, "cvel_0", 6, _CVEL0_DECL)
  _gravity_acc(M, E)
  E("double acca_0[6]; mjh::copy(acca_0, cacc_0, 6);")
  E(f"double qacc[{nv}];")
  # the cdof stack of the current path (VA_LDS_SLOTS), in the pos stage's trig region
  slot = M.va_slot
  sl, ss = _ll("va")[0], _ll("va")[1]
  if slot:
    E("double* const cstk = trig;")
  # row-major qfrc_inverse copy, or (no output array) a harmless second write of the mirror
  # slot: a select instead of a branch keeps the pass one scheduling region
  # the row-major qfrc_inverse copy goes through LDS (qo_lds[lane][k]); the kernel wrapper
  # writes the block's rows out coalesced after the body (an in-place row-major store per
  # dof would scatter 64 lanes over 64 rows)

  def recompute_body(i):
    """Body i's frame, cinert_i and cdof of its dofs (mj_kinematics, mj_comPos :211-268)."""
    _emit_frame(G, i, store=False)
    _emit_local2global(G, f"xipos_{i}", f"ximat_{i}", m.body_ipos[i], m.body_iquat[i], i,
                       int(m.body_sameframe[i]))
    E(f"double cinert_{i}[10];")
    E.open()
    E("double off[3];")
    E(f"mjh::sub3(off, xipos_{i}, keep_stc_{M.rootid[i]});")
    E(f"const double inert[3] = {arr_lit(m.body_inertia[i])};")
    E(f"mjh::inertCom(cinert_{i}, inert, ximat_{i}, off, {lit(M.mass[i])});")
    E.close()
    ja, jn = int(m.body_jntadr[i]), int(m.body_jntnum[i])
    for j in range(ja, ja + jn):
      da, t = int(m.jnt_dofadr[j]), int(m.jnt_type[j])
      for k in range(M.jnt_ndof(j)):
        E(f"double cdof_{da + k}[6];")
      E.open()
      E("double off[3], axis[3];")
      E(f"mjh::sub3(off, keep_stc_{M.rootid[i]}, xanchor_{j});")
      skip = 0
      if t == FREE:
        for k in range(3):
          E(f"mjh::zero(cdof_{da + k}, 6); cdof_{da + k}[{3 + k}] = 1.0;")
        skip = 3
      if t in (FREE, BALL):
        for k in range(3):
          E(f"axis[0] = xmat_{i}[{k}]; axis[1] = xmat_{i}[{k + 3}]; axis[2] = xmat_{i}[{k + 6}];")
          E(f"mjh::dofComHinge(cdof_{da + skip + k}, axis, off);")
      elif t == SLIDE:
        E(f"mjh::zero3(cdof_{da}); mjh::copy3(cdof_{da} + 3, xaxis_{j});")
      else:
        E(f"mjh::dofComHinge(cdof_{da}, xaxis_{j}, off);")
      E.close()

  def pre(i):
    if not i:
      return
    bda, dn = M.bdofadr[i], M.bdofnum[i]
    p = M.parent[i]
    E.open(f"{{  // body {i}")
    if recompute:
      recompute_body(i)
    for k in range(bda, bda + dn):
      if k in slot:
        E(f"mjh::put6(cstk, {slot[k]}, {ss}, {sl}, cdof_{k});")
    E(f"double cvel_{i}[6];")
    E(f"mjh::copy(cvel_{i}, cvel_{p}, 6);")
    j = 0
    while j < dn:
      t = int(m.jnt_type[M.djnt[bda + j]])
      if t == FREE:
        for k in range(3):
          E(f"double cdofdot_{bda + k}[6] = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};")
        E.open()
        E("double tmp[6];")
        E("mjh::zero(tmp, 6);")
        for r in range(3):
          E(f"mjh::addToSclIf(tmp, cdof_{bda + r}, qvel[{bda + r}], 6);")
        E(f"mjh::addTo(cvel_{i}, tmp, 6);")
        E.close()
        j += 3
        t = BALL
      if t == BALL:
        for k in range(3):
          E(f"double cdofdot_{bda + j + k}[6];")
          E(f"mjh::crossMotion(cdofdot_{bda + j + k}, cvel_{i}, cdof_{bda + j + k});")
        E.open()
        E("double tmp[6];")
        E("mjh::zero(tmp, 6);")
        for r in range(3):
          E(f"mjh::addToSclIf(tmp, cdof_{bda + j + r}, qvel[{bda + j + r}], 6);")
        E(f"mjh::addTo(cvel_{i}, tmp, 6);")
        E.close()
        j += 3
      else:
        E(f"double cdofdot_{bda + j}[6];")
        E(f"mjh::crossMotion(cdofdot_{bda + j}, cvel_{i}, cdof_{bda + j});")
        E.open()
        E("double tmp[6];")
        E(f"mjh::scl(tmp, cdof_{bda + j}, qvel[{bda + j}], 6);")
        E(f"mjh::addTo(cvel_{i}, tmp, 6);")
        E.close()
        j += 1
    G.stv("cvel", 6 * i, f"cvel_{i}", 6)
    for k in range(bda, bda + dn):
      if const_cdof(m, k) is None:
        G.stv("cdof_dot", 6 * k, f"cdofdot_{k}", 6)
      else:         # a free joint's translational rows: the zeros declared above
        G.stv_const("cdof_dot", 6 * k, f"cdofdot_{k}", 6,
                    f"double cdofdot_{k}[6] = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};")
    # forward step of both recursions (engine_core_smooth.c:1986-2006)
    E(f"double cacc_{i}[6], cfrc_{i}[6], acca_{i}[6], frca_{i}[6];")
    E.open()
    E("double tmp[6], tmp1[6];")
    _emit_muldofvec(E, "tmp", "cdofdot", bda, dn, "qvel")
    E("mjh::pin(tmp, 6);")       # shared with _gen_acc: both round these terms alike
    E(f"mjh::add(cacc_{i}, cacc_{p}, tmp, 6);")
    E(f"mjh::add(acca_{i}, acca_{p}, tmp, 6);")
    _emit_muldofvec(E, "tmp", "cdof", bda, dn, "qacc")
    E(f"mjh::addTo(acca_{i}, tmp, 6);")
    E(f"mjh::mulInertVec(cfrc_{i}, cinert_{i}, cacc_{i});")
    E(f"mjh::mulInertVec(frca_{i}, cinert_{i}, acca_{i});")
    E(f"mjh::mulInertVec(tmp, cinert_{i}, cvel_{i});")
    E(f"mjh::crossForce(tmp1, cvel_{i}, tmp);")
    E("mjh::pin(tmp1, 6);")
    E(f"mjh::addTo(cfrc_{i}, tmp1, 6);")
    E(f"mjh::addTo(frca_{i}, tmp1, 6);")
    E.close()

  def post(i):
    if not i:
      return
    # cfrc_i is final (children added in descending order): project, then add to the parent
    # (engine_core_smooth.c:2008-2022); qfrc_inverse += armature*qacc - passive - constraint
    cd = "cdofp"
    for k in range(M.bdofadr[i], M.bdofadr[i] + M.bdofnum[i]):
      if k in slot:
        E(f"mjh::get6({cd}_{k}, cstk, {slot[k]}, {ss}, {sl});")
    for k in range(M.bdofadr[i], M.bdofadr[i] + M.bdofnum[i]):
      G.st("qfrc_bias", k, f"mjh::dot6({cd}_{k}, cfrc_{i})")
      E.open()
      E(f"double qfi = mjh::dot6({cd}_{k}, frca_{i});")
      if M.cmode == "all":     # raw rne: k_constraint assembles every instance
        G.st("qfrc_inverse", k, "qfi")
      else:
        E(f"const double qfa = qfi + ({lit(m.dof_armature[k])} * qacc[{k}] - {qfp(k)} - 0.0);")
        if M.cmode == "list":
          E("qfi = cflag ? qfi : qfa;")
        else:
          E("qfi = qfa;")
        G.st_const("qfrc_constraint", k, "0.0")
        G.st("qfrc_inverse", k, "qfi")
        E(f"qo_lds[{_ll('va')[0]}*{nv} + {k}] = qfi;")
      E.close()
    if M.parent[i]:
      E(f"mjh::addTo(cfrc_{M.parent[i]}, cfrc_{i}, 6);")
      E(f"mjh::addTo(frca_{M.parent[i]}, frca_{i}, 6);")
    E.close()

  def qfp(k):
    return f"qfp[{k}]" if keep_qfp else f"qfp_{k}"

  def cdof_decl(nm, k):
    """cdof of dof k under the name nm: a literal where it is a model constant."""
    c = const_cdof(m, k)
    return f"double {nm}_{k}[6];" if c is None else f"const double {nm}_{k}[6] = {arr_lit(c)};"

  def loads(kind, i):
    dofs = range(M.bdofadr[i], M.bdofadr[i] + M.bdofnum[i])
    if recompute and kind == "pre":     # cinert and cdof recomputed, qacc from the mirror
      return [], [(f"qacc[{k}]", "qacc", k) for k in dofs]
    if kind == "pre":
      decls = [f"double cinert_{i}[10];"] + [cdof_decl("cdof", k) for k in dofs]
      ld = _vec_loads(f"cinert_{i}", "cinert", 10 * i, 10)
      for k in dofs:
        if const_cdof(m, k) is None:
          ld += _vec_loads(f"cdof_{k}", "cdof", 6 * k, 6)
        ld += [(f"qacc[{k}]", "qacc", k)]
    else:
      # the projections take cdof from the path's LDS stack; a dof past its capacity reloads
      # it from the mirror rather than keeping it live along the path
      decls = [cdof_decl("cdofp", k) for k in dofs]
      ld = []
      for k in dofs:
        if k not in slot and const_cdof(m, k) is None:
          ld += _vec_loads(f"cdofp_{k}", "cdof", 6 * k, 6)
        if not keep_qfp and M.cmode != "all":
          decls.append(f"double qfp_{k};")
          ld += [(f"qfp_{k}", "qfrc_passive", k)]
    return decls, ld

  _prefetched_dfs(G, loads, pre, post, PREFETCH)
  if M.cmode == "none":
    E("ec[0] = 0; ec[64] = 0; ec[128] = 0; ec[192] = 0;")
  elif M.cmode == "list":   # served instances get their counts from k_constraint
    E("if (!cflag) { ec[0] = 0; ec[64] = 0; ec[128] = 0; ec[192] = 0; }")
  E("if (status) status[inst] = 0;")
  return E.text()


def _perturb_loads(body: str, which: dict) -> str:
  """mjd_inverseFD's perturbation applied as an input lands: `arr[k] = <load>;` becomes
  `arr[k] = k == idx ? <load> + eps : <load>;` for arr in `which` (arr -> index variable), the
  sum k_fd_expand would have stored (engine_derivative_fd.c:646-699: x[i] + eps)."""
  import re

  def sub(mt):
    arr, k, rhs = mt.group(2), mt.group(3), mt.group(4)
    return (f"{mt.group(1)}{arr}[{k}] = ({which[arr]} == {k}) ? ({rhs}) + eps : ({rhs});")
  names = "|".join(which)
  out, n = re.subn(rf"^(\s*)({names})\[(\d+)\] = (.*P_(?:{names})\[\d+\*64\].*);$", sub,
                   body, flags=re.M)
  # every line that loads a perturbed input must have been rewritten: a load of another shape
  # would silently leave that Jacobian column unperturbed (zero)
  loads = len(re.findall(rf"^.*P_(?:{names})\[[^\]]+\](?!\)? ?=[^=]).*$", body, flags=re.M))
  assert n == loads, f"_perturb_loads: rewrote {n} of {loads} lines loading {sorted(which)}"
  return out


def _gen_acc(M: _Model, store_fields=None) -> str:
  """The acceleration stage alone: mj_inverseSkip(mjSTAGE_VEL) (engine_inverse.c:197-261)
  with the position and velocity stages' outputs read from the mirror. One tree pass of
  mj_rne(flg_acc = 1) (engine_core_smooth.c:1969-2023) over the stored cinert, cdof, cvel and
  cdof_dot, then the assembly qfrc_inverse += armature*qacc - passive - constraint, with the
  same operations as the va stage's second recursion, so the result is its bit for bit. An
  instance with rows (work-list models) stores the raw RNE for the rows pass (k_skip_rows)."""
  G = _Stage(M, store_fields)
  E, m = G.E, M.m
  nv = M.nv
  G.prologue()
  if M.cmode == "list":
    E("const bool cflag = ec[0] != 0;")
  G.pointers(["qvel", "qacc", "cinert", "cdof", "cvel", "cdof_dot", "qfrc_passive",
              "qfrc_constraint", "qfrc_inverse"])
  G.load("qvel", "qvel", nv)
  E(f"double qacc[{nv}];")
  E("// ---- tree pass: mj_rne(flg_acc=1) over the stored velocity-stage outputs")
  _gravity_acc(M, E)
  E("double acca_0[6]; mjh::copy(acca_0, cacc_0, 6);")

  def pre(i):
    if not i:
      return
    bda, dn = M.bdofadr[i], M.bdofnum[i]
    p = M.parent[i]
    E.open(f"{{  // body {i}")
    E(f"double acca_{i}[6], frca_{i}[6];")
    E.open()
    E("double tmp[6], tmp1[6];")
    _emit_muldofvec(E, "tmp", "cdofdot", bda, dn, "qvel")
    E("mjh::pin(tmp, 6);")       # as _gen_va pins them (there each has two uses)
    E(f"mjh::add(acca_{i}, acca_{p}, tmp, 6);")
    _emit_muldofvec(E, "tmp", "cdof", bda, dn, "qacc")
    E(f"mjh::addTo(acca_{i}, tmp, 6);")
    E(f"mjh::mulInertVec(frca_{i}, cinert_{i}, acca_{i});")
    E(f"mjh::mulInertVec(tmp, cinert_{i}, cvel_{i});")
    E(f"mjh::crossForce(tmp1, cvel_{i}, tmp);")
    E("mjh::pin(tmp1, 6);")
    E(f"mjh::addTo(frca_{i}, tmp1, 6);")
    E.close()

  def post(i):
    if not i:
      return
    for k in range(M.bdofadr[i], M.bdofadr[i] + M.bdofnum[i]):
      E.open()
      E(f"double qfi = mjh::dot6(cdofp_{k}, frca_{i});")
      if M.cmode == "all":
        G.st("qfrc_inverse", k, "qfi")
      else:
        E(f"const double qfa = qfi + ({lit(m.dof_armature[k])} * qacc[{k}] - qfp_{k} - 0.0);")
        E("qfi = cflag ? qfi : qfa;" if M.cmode == "list" else "qfi = qfa;")
        G.st_const("qfrc_constraint", k, "0.0")
        G.st("qfrc_inverse", k, "qfi")
        E(f"qo_lds[{_ll('va')[0]}*{nv} + {k}] = qfi;")
      E.close()
    if M.parent[i]:
      E(f"mjh::addTo(frca_{M.parent[i]}, frca_{i}, 6);")
    E.close()

  def loads(kind, i):
    dofs = range(M.bdofadr[i], M.bdofadr[i] + M.bdofnum[i])
    if kind == "pre":
      decls = [f"double cinert_{i}[10], cvel_{i}[6];"] + \
          [f"double cdof_{k}[6], cdofdot_{k}[6];" for k in dofs]
      ld = _vec_loads(f"cinert_{i}", "cinert", 10 * i, 10) + \
          _vec_loads(f"cvel_{i}", "cvel", 6 * i, 6)
      for k in dofs:
        ld += _vec_loads(f"cdof_{k}", "cdof", 6 * k, 6) + \
            _vec_loads(f"cdofdot_{k}", "cdof_dot", 6 * k, 6) + [(f"qacc[{k}]", "qacc", k)]
    else:
      decls = [f"double cdofp_{k}[6], qfp_{k};" for k in dofs]
      ld = []
      for k in dofs:
        ld += _vec_loads(f"cdofp_{k}", "cdof", 6 * k, 6) + [(f"qfp_{k}", "qfrc_passive", k)]
    return decls, ld

  _prefetched_dfs(G, loads, pre, post, PREFETCH)
  E("if (status) status[inst] = 0;")
  return E.text()


def _emit_applyforce(E, M, b):
  """mj_gravcomp -> mj_applyFT(force, torque = 0, xipos, body) (engine_passive.c:381-399,
  engine_support.c:1194-1251, mj_jac :389-441) accumulated into qfg. Reads xipos, subtree_com
  and cdof from the mirror (k_pos wrote them)."""
  m, nv = M.m, M.nv
  g = [float(x) for x in m.opt["gravity"]]
  s = -(float(m.body_mass[b]) * float(m.body_gravcomp[b]))
  r = M.rootid[b]
  E.open()
  E(f"double force[3] = {{{lit(g[0])}*{lit(s)}, {lit(g[1])}*{lit(s)}, {lit(g[2])}*{lit(s)}}};")
  E(f"double jacp[{3*nv}], jacr[{3*nv}], qforce[{nv}], off[3];")
  E(f"mjh::zero(jacp, {3*nv}); mjh::zero(jacr, {3*nv});")
  E(f"off[0] = P_xipos[{3*b}*64] - P_subtree_com[{3*r}*64];")
  E(f"off[1] = P_xipos[{3*b + 1}*64] - P_subtree_com[{3*r + 1}*64];")
  E(f"off[2] = P_xipos[{3*b + 2}*64] - P_subtree_com[{3*r + 2}*64];")
  body = b
  while body and not m.body_dofnum[body]:
    body = int(m.body_parentid[body])
  if body:
    i = int(m.body_dofadr[body] + m.body_dofnum[body] - 1)
    while i >= 0:
      E.open()
      E("double cd[6], tmp[3];")
      for c in range(6):
        E(f"cd[{c}] = P_cdof[{6*i + c}*64];")
      E(f"jacr[{i}] = cd[0]; jacr[{i + nv}] = cd[1]; jacr[{i + 2*nv}] = cd[2];")
      E("mjh::cross(tmp, cd, off);")
      E(f"jacp[{i}] = cd[3] + tmp[0]; jacp[{i + nv}] = cd[4] + tmp[1]; "
        f"jacp[{i + 2*nv}] = cd[5] + tmp[2];")
      E.close()
      i = int(m.dof_parentid[i])
  E(f"mjh::mulMatTVec(qforce, jacp, force, 3, {nv}); mjh::addTo(qfg, qforce, {nv});")
  E("double zt[3] = {0.0, 0.0, 0.0};")
  E(f"mjh::mulMatTVec(qforce, jacr, zt, 3, {nv}); mjh::addTo(qfg, qforce, {nv});")
  E.close()


# ------------------------------------------------------------------------------ assembly
def model_hash(m) -> str:
  h = hashlib.sha1()
  for f in fields.MODEL_FIELDS:
    h.update(np.ascontiguousarray(getattr(m, f.name)).tobytes())
  h.update(repr(sorted(m.opt.items())).encode())
  return h.hexdigest()[:12]


_SIG = {
    "pos": ("const double* __restrict__ qpos_in, const double* __restrict__ qvel_in, "
            "const double* __restrict__ qacc_in, int* __restrict__ worklist, "
            "int* __restrict__ worklist_count, int* __restrict__ worklist_next, "
            "int* __restrict__ efc_count, double* __restrict__ trig, "
            "double* __restrict__ qo_lds",
            "qpos_in, qvel_in, qacc_in, worklist, worklist_count, worklist_next, efc_count, trig, "
            "qo_lds"),
    "fac": ("int* __restrict__ efc_count, const double* __restrict__ trig, "
            "const double* __restrict__ qo_lds", "efc_count, trig, qo_lds"),
    "va": ("double* __restrict__ qfrc_out, int* __restrict__ status, "
           "int* __restrict__ efc_count, double* __restrict__ qo_lds, "
           "double* __restrict__ trig",
           "qfrc_out, status, efc_count, qo_lds, trig"),
}
# the pos and fac bodies take the qM hand-off's switch (QM_HANDOFF); only k_all and the host
# entry instantiate it set, and the LDS pointers of every other caller may be null
_HO_PARAM = {"pos": ", bool HO = false", "fac": ", bool HO = false", "va": ""}
_GEN = {"pos": lambda M, sf: _gen_pos(M, sf), "fac": lambda M, sf: _gen_fac(M, sf),
        "va": lambda M, sf: _gen_va(M, sf)}


def generate(m, name: str, store_fields=None, extern_c: bool = False, shared: bool = False,
             va_slots=None, handoff=None) -> str:
  """HIP source of the four stage kernels of model `m` (skipstage = mjSTAGE_NONE).

  Also emits `fast_body_<name>`, which runs fast_const_<name> and then the stage bodies for
  one instance in order (the host harness's entry), `launch_fast_<name>`, which launches the
  kernels, and with CONST_ONCE `k_const_<name>` / `launch_const_<name>` /
  `const_stores_<name>` (a run-time code object: `k_const_<name>` and the device global
  `k_const_count_<name>`, both with C linkage, whether the switch is on or not).
  store_fields: optional set of mirror fields to store (default: all); used only by
  performance experiments (tools/exp_bounds.py) to separate compute from store costs.
  shared: the launch functions get external linkage (a model compiled in another
  translation unit than the registry, generate_registries).
  extern_c: give k_all_<name> C linkage (a run-time code object, specialize.py, whose
  kernel mjhip_contextLoadKernel looks up by name).
  va_slots: capacity of the va stage's cdof stack (default VA_LDS_SLOTS).
  handoff: False leaves the qM hand-off out of the text (default QM_HANDOFF).
  """
  why = fast_path_supported(m)
  if why:
    raise ValueError(f"model '{name}' cannot use the straight-line kernels: {why}")
  M = _Model(m, va_slots, handoff)
  # the forwarded qM entries (QM_FORWARD) travel from the pos body to the fac body in a local
  # array of the caller's, fw: registers once the bodies are inlined into k_all. Every other
  # caller passes null, and with HO = false neither body touches it.
  sig = dict(_SIG)
  nfw = len(M.forward)
  if nfw:
    sig["pos"] = (_SIG["pos"][0] + ", double* __restrict__ fw", _SIG["pos"][1] + ", fw")
    sig["fac"] = (_SIG["fac"][0] + ", const double* __restrict__ fw", _SIG["fac"][1] + ", fw")
  fw_decl = f"double fw[{nfw}];   // the forwarded qM entries (QM_FORWARD)\n" if nfw else ""
  # the pos and fac bodies' HO argument where the hand-off is on (k_all's kernel template
  # argument, the literal in the host entry and in a run-time code object)
  ho = {st: "" if not _HO_PARAM[st] else ", true" if M.handoff or M.forward else ", false"
        for st in STAGES}
  # the region the pos stage's trig and the va stage's cdof stack share, and qo_lds, in
  # doubles per 64 lanes; every wrapper that runs the va body declares the region
  nreg64 = _lds_doubles(m, M.va_nslot, 64)[0]
  assert 8 * sum(_lds_doubles(m, M.va_nslot)) <= LDS_BUDGET, \
      f"k_all_{name}: {8 * sum(_lds_doubles(m, M.va_nslot))} B of LDS, three workgroups per CU"
  # the hand-off lives in the arrays declared below and nowhere else: k_all's static LDS is
  # what it is without it
  assert all(0 <= s < sum(_lds_doubles(m, M.va_nslot, 64)) // 64 for s in M.handoff.values())
  assert len(set(M.handoff.values())) == len(M.handoff)
  bodies = {st: _GEN[st](M, store_fields) for st in STAGES}
  if NT_STORES:
    import re
    # the fac stage's re-reads stay temporal; the other stages' re-reads stream only in the
    # SV = true instantiation of k_all (a batch large enough to oversubscribe L2, NT_SV_MIN_B)
    reread = set(re.findall(r"= P_(\w+)\[", bodies["fac"])) | \
        ({"qM"} if M.handoff or M.forward else set())
    later = set(re.findall(r"= P_(\w+)\[", "\n".join(bodies.values()))) - reread
    if NT_TEMPORAL is not None:
      reread, later = set(NT_TEMPORAL), set()
    store = re.compile(r"^(\s*)P_(\w+)\[(\d+)\*64\] = (.+);$")

    def nt(line):
      mt = store.match(line)
      if mt and mt.group(2) == "qM" and int(mt.group(3)) in M.handoff and "qM" in reread:
        # a handed entry is not re-read where it is handed: it streams there like every
        # write-only field, and stays temporal for the kernels whose fac stage re-reads it
        return f"{mt.group(1)}MJH_NT_STORE_IF(HO, P_qM[{mt.group(3)}*64], {mt.group(4)});"
      if not mt or mt.group(2) in reread:
        return line
      if mt.group(2) in later:
        return (f"{mt.group(1)}MJH_NT_STORE_IF(SV, P_{mt.group(2)}[{mt.group(3)}*64], "
                f"{mt.group(4)});")
      return f"{mt.group(1)}MJH_NT_STORE(P_{mt.group(2)}[{mt.group(3)}*64], {mt.group(4)});"
    bodies = {st: ("\n".join(nt(x) for x in b.split("\n")) if st in NT_STAGES else b)
              for st, b in bodies.items()}
    load = re.compile(r"= P_(\w+)\[(\d+)\*64\];")
    bodies = {st: (load.sub(lambda mt: f"= MJH_NT_LOAD(P_{mt.group(1)}[{mt.group(2)}*64]);", b)
                   if st in NT_LOAD_STAGES else b) for st, b in bodies.items()}
    bodies = {st: (load.sub(lambda mt: f"= MJH_NT_LOAD_IF(SV, P_{mt.group(1)}[{mt.group(2)}*64]);",
                            b)
                   if st in NT_LOAD_SV_STAGES and st not in NT_LOAD_STAGES else b)
              for st, b in bodies.items()}
  # the generator-constant stores (CONST_ONCE): every lane of every block of the capacity, so
  # no instance bound; plain stores (one launch per context, nothing to keep out of L2)
  nconst = len(M.consts)
  const_text = ""
  if CONST_ONCE:
    C = _Stage(M)
    C.pointers(sorted({f for f, _ in M.consts}))
    for d in M.const_decls:
      for line in d.split("\n"):
        C.E(line)
    for (f, k), expr in M.consts.items():
      C.E(f"P_{f}[{k}*64] = {expr};")
    C.E("(void)mr; (void)blk; (void)lane;")
    const_text = C.E.text()
  if M.cmode in ("none", "list") and store_fields is None:
    # the host entry's FD blocks keep the elided fields untouched, constants included (on the
    # device k_const runs the plain instantiation over the whole capacity)
    elided = fd_elided(list(bodies.values()) + [const_text])
    bodies = {st: _elide_stores(b, elided) for st, b in bodies.items()}
    const_text = _elide_stores(const_text, elided)
  out = [f"// GENERATED by mujoco_inversedynamicstest_amd/codegen.py -- do not edit.",
         f"// model '{name}' (nq={m.nq} nv={m.nv} nbody={m.nbody}), hash {model_hash(m)}"]
  exact = exact_fp(m)
  if exact:   # frames for the native solver: every operation rounded (exact_fp)
    out.append("#if defined(__clang__)\n#pragma clang fp contract(off)\n#endif")
  for st in STAGES:
    params, args = sig[st]
    out.append(f"template <bool SV = true, bool FD = false{_HO_PARAM[st]}>\n"
               f"MJH_HD void fast_{st}_{name}(const Mirror& mr, int blk, int lane, int B, "
               f"{params}) {{\n{bodies[st]}\n}}\n")
  const_call = ""
  if CONST_ONCE:
    out.append(f"template <bool FD = false>\n"
               f"MJH_HD void fast_const_{name}(const Mirror& mr, int blk, int lane) {{\n"
               f"{const_text}\n}}\n")
    const_call = (f"  if (fd) fast_const_{name}<true>(mr, blk, lane);\n"
                  f"  else fast_const_{name}<false>(mr, blk, lane);\n")
  out.append(f"""MJH_HD void fast_body_{name}(
    const Mirror& mr, int blk, int lane, int B, const double* __restrict__ qpos_in,
    const double* __restrict__ qvel_in, const double* __restrict__ qacc_in,
    double* __restrict__ qfrc_out, int* __restrict__ status, int* __restrict__ worklist,
    int* __restrict__ worklist_count, int* __restrict__ worklist_next,
    int* __restrict__ efc_count) {{
  double trig[{nreg64}];   // LDS on the device (k_pos's trig, then k_va's cdof stack)
  double qo_lds[{64 * max(M.nv, 1)}];             // LDS on the device (k_va; the qM hand-off)
  const bool fd = mr.fd_elide && blk >= mr.full_blk;   // mjd_inverseFD's perturbed blocks
""" + ("  " + fw_decl if nfw else "") + const_call + "".join(f"  if (fd) fast_{st}_{name}<true, true{ho[st]}>(mr, blk, lane, B, {sig[st][1]});\n"
              f"  else fast_{st}_{name}<true, false{ho[st]}>(mr, blk, lane, B, {sig[st][1]});\n"
              for st in STAGES)
             + (f"""  if (qfrc_out && (long)blk*64 + lane < B) {{
    for (int k = 0; k < {M.nv}; k++) qfrc_out[((long)blk*64 + lane)*{M.nv} + k] = qo_lds[lane*{M.nv} + k];
  }}
""" if M.cmode != "all" else "  (void)qo_lds;\n") + "}\n")
  out.append("#if defined(__HIPCC__)")
  for st in STAGES:
    params, args = sig[st]
    tail = ""
    nl = LANES[st]
    sub = 64 // nl    # workgroups per 64-instance block
    if st == "pos":                                # staged: qM goes through the mirror
      params = params.replace(", double* __restrict__ trig", "")
      params = params.replace(", double* __restrict__ qo_lds", "")
      params = params.replace(", double* __restrict__ fw", "")
      args = args.replace(", qo_lds", ", nullptr").replace(", fw", ", nullptr")
      decl = f"  __shared__ double trig[{max(1, 2 * len(M.trig) * nl)}];\n"
    elif st == "va":
      params = params.replace(", double* __restrict__ qo_lds", "")
      params = params.replace(", double* __restrict__ trig", "")
      # staged k_va: no LDS trig (not fused), a region of its own for the cdof stack
      decl = f"  __shared__ double qo_lds[{nl * max(M.nv, 1)}];\n"
      if M.va_slot:
        decl += f"  __shared__ double trig[{6 * M.va_nslot * nl}];\n"
      else:
        args = args.replace(", trig", ", nullptr")
      if M.cmode != "all":   # coalesced row-major copy of the workgroup's qfrc_inverse rows
        tail = (f"  if (!qfrc_out) return;\n  __syncthreads();\n"
                f"  const long r0 = (long)blockIdx.x*{nl};\n"
                f"  const long n = ((long)B - r0 < {nl} ? (long)B - r0 : {nl}) * {M.nv};\n"
                f"  double* dst = qfrc_out + r0*{M.nv};\n"
                f"  for (long r = threadIdx.x; r < n; r += {nl}) dst[r] = qo_lds[r];\n")
    else:
      params = params.replace(", const double* __restrict__ trig", "")
      params = params.replace(", const double* __restrict__ qo_lds", "")
      params = params.replace(", const double* __restrict__ fw", "")
      args = args.replace(", trig, qo_lds", ", nullptr, nullptr").replace(", fw", ", nullptr")
      decl = ""
    if sub == 1:
      bl = "blockIdx.x, threadIdx.x"
    else:
      bl = f"blockIdx.x / {sub}, (blockIdx.x % {sub})*{nl} + threadIdx.x"
    out.append(f"__global__ __launch_bounds__({nl}, 1) void k_{st}_{name}(Mirror mr, int B, "
               f"{params}) {{\n{decl}  fast_{st}_{name}(mr, {bl}, B, {args});\n"
               f"{tail}}}")
  # k_all: the three stage bodies back to back in one launch. Each stage re-reads what the
  # previous one stored (a compiler memory barrier between them keeps the reloads), so the
  # live ranges stay those of the staged kernels; the reloads hit the wave's own freshly
  # written lines in L2, and no wave waits for the whole grid at a kernel boundary.
  nl = ALL_LANES
  if nl != 64:
    assert all(LANES[st] == nl for st in STAGES), "stage LDS indexing must match ALL_LANES"
  sub = 64 // nl
  ntrig, nqo = _lds_doubles(m, M.va_nslot, nl)
  # kernels that run the va body without the pos stage before it (64 lanes each) hold the
  # cdof stack in an array of their own
  stk_decl = f"  __shared__ double trig[{6 * M.va_nslot * 64}];\n" if M.va_slot else ""
  stk_arg = "trig" if M.va_slot else "nullptr"
  fuse_tail = ""
  if M.cmode != "all":
    fuse_tail = (f"  if (!qfrc_out) return;\n  __syncthreads();\n"
                 f"  const long r0 = (long)blockIdx.x*{nl};\n"
                 f"  const long n = ((long)B - r0 < {nl} ? (long)B - r0 : {nl}) * {M.nv};\n"
                 f"  double* dst = qfrc_out + r0*{M.nv};\n"
                 f"  for (long r = threadIdx.x; r < n; r += {nl}) dst[r] = qo_lds[r];\n")
  bl = "blk0 + blockIdx.x, threadIdx.x" if sub == 1 else \
      f"blk0 + blockIdx.x / {sub}, (blockIdx.x % {sub})*{nl} + threadIdx.x"
  fuse_tail = fuse_tail.replace("(long)blockIdx.x*", f"((long)blk0*{sub} + blockIdx.x)*")
  linkage = 'extern "C" ' if extern_c else ""
  # range: null, or a device-side instance range {first, end} (first a multiple of 64) read
  # at the start of the launch, so a launch's extent can be decided by an earlier kernel on
  # the stream (mjhip_inverseFDBatch's limit-centre fall-back) without a host round trip.
  # The next call's work-list counter is zeroed by the launch's first thread, before any
  # instance bound, so an empty range still hands the counters on.
  # SV: the va stage's re-read fields stream too (a batch that oversubscribes L2); a
  # run-time code object (C linkage, no template) has the SV = true kernel only.
  # HO: the pos stage hands the qM entries of M.handoff to the fac stage in LDS
  # (QM_HANDOFF); a run-time code object's one kernel has it set whenever the plan is not empty
  tmpl = "" if extern_c else "template <bool SV, bool FD, bool HO>\n"
  sv = "true" if extern_c else "SV"
  kho = ho if extern_c else {st: ", HO" if _HO_PARAM[st] else "" for st in STAGES}

  def stage_calls(fd, ind="  "):
    return "\n".join(f"{ind}fast_{st}_{name}<{sv}, {fd}{kho[st]}>(mr, {bl}, B, "
                     f"{sig[st][1].replace('worklist_next', 'nullptr')});\n"
                     f"{ind}asm volatile(\"\" ::: \"memory\"); MJH_SCHED_FENCE(); MJH_PHASE({20 + k});"
                     for k, st in enumerate(STAGES))
  # the FD instantiation (mjd_inverseFD's stage-skip layout): the plain bodies on the centres'
  # blocks, the bodies without the elided stores on the blocks past them (Mirror::full_blk)
  blkexpr = "blk0 + (int)blockIdx.x" if sub == 1 else f"blk0 + (int)blockIdx.x / {sub}"
  all_calls = stage_calls("false") if extern_c else (
      f"  if (FD && mr.fd_elide && {blkexpr} >= mr.full_blk) {{\n{stage_calls('true', '    ')}\n"
      f"  }} else {{\n{stage_calls('false', '    ')}\n  }}")
  out.append(f"""{tmpl}{linkage}__global__ __launch_bounds__({nl}, {ALL_WAVES}) void k_all_{name}(Mirror mr, int B,
    const double* __restrict__ qpos_in, const double* __restrict__ qvel_in,
    const double* __restrict__ qacc_in, double* __restrict__ qfrc_out, int* __restrict__ status,
    int* __restrict__ worklist, int* __restrict__ worklist_count, int* __restrict__ worklist_next,
    int* __restrict__ efc_count, const int* __restrict__ range) {{
  __shared__ double trig[{ntrig}];
  __shared__ double qo_lds[{nqo}];
  if (worklist_next && blockIdx.x == 0 && threadIdx.x == 0) *worklist_next = 0;
  int blk0 = 0;
  if (range) {{ blk0 = range[0] >> 6; B = range[1]; }}
  MJH_PHASE0(19, 27);
""" + ("  " + fw_decl if nfw else "") + all_calls + "\n" + fuse_tail + "}")
  # batched mj_inverseSkip(POS / VEL) of a model whose rows serve every instance (contacts):
  # k_va (the staged va kernel) or k_acc store the raw RNE, and k_skip_rows (mjhip.hip)
  # finishes every instance -- the previous call's rows (referenceConstraint for POS,
  # invConstraint) and the assembly -- and writes the row-major output
  if M.cmode == "all" and not extern_c:
    import re
    ab = _gen_acc(M)
    if NT_STORES:
      ab = re.sub(r"^(\s*)P_(\w+)\[(\d+)\*64\] = (.+);$",
                  lambda mt: f"{mt.group(1)}MJH_NT_STORE(P_{mt.group(2)}[{mt.group(3)}*64], "
                             f"{mt.group(4)});", ab, flags=re.M)
    out.append(f"MJH_HD void fast_acc_{name}(const Mirror& mr, int blk, int lane, int B, "
               f"{sig['va'][0]}) {{\n{ab}\n}}\n")
    out.append(f"""__global__ __launch_bounds__(64, 1) void k_acc_{name}(Mirror mr, int B,
    double* __restrict__ qfrc_out, int* __restrict__ status, int* __restrict__ efc_count) {{
  fast_acc_{name}(mr, blockIdx.x, threadIdx.x, B, qfrc_out, status, efc_count, nullptr,
                  nullptr);
}}
{"" if shared else "static "}void launch_skip_{name}(hipStream_t s, const Mirror& mr, int B, int skipstage,
                              double* qfrc_out, int* status, int* efc_count) {{
  (void)qfrc_out;      // raw RNE only: k_skip_rows assembles and writes the output
  if (skipstage == 1) {{
    hipLaunchKernelGGL(k_va_{name}, dim3((B + 63) / 64), dim3(64), 0, s, mr, B, nullptr,
                       status, efc_count);
  }} else {{
    hipLaunchKernelGGL(k_acc_{name}, dim3((B + 63) / 64), dim3(64), 0, s, mr, B, nullptr,
                       status, efc_count);
  }}
}}""")
  # (the skip kernels below are not emitted into a run-time code object: the library looks up
  # only its k_all, mjhip_contextLoadKernel)
  # k_vaskip: the va stage of mj_inverseSkip(mjSTAGE_POS) for mjd_inverseFD's qvel and qacc
  # perturbations (engine_derivative_fd.c:646-699). Instance off + t reads every position-
  # stage output (the va pointers it never stores) from its centre instance
  # (t / per)*sstride, which ran the full kernel; its own qvel/qacc and every field the stage
  # stores stay its own. Skipped stages see unchanged inputs, so the operations are the full
  # pipeline's (the results within the contraction bound, FD_KEEP above). Work-list models: a centre with limit rows sets *needfull, and
  # k_fd_gate (mjhip.hip) then opens the range of a second k_all over the qvel/qacc
  # perturbations, which runs their full pipeline.
  if M.cmode in ("none", "list") and not extern_c:
    import re
    vb = bodies["va"]
    # the fields the va stage stores, as recorded by _Stage.st while emitting it; a store the
    # record missed would leave that pointer based at the centre instance, and all 2nv
    # perturbations would write the centre's slot concurrently, so the text is checked too
    textual = set(re.findall(r"P_(\w+)\[[^\]]+\]\)? ?=[^=]", vb)) | \
        set(re.findall(r"MJH_NT_STORE\(P_(\w+)\[", vb))
    # qpos/qvel/qacc are based at the centre instance unless stored (then `own` keeps them)
    assert textual <= M.va_stored, \
        f"k_vaskip: va stores outside the record: {textual - M.va_stored}"
    # qpos, qvel and qacc are read from the centre too: k_fd_expand writes only the
    # position-stage block, and the perturbed component is added as the loads land (pa / pv:
    # the qacc / qvel dof this instance perturbs, -1 for none)
    own = set(M.va_stored)
    skip_body = re.sub(r"(double\* __restrict__ P_(\w+) = mr\.\w+ \+ \(\(long\))blk(\*\d+\)\*64 \+ )lane;",
                       lambda mt: mt.group(0) if mt.group(2) in own else
                       f"{mt.group(1)}sblk{mt.group(3)}slane;", vb)
    skip_body = skip_body.replace("const bool cflag = ec[0] != 0;",
                                  "const bool cflag = ecs[0] != 0;")
    skip_body = skip_body.replace("MJH_NT_STORE_IF(SV, ", "MJH_NT_STORE_IF(true, ")
    skip_body = skip_body.replace("if constexpr (!FD) {", "if constexpr (false) {")
    assert "FD" not in re.sub(r"\w*FD\w+|\w+FD\w*", "", skip_body), "k_vaskip: FD left"
    skip_body = skip_body.replace("MJH_NT_LOAD_IF(SV, ", "MJH_NT_LOAD_IF(false, ")
    skip_body = _perturb_loads(skip_body, {"qvel": "pv", "qacc": "pa"})
    out.append(f"MJH_HD void fast_vaskip_{name}(const Mirror& mr, int blk, int lane, int sblk, "
               f"int slane, int B, const int* __restrict__ ecs, int pa, int pv, double eps, "
               f"{sig['va'][0]}) {{\n{skip_body}\n}}\n")
  if M.cmode in ("none", "list") and not extern_c:
    # the acceleration stage alone (mj_inverseSkip(mjSTAGE_VEL)): k_acc for batched calls
    import re
    ab = _gen_acc(M)
    if NT_STORES:
      ab = re.sub(r"^(\s*)P_(\w+)\[(\d+)\*64\] = (.+);$",
                  lambda mt: f"{mt.group(1)}MJH_NT_STORE(P_{mt.group(2)}[{mt.group(3)}*64], "
                             f"{mt.group(4)});", ab, flags=re.M)
    out.append(f"MJH_HD void fast_acc_{name}(const Mirror& mr, int blk, int lane, int B, "
               f"{sig['va'][0]}) {{\n{ab}\n}}\n")
  if M.cmode in ("none", "list") and not extern_c:
    flag = ("  if (ecs[0] != 0) needfull[0] = 1;\n" if M.cmode == "list" else "")
    out.append(f"""// layout 1 over [off, B): per = 2nv perturbations per centre, the first nv of qacc, the
// next nv of qvel (engine_derivative_fd.c:646-699 order)
__global__ __launch_bounds__(64, 1) void k_vaskip_{name}(Mirror mr, int B, int off,
    int per, int sstride, int* __restrict__ efc_count, int* __restrict__ needfull, double eps) {{
  __shared__ double qo_lds[{64 * max(M.nv, 1)}];
{stk_decl}  const long gi = (long)off + (long)blockIdx.x*64 + threadIdx.x;
  if (gi >= B) return;
  const long si = (gi - off) / per * sstride;
  const int j = (int)((gi - off) % per);
  const int* ecs = efc_count + (si >> 6)*4*64 + (si & 63);
{flag}  fast_vaskip_{name}(mr, (int)(gi >> 6), (int)(gi & 63), (int)(si >> 6), (int)(si & 63), B,
                    ecs, j < {M.nv} ? j : -1, j < {M.nv} ? -1 : j - {M.nv}, eps, nullptr,
                    nullptr, efc_count, qo_lds, {stk_arg});
}}
{"" if shared else "static "}void launch_vaskip_{name}(hipStream_t s, const Mirror& mr, int B, int off, int per,
                                int sstride, int* efc_count, int* needfull, double eps) {{
  hipLaunchKernelGGL(k_vaskip_{name}, dim3((B - off + 63) / 64), dim3(64), 0, s, mr, B, off,
                     per, sstride, efc_count, needfull, eps);
}}
// batched mj_inverseSkip on the straight-line path: POS runs the va stage (k_va), VEL the
// acceleration stage (k_acc); rows of the previous call go through k_skip_rows (mjhip.hip)
__global__ __launch_bounds__(64, 1) void k_acc_{name}(Mirror mr, int B,
    double* __restrict__ qfrc_out, int* __restrict__ status, int* __restrict__ efc_count) {{
  __shared__ double qo_lds[{64 * max(M.nv, 1)}];
  fast_acc_{name}(mr, blockIdx.x, threadIdx.x, B, qfrc_out, status, efc_count, qo_lds, nullptr);
  if (!qfrc_out) return;
  __syncthreads();
  const long r0 = (long)blockIdx.x*64;
  const long n = ((long)B - r0 < 64 ? (long)B - r0 : 64) * {M.nv};
  double* dst = qfrc_out + r0*{M.nv};
  for (long r = threadIdx.x; r < n; r += 64) dst[r] = qo_lds[r];
}}
{"" if shared else "static "}void launch_skip_{name}(hipStream_t s, const Mirror& mr, int B, int skipstage,
                              double* qfrc_out, int* status, int* efc_count) {{
  if (skipstage == 1) {{
    hipLaunchKernelGGL(k_va_{name}, dim3((B + 63) / 64), dim3(64), 0, s, mr, B, qfrc_out,
                       status, efc_count);
  }} else {{
    hipLaunchKernelGGL(k_acc_{name}, dim3((B + 63) / 64), dim3(64), 0, s, mr, B, qfrc_out,
                       status, efc_count);
  }}
}}""")
  # k_const: one lane per instance slot of the whole capacity (nblk blocks of 64), launched by
  # the library when the context's constant slots may be stale (mjhip.hip ensure_const). A
  # run-time code object always has one, and its count as a device global, both found by name
  if CONST_ONCE or extern_c:
    kbody = f"  fast_const_{name}(mr, blockIdx.x, threadIdx.x);" if CONST_ONCE else "  (void)mr;"
    out.append(f"{linkage}__global__ __launch_bounds__(64) void k_const_{name}(Mirror mr) {{\n"
               f"{kbody}\n}}")
    if extern_c:
      out.append(f'extern "C" __device__ __attribute__((used)) int k_const_count_{name} = '
                 f"{nconst};")
    else:
      out.append(f"""{"" if shared else "static "}void launch_const_{name}(hipStream_t s, const Mirror& mr, int nblk) {{
  hipLaunchKernelGGL(k_const_{name}, dim3(nblk), dim3(64), 0, s, mr);
}}
{"" if shared else "static "}int const_stores_{name}() {{ return {nconst}; }}""")
  assert len(M.consts) == nconst, "a constant store emitted after fast_const was written"
  # the qM entries per instance that k_all's HO instantiation hands on-chip
  # (mjhip_contextQmHandoff); a run-time code object carries the count as a device global
  if extern_c:
    out.append(f'extern "C" __device__ __attribute__((used)) int k_qm_handoff_{name} = '
               f"{len(M.handoff)};")
    out.append(f'extern "C" __device__ __attribute__((used)) int k_qm_forward_{name} = {nfw};')
  else:
    out.append(f"{'' if shared else 'static '}int qm_handoff_{name}() "
               f"{{ return {len(M.handoff) if FUSE else 0}; }}")
    out.append(f"{'' if shared else 'static '}int qm_forward_{name}() "
               f"{{ return {nfw if FUSE else 0}; }}")
  out.append(f"""{"" if shared else "static "}void launch_fast_{name}(dim3 g, dim3 b, hipStream_t s, const Mirror& mr,
    int B, const double* qpos_in, const double* qvel_in, const double* qacc_in, double* qfrc_out,
    int* status, int* worklist, int* worklist_count, int* worklist_next, int* efc_count,
    const int* range) {{""")
  if FUSE:
    gb = "g, b" if ALL_LANES == 64 else f"dim3(g.x*{64 // ALL_LANES}), dim3({ALL_LANES})"
    variants = ((f"B >= {NT_SV_MIN_B}", "<true, false>"), ("true", "<false, false>")) \
        if not extern_c else (("true", ""),)
    if not extern_c and M.cmode in ("none", "list"):   # mjd_inverseFD's perturbed instances
      variants = ((f"mr.fd_elide && B >= {NT_SV_MIN_B}", "<true, true>"),
                  ("mr.fd_elide", "<false, true>")) + variants
    if not extern_c:   # each with the qM hand-off (Mirror::qm_handoff) where there is a plan
      out.append(f"  const bool ho = mr.qm_handoff > 1 || (mr.qm_handoff == 1 && "
                 f"B >= {QM_HANDOFF_MIN_B});")
      variants = tuple(x for cond, v in variants for x in
                       ([(f"ho && ({cond})", v[:-1] + ", true>")] if M.handoff or M.forward else []) +
                       [(cond, v[:-1] + ", false>")])
      if not (M.handoff or M.forward):
        out.append("  (void)ho;")
    for cond, v in variants:
      out.append(f"  if ({cond}) {{\n    hipLaunchKernelGGL((k_all_{name}{v}), {gb}, 0, s, mr, B, "
                 f"qpos_in, qvel_in, qacc_in, qfrc_out, status, worklist, worklist_count, "
                 f"worklist_next, efc_count, range);\n    return;\n  }}")
  else:   # staged kernels (experiments): the whole [0, B) range only
    out.append("  if (range) return;   // device-side ranges need k_all")
    for st in STAGES:
      args = sig["va"][1].replace(", trig", "").replace(", qo_lds", "") if st == "va" else \
          sig[st][1].replace(", trig, qo_lds", "")
      gb = "g, b" if LANES[st] == 64 else f"dim3(g.x*{64 // LANES[st]}), dim3({LANES[st]})"
      out.append(f"  hipLaunchKernelGGL(k_{st}_{name}, {gb}, 0, s, mr, B, {args});")
  out.append("}")
  # the static LDS of the k_all variants, as compiled (mjhip_contextCreate's guard)
  if FUSE and not extern_c:
    out.append(f"{'' if shared else 'static '}int lds_fast_{name}() {{\n"
               f"  hipFuncAttributes a;\n  size_t n = 0;")
    for _, v in variants:
      out.append(f"  if (hipFuncGetAttributes(&a, (const void*)k_all_{name}{v}) != hipSuccess) "
                 f"return -1;\n  n = a.sharedSizeBytes > n ? a.sharedSizeBytes : n;")
    out.append("  return (int)n;\n}")
  else:
    out.append(f"{'' if shared else 'static '}int lds_fast_{name}() {{ return 0; }}")
  out.append("#endif")
  if exact:
    out.append("#if defined(__clang__)\n#pragma clang fp contract(fast)\n#endif")
  return "\n".join(out) + "\n"


def const_slots(m, va_slots=None) -> list:
  """The (field, index) mirror slots whose stores CONST_ONCE moves from the stage bodies of
  model m into fast_const_<name>, in emission order (empty with the switch off): what
  mjhip_contextConstStores counts."""
  M = _Model(m, va_slots)
  for st in STAGES:
    _GEN[st](M, None)
  return list(M.consts)


_TOKEN = re.compile(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'|//[^\n]*|/\*.*?\*/|\s+',
                    re.S)


def code_text(src: str) -> str:
  """C/C++ source with comments removed and every whitespace run collapsed to one space
  (string and character literals kept as written): what the compiler sees, so an edit to a
  comment or to indentation does not change it."""
  parts, pos = [], 0
  for mt in _TOKEN.finditer(src):
    if mt.start() > pos:
      parts.append(src[pos:mt.start()])
    t = mt.group(0)
    if t[0] in "\"'":
      parts.append(t)
    elif parts and parts[-1] != " ":
      parts.append(" ")
    pos = mt.end()
  parts.append(src[pos:])
  return "".join(parts).strip()


# the device sources a generated kernel's translation unit compiles besides its own text
HASHED_HEADERS = ("engine_device.h", "fast_kernels.h", "kernels.h", "post_pass.h",
                  "pair_program.h", "kern_constraint.hip")


def source_hash(m, name: str) -> str:
  """Identity of the code a kernel of model m named `name` is built from: its generated
  source, the device headers it includes and the constraint kernels launched beside it, each
  with comments and whitespace removed (code_text). Keys committed PMC and rocprof summaries
  to the kernels they measured, so a comment edit after the final profiles keeps them
  matched; a run-time kernel, rt_*, has C linkage."""
  import os
  h = hashlib.sha256(code_text(generate(m, name, extern_c=name.startswith("rt_"))).encode())
  csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
  for f in HASHED_HEADERS:
    with open(os.path.join(csrc, f), encoding="utf-8") as fh:
      h.update(code_text(fh.read()).encode())
  return h.hexdigest()[:16]


def hot_kernels(name: str) -> list:
  """Names of the kernels one fast-path launch of model `name` runs (profiles, bench)."""
  return [f"k_all_{name}"] if FUSE else [f"k_{st}_{name}" for st in STAGES]


def generate_registries(entries) -> tuple:
  """entries: list of (name, model). Returns (gen_fast.inc, gen_fast_exact.inc): the models
  with native-solver pairs (exact_fp) go to a translation unit of their own, compiled without
  multiply-add contraction throughout (gen_fast_exact.hip) so they round every operation as
  the oracle does; the others, and the registry of all, to gen_fast.inc."""
  head = ["// GENERATED by mujoco_inversedynamicstest_amd/codegen.py (build()) -- do not edit."]
  main = head + ["// Straight-line mj_inverse kernels for the bundled models + their signatures.", ""]
  exact = head + ["// Straight-line kernels of the bundled models with native-solver pairs.", ""]
  reg = []
  for name, m in entries:
    vaskip = constraint_mode(m) in ("none", "list")
    if exact_fp(m):
      exact.append(generate(m, name, shared=True))
      main.append(f"void launch_fast_{name}(dim3, dim3, hipStream_t, const Mirror&, int, "
                  "const double*, const double*, const double*, double*, int*, int*, int*, "
                  "int*, int*, const int*);")
      if vaskip:
        main.append(f"void launch_vaskip_{name}(hipStream_t, const Mirror&, int, int, int, int, "
                    "int*, int*, double);")
      main.append(f"void launch_skip_{name}(hipStream_t, const Mirror&, int, int, double*, "
                  "int*, int*);")
      main.append(f"int lds_fast_{name}();")
      if CONST_ONCE:
        main.append(f"void launch_const_{name}(hipStream_t, const Mirror&, int);")
        main.append(f"int const_stores_{name}();")
      main.append(f"int qm_handoff_{name}();")
      main.append(f"int qm_forward_{name}();")
    else:
      main.append(generate(m, name))
    vaskip_fn = f"launch_vaskip_{name}" if vaskip else "nullptr"
    const = f"launch_const_{name}, const_stores_{name}" if CONST_ONCE else "nullptr, nullptr"
    reg.append(f'  {{0x{fields.model_signature(m):016x}ull, launch_fast_{name}, "{name}", '
               f'{CONSTRAINT_MODES[constraint_mode(m)]}, {vaskip_fn}, launch_skip_{name}, '
               f'lds_fast_{name}, {const}, qm_handoff_{name}, qm_forward_{name}}},')
  main.append("static const FastKernelEntry g_fast_kernels[] = {")
  main.extend(reg)
  main.append("  {0ull, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, "
              "nullptr, nullptr}};")
  return "\n".join(main) + "\n", "\n".join(exact) + "\n"
