"""Models and states of the constraint-solver tests (tests/test_solver_cpu.py and
tests/test_solver_gpu.py), the restatement's inputs from the oracle's position and velocity
stages, and the forward/inverse identity (the reference's ForwardInverseMatch,
test/engine/engine_inverse_test.cc:35-56) measured with the oracle's mj_inverse."""
import numpy as np

import reference_model_states as rms
import rne_post_cases as rp
import solver_ref
from mujoco_inversedynamicstest_amd import mjcf, models
from mujoco_inversedynamicstest_amd.sampler import sample_contact_states
from oracle.oracle import Oracle

# two hinges, each with a joint limit (the LIMIT model of tests/test_step_cpu.py with a second
# link): nv = 2, no gravity, so the rows come from the pose alone
TWO_HINGE_LIMIT = """
<mujoco>
  <compiler angle="radian"/>
  <option gravity="0 0 0"/>
  <worldbody>
    <body>
      <joint axis="0 1 0" limited="true" range="-0.05 0.05"/>
      <geom type="capsule" size=".01" fromto="0 0 0 .1 0 0"/>
      <body pos=".1 0 0">
        <joint axis="0 1 0" limited="true" range="-0.05 0.05"/>
        <geom type="capsule" size=".01" fromto="0 0 0 .1 0 0"/>
      </body>
    </body>
  </worldbody>
</mujoco>
"""

FWDINV_REFERENCE_BOUND = 1e-10               # engine_inverse_test.cc:50
FWDINV_FLOOR = 1e-12
FWDINV_FACTOR = 8


def two_hinge():
  return mjcf.load_xml_string(TWO_HINGE_LIMIT)


def two_hinge_states(n, seed=3):
  """About half of the states have no row: each joint is inside its range with probability
  0.7 (0.7^2 = 0.49), else beyond one end by up to 0.03; qvel ~ N(0, 0.5)."""
  rng = np.random.default_rng(seed)
  inside = rng.random((n, 2)) < 0.7
  q = np.where(inside, rng.uniform(-0.04, 0.04, (n, 2)),
               rng.choice([-1.0, 1.0], (n, 2)) * rng.uniform(0.051, 0.08, (n, 2)))
  return q, 0.5 * rng.normal(size=(n, 2))


def connect_model():
  return rp.load("connect_multiple_constraints")


def weld_model():
  return rp.load("weld_tfratio0_multiple_constraints")


def equality_states(m, n, seed=5):
  """Around qpos0: the equality rows are always there, and the friction-loss dof moves."""
  rng = np.random.default_rng(seed)
  q = np.tile(np.asarray(m.qpos0, dtype=np.float64), (n, 1))
  v = 0.3 * rng.normal(size=(n, m.nv))
  dq = 0.02 * rng.normal(size=(n, m.nv))
  q = np.array([rp.integrate_pos(m, q[i], dq[i]) for i in range(n)])
  return q, v


def humanoid():
  return models.load("humanoid")


def humanoid_states(m, n, first=0):
  q, v, _ = sample_contact_states(m, n, first=first)
  return q, v


def reference_model():
  return rms.model()


def reference_states(m, n, seed=0):
  q, v, _ = rms.states(m, n, seed=seed)
  return q, v


class OracleProblem:
  """The oracle's position and velocity stages at one state (or_forward: constraint-free
  qacc) and, from them, the restatement's Problem."""

  def __init__(self, m):
    self.m = m
    self.o = Oracle(m)

  def problem(self, qpos, qvel):
    o, m = self.o, self.m
    o.set_state(qpos, qvel)
    nefc = o.forward()
    e = o.efc
    f = lambda n: np.array(o.efc_field(n), dtype=np.float64).copy()
    return solver_ref.Problem(m, o.d.qM, o.d.qfrc_smooth, o.d.qacc_smooth, f("efc_J"),
                              f("efc_D"), f("efc_R"), f("efc_aref"), f("efc_frictionloss"),
                              e.ne if nefc else 0, e.nf if nefc else 0)

  def fwdinv(self, qpos, qvel, qacc, qfrc_constraint):
    """mj_compareFwdInv's two numbers for a forward solution: |qfrc_constraint(fwd) -
    qfrc_constraint(inv)| and |qfrc_applied + qfrc_actuator + J'xfrc_applied - qfrc_inverse|,
    with the oracle's mj_inverse on qacc."""
    o = self.o
    finv = o.inverse(qpos, qvel, qacc)
    qforce = o.d.qfrc_applied + o.d.qfrc_actuator
    o.xfrc_accumulate(qforce)
    return (float(np.linalg.norm(np.asarray(qfrc_constraint) - o.d.qfrc_constraint)),
            float(np.linalg.norm(qforce - finv)))


def fwdinv_bound(values, reference_model=False):
  """The identity's bound on a model: the reference's own 1e-10 on its own model; elsewhere
  FWDINV_FACTOR times the largest value the restatement reaches on the test's states, floored
  at FWDINV_FLOOR. Newton's terminal residual is round-off noise, not a smooth function of
  the inputs, so equality with the restatement's value is not to be expected of another
  libm or summation order; a small integer factor is."""
  if reference_model:
    return FWDINV_REFERENCE_BOUND
  return max(FWDINV_FACTOR * max(values), FWDINV_FLOOR)
