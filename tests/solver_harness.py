"""Build/load the test-only host compilation of the device mj_forward with the Newton
constraint solver (solver_harness.cpp over csrc/solver.h)."""
import ctypes
import os
import subprocess

import numpy as np

from kernel_harness import BUILD, HERE, KernelCPU

SO = os.path.join(BUILD, "libsolver_cpu.so")
CSRC = os.path.join(HERE, "..", "mujoco_inversedynamicstest_amd", "csrc")
SRC = [os.path.join(HERE, "solver_harness.cpp"), os.path.join(HERE, "cpu_kernel_harness.cpp"),
       os.path.join(CSRC, "solver.h"), os.path.join(CSRC, "engine_device.h"),
       os.path.join(CSRC, "pair_program.h"),
       os.path.join(HERE, "..", "include", "mjhip.h"),
       os.path.join(HERE, "..", "include", "mjhip_fields.h"),
       os.path.join(HERE, "..", "include", "mjhip_contact.h")]
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off"]

_lib = None
_D = ctypes.POINTER(ctypes.c_double)


class SoOpt(ctypes.Structure):
  _fields_ = [("iterations", ctypes.c_int), ("ls_iterations", ctypes.c_int),
              ("tolerance", ctypes.c_double), ("ls_tolerance", ctypes.c_double),
              ("meaninertia", ctypes.c_double)]


class SoOut(ctypes.Structure):
  _fields_ = [("cost", ctypes.c_double), ("niter", ctypes.c_int), ("nalpha", ctypes.c_int),
              ("nupdate", ctypes.c_int), ("ndowndate", ctypes.c_int),
              ("nrefactor", ctypes.c_int), ("warm", ctypes.c_int)]


def lib():
  global _lib
  if _lib is None:
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in SRC):
      # -ffp-contract=off: the rounding of the oracle's scalar C build and of kern_solver.hip
      tmp = f"{SO}.{os.getpid()}"
      subprocess.run(["g++", *FLAGS, "-fPIC", "-shared", "-o", tmp, SRC[0]], check=True)
      os.replace(tmp, SO)
    L = ctypes.CDLL(SO)
    L.so_scratchDoubles.restype = ctypes.c_long
    L.so_scratchDoubles.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.so_warmstartOffset.restype = ctypes.c_int
    L.so_warmstartOffset.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.so_forward.restype = ctypes.c_int
    L.so_forward.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_int, ctypes.c_int, _D, _D, ctypes.c_void_p, _D,
                             ctypes.c_int, ctypes.c_void_p]
    _lib = L
  return _lib


def solver_options(m, **over):
  """The call's options as InverseEngine.forward_solve fills them (engine.solve_options)."""
  from mujoco_inversedynamicstest_amd import engine
  sin = engine.solve_options(m, **over)
  return {k: getattr(sin, k) for k in ("iterations", "ls_iterations", "tolerance",
                                       "ls_tolerance", "meaninertia")}


class SolverCPU(KernelCPU):
  """One instance of the device mj_forward with the solver on the host. The state and the
  applied forces live in self.d; the kept warmstart in self.solver_scratch."""

  ALPHA_CAP = 256

  def __init__(self, m, efc_cap=None, con_cap=None):
    super().__init__(m, efc_cap, con_cap)
    n = lib().so_scratchDoubles(ctypes.byref(self.cm), self.efc_cap)
    self.solver_scratch = np.zeros(n + 1)
    self._woff = lib().so_warmstartOffset(ctypes.byref(self.cm), self.efc_cap)
    self.act3 = np.zeros(3 * max(m.na, 1))

  @property
  def qacc_warmstart(self):
    return self.solver_scratch[self._woff:self._woff + self.m.nv]

  def forward_solve(self, qpos, qvel, qacc_warmstart=None, **over):
    """mj_forward at (qpos, qvel). qacc_warmstart None: the kept one. Returns a dict: qacc,
    qfrc_constraint, efc_force, efc_state, niter, cost, alpha (per iteration), status, and
    the trace counters."""
    m = self.m
    self.d.qpos[:] = qpos
    self.d.qvel[:] = qvel
    if qacc_warmstart is not None:
      self.qacc_warmstart[:] = qacc_warmstart
    o = SoOpt(**solver_options(m, **over))
    out = SoOut()
    alpha = np.zeros(self.ALPHA_CAP)
    st = lib().so_forward(ctypes.byref(self.cm), ctypes.byref(self.d.struct),
                          self.scratch.ctypes.data, self.iscratch.ctypes.data, self.efc_cap,
                          self.con_cap, self.solver_scratch.ctypes.data_as(_D),
                          self.act3.ctypes.data_as(_D), ctypes.byref(o),
                          alpha.ctypes.data_as(_D), self.ALPHA_CAP, ctypes.byref(out))
    nefc = int(self.field("efc_count")[0])
    return dict(qacc=self.d.qacc.copy(), qfrc_constraint=self.d.qfrc_constraint.copy(),
                qacc_smooth=self.d.qacc_smooth.copy(),
                efc_force=self.field("efc_force")[:nefc].copy(),
                efc_state=self.field("efc_state")[:nefc].copy(),
                jar=None, nefc=nefc, niter=out.niter, cost=out.cost,
                alpha=alpha[:out.nalpha].copy(), status=st, nupdate=out.nupdate,
                ndowndate=out.ndowndate, nrefactor=out.nrefactor, warm=out.warm)
