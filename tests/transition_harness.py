"""Build/load the test-only host compilation of the device mjd_transitionFD
(transition_harness.cpp): the lane functions of csrc/transition.h in the kernels' order."""
import ctypes
import os
import subprocess

import numpy as np

from kernel_harness import BUILD, HERE, KernelCPU

SO = os.path.join(BUILD, "libtransition_cpu.so")
CSRC = os.path.join(HERE, "..", "mujoco_inversedynamicstest_amd", "csrc")
SRC = [os.path.join(HERE, "transition_harness.cpp"), os.path.join(HERE, "cpu_kernel_harness.cpp"),
       os.path.join(CSRC, "transition.h"), os.path.join(CSRC, "step.h"),
       os.path.join(CSRC, "engine_device.h"), os.path.join(CSRC, "pair_program.h"),
       os.path.join(HERE, "..", "include", "mjhip.h"),
       os.path.join(HERE, "..", "include", "mjhip_fields.h"),
       os.path.join(HERE, "..", "include", "mjhip_contact.h")]
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off"]

_lib = None
_D = ctypes.POINTER(ctypes.c_double)


class ThSlot(ctypes.Structure):
  _fields_ = [("d", ctypes.c_void_p), ("scratch", ctypes.c_void_p),
              ("iscratch", ctypes.c_void_p), ("step_scratch", ctypes.c_void_p)]


def lib():
  global _lib
  if _lib is None:
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in SRC):
      # -ffp-contract=off: the rounding of the oracle's scalar C build and of
      # kern_transition.hip
      tmp = f"{SO}.{os.getpid()}"
      subprocess.run(["g++", *FLAGS, "-fPIC", "-shared", "-o", tmp, SRC[0]], check=True)
      os.replace(tmp, SO)
    L = ctypes.CDLL(SO)
    L.th_scratchDoubles.restype = ctypes.c_long
    L.th_scratchDoubles.argtypes = [ctypes.c_void_p]
    L.th_slots.restype = ctypes.c_int
    L.th_slots.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.th_transition.restype = ctypes.c_int
    L.th_transition.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                ctypes.c_int, _D, _D, _D, _D, _D, _D, ctypes.c_double,
                                ctypes.c_int, ctypes.c_int, _D, _D, _D,
                                ctypes.POINTER(ctypes.c_int)]
    _lib = L
  return _lib


def _p(a):
  return None if a is None else a.ctypes.data_as(_D)


def _vec(a, n):
  if a is None or n == 0:
    return None
  return np.ascontiguousarray(a, dtype=np.float64).reshape(n)


class _Slot(KernelCPU):
  """One data slot: mjhipData, the pipeline's scratch and the integrators' scratch."""

  def __init__(self, m):
    super().__init__(m)
    self.step_scratch = np.zeros(max(lib().th_scratchDoubles(ctypes.byref(self.cm)), 1) + 1)
    self.c = ThSlot(ctypes.addressof(self.d.struct), self.scratch.ctypes.data,
                    self.iscratch.ctypes.data, self.step_scratch.ctypes.data)

  def snapshot(self):
    """Every byte of the slot: the data fields, the rows and both scratch buffers."""
    arrs = list(self.d._arrays.values()) + list(self.d._rows.values()) + \
        list(self.d._sparse.values()) + [self.scratch, self.iscratch, self.step_scratch]
    return [a.copy() for a in arrs]


class TransitionCPU:
  """mjd_transitionFD of the device path on the host for one base state at a time, with a
  centre slot and an evaluation slot as the kernels have."""

  def __init__(self, m):
    self.m = m
    self.centre, self.eval = _Slot(m), _Slot(m)

  def slots(self, want_A=True, want_B=True, centered=False):
    return lib().th_slots(ctypes.byref(self.centre.cm), int(want_A), int(want_B), int(centered))

  def transition_fd(self, qpos, qvel, ctrl=None, act=None, eps=1e-6, centered=False,
                    qfrc_applied=None, xfrc_applied=None, want_A=True, want_B=True, between=None):
    """(A, B, status, rc); rc is th_transition's return (MJHIP_ERR_MODEL for RK4). between():
    called after the centre's evaluation and before the perturbed ones."""
    m = self.m
    ndx, nstate = 2*m.nv + m.na, m.nq + m.nv + m.na
    A = np.zeros((ndx, ndx)) if want_A else None
    B = np.zeros((ndx, m.nu)) if want_B and m.nu else None
    P = self.slots(want_A, want_B, centered)
    Y = np.zeros((1 + P, nstate))
    st = ctypes.c_int(0)
    args = lambda phase: (ctypes.byref(self.centre.cm), ctypes.byref(self.centre.c),
                          ctypes.byref(self.eval.c), self.centre.efc_cap, self.centre.con_cap,
                          _p(_vec(qpos, m.nq)), _p(_vec(qvel, m.nv)), _p(_vec(act, m.na)),
                          _p(_vec(ctrl, m.nu)), _p(_vec(qfrc_applied, m.nv)),
                          _p(_vec(xfrc_applied, 6*m.nbody)), float(eps), int(centered), phase,
                          _p(Y), _p(A), _p(B), ctypes.byref(st))
    rc = lib().th_transition(*args(1))
    if rc == 0:
      if between is not None:
        between()
      rc = lib().th_transition(*args(2))
    self.Y = Y
    return A, B, st.value, rc
