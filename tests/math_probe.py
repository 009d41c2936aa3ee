"""Builds and loads tests/native/math_probe.hip: one launcher per primitive of csrc/ta_math.h, ta_dual.h and
ta_reduce.h (tests/test_gpu_math.py). The probe is compiled with the library's own flags, so the device code
under test is the code the product kernels inline."""
import ctypes as C
import os
import subprocess

import numpy as np

from tensoralloy_amd import _lib

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "math_probe.hip")
OBJECT = os.path.join(os.path.dirname(SOURCE), "libmath_probe.so")

# launcher: (leading int argument?, input rows, output rows)
LAUNCHERS = {
    "mp_exp": (False, 1, 1), "mp_cutoff": (True, 1, 6), "mp_softplus": (False, 1, 2),
    "mp_rcp_1_3": (False, 1, 1), "mp_activation": (True, 1, 5), "mp_pow_int_m1": (False, 2, 1),
    "mp_safe_pow": (True, 2, 2), "mp_dual_ops": (False, 5, 2), "mp_term_index": (False, 3, 2),
    "mp_lane_sums": (False, 1, 4),
}

# opcodes of mp_dual_ops (DualOp in the probe); + PLAIN: the same expression on plain doubles
DUAL_OPS = {"neg": 0, "add_dd": 1, "add_ds": 2, "add_sd": 3, "sub_dd": 4, "sub_ds": 5, "sub_sd": 6,
            "mul_dd": 7, "mul_ds": 8, "mul_sd": 9, "div_dd": 10, "div_ds": 11, "div_sd": 12, "iadd": 13,
            "t_val": 14, "t_exp": 15, "t_exp_libm": 16, "t_log": 17, "t_sqrt": 18, "t_pow_dd": 19,
            "t_pow_ds": 20, "t_pow_sd": 21, "t_floor_at": 22}
PLAIN = 256


def dependencies():
    return [SOURCE, str(_lib.INCLUDE_DIR / "tensoralloy_amd.h")] + sorted(str(p) for p in _lib.CSRC_DIR.glob("*.h"))


def compile_command(out=OBJECT):
    return [_lib.hipcc_path()] + _lib._compile_flags() + ["-shared", SOURCE, "-o", out]


def build(force=False):
    """Compile the probe for gfx950 (needs hipcc, no GPU) unless the object is newer than its sources."""
    if not force and os.path.exists(OBJECT) and \
            os.path.getmtime(OBJECT) >= max(os.path.getmtime(p) for p in dependencies()):
        return OBJECT
    tmp = OBJECT + f".tmp{os.getpid()}"
    done = subprocess.run(compile_command(tmp), capture_output=True, text=True)
    if done.returncode != 0:
        raise RuntimeError("math probe did not compile:\n" + done.stderr[-4000:])
    os.replace(tmp, OBJECT)
    return OBJECT


_probe = None


def load():
    global _probe
    if _probe is None:
        lib = C.CDLL(build())
        ptr = C.POINTER(C.c_double)
        for name, (lead, _, _) in LAUNCHERS.items():
            fn = getattr(lib, name)
            fn.restype = C.c_int
            fn.argtypes = ([C.c_int] if lead else []) + [ptr, ptr, C.c_int64]
        _probe = lib
    return _probe


def call(name, *rows, arg=None):
    """Run launcher `name` on equally long input rows; returns the array [output rows, n]."""
    lead, n_in, n_out = LAUNCHERS[name]
    assert len(rows) == n_in and (arg is not None) == lead, name
    x = np.ascontiguousarray(np.broadcast_arrays(*[np.asarray(r, dtype=np.float64) for r in rows]))
    n = x.shape[1]
    out = np.zeros((n_out, n))
    ptr = C.POINTER(C.c_double)
    args = ([int(arg)] if lead else []) + [x.ctypes.data_as(ptr), out.ctypes.data_as(ptr), n]
    status = getattr(load(), name)(*args)
    if status != _lib.TA_OK:
        raise RuntimeError(f"{name} returned {status}")
    return out
