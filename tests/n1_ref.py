"""The N-1 screen's value rule restated in numpy float32 (include/gridpf.h gpf_set_n1_screen; grid2op_amd/csrc/gridpf_n1.hpp n1_value), the
bound a recorded value is held to, and the library's rule core on the host (tests/native/n1_emul.cpp).

The reference (Reward/n1Reward.py:64-101): is_done -> reward_min (BaseReward's 0.0); the copy's power flow did not converge -> -1; else
``th_lim[th_lim <= 1] = 1; (a_or / th_lim).max()`` in float32.  One correctly rounded division per line and an exact maximum: the
restatement, the emulator and the kernel agree bit for bit on the same float32 inputs.

The bound against a RECORDING is the project's float32 output tolerance of ``a_or`` (tests/test_gpu_parity.py: rtol 2e-5, atol 1e-3, the
engine's results against the float64 oracle) carried through the division, plus one float32 spacing of the value."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
A_OR_RTOL, A_OR_ATOL = 2e-5, 1e-3          # tests/test_gpu_parity.py, a_or
DONE, DIVERGED = np.float32(0.0), np.float32(-1.0)


def clamp_limits(thermal):
    th = np.array(thermal, np.float32)
    th[th <= 1] = 1
    return th


def value(a_or, thermal, done=False, converged=True) -> np.float32:
    """one contingency: float32"""
    if done:
        return DONE
    if not converged:
        return DIVERGED
    return np.float32((np.asarray(a_or, np.float32) / clamp_limits(thermal)).max())


def values(a_or_rows, thermal, done, converged) -> np.ndarray:
    """[K] from the K contingency rows of one environment"""
    return np.array([value(a, thermal, done, c) for a, c in zip(a_or_rows, converged)], np.float32)


def bound(a_or, thermal, v) -> float:
    """max_l tol(a_or_l) / max(th_l, 1) + one float32 spacing of the value"""
    a = np.abs(np.asarray(a_or, np.float64))
    return float(((A_OR_ATOL + A_OR_RTOL * a) / clamp_limits(thermal).astype(np.float64)).max() + np.spacing(np.float32(abs(v))))


def summary(vals):
    """(worst, arg_worst, n_insecure, n_diverged) of one environment's values: a diverged contingency outranks every value, then the larger
    value, then the lower index"""
    v = np.asarray(vals, np.float32)
    div = v == DIVERGED
    arg = int(np.flatnonzero(div)[0]) if div.any() else int(np.argmax(v))
    return np.float32(v[arg]), arg, int((div | (v > 1)).sum()), int(div.sum())


# ---- the library's rule core on the host (tests/native/n1_emul.cpp) ----
_BUILD = os.path.join(tempfile.gettempdir(), f"gridpf_n1_emul_{os.getuid()}")
SRC = os.path.join(HERE, "native", "n1_emul.cpp")
_emul = None


def _compile(out, flags):
    os.makedirs(_BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_n1.hpp"), os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_episode.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


def emul_lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(_compile(os.path.join(_BUILD, "libn1emul.so"), ["-O2", "-fPIC", "-shared"]))
        _emul.n1_emul_value.restype = C.c_float
        _emul.n1_emul_summary.restype = None
    return _emul


def sanitized_program():
    return _compile(os.path.join(_BUILD, "n1_emul_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DN1_EMUL_MAIN"])


def emul_value(a_or, thermal, done=False, converged=True) -> np.float32:
    a, th = np.ascontiguousarray(a_or, np.float32), np.ascontiguousarray(thermal, np.float32)
    return np.float32(emul_lib().n1_emul_value(int(bool(done)), int(bool(converged)), C.c_int(len(a)), a.ctypes.data_as(C.c_void_p), th.ctypes.data_as(C.c_void_p)))


def emul_summary(vals):
    v = np.ascontiguousarray(vals, np.float32)
    w, info = np.zeros(1, np.float32), np.zeros(3, np.int32)
    emul_lib().n1_emul_summary(C.c_int(len(v)), v.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p))
    return np.float32(w[0]), int(info[0]), int(info[1]), int(info[2])
