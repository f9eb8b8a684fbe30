"""The look-ahead chain's rules restated in numpy (include/gridpf.h gpf_set_lookahead_chain; grid2op_amd/csrc/gridpf_lookahead.hpp) and the
library's rule functions on the host (tests/native/lookahead_chain_emul.cpp).

  per lane    steps h = 1 .. H in order; the first step whose done flag is set is the failure: survived = the steps before it, value_h =
              the float32 rho row's maximum up to there and +inf from there on, peak = the maximum over the survived steps (-inf: none),
              value = the maximum of value_h; whatever later steps of a failed lane leave is ignored
  fall-back   among the slots that are neither illegal nor ambiguous: most survived steps, then the lowest peak, then the lowest slot
  pick        play 1: best, else -1; play 2: best, else fall-back, else -1
  row         forecast row of step h of the observation at row idx: n_h idx + (h - 1)
Test helper only: the engine never imports it."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from lookahead_ref import AMBIGUOUS, DONE, ILLEGAL, MARGIN, RHO_TOL, summary  # noqa: F401  (one statement of the look-ahead's own rules)


def lane(rho, done):
    """rho [H, n_line] float32, done [H] -> dict(survived, peak, value, value_h [H], failed)"""
    rho, done = np.asarray(rho, np.float32), np.asarray(done).astype(bool)
    H = len(done)
    first = int(np.flatnonzero(done)[0]) if done.any() else H        # steps survived
    value_h = np.full(H, np.inf, np.float32)
    value_h[:first] = rho[:first].max(axis=1) if first else []
    peak = np.float32(value_h[:first].max()) if first else np.float32(-np.inf)
    return dict(survived=first, peak=peak, value=np.float32(value_h.max()), value_h=value_h, failed=first < H)


def fallback(survived, peak, flags):
    """(slot, steps) of one environment"""
    sv, pk, f = np.asarray(survived), np.asarray(peak, np.float32), np.asarray(flags, np.uint8)
    ok = np.flatnonzero((f & (ILLEGAL | AMBIGUOUS)) == 0)
    if not len(ok):
        return -1, 0
    k = int(ok[np.lexsort((ok, pk[ok], -sv[ok]))][0])
    return k, int(sv[k])


def fallback_margin(survived, peak, flags) -> float:
    """distance in peak between the fall-back and the runner-up with as many survived steps (inf: none)"""
    k, steps = fallback(survived, peak, flags)
    if k < 0 or steps == 0:                 # (no step survived: every peak is -inf and the slot index decides)
        return float("inf")
    f = np.asarray(flags, np.uint8)
    same = [j for j in range(len(f)) if j != k and (f[j] & 3) == 0 and survived[j] == steps]
    return float(min((abs(float(peak[j]) - float(peak[k])) for j in same), default=np.inf))


def pick(play, best, fb):
    return best if best >= 0 else (fb if play == 2 else -1)


def chain_flags(flags1, failed):
    """the chain's flags: step 1's illegal / ambiguous bits, LA_DONE when the lane failed anywhere"""
    return ((np.asarray(flags1, np.uint8) & 3) | np.where(failed, DONE, 0)).astype(np.uint8)


# ---- the library's rule functions on the host (tests/native/lookahead_chain_emul.cpp) ----
_SRC = os.path.join(ROOT, "tests", "native", "lookahead_chain_emul.cpp")
_HDR = os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_lookahead.hpp")
_BUILD = os.path.join(ROOT, "tests", "native", "_build")
_lib = None


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in (_SRC, _HDR))


def emulator():
    global _lib
    so = os.path.join(_BUILD, "liblookaheadchainemul.so")
    if _lib is None or _stale(so):
        if _stale(so):
            os.makedirs(_BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", _SRC, "-o", so + ".tmp"])
            os.replace(so + ".tmp", so)
        _lib = C.CDLL(so)
        _lib.la_chain_emul_lane.restype = None
        _lib.la_chain_emul_fallback.restype = None
        _lib.la_chain_emul_outranks.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int]
        _lib.la_chain_emul_pick.argtypes = [C.c_int, C.c_int, C.c_int]
        _lib.la_chain_emul_row.argtypes = [C.c_int, C.c_int, C.c_int]
    return _lib


def sanitized_program():
    """the same file with its own main, built with the address and undefined-behaviour sanitizers: a stand-alone program"""
    exe = os.path.join(_BUILD, "lookahead_chain_emul_san")
    if _stale(exe):
        os.makedirs(_BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLA_CHAIN_EMUL_MAIN", _SRC, "-o", exe])
    return exe


def emul_lane(rho, done):
    rho, done = np.ascontiguousarray(rho, np.float32), np.ascontiguousarray(done, np.uint8)
    H, L = rho.shape
    vh, f, i = np.zeros(H, np.float32), np.zeros(2, np.float32), np.zeros(2, np.int32)
    emulator().la_chain_emul_lane(C.c_int(H), C.c_int(L), rho.ctypes.data_as(C.c_void_p), done.ctypes.data_as(C.c_void_p), vh.ctypes.data_as(C.c_void_p),
                                  f.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p))
    return dict(survived=int(i[0]), peak=np.float32(f[1]), value=np.float32(f[0]), value_h=vh, failed=bool(i[1]))


def emul_fallback(survived, peak, flags):
    sv, pk, f = np.ascontiguousarray(survived, np.int32), np.ascontiguousarray(peak, np.float32), np.ascontiguousarray(flags, np.uint8)
    out = np.zeros(2, np.int32)
    emulator().la_chain_emul_fallback(C.c_int(len(sv)), sv.ctypes.data_as(C.c_void_p), pk.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return int(out[0]), int(out[1])


def same_lane(a, b):
    return (a["survived"], a["failed"], a["peak"].tobytes(), a["value"].tobytes(), a["value_h"].tobytes()) == \
           (b["survived"], b["failed"], b["peak"].tobytes(), b["value"].tobytes(), b["value_h"].tobytes())
