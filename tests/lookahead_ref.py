"""The look-ahead screen's rules restated in numpy (include/gridpf.h gpf_set_lookahead; grid2op_amd/csrc/gridpf_lookahead.hpp) and the
library's rule core on the host (tests/native/lookahead_emul.cpp).

  value       the maximum of the scratch lane's float32 rho row, +inf when the simulated step ended the episode (exact: a maximum)
  flags       LA_ILLEGAL / LA_AMBIGUOUS: the verdict of steps 1-3 of the acting path (tests/topo_rules_ref.TopoRules.pre) on the
              environment's row with the maintenance ahead taken out first; LA_DONE: the done flag
  ranking     the playable slot (no flag) with the lowest value, the lowest slot on a tie; none: -1 and +inf
  maintenance _ObsEnv.init (Environment/_obsEnv.py:361-385): the forecast `time_step` rows ahead has a line out when the first flagged
              row of its maintenance column from the observation's row on is <= row + time_step and every row from there to row +
              time_step is flagged
Test helper only: the engine never imports it."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

ILLEGAL, AMBIGUOUS, DONE = 1, 2, 4
RHO_TOL = 3e-5                 # tests/test_gpu_simulate.py: the step kernel's rho against a recording of obs.simulate
MARGIN = 6e-5                  # twice that: a recorded best whose runner-up is further away is the device's best too


def value(rho_row, done) -> np.float32:
    return np.float32(np.inf) if done else np.float32(np.asarray(rho_row, np.float32).max())


def summary(values, flags):
    """(best, best_value, n_playable, n_done) of one environment"""
    v, f = np.asarray(values, np.float32), np.asarray(flags, np.uint8)
    ok = np.flatnonzero(f == 0)
    n_done = int(((f & DONE) != 0).sum())
    if not len(ok):
        return -1, np.float32(np.inf), 0, n_done
    best = int(ok[np.lexsort((ok, v[ok]))][0])
    return best, np.float32(v[best]), len(ok), n_done


def margin(values, flags) -> float:
    """distance between the best playable value and the runner-up (inf: fewer than two playable slots)"""
    v = np.sort(np.asarray(values, np.float64)[np.asarray(flags) == 0])
    return float(v[1] - v[0]) if len(v) > 1 else float("inf")


def maintenance_ahead(M, idx, time_step) -> np.ndarray:
    """bool [n_line] from one maintenance table M [T, n_line]"""
    M = np.asarray(M) != 0
    T, L = M.shape
    out = np.zeros(L, bool)
    tgt = idx + time_step
    if time_step < 1 or tgt >= T:
        return out
    for l in range(L):
        hit = np.flatnonzero(M[idx:tgt + 1, l])
        out[l] = len(hit) > 0 and M[idx + hit[0]:tgt + 1, l].all()
    return out


def verdicts(rules, topo, line_cd, sub_cd, last_bus, cands, out_lines=None):
    """(flags & 3 [K], rows [K, dim_topo]) of one environment: `out_lines` (bool [n_line], the maintenance ahead) go out first"""
    row = np.array(topo, np.int64)
    if out_lines is not None and np.any(out_lines):
        row[rules.lo[out_lines]] = -1
        row[rules.le[out_lines]] = -1
    flags, rows = [], []
    for a in cands:
        new, ill, amb, _, _ = rules.pre(row, line_cd, sub_cd, last_bus, int(a))
        flags.append((ILLEGAL if ill else 0) | (AMBIGUOUS if amb else 0))
        rows.append(new)
    return np.array(flags, np.uint8), np.array(rows)


# ---- the library's rule core on the host (tests/native/lookahead_emul.cpp) ----
_SRC = os.path.join(ROOT, "tests", "native", "lookahead_emul.cpp")
_HDR = os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_lookahead.hpp")
_BUILD = os.path.join(ROOT, "tests", "native", "_build")
_lib = None


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in (_SRC, _HDR))


def emulator():
    global _lib
    so = os.path.join(_BUILD, "liblookaheademul.so")
    if _lib is None or _stale(so):
        if _stale(so):
            os.makedirs(_BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", _SRC, "-o", so + ".tmp"])
            os.replace(so + ".tmp", so)
        _lib = C.CDLL(so)
        _lib.la_emul_value.restype = C.c_float
        _lib.la_emul_summary.restype = None
        _lib.la_emul_maintenance.restype = None
        _lib.la_emul_outranks.argtypes = [C.c_float, C.c_int, C.c_float, C.c_int]
    return _lib


def sanitized_program():
    """the same file with its own main, built with the address and undefined-behaviour sanitizers: a stand-alone program"""
    exe = os.path.join(_BUILD, "lookahead_emul_san")
    if _stale(exe):
        os.makedirs(_BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLA_EMUL_MAIN", _SRC, "-o", exe])
    return exe


def emul_value(rho_row, done) -> np.float32:
    r = np.ascontiguousarray(rho_row, np.float32)
    return np.float32(emulator().la_emul_value(int(bool(done)), C.c_int(len(r)), r.ctypes.data_as(C.c_void_p)))


def emul_summary(values, flags):
    v, f = np.ascontiguousarray(values, np.float32), np.ascontiguousarray(flags, np.uint8)
    bv, info = np.zeros(1, np.float32), np.zeros(3, np.int32)
    emulator().la_emul_summary(C.c_int(len(v)), v.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), bv.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p))
    return int(info[0]), np.float32(bv[0]), int(info[1]), int(info[2])


def emul_maintenance(M, idx, time_step) -> np.ndarray:
    M = np.ascontiguousarray(M, np.uint8)
    out = np.zeros(M.shape[1], np.uint8)
    emulator().la_emul_maintenance(M.ctypes.data_as(C.c_void_p), C.c_int(M.shape[0]), C.c_int(M.shape[1]), C.c_int(idx), C.c_int(time_step), out.ctypes.data_as(C.c_void_p))
    return out.astype(bool)
