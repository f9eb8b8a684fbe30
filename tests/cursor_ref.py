"""The chronics cursor of the batched acting path (include/gridpf.h gpf_set_chronics_cursor) restated in numpy -- what
tests/test_cursor_cpu.py holds against the resets recorded from the unmodified reference (tests/golden/chronics_cursor_case14.npz) and what
the device is held to --, and the loader of the g++ host emulator of the library's rule (tests/native/cursor_emul.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from opponent_ref import philox4x32_10, philox_u

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEQUENTIAL, SAMPLED = 0, 1
TABLE, PHILOX = 0, 1
FLAG_DRAWS_EXHAUSTED, FLAG_NEXT_POS_WRAPPED = 1, 2
STATE_INTS = 7
PHILOX_STREAM = 0x63757273
COLS = ("table", "offset", "pos", "next_pos", "n_started", "draws_used", "flags")


def cdf_of(probabilities):
    """Multifolder.sample_next_chronics + RandomState.choice: float32 probabilities over their float32 sum, a float64 cumulative sum
    over its last entry"""
    p = np.array(probabilities, dtype=np.float32)
    p /= p.sum()
    cdf = p.astype(np.float64).cumsum()
    cdf /= cdf[-1]
    return cdf


def search(cdf, u):
    return int(min(np.searchsorted(cdf, u, side="right"), len(cdf) - 1))


def offset_of(row, t, T):
    """the lane_offset with which (t + offset) mod T is `row`, in [0, T)"""
    return int((int(row) - int(t)) % int(T))


class CursorRef:
    """every lane's cursor: arrays [n_lanes] named as COLS"""

    def __init__(self, n_lanes, order, T, policy=SEQUENTIAL, cdf=None, first_row=0, next_pos=None, draws=None, seed=None, lane_base=0):
        self.n, self.order, self.T, self.policy = int(n_lanes), [int(x) for x in order], int(T), int(policy)
        self.cdf = None if cdf is None else np.asarray(cdf, np.float64)
        self.first_row = np.broadcast_to(np.asarray(first_row, np.int64), (self.n,)).copy()
        if next_pos is None:
            next_pos = 0 if self.policy == SEQUENTIAL else -1
        self.next_pos = np.maximum(np.broadcast_to(np.asarray(next_pos, np.int64), (self.n,)), -1).copy()
        self.table, self.offset = np.zeros(self.n, np.int64), np.zeros(self.n, np.int64)
        self.pos = np.full(self.n, -1, np.int64)
        self.n_started, self.draws_used, self.flags = (np.zeros(self.n, np.int64) for _ in range(3))
        self.draws = None if draws is None else np.asarray(draws, np.float64).reshape(self.n, -1)
        self.seed, self.lane_base = seed, int(lane_base)

    def _draw(self, k):
        if self.seed is not None:
            x = philox4x32_10((int(self.n_started[k]), 0, k + self.lane_base, PHILOX_STREAM), (self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF))
            self.draws_used[k] += 1
            return philox_u(x[0], x[1])
        if self.draws is None or self.draws_used[k] >= self.draws.shape[1]:
            self.flags[k] |= FLAG_DRAWS_EXHAUSTED
            return None
        u = self.draws[k, self.draws_used[k]]
        self.draws_used[k] += 1
        return float(u)

    def pick(self, k):
        n, p = len(self.order), int(self.next_pos[k])
        if p >= n:
            p %= n
            self.flags[k] |= FLAG_NEXT_POS_WRAPPED
        if self.policy == SEQUENTIAL:
            if p < 0:
                p = max(int(self.pos[k]) + 1, 0) % n
            self.next_pos[k] = (p + 1) % n
            return p
        self.next_pos[k] = -1
        if p >= 0:
            return p
        u = self._draw(k)
        if u is None:
            return max(int(self.pos[k]), 0) % n
        return search(self.cdf, u)

    def start(self, k, t):
        """lane k starts an episode in the launch at time index t"""
        p = self.pick(k)
        self.table[k], self.offset[k], self.pos[k] = self.order[p], offset_of(self.first_row[k], t, self.T), p
        self.n_started[k] += 1

    def prestep(self, t, steps_survived, skip=None):
        """the kernel: every lane whose episode[lane][0] is 0 before the step, and that is no scratch lane, starts an episode"""
        for k in range(self.n):
            if steps_survived[k] == 0 and not (skip is not None and skip[k]):
                self.start(k, t)

    def rows(self):
        return np.stack([getattr(self, c) for c in COLS], axis=1).astype(np.int32)


# ---- the library's rule compiled with g++ (tests/native/cursor_emul.cpp) ----
_BUILD = os.path.join(tempfile.gettempdir(), f"gridpf_cursor_emul_{os.getuid()}")
SRC = os.path.join(HERE, "native", "cursor_emul.cpp")
_emul = None


def _compile(out, flags):
    os.makedirs(_BUILD, exist_ok=True)
    csrc = os.path.join(ROOT, "grid2op_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in ("gridpf_cursor.hpp", "gridpf_opponent.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


def emul_lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(_compile(os.path.join(_BUILD, "libcursoremul.so"), ["-O2", "-fPIC", "-shared"]))
        _emul.cursor_emul_start.restype = None
        _emul.cursor_emul_philox_u.restype = C.c_double
        assert _emul.cursor_emul_state_ints() == STATE_INTS
    return _emul


def sanitized_program():
    return _compile(os.path.join(_BUILD, "cursor_emul_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCURSOR_EMUL_MAIN"])


def emul_philox_u(n_started, global_lane, seed):
    return float(emul_lib().cursor_emul_philox_u(C.c_uint32(n_started), C.c_uint32(global_lane), C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32((seed >> 32) & 0xFFFFFFFF)))


class CursorEmul:
    """the same lanes through the library's cursor_start, one call per episode start; state rows int32 [n_lanes][STATE_INTS]"""

    def __init__(self, n_lanes, order, T, policy=SEQUENTIAL, cdf=None, first_row=0, next_pos=None, draws=None, seed=None, lane_base=0):
        ref = CursorRef(n_lanes, order, T, policy, cdf, first_row, next_pos, draws, seed, lane_base)
        self.n, self.T, self.policy, self.lane_base, self.seed = ref.n, ref.T, ref.policy, ref.lane_base, seed
        self.order = np.ascontiguousarray(order, np.int32)
        self.cdf = None if cdf is None else np.ascontiguousarray(cdf, np.float64)
        self.first_row = ref.first_row.astype(np.int32)
        self.state = np.ascontiguousarray(ref.rows())
        self.draws = None if draws is None else np.ascontiguousarray(np.asarray(draws, np.float64).reshape(self.n, -1))

    def start(self, k, t):
        seed = 0 if self.seed is None else self.seed
        dr = None if self.draws is None else self.draws[k]
        emul_lib().cursor_emul_start(
            C.c_int(len(self.order)), self.order.ctypes.data_as(C.c_void_p), C.c_int(self.policy),
            None if self.cdf is None else self.cdf.ctypes.data_as(C.c_void_p), C.c_int(TABLE if self.seed is None else PHILOX),
            C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32((seed >> 32) & 0xFFFFFFFF), C.c_int(self.lane_base),
            C.c_int(0 if dr is None else len(dr)), None if dr is None else dr.ctypes.data_as(C.c_void_p), C.c_int(self.T),
            C.c_int(int(self.first_row[k])), C.c_int(k), C.c_int(int(t)), self.state[k].ctypes.data_as(C.c_void_p))

    def prestep(self, t, steps_survived, skip=None):
        for k in range(self.n):
            if steps_survived[k] == 0 and not (skip is not None and skip[k]):
                self.start(k, t)

    def rows(self):
        return self.state.copy()
