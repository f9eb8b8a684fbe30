"""Python restatement of the multi-area opponent of the batched acting path (include/gridpf.h gpf_set_opponent_areas), test
infrastructure: the reference's GeometricOpponentMultiArea.attack / reset (Opponent/geometricOpponentMultiArea.py:88-149) over one
GeometricOpponent per area (the `OpponentRef` of tests/opponent_ref.py, fed by the lane's ONE stream of draws) under OpponentSpace.attack
(Opponent/opponentSpace.py:177-249) with BaseActionBudget (one unit per attacked line).  Also the loader of the g++ host emulator of the
library's rule core (tests/native/opponent_area_emul.cpp)."""
import ctypes as C
import os

import numpy as np

import opponent_ref as R
from opponent_ref import FLAG_DRAWS_EXHAUSTED, FLAG_SCHEDULE_CAPPED, GEOMETRIC, PHILOX, TABLE, TIME_NONE  # noqa: F401

AREA_STATE_INTS = 8
MAX_AREAS = 16
# columns of an area row / of the lane row
A_COUNTER, A_LINE, A_NEXT_TIME, A_ATTACK_COUNTER, A_N_SCHED, A_INFO_LINE = range(6)


def split_areas(lines, area_of_line):
    """the areas' line lists: an area's entries of the descriptor's list, in descriptor order"""
    lines, area_of_line = np.asarray(lines), np.asarray(area_of_line)
    return [lines[area_of_line == a] for a in range(int(area_of_line.max()) + 1)]


class _Sub(R.OpponentRef):
    """one area's GeometricOpponent: draws come from the lane's stream, flags go to the lane"""

    def __init__(self, owner, lines, **kw):
        super().__init__(GEOMETRIC, lines, **kw)
        self.owner = owner

    def draw(self):
        return self.owner.draw()

    def sample_schedule(self):
        super().sample_schedule()
        self.owner.flags |= self.flags
        self.flags = 0


class OpponentAreaRef(R.OpponentRef):
    """One lane's OpponentSpace + GeometricOpponentMultiArea.  ``prestep`` is one launch: returns (sorted list of attacked lines,
    opponent_attack_duration)."""

    def __init__(self, lines, area_of_line, schedules=None, **kw):
        super().__init__(GEOMETRIC, lines, **kw)
        sub_kw = {k: v for k, v in kw.items() if k not in ("draws", "schedule", "global_lane", "seed", "draw_source")}
        self.areas = [_Sub(self, ls, **sub_kw) for ls in split_areas(lines, area_of_line)]
        for a, sub in enumerate(self.areas):
            if schedules is not None:
                sub.waits, sub.durs = [int(w) for w, _ in schedules[a]], [int(d) for _, d in schedules[a]]
        self.counters = [-1] * len(self.areas)
        self.previous = [-1] * len(self.areas)       # _previous_attacks: the line, -1 for None
        self.info_lines = [-1] * len(self.areas)

    def reset(self):
        """OpponentSpace.reset + GeometricOpponentMultiArea.reset: _previous_attacks stays"""
        self.budget = self.init_budget
        self.previous_fails, self.duration, self.cooldown, self.line = False, 0, self.attack_cooldown, -1
        self.episode += 1
        self.info_line, self.info_duration = -1, 0
        if self.source == PHILOX:
            self.cursor = 0
        self.counters = [-1] * len(self.areas)
        self.info_lines = [-1] * len(self.areas)
        for sub in self.areas:
            sub.next_time, sub.counter = None, 0
            if self.source == PHILOX:
                sub.sample_schedule()

    def _attack(self, rho, status_all):
        """GeometricOpponentMultiArea.attack: the union (list of lines), duration 1"""
        self.counters = [max(c - 1, -1) for c in self.counters]
        union = []
        for a, sub in enumerate(self.areas):
            if self.counters[a] == -1:
                sub.previous_fails = self.previous_fails
                line, dur = sub._attack(rho, status_all)
                self.margin = min(self.margin, sub.margin)
                if line >= 0:
                    self.counters[a], self.previous[a] = int(dur), line
                    union.append(line)
                else:
                    self.previous[a] = -1
            else:
                sub.next_time = None                   # tell_attack_continues
                if self.previous[a] >= 0:
                    union.append(self.previous[a])
        return union, 1

    def prestep(self, steps_survived, done, rho, line_status):
        if steps_survived == 0:
            self.reset()
            return [], 0
        if done:
            return sorted(l for l in self.info_lines if l >= 0), self.info_duration
        self.budget = self.budget + self.budget_per_ts
        self.duration, self.cooldown = max(0, self.duration - 1), max(0, self.cooldown - 1)
        union = []
        if self.duration == 0 and self.cooldown <= self.attack_cooldown:
            union, duration = self._attack(np.asarray(rho), np.asarray(line_status))
            self.previous_fails = False
            if duration > self.attack_max_duration:
                union, self.previous_fails = [], True
            cost = np.int64(len(union)) if union else 0            # compute_budget(None) is the int 0
            if duration * cost > self.budget:
                union, self.previous_fails = [], True
            if union:
                self.duration = int(duration)
                self.cooldown += self.attack_cooldown
        else:                                          # (the reference raises here: "I should not get there !")
            self.previous_fails = False
        if union:
            self.budget = self.budget - np.int64(len(union))        # numpy widens float32 - int64 to float64
        self.info_lines = [p if union else -1 for p in self.previous]
        first = next((l for l in self.info_lines if l >= 0), -1)
        self.line = self.info_line = first
        self.info_duration = self.duration if union else 0
        return sorted(union), self.info_duration

    def row(self):
        return [int(np.asarray(self.budget).dtype == np.float32), self.duration, self.cooldown, self.line, int(self.previous_fails),
                TIME_NONE, 0, 0, self.cursor, self.episode, self.flags, self.info_line, self.info_duration, 0]

    def area_rows(self):
        return [[self.counters[a], self.previous[a], TIME_NONE if s.next_time is None else s.next_time, s.counter, len(s.waits), self.info_lines[a], 0, 0]
                for a, s in enumerate(self.areas)]

    def set_rows(self, budget, row, area_rows, schedules=None):
        self.set_row(budget, row)
        for a, (r, s) in enumerate(zip(area_rows, self.areas)):
            self.counters[a], self.previous[a], self.info_lines[a] = int(r[A_COUNTER]), int(r[A_LINE]), int(r[A_INFO_LINE])
            s.next_time = None if r[A_NEXT_TIME] == TIME_NONE else int(r[A_NEXT_TIME])
            s.counter = int(r[A_ATTACK_COUNTER])
            if schedules is not None:
                n = int(r[A_N_SCHED])
                s.waits, s.durs = [int(x) for x in schedules[a][:n, 0]], [int(x) for x in schedules[a][:n, 1]]


def apply_attack(lines, topo_row, cooldown_row, or_pos, ex_pos):
    """BaseEnv._aux_handle_attack (baseEnv.py:3158-3169) for the union of a step (duration 1)"""
    for line in lines:
        R.apply_attack(line, 1, topo_row, cooldown_row, or_pos, ex_pos)


# ---- the library's rule core on the host (tests/native/opponent_area_emul.cpp) -------------------------------------------------
SRC = os.path.join(R.HERE, "native", "opponent_area_emul.cpp")
_emul = None


def _compile(out, flags):
    import subprocess
    os.makedirs(R._BUILD, exist_ok=True)
    deps = [SRC, os.path.join(R.ROOT, "grid2op_amd", "csrc", "gridpf_opponent.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


def emul_lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(_compile(os.path.join(R._BUILD, "libopponentareaemul.so"), ["-O2", "-fPIC", "-shared"]))
        _emul.opp_area_emul_prestep.restype = C.c_int
    return _emul


def sanitized_program():
    return _compile(os.path.join(R._BUILD, "opponent_area_emul_san"),
                    ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DOPPONENT_AREA_EMUL_MAIN"])


class AreaEmulator(R.Emulator):
    """The library's rule core (opp_area_prestep_serial) on `n_lanes` lanes of host memory, with the state layout of the engine."""

    def __init__(self, n_lanes, n_line, or_pos, ex_pos, lines, area_of_line, **kw):
        super().__init__(n_lanes, n_line, or_pos, ex_pos, GEOMETRIC, lines, **kw)
        groups = split_areas(lines, area_of_line)
        self.n_area = len(groups)
        self.area_lines = np.ascontiguousarray(np.concatenate(groups), dtype=np.int32)
        self.area_count = np.array([len(g) for g in groups], dtype=np.int32)
        self.area_offset = np.ascontiguousarray(np.concatenate([[0], np.cumsum(self.area_count)[:-1]]), dtype=np.int32)
        self.area_state = np.zeros((n_lanes, self.n_area, AREA_STATE_INTS), dtype=np.int32)
        self.area_state[:, :, A_COUNTER] = self.area_state[:, :, A_LINE] = self.area_state[:, :, A_INFO_LINE] = -1
        self.area_state[:, :, A_NEXT_TIME] = TIME_NONE
        self.area_sched = np.zeros((n_lanes, self.n_area, max(self.cap, 1), 2), dtype=np.int32)

    def prestep(self, steps_survived, done, rho, line_status, topo, cooldown):
        ip = C.POINTER(C.c_int32)
        st = np.ascontiguousarray(steps_survived, dtype=np.int32)
        dn = np.ascontiguousarray(done, dtype=np.uint8)
        rh = np.ascontiguousarray(rho, dtype=np.float32)
        ls = np.ascontiguousarray(line_status, dtype=np.uint8)
        assert topo.dtype == np.int32 and cooldown.dtype == np.int32 and topo.flags.c_contiguous and cooldown.flags.c_contiguous
        assert rh.shape == (self.n, self.n_line) and ls.shape == rh.shape and cooldown.shape == rh.shape and topo.shape[0] == self.n
        rc = emul_lib().opp_area_emul_prestep(
            C.byref(self.cfg), self.n, self.n_line, topo.shape[1], self.or_pos.ctypes.data_as(ip), self.ex_pos.ctypes.data_as(ip),
            self.budget.ctypes.data_as(C.POINTER(C.c_double)), self.state.ctypes.data_as(ip), self.draws.ctypes.data_as(C.POINTER(C.c_double)),
            C.c_int(self.n_area), self.area_lines.ctypes.data_as(ip), self.area_offset.ctypes.data_as(ip), self.area_count.ctypes.data_as(ip),
            self.area_state.ctypes.data_as(ip), self.area_sched.ctypes.data_as(ip), st.ctypes.data_as(ip), dn.ctypes.data_as(C.POINTER(C.c_uint8)),
            rh.ctypes.data_as(C.POINTER(C.c_float)), ls.ctypes.data_as(C.POINTER(C.c_uint8)), topo.ctypes.data_as(ip), cooldown.ctypes.data_as(ip))
        assert rc == 0

    def attack_lines(self):
        out = np.zeros((self.n, self.n_line), dtype=bool)
        for k in range(self.n):
            for l in self.area_state[k, :, A_INFO_LINE]:
                if l >= 0:
                    out[k, l] = True
        return out
