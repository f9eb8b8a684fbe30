"""Episode time limits of the batched acting path (include/gridpf.h gpf_set_episode_limit) restated in numpy -- what
tests/test_episode_limit_cpu.py holds against the episodes recorded from the unmodified reference (tests/golden/episode_limit_*.npz) and
what the device is held to --, and the loader of the g++ host emulator of the library's rules (tests/native/episode_emul.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import reward_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MAX_SLOTS = 8
REWARD_NAMES = R.REWARD_NAMES


def truncated(steps, limit, done):
    """the rule: a step that fails at the limit is terminated, not truncated"""
    return (not done) and limit > 0 and steps >= limit


def length(terminated, trunc, steps_before, steps_after):
    return steps_before + 1 if terminated else (steps_after if trunc else 0)


def duration_reward(ended, length_, limit, per_timestep=1.0):
    """EpisodeDurationReward: float32; total_time_steps is a float32 product, the quotient is rounded once"""
    if not ended:
        return np.float32(0.0)
    if limit <= 0:
        return np.float32(length_)
    total = np.float32(limit) * np.float32(per_timestep)
    return np.float32(np.float64(length_) / np.float64(total))


def value(kind, p, *, trunc=False, **row):
    """one reward slot with the reference's is_done = failed or truncated (reward_ref.value is the rest)"""
    bad = bool(row["illegal"]) or bool(row["ambiguous"])
    if trunc and not row["failed"]:
        if kind == R.L2RPN:
            return np.float32(0.0)
        if kind == R.REDISP and bad:
            return np.float32(float(p[2]))
    return R.value(kind, p, **row)


def constant_branch(kind, failed, illegal, ambiguous, trunc=False):
    if trunc and not failed and (kind == R.L2RPN or (kind == R.REDISP and (illegal or ambiguous))):
        return True
    return R.constant_branch(kind, failed, illegal, ambiguous)


def lane_values(slots, trunc=False, **row):
    return np.array([value(k, p, trunc=trunc, **row) for k, p in slots], np.float32)


class EpisodeRef:
    """one lane across launches: flags, length, duration reward, sequential float64 returns"""

    def __init__(self, n_slot=0, per_timestep=1.0):
        self.n_slot, self.per_timestep = n_slot, per_timestep
        self.running, self.last = np.zeros(n_slot, np.float64), np.zeros(n_slot, np.float64)
        self.length_last = self.n_episodes = self.steps_prev = 0

    def poststep(self, steps_after, limit, done, rewards=None):
        term = bool(done)
        trunc = truncated(steps_after, limit, term)
        fresh = term or (trunc and self.steps_prev < limit)
        self.terminated, self.truncated = term, trunc
        self.length = length(term, trunc, self.steps_prev, steps_after)
        self.duration_reward = duration_reward(term or trunc, self.length, limit, self.per_timestep)
        if rewards is not None:
            for s in range(self.n_slot):
                r = self.running[s] + np.float64(np.float32(rewards[s]))          # ONE add per slot and launch, in launch order
                if fresh:
                    self.last[s], self.running[s] = r, 0.0
                else:
                    self.running[s] = r
        if fresh:
            self.length_last = self.length
            self.n_episodes += 1
        self.steps_prev = steps_after
        return fresh


# ---- the recorded episodes (tests/golden/episode_limit_*.npz) ----
def fixture_row(fx, i, storage_key="storage_power"):
    """reward_ref.fixture_row with the two meanings of `done` apart: failed = terminated"""
    row = R.fixture_row(fx, i, storage_key)
    row["failed"] = bool(fx["terminated"][i])
    return row


# ---- the library's rules on the host (tests/native/episode_emul.cpp) ----
_BUILD = os.path.join(tempfile.gettempdir(), f"gridpf_episode_emul_{os.getuid()}")
SRC = os.path.join(HERE, "native", "episode_emul.cpp")
_emul = None


def _compile(out, flags):
    os.makedirs(_BUILD, exist_ok=True)
    csrc = os.path.join(ROOT, "grid2op_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in ("gridpf_episode.hpp", "gridpf_reward.hpp", "gridpf_alert.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


def emul_lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(_compile(os.path.join(_BUILD, "libepisodeemul.so"), ["-O2", "-fPIC", "-shared"]))
        _emul.episode_emul_reward_lane.restype = None
        _emul.episode_emul_poststep.restype = C.c_int
        _emul.episode_emul_truncated.restype = C.c_int
        _emul.episode_emul_alert_poststep.restype = C.c_float
        assert _emul.episode_emul_slot_bytes() == C.sizeof(R.Slot) and _emul.episode_emul_stats_bytes() == C.sizeof(Stats)
    return _emul


def sanitized_program():
    return _compile(os.path.join(_BUILD, "episode_emul_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEPISODE_EMUL_MAIN"])


class Lane(C.Structure):
    _fields_ = [("terminated", C.c_int), ("truncated", C.c_int), ("length", C.c_int), ("duration_reward", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("running", C.c_double * MAX_SLOTS), ("last", C.c_double * MAX_SLOTS), ("length_last", C.c_int), ("n_episodes", C.c_int),
                ("steps_prev", C.c_int)]


def emul_truncated(steps, limit, done):
    return bool(emul_lib().episode_emul_truncated(int(steps), int(limit), int(bool(done))))


def emul_poststep(stats, steps_after, limit, done, per_timestep, rewards):
    """the library's episode_poststep_serial on one lane: (fresh, Lane); `stats` (a Stats) is updated in place"""
    lane = Lane()
    rw = None if rewards is None else np.ascontiguousarray(rewards, np.float32)
    fresh = emul_lib().episode_emul_poststep(int(steps_after), int(limit), int(bool(done)), C.c_float(per_timestep),
                                             None if rw is None else rw.ctypes.data_as(C.c_void_p), 0 if rw is None else len(rw),
                                             C.byref(lane), C.byref(stats))
    return bool(fresh), lane


def emul_reward_lane(slots, trunc, *, gen_p, load_p, a_or, rho, line_status, thermal, dispatch, storage, cost, failed, illegal, ambiguous):
    """reward_value on one lane: float32 [n_slot]; trunc None: the six-argument call (the parameter's default)"""
    def arr(a, dt):
        return np.ascontiguousarray(a, dtype=dt)
    g, ld, ao, rh, th, co = (arr(x, np.float32) for x in (gen_p, load_p, a_or, rho, thermal, cost))
    ls = arr(np.asarray(line_status).astype(bool), np.uint8)
    st = arr(np.asarray(storage, np.float32), np.float64)
    di = None if dispatch is None else arr(dispatch, np.float32)
    out = np.zeros(len(slots), np.float32)

    def fp(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    emul_lib().episode_emul_reward_lane(len(slots), R.c_slots(slots), C.c_int(len(g)), C.c_int(len(ld)), C.c_int(len(ao)), C.c_int(len(st)), fp(g),
                                        fp(ld), fp(ao), fp(rh), fp(ls), fp(th), fp(di), fp(st), fp(co), int(bool(failed)), int(bool(illegal)),
                                        int(bool(ambiguous)), -1 if trunc is None else int(bool(trunc)), fp(out))
    return out
