"""Python restatement of the alert bookkeeping and of AlertReward of the batched acting path (include/gridpf.h gpf_set_alerts), written
from the reference (Environment/baseEnv.py:3295-3329, 1677-1685; Reward/alertReward.py:105-207) with numpy as the reference does it, the
state-row layout of ``gpf_get_alert_state``, and the loader of the g++ host emulator of the library's rule core
(tests/native/alert_emul.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENV_ARRAYS = ("last_alert", "is_already_attacked", "time_since_last_alert", "alert_duration", "time_since_last_attack", "attack_under_alert",
              "was_alert_used_after_attack")
OBS_ATTRS = ("active_alert", "time_since_last_alert", "alert_duration", "total_number_of_alert", "time_since_last_attack", "attack_under_alert",
             "was_alert_used_after_attack")
DEFAULTS = (-1.0, -10.0, 1.0, 2.0)           # min_no_blackout, min_blackout, max_no_blackout, max_blackout


def state_ints(A, W):
    return 8 * A + 3 + 2 * (W + 2) * A


def mask_of(bits):
    """uint64 mask of a boolean vector (bit i = element i)"""
    return sum(1 << int(i) for i in np.flatnonzero(np.asarray(bits)))


class AlertRef:
    """one lane: the environment's arrays and the reward's rings, updated as the reference updates them"""

    def __init__(self, A, time_window=12, constants=DEFAULTS):
        self.A, self.W, self.R = int(A), int(time_window), int(time_window) + 2
        self.c = [np.float32(x) for x in constants]
        self.ran = False
        self.reward = np.float32(0.0)
        self.reset()

    def reset(self):
        A = self.A
        self.last_alert = np.zeros(A, bool)
        self.is_already_attacked = np.zeros(A, bool)
        self.time_since_last_alert = np.full(A, -1, np.int32)
        self.alert_duration = np.zeros(A, np.int32)
        self.total_number_of_alert = 0
        self.time_since_last_attack = np.full(A, -1, np.int32)
        self.was_alert_used_after_attack = np.zeros(A, np.int32)
        self.attack_under_alert = np.zeros(A, np.int32)
        self.ts_attack = np.zeros((self.R, A), bool)
        self.alert_launched = np.zeros((self.R, A), bool)
        self.current_id = 0
        self.currently_attacked = np.zeros(A, bool)
        self.ran = False

    def prestep(self, steps_survived, done, raise_alert, attacked):
        """raise_alert / attacked: boolean [A]; an all-False `attacked` is the reference's opponent_attack_line None"""
        if steps_survived == 0:
            self.reset()
            return
        if done:
            self.ran = False
            return
        raise_alert, att = np.asarray(raise_alert, bool), np.asarray(attacked, bool)
        self.last_alert[:] = raise_alert
        self.time_since_last_alert[~self.last_alert & (self.time_since_last_alert != -1)] += 1
        self.time_since_last_alert[self.last_alert] = 0
        self.alert_duration[self.last_alert] += 1
        self.alert_duration[~self.last_alert] = 0
        self.total_number_of_alert += int(self.last_alert.sum())
        if att.any():
            first = att & ~self.is_already_attacked
            self.time_since_last_attack[first] = 0
            self.time_since_last_attack[~first & (self.time_since_last_attack != -1)] += 1
            self.is_already_attacked[att] = True
        else:
            self.time_since_last_attack[self.time_since_last_attack != -1] += 1
            self.is_already_attacked[:] = False
        new = self.time_since_last_attack == 0
        self.attack_under_alert[new] = 2 * self.last_alert[new] - 1
        self.attack_under_alert[self.time_since_last_attack > self.W] = 0
        # AlertReward._update_state
        self.current_id = (self.current_id + 1) % self.R
        if not att.any():
            self.currently_attacked[:] = False
            self.ts_attack[self.current_id, :] = False
        else:
            self.ts_attack[self.current_id, att & ~self.currently_attacked] = True
            self.currently_attacked[:] = att
        self.alert_launched[self.current_id, :] = raise_alert
        self.was_alert_used_after_attack[:] = 0
        self.ran = True

    def poststep(self, blackout):
        if not self.ran:
            self.reward = np.float32(0.0)
            return self.reward
        mn_nb, mn_b, mx_nb, mx_b = self.c
        res = 0.0
        if blackout:
            idx = (np.arange(-self.W, 1) + self.current_id) % self.R
            ts = self.ts_attack[idx, :]
            if ts.any():
                ts_ind, line_ind = ts.nonzero()
                lines, first = np.unique(line_ind, return_index=True)
                rows = idx[ts_ind[first]]
                self.was_alert_used_after_attack[lines] = self.alert_launched[rows, lines] * 2 - 1
                res = np.mean(self.alert_launched[rows, lines]) * (mx_b - mn_b) + mn_b
        else:
            iw = (self.current_id - self.W) % self.R
            la = self.ts_attack[iw, :]
            if la.any():
                sent = self.alert_launched[iw, la]
                self.was_alert_used_after_attack[la] = 1 - sent * 2
                res = (mn_nb - mx_nb) * np.mean(sent) + mx_nb
                self.ts_attack[iw, :] = False
        self.reward = np.float32(res)
        return self.reward

    def row(self):
        A = self.A
        return np.concatenate([self.last_alert, self.is_already_attacked, self.time_since_last_alert, self.alert_duration, self.time_since_last_attack,
                               self.attack_under_alert, self.was_alert_used_after_attack, [self.total_number_of_alert, self.current_id, int(self.ran)],
                               self.currently_attacked, self.ts_attack.reshape(-1), self.alert_launched.reshape(-1)]).astype(np.int32)

    def set_row(self, row):
        A, R = self.A, self.R
        row = np.asarray(row)
        assert row.shape == (state_ints(A, self.W),)
        self.last_alert, self.is_already_attacked = row[:A].astype(bool), row[A:2 * A].astype(bool)
        self.time_since_last_alert, self.alert_duration = row[2 * A:3 * A].astype(np.int32), row[3 * A:4 * A].astype(np.int32)
        self.time_since_last_attack, self.attack_under_alert = row[4 * A:5 * A].astype(np.int32), row[5 * A:6 * A].astype(np.int32)
        self.was_alert_used_after_attack = row[6 * A:7 * A].astype(np.int32)
        self.total_number_of_alert, self.current_id, self.ran = int(row[7 * A]), int(row[7 * A + 1]), bool(row[7 * A + 2])
        self.currently_attacked = row[7 * A + 3:8 * A + 3].astype(bool)
        self.ts_attack = row[8 * A + 3:8 * A + 3 + R * A].astype(bool).reshape(R, A)
        self.alert_launched = row[8 * A + 3 + R * A:].astype(bool).reshape(R, A)

    def obs(self, game_over=False):
        """the seven observation attributes as float32 (Observation/baseObservation.py:4630-4636, game over: 1681-1687)"""
        A = self.A
        if game_over:
            return dict(active_alert=np.zeros(A, np.float32), time_since_last_alert=np.zeros(A, np.float32), alert_duration=np.zeros(A, np.float32),
                        total_number_of_alert=np.zeros(1, np.float32), time_since_last_attack=np.full(A, -1, np.float32),
                        attack_under_alert=self.attack_under_alert.astype(np.float32),
                        was_alert_used_after_attack=self.was_alert_used_after_attack.astype(np.float32))
        return dict(active_alert=self.last_alert.astype(np.float32), time_since_last_alert=self.time_since_last_alert.astype(np.float32),
                    alert_duration=self.alert_duration.astype(np.float32), total_number_of_alert=np.array([self.total_number_of_alert], np.float32),
                    time_since_last_attack=self.time_since_last_attack.astype(np.float32), attack_under_alert=self.attack_under_alert.astype(np.float32),
                    was_alert_used_after_attack=self.was_alert_used_after_attack.astype(np.float32))


def fixture_row(fx, i):
    """the state row of launch i of a recorded episode (the ran flag: a step, not a reset)"""
    return np.concatenate([fx["env_last_alert"][i], fx["env_is_already_attacked"][i], fx["env_time_since_last_alert"][i], fx["env_alert_duration"][i],
                           fx["env_time_since_last_attack"][i], fx["env_attack_under_alert"][i], fx["env_was_alert_used_after_attack"][i],
                           [fx["total_number_of_alert"][i], fx["current_id"][i], 0 if fx["is_reset"][i] else 1], fx["currently_attacked"][i],
                           fx["ts_attack"][i].reshape(-1), fx["alert_launched"][i].reshape(-1)]).astype(np.int32)


# ---- the library's rule core on the host (tests/native/alert_emul.cpp) ------------------------------------------------------------------
_BUILD = os.path.join(tempfile.gettempdir(), f"gridpf_alert_emul_{os.getuid()}")
SRC = os.path.join(HERE, "native", "alert_emul.cpp")
_emul = None


def _compile(out, flags):
    os.makedirs(_BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_alert.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


def emul_lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(_compile(os.path.join(_BUILD, "libalertemul.so"), ["-O2", "-fPIC", "-shared"]))
        _emul.alert_emul_poststep.restype = C.c_float
    return _emul


def sanitized_program():
    return _compile(os.path.join(_BUILD, "alert_emul_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DALERT_EMUL_MAIN"])


class AlertEmulator:
    """the library's rule core (alert_prestep_serial / alert_poststep_serial) on `n` lanes of host memory, with the engine's two blocks;
    rows() is the layout of gpf_get_alert_state"""

    def __init__(self, n, A, time_window=12, constants=DEFAULTS):
        self.n, self.A, self.W, self.R = n, int(A), int(time_window), int(time_window) + 2
        self.c = (C.c_float * 4)(*constants)
        self.ob = np.zeros((n, 6 * self.A + 1), np.int32)
        self.ax = np.zeros((n, 3 + 2 * self.R), np.uint64)
        self.reward = np.zeros(n, np.float32)
        self.prestep(np.zeros(n, int), np.zeros(n, int), np.zeros(n, np.uint64), np.zeros(n, np.uint64))

    def prestep(self, steps_survived, done, raise_mask, att_mask):
        L = emul_lib()
        for k in range(self.n):
            L.alert_emul_prestep(C.c_int(self.A), C.c_int(self.W), self.c, self.ob[k].ctypes.data_as(C.c_void_p), self.ax[k].ctypes.data_as(C.c_void_p),
                                 C.c_int(int(steps_survived[k])), C.c_int(int(done[k])), C.c_uint64(int(raise_mask[k])), C.c_uint64(int(att_mask[k])))

    def poststep(self, blackout):
        L = emul_lib()
        for k in range(self.n):
            self.reward[k] = L.alert_emul_poststep(C.c_int(self.A), C.c_int(self.W), self.c, self.ob[k].ctypes.data_as(C.c_void_p),
                                                   self.ax[k].ctypes.data_as(C.c_void_p), C.c_int(int(blackout[k])))
        return self.reward

    def rows(self):
        A, R = self.A, self.R
        out = np.zeros((self.n, state_ints(A, self.W)), np.int32)
        bits = lambda w: (w[..., None] >> np.arange(A, dtype=np.uint64)) & np.uint64(1)          # noqa: E731
        o = self.ob
        out[:, :A] = o[:, :A]
        out[:, A:2 * A] = bits(self.ax[:, 0])
        out[:, 2 * A:3 * A], out[:, 3 * A:4 * A], out[:, 4 * A:5 * A] = o[:, A:2 * A], o[:, 2 * A:3 * A], o[:, 3 * A:4 * A]
        out[:, 5 * A:6 * A], out[:, 6 * A:7 * A], out[:, 7 * A] = o[:, 4 * A:5 * A], o[:, 5 * A:6 * A], o[:, 6 * A]
        out[:, 7 * A + 1] = (self.ax[:, 2] & np.uint64(0xFFFFFFFF)).astype(np.int32)
        out[:, 7 * A + 2] = ((self.ax[:, 2] >> np.uint64(32)) & np.uint64(1)).astype(np.int32)
        out[:, 7 * A + 3:8 * A + 3] = bits(self.ax[:, 1])
        out[:, 8 * A + 3:] = bits(self.ax[:, 3:]).reshape(self.n, -1)
        return out
