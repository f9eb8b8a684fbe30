"""The environment's rewards of the batched acting path (include/gridpf.h gpf_set_rewards) restated in numpy float64 on the float32 inputs
the engine reads -- what tests/test_reward_cpu.py holds against the episodes recorded from the unmodified reference and what the device is
held to at one float32 spacing --, the bounds of the reference's own float32 evaluation, and the loader of the g++ host emulator of the
library's rule core (tests/native/reward_emul.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

REDISP, L2RPN, LINES_CAPACITY, ECONOMIC, GAMEPLAY = 1, 2, 3, 4, 5
KINDS = (REDISP, L2RPN, LINES_CAPACITY, ECONOMIC, GAMEPLAY)
U = 2.0 ** -24                       # one float32 rounding, relative to the magnitude it rounds

f64 = np.float64


def _f32in(a):
    """the engine's float32 input, as float64"""
    return np.asarray(a, np.float32).astype(f64)


def value(kind, p, *, gen_p, load_p, a_or, rho, line_status, thermal, dispatch, storage, cost, failed, illegal, ambiguous, variant=None):
    """One slot of one lane: np.float32.  ``dispatch`` None: none.  ``variant`` (the discrimination check only): "no_alpha", "no_storage",
    "min_cost" change the RedispReward formula the way a wrong implementation would."""
    bad = bool(illegal) or bool(ambiguous)
    p = [float(x) for x in p]
    if kind == REDISP:
        if failed:
            return np.float32(p[2])
        if bad:
            return np.float32(p[3])
        g, ld = _f32in(gen_p), _f32in(load_p)
        sg, sl = g.sum(), ld.sum()
        sd = np.abs(_f32in(dispatch)).sum() if dispatch is not None else f64(0.0)
        ss = np.abs(_f32in(storage)).sum()
        on = np.asarray(gen_p, np.float32) > 0
        if not on.any():
            return np.float32(np.nan)
        c = _f32in(cost)[on]
        mc = c.min() if variant == "min_cost" else c.max()
        alpha = 0.0 if variant == "no_alpha" else p[0]
        if variant == "no_storage":
            ss = f64(0.0)
        regret = (mc * p[4]) * (((sg - sl) + alpha * sd) + ss)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.float32((f64(p[1]) - regret) / sl)
    if kind == L2RPN:
        if failed:
            return np.float32(0.0)
        rel = np.minimum(np.abs(_f32in(a_or)) / (np.abs(_f32in(thermal)) + f64(np.float32(0.1))), 1.0)
        return np.float32(np.maximum(1.0 - rel * rel, 0.0).sum())
    if kind == LINES_CAPACITY:
        if failed or bad:
            return np.float32(0.0)
        ls = np.asarray(line_status).astype(bool)
        n = f64(ls.sum())
        us = _f32in(rho)[ls].sum()
        if n == 0:
            return np.float32(LINES_CAPACITY_NONE)
        u = min(max(us, 0.0), n)
        return np.float32((n - u) / n)
    if kind == ECONOMIC:
        if failed or bad:
            return np.float32(p[1])
        c = (_f32in(gen_p) * _f32in(cost)).sum() * p[3]
        v = min(max(p[0] - c, 0.0), p[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.float32(p[1] + (p[2] - p[1]) * (f64(v) / f64(p[0])))
    if kind == GAMEPLAY:
        if failed:
            return np.float32(p[0])
        if bad:
            return np.float32(p[0]) / np.float32(2.0)
        return np.float32(p[1])
    raise ValueError(kind)


LINES_CAPACITY_NONE = 1.0            # numpy.interp(0, [0, 0], [0, 1]): pinned against numpy by tests/test_reward_cpu.py


def constant_branch(kind, failed, illegal, ambiguous):
    """the slot takes no arithmetic: device, emulator and restatement must agree bit for bit"""
    bad = bool(illegal) or bool(ambiguous)
    return bool(failed) if kind == L2RPN else (bool(failed) or bad or kind == GAMEPLAY)


def lane_values(slots, **row):
    return np.array([value(k, p, **row) for k, p in slots], np.float32)


def spacing_ok(got, want):
    """got within one float32 spacing of want (both float32); NaN equals NaN, infinities must be equal"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(want) & np.isfinite(got)
        ok = np.where(fin, np.abs(got.astype(f64) - want.astype(f64)) <= np.spacing(np.abs(want)).astype(f64), False)
    same = (np.isnan(got) & np.isnan(want)) | (got == want)
    return ok | same


# ---- bounds of the reference's float32 evaluation: at most K roundings, each at most 2^-24 times the largest intermediate magnitude ----
def bound(kind, p, *, gen_p, load_p, a_or, rho, line_status, thermal, dispatch, storage, cost, **_):
    p = [float(x) for x in p]
    if kind == REDISP:
        g, ld = _f32in(gen_p), _f32in(load_p)
        on = g > 0
        mc = _f32in(cost)[on].max()
        sd = np.abs(_f32in(dispatch)).sum() if dispatch is not None else 0.0
        K = len(g) + len(ld) + len(np.atleast_1d(storage)) + 16
        return K * U * (abs(p[1]) + mc * p[4] * (np.abs(g).sum() + np.abs(ld).sum() + p[0] * sd + np.abs(_f32in(storage)).sum())) / ld.sum()
    if kind == L2RPN:
        rel = np.minimum(np.abs(_f32in(a_or)) / (np.abs(_f32in(thermal)) + f64(np.float32(0.1))), 1.0)
        return (len(rel) + 8) * U * max(np.maximum(1.0 - rel * rel, 0.0).sum(), 1.0)
    if kind == LINES_CAPACITY:
        # the float32 sum of rho over the connected lines: n_line roundings of magnitude <= max(sum |rho|, n); the rest is float64 and one
        # final rounding of a value in [0, 1]; the value is the sum's error divided by n
        ls = np.asarray(line_status).astype(bool)
        n = max(float(ls.sum()), 1.0)
        return (len(ls) + 8) * U * max(np.abs(_f32in(rho))[ls].sum(), n) / n + U
    if kind == ECONOMIC:
        # n_gen products and n_gen additions in float32 of magnitude <= sum |gen_p cost|, times dts; then the subtraction from worst_cost
        # and the map onto [reward_min, reward_max] (8 more roundings of magnitude <= worst_cost)
        g = _f32in(gen_p)
        mag = max((np.abs(g) * _f32in(cost)).sum() * p[3], abs(p[0]))
        return (2 * len(g) + 8) * U * mag * abs(p[2] - p[1]) / abs(p[0]) + U * max(abs(p[1]), abs(p[2]))
    if kind == GAMEPLAY:
        return 0.0
    raise ValueError(kind)


# ---- the rows of a recorded episode (tests/golden/reward_*.npz) ----
def fixture_slots(fx):
    """[(kind, p)] of the five recorded rewards, from the values the reference's initialize methods left (stored in the fixture)"""
    dts = float(fx["delta_time_seconds"]) / 3600.0
    return [(REDISP, [float(fx["redisp_alpha"]), float(fx["redisp_max_regret"]), float(fx["redisp_min_reward"]), float(fx["redisp_illegal_ambiguous"]), dts]),
            (L2RPN, []), (LINES_CAPACITY, []),
            (ECONOMIC, [float(fx["economic_worst_cost"]), float(fx["economic_reward_min"]), float(fx["economic_reward_max"]), dts]),
            (GAMEPLAY, [float(fx["gameplay_reward_min"]), float(fx["gameplay_reward_max"])])]


def fixture_row(fx, i, storage_key="storage_power"):
    return dict(gen_p=fx["gen_p"][i], load_p=fx["load_p"][i], a_or=fx["a_or"][i], rho=fx["rho"][i], line_status=fx["line_status"][i],
                thermal=fx["thermal_limit"], dispatch=fx["actual_dispatch"][i], storage=fx[storage_key][i], cost=fx["gen_cost_per_MW"],
                failed=bool(fx["done"][i]), illegal=bool(fx["is_illegal"][i]) or bool(fx["failed_redisp"][i]), ambiguous=bool(fx["is_ambiguous"][i]))


REWARD_NAMES = ("redisp", "l2rpn", "lines_capacity", "economic", "gameplay")


def fixture_rewards(fx, i):
    return np.array([fx["reward_" + k][i] for k in REWARD_NAMES], np.float32)


# ---- the library's rule core on the host (tests/native/reward_emul.cpp) ----
_BUILD = os.path.join(tempfile.gettempdir(), f"gridpf_reward_emul_{os.getuid()}")
SRC = os.path.join(HERE, "native", "reward_emul.cpp")
_emul = None


class Slot(C.Structure):
    _fields_ = [("kind", C.c_int32), ("p", C.c_double * 6)]


def _compile(out, flags):
    os.makedirs(_BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_reward.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


def emul_lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(_compile(os.path.join(_BUILD, "librewardemul.so"), ["-O2", "-fPIC", "-shared"]))
        _emul.reward_emul_lane.restype = None
        assert _emul.reward_emul_slot_bytes() == C.sizeof(Slot)
    return _emul


def sanitized_program():
    return _compile(os.path.join(_BUILD, "reward_emul_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DREWARD_EMUL_MAIN"])


def c_slots(slots):
    arr = (Slot * len(slots))()
    for i, (k, p) in enumerate(slots):
        arr[i].kind = int(k)
        for j, x in enumerate(p):
            arr[i].p[j] = float(x)
    return arr


def emul_lane(slots, *, gen_p, load_p, a_or, rho, line_status, thermal, dispatch, storage, cost, failed, illegal, ambiguous):
    """the library's rule core on one lane: float32 [n_slot]"""
    def arr(a, dt):
        return np.ascontiguousarray(a, dtype=dt)
    g, ld, ao, rh, th, co = (arr(x, np.float32) for x in (gen_p, load_p, a_or, rho, thermal, cost))
    ls = arr(np.asarray(line_status).astype(bool), np.uint8)
    st = arr(np.asarray(storage, np.float32), np.float64)             # (the injection row holds float64)
    di = None if dispatch is None else arr(dispatch, np.float32)
    out = np.zeros(len(slots), np.float32)

    def fp(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    emul_lib().reward_emul_lane(len(slots), c_slots(slots), C.c_int(len(g)), C.c_int(len(ld)), C.c_int(len(ao)), C.c_int(len(st)), fp(g), fp(ld),
                                fp(ao), fp(rh), fp(ls), fp(th), fp(di), fp(st), fp(co), int(bool(failed)), int(bool(illegal)), int(bool(ambiguous)), fp(out))
    return out
