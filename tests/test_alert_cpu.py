"""Alerts and AlertReward of the batched acting path (include/gridpf.h gpf_set_alerts), the parts that need no GPU: the Python restatement
(tests/alert_ref.py) and the library's rule core compiled with g++ into a host emulator (tests/native/alert_emul.cpp) reproduce the
episodes recorded from the unmodified reference environment (tests/golden/alert_*.npz) exactly, rewards bit for bit; emulator against
restatement on random steps at the edge sizes; every refusal through a header-only handle; the ``dim_alerts`` layout of `ObsSpec` against
the recorded ``obs.to_vect()``; `alert_config`."""
import subprocess

import numpy as np
import pytest

import alert_ref as AR
from conftest import golden_path

TAGS = ("wcci118", "case14")


@pytest.fixture(scope="module", params=TAGS)
def recorded(request):
    return dict(np.load(golden_path(f"alert_{request.param}.npz")))


def _att(fx, i):
    return fx["info_lines"][i][fx["lines"]]


def test_fixtures_cover_the_alert_automaton():
    w, c = (dict(np.load(golden_path(f"alert_{t}.npz"))) for t in TAGS)
    assert int(w["time_window"]) == 12 and int(c["time_window"]) == 4
    assert np.array_equal(w["reward_constants"], np.array(AR.DEFAULTS, np.float32))
    for fx in (w, c):
        step = fx["is_reset"] == 0
        used, done = fx["env_was_alert_used_after_attack"], fx["done"].astype(bool)
        # attacks scored without blackout, with (-1) and without (+1) an alert
        assert ((used == -1).any(axis=1) & step & ~done).any() and ((used == 1).any(axis=1) & step & ~done).any()
        assert (fx["alert_reward"][step & ~done] != 0).sum() >= 5
        # an attack older than the window: attack_under_alert back to 0
        assert (fx["env_time_since_last_attack"] > int(fx["time_window"])).any()
        # an alert raised with an illegal agent action
        assert (fx["alert_mask"].any(axis=1) & (fx["is_illegal"] == 1)).any()
        assert (fx["has_attack"] == fx["info_lines"].any(axis=1)).all()
    # the is_already_attacked quirk: a line leaves a continuing multi-line attack and stays "already attacked"
    quirk = 0
    for i in range(1, len(w["is_reset"])):
        a0, a1 = _att(w, i - 1), _att(w, i)
        quirk += int(a1.any() and (a0 & ~a1 & w["env_is_already_attacked"][i]).any())
    assert quirk >= 1
    # case14: blackouts inside the window with and without an alert, a blackout without an attack in the window, resets
    used, done = c["env_was_alert_used_after_attack"], c["done"].astype(bool)
    assert (used[done] == 1).any() and (used[done] == -1).any() and ((used[done] == 0).all(axis=1) & (c["alert_reward"][done] == 0)).any()
    assert int(c["is_reset"].sum()) >= 3 and int(done.sum()) >= 3


def test_restatement_reproduces_the_recorded_episodes(recorded):
    fx = recorded
    ref = AR.AlertRef(len(fx["lines"]), int(fx["time_window"]), fx["reward_constants"])
    for i in range(len(fx["is_reset"])):
        ref.prestep(0 if fx["is_reset"][i] else 1, False, fx["alert_mask"][i], _att(fx, i))
        r = ref.poststep(bool(fx["done"][i]))
        assert np.array_equal(ref.row(), AR.fixture_row(fx, i)), (i, np.flatnonzero(ref.row() != AR.fixture_row(fx, i)))
        assert r.tobytes() == np.float32(fx["alert_reward"][i]).tobytes(), (i, r, fx["alert_reward"][i])
        for k, v in ref.obs(game_over=bool(fx["done"][i])).items():
            # (set_game_over leaves attack_under_alert "not updated" on a FRESH observation, baseObservation.py:1687: the recorded values of
            #  a game-over step are uninitialised memory there; the engine writes the environment's values)
            if not (fx["done"][i] and k == "attack_under_alert"):
                assert np.array_equal(v, np.asarray(fx["obs_" + k][i], np.float32).reshape(-1)), (i, k)


def test_emulator_reproduces_the_recorded_episodes(recorded):
    """the library's rule core on 3 lanes; lane 2 additionally sits out a few launches as a done lane and is then put back"""
    fx = recorded
    A, W = len(fx["lines"]), int(fx["time_window"])
    n = 3
    emu = AR.AlertEmulator(n, A, W, fx["reward_constants"])
    for i in range(len(fx["is_reset"])):
        raise_mask, att_mask = AR.mask_of(fx["alert_mask"][i]), AR.mask_of(_att(fx, i))
        emu.prestep(np.full(n, 0 if fx["is_reset"][i] else 1), np.zeros(n), np.full(n, raise_mask, np.uint64), np.full(n, att_mask, np.uint64))
        rew = emu.poststep(np.full(n, int(fx["done"][i])))
        rows = emu.rows()
        for lane in range(n):
            assert np.array_equal(rows[lane], AR.fixture_row(fx, i)), (i, lane, np.flatnonzero(rows[lane] != AR.fixture_row(fx, i)))
        assert rew.tobytes() == np.full(n, fx["alert_reward"][i], np.float32).tobytes(), (i, rew, fx["alert_reward"][i])
    # a done lane is left alone and scores 0
    before = emu.rows()[0].copy()
    emu.prestep(np.full(n, 5), np.ones(n), np.full(n, 1, np.uint64), np.full(n, 1, np.uint64))
    assert (emu.poststep(np.ones(n)) == 0).all()
    after = emu.rows()[0]
    before[7 * A + 2] = 0                                               # (only the ran flag)
    assert np.array_equal(before, after)


@pytest.mark.parametrize("A,W", [(1, 1), (22, 12), (64, 1), (64, 62), (3, 62)])
def test_emulator_on_random_steps_equals_the_restatement(A, W):
    rng = np.random.default_rng(100 * A + W)
    n, steps = 5, max(300, 12 * W)
    p_black, p_reset = 1.5 / (W + 10), 0.3 / (W + 10)        # (a lane must outlive the window now and then, or nothing is scored without blackout)
    consts = (-1.0, -10.0, 1.0, 2.0) if A != 22 else (-0.3, -7.0, 0.7, 1.1)
    emu = AR.AlertEmulator(n, A, W, consts)
    refs = [AR.AlertRef(A, W, consts) for _ in range(n)]
    survived = np.zeros(n, int)
    att = np.zeros((n, A), bool)
    seen = dict(blackout_scored=0, scored=0, bit63=0)
    for t in range(steps):
        raise_ = rng.random((n, A)) < 0.3
        what = rng.integers(0, 5, n)
        att = np.where((what == 0)[:, None], rng.random((n, A)) < 0.4, np.where((what == 1)[:, None], False, np.where((what == 2)[:, None], att & (rng.random((n, A)) < 0.6), att)))
        done = (rng.random(n) < 0.05) & (survived > 0)
        black = rng.random(n) < p_black
        for k in range(n):
            refs[k].prestep(int(survived[k]), bool(done[k]), raise_[k], att[k])
            refs[k].poststep(bool(black[k]))
        emu.prestep(survived, done, [AR.mask_of(x) for x in raise_], [AR.mask_of(x) for x in att])
        rew = emu.poststep(black)
        want = np.array([r.row() for r in refs])
        assert np.array_equal(emu.rows(), want), (t, np.argwhere(emu.rows() != want)[:5])
        assert rew.tobytes() == np.array([r.reward for r in refs], np.float32).tobytes(), t
        ran = np.array([r.ran for r in refs])
        seen["blackout_scored"] += int((ran & black & (rew != 0)).sum())
        seen["scored"] += int((ran & ~black & (rew != 0)).sum())
        seen["bit63"] += int(A == 64 and raise_[:, 63].any())
        survived = np.where((black & ran) | (rng.random(n) < p_reset), 0, survived + 1)
    assert seen["blackout_scored"] >= 5 and seen["scored"] >= 20 and (A != 64 or seen["bit63"] >= 50), seen


GOOD = dict(kind=3, lines=[0, 1, 2], init_budget=1.0, budget_per_ts=0.1, attack_duration=3, attack_cooldown=1, attack_hazard_rate=0.1,
            recovery_rate=0.2, recovery_minimum_duration=1, pmax_pmin_ratio=4.0, episode_max_time=100, schedule_cap=8, draw_source=1)


def test_every_refusal_on_a_header_only_handle(load_model):
    from grid2op_amd.engine import GridPFError, PowerFlowEngine
    eng = PowerFlowEngine(load_model("l2rpn_wcci_2022_dev"), n_lanes=4, device=-1)
    with pytest.raises(GridPFError, match="no opponent"):
        eng.set_alerts()
    with pytest.raises(GridPFError, match="alerts are off"):
        eng.set_lane_alerts(np.zeros(4, np.uint64))
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_opponent(**dict(GOOD, lines=list(range(65))))
    with pytest.raises(GridPFError, match="65 alertable lines: more than GPF_ALERT_MAX_LINES = 64"):
        eng.set_alerts()
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_opponent(**GOOD)
    for w in (0, -3, 63):
        with pytest.raises(GridPFError, match=r"time_window -?\d+ is outside \[1, GPF_ALERT_MAX_WINDOW = 62\]"):
            eng.set_alerts(time_window=w)
    for name in ("reward_min_no_blackout", "reward_min_blackout", "reward_max_no_blackout", "reward_max_blackout"):
        for bad in (float("nan"), float("inf")):
            with pytest.raises(GridPFError, match="not finite"):
                eng.set_alerts(**{name: bad})
    with pytest.raises(GridPFError, match="alerts are off"):           # a refused descriptor leaves alerts off
        eng.set_lane_alerts(np.zeros(4, np.uint64))
    for w in (1, 12, 62):
        with pytest.raises(GridPFError, match="no HIP device"):         # a good call gets as far as the missing device
            eng.set_alerts(time_window=w)
    with pytest.raises(GridPFError, match=r"lane 2: an alert on a line at or above the 3 alertable lines"):
        eng.set_lane_alerts(np.array([0, 7, 8, 0], np.uint64))
    with pytest.raises(GridPFError, match="at or above"):
        eng.set_lane_alerts(np.array([1 << 63, 0, 0, 0], np.uint64))
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_lane_alerts(np.array([[1, 0, 1]] * 4, bool))
    with pytest.raises(GridPFError, match="no HIP device"):             # gpf_set_opponent turns alerts off
        eng.set_opponent(**GOOD)
    with pytest.raises(GridPFError, match="alerts are off"):
        eng.set_lane_alerts(None)
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_alerts()
    with pytest.raises(GridPFError, match="no HIP device"):             # ... and so does gpf_set_opponent_areas
        eng.set_opponent_areas([0, 0, 1])
    with pytest.raises(GridPFError, match="alerts are off"):
        eng.set_lane_alerts(None)
    for fn in (eng.alert_state, eng.alert_reward, lambda: eng.alerts_on_device(True)):
        with pytest.raises(GridPFError, match="alerts are off"):
            fn()
    eng.set_opponent(None)
    with pytest.raises(GridPFError, match="no opponent"):
        eng.set_alerts()
    eng.set_alerts(None)                                                # off is always possible
    eng.close()


def test_alert_kinds_of_the_observation_spec_are_refused_while_alerts_are_off(load_model):
    from grid2op_amd.engine import GridPFError, PowerFlowEngine
    from grid2op_amd.obs_spec import KIND, ObsSpec
    m = load_model("l2rpn_case14_sandbox")
    eng = PowerFlowEngine(m, n_lanes=2, device=-1)
    assert len(KIND) == 31 and max(KIND.values()) == 30
    with pytest.raises(GridPFError, match=r"segment 1 \(time_since_last_attack\): alerts are off"):
        eng.set_obs_spec(ObsSpec(m, ["rho", "time_since_last_attack"], dim_alerts=3))
    seg = np.array([[99, 0, 1, 0, 0]], np.int32)
    from grid2op_amd._capi import ptr
    import ctypes as C
    assert eng._lib.gpf_set_obs_spec(eng._h, 1, ptr(seg, C.c_int32), 1, None, None, 1) != 0
    assert b"unknown source kind 99" in eng._lib.gpf_last_error()
    seg[0, 0] = 31
    assert eng._lib.gpf_set_obs_spec(eng._h, 1, ptr(seg, C.c_int32), 1, None, None, 1) != 0
    assert b"unknown source kind 31" in eng._lib.gpf_last_error()
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_opponent(**GOOD)
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_alerts()
    with pytest.raises(GridPFError, match=r"\(active_alert\): source range \[0, 4\) is outside the 3 elements"):
        eng.set_obs_spec(ObsSpec(m, ["active_alert"], dim_alerts=4))
    with pytest.raises(GridPFError, match="header-only handle"):        # a good spec gets as far as the missing device
        eng.set_obs_spec(ObsSpec(m, ["active_alert", "total_number_of_alert"], dim_alerts=3))
    eng.close()


def test_obs_spec_layout_with_dim_alerts_equals_the_recorded_vector(recorded, load_model):
    from grid2op_amd.obs_spec import GO_KEEP, GO_MINUS1, GO_ZERO, KIND, ObsSpec
    fx = recorded
    m = load_model(str(fx["grid"]))
    A = len(fx["lines"])
    sp = ObsSpec.complete(m, fill=True, dim_alerts=A)
    assert sp.dim == fx["vect"].shape[0] == int(fx["vect_sizes"].sum()) and len(sp.segments) <= 64
    off = 0
    for name, size in zip(fx["vect_names"], fx["vect_sizes"]):
        if str(name) in sp.offsets:
            assert sp.offsets[str(name)] == slice(off, off + int(size)), name
        off += int(size)
    i = int(fx["vect_launch"])
    for k in AR.OBS_ATTRS:
        assert k in sp.offsets and np.array_equal(fx["vect"][sp.offsets[k]], np.asarray(fx["obs_" + k][i], np.float32).reshape(-1)), k
    assert sp.offsets["total_number_of_alert"].stop - sp.offsets["total_number_of_alert"].start == 1
    go = {str(n): int(s[4]) & 3 for n, s in zip(sp.names, sp.segments)}
    kinds = {str(n): int(s[0]) for n, s in zip(sp.names, sp.segments)}
    assert [go[k] for k in AR.OBS_ATTRS] == [GO_ZERO, GO_ZERO, GO_ZERO, GO_ZERO, GO_MINUS1, GO_KEEP, GO_KEEP]
    assert [kinds[k] for k in AR.OBS_ATTRS] == [KIND[k] for k in AR.OBS_ATTRS] == list(range(24, 31))


def test_obs_spec_without_the_keyword_is_what_it_was(load_model):
    from grid2op_amd.obs_spec import ObsSpec
    for name in ("l2rpn_wcci_2022_dev", "l2rpn_idf_2023"):
        m = load_model(name)
        old, new = ObsSpec.complete(m, fill=True), ObsSpec.complete(m, fill=True, dim_alerts=22)
        assert len(old.segments) == 51 and len(new.segments) == 58 <= 64 and new.dim == old.dim + 6 * 22 + 1     # the complete layout still fits
        assert not set(AR.OBS_ATTRS) & set(old.names) and old.dim_alerts == 0
        assert np.array_equal(ObsSpec.complete(m, fill=True, dim_alerts=0).segments, old.segments)
        for k in AR.OBS_ATTRS:
            with pytest.raises(ValueError, match="not assembled by the engine \\(a feature it does not model\\)"):
                ObsSpec(m, ["rho", k])
        with pytest.raises(ValueError, match="dim_alerts 65 is outside"):
            ObsSpec(m, ["rho"], dim_alerts=65)


def test_alert_config_and_exported_symbols():
    from grid2op_amd import _capi, engine
    names = ("gpf_set_alerts", "gpf_set_lane_alerts", "gpf_alerts_on_device", "gpf_alert_state_ints", "gpf_get_alert_state", "gpf_set_alert_state",
             "gpf_get_alert_reward", "gpf_alert_device_pointers")
    assert all(n in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), n) for n in names)
    assert _capi.ABI_VERSION == 326 and _capi.N_DEVICE_POINTERS == 34 and _capi.N_ALERT_POINTERS == 3
    assert engine.alert_config() == dict(time_window=12, reward_min_no_blackout=-1.0, reward_min_blackout=-10.0, reward_max_no_blackout=1.0,
                                         reward_max_blackout=2.0)

    class P:
        ALERT_TIME_WINDOW = 4
    assert engine.alert_config(P(), reward_max_blackout=3)["time_window"] == 4 and engine.alert_config(dict(ALERT_TIME_WINDOW=7))["time_window"] == 7
    for bad in (0, 63):
        with pytest.raises(ValueError, match="ALERT_TIME_WINDOW"):
            engine.alert_config(dict(ALERT_TIME_WINDOW=bad))


def test_sharded_engine_forwards_the_alerts(load_model):
    from stub_engine import StubEngine
    from grid2op_amd.sharding import ShardedEngine

    class Stub(StubEngine):
        def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
            super().__init__(model, n_lanes, device, n_busbar)
            self.calls, self.n_lanes_ = [], n_lanes

        def set_alerts(self, time_window=12, **constants):
            self.calls.append(("alerts", time_window, constants))

        def set_lane_alerts(self, alerts):
            self.calls.append(("lane", None if alerts is None else np.array(alerts)))

        def alerts_on_device(self, on=True):
            self.calls.append(("device", on))

        def alert_state(self, lane0=0, n=None):
            n = self.n_lanes_ - lane0 if n is None else n
            return np.tile((1000 * self.device + lane0 + np.arange(n))[:, None], (1, 4)).astype(np.int32)

        def set_alert_state(self, rows, lane0=0):
            self.calls.append(("state", lane0, np.array(rows)))

        def alert_reward(self, lane0=0, n=None):
            n = self.n_lanes_ - lane0 if n is None else n
            return (1000 * self.device + lane0 + np.arange(n)).astype(np.float32)

    m = load_model("l2rpn_case14_sandbox")
    se = ShardedEngine(m, 10, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: Stub(mm, n, dev, nbb))
    se.set_alerts(4, reward_max_blackout=3.0)
    assert all(e.calls[-1] == ("alerts", 4, dict(reward_max_blackout=3.0)) for e in se.engines)
    masks = np.arange(10, dtype=np.uint64)
    se.set_lane_alerts(masks)
    for e, (b0, bn) in zip(se.engines, se.blocks):
        assert np.array_equal(e.calls[-1][1], masks[b0:b0 + bn])
    se.set_lane_alerts(None)
    assert all(e.calls[-1][1] is None for e in se.engines)
    se.alerts_on_device()
    assert all(e.calls[-1] == ("device", True) for e in se.engines)
    want = np.concatenate([1000 * e.device + np.arange(bn) for e, (_, bn) in zip(se.engines, se.blocks)])
    assert np.array_equal(se.alert_state(2, 7)[:, 0], want[2:9]) and np.array_equal(se.alert_reward(1, 8), want[1:9].astype(np.float32))
    rows = np.tile(np.arange(10)[:, None], (1, 4))
    se.set_alert_state(rows)
    for e, (b0, bn) in zip(se.engines, se.blocks):
        tag, lane0, r = e.calls[-1]
        assert tag == "state" and lane0 == 0 and np.array_equal(r[:, 0], np.arange(b0, b0 + bn))


def test_sanitized_stand_alone_alert_emulator_runs_clean():
    p = subprocess.run([AR.sanitized_program()], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK") and not p.stderr, (p.stdout, p.stderr[-2000:])
