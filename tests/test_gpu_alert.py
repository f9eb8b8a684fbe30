"""Alerts and AlertReward of the batched acting path on the device (include/gridpf.h gpf_set_alerts, grid2op_amd/csrc/gridpf_alert.hpp
alert_prestep_kernel / alert_poststep_kernel): the episodes recorded from the unmodified reference environment replayed launch by launch
(tests/golden/alert_*.npz), the kernels against the Python restatement (tests/alert_ref.py) fed with the device's own attacks and game
overs at the edge sizes, masks written on the device, state round trips, copy / reset, sharding, and alerts that change nothing else."""
import numpy as np
import pytest

import alert_ref as AR
import opponent_ref as R
from conftest import golden_path

pytestmark = pytest.mark.gpu

STEP = dict(cascade=False, nb_ts_reco=10, auto_reset=True)
GEO = dict(kind=R.GEOMETRIC, attack_hazard_rate=0.3, recovery_rate=0.5, recovery_minimum_duration=1, pmax_pmin_ratio=4.0, episode_max_time=100,
           schedule_cap=6, init_budget=3.0, budget_per_ts=0.7, attack_duration=3, draw_source=R.PHILOX)
BAD_EVERY, BAD_AT, BAD_SCALE = 29, 17, 40.0


def _engine(name, n, offsets, bad_rows=False, factory=None):
    """an engine on the golden chronics; bad_rows: every 29th row asks for 40 times the load, which no power flow serves -- the lane
    that reads it is game over at that step (known beforehand from its offset: `_bad_steps`)"""
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path(f"{name}.grid.npz"))
    ch = dict(np.load(golden_path(f"{name}.chronics.npz")))
    if "prod_v" not in ch:
        ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
    if bad_rows:
        for k in ("load_p", "load_q"):
            ch[k] = ch[k].copy()
            ch[k][BAD_AT::BAD_EVERY] *= BAD_SCALE
    eng = factory(m, n) if factory else PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    eng.set_lane_chronics(lane_offset=offsets)
    eng.set_thermal_limits(ch["thermal_limits"])
    return m, eng, ch["load_p"].shape[0]


def _bad_steps(offsets, T, steps):
    t = np.arange(steps)[:, None]
    return ((t + np.asarray(offsets)[None, :]) % T) % BAD_EVERY == BAD_AT        # [steps, lanes]


def _alertable(eng_lines, area_of_line):
    """the alertable list: the opponent's lines, grouped by area in descriptor order"""
    if area_of_line is None:
        return [int(x) for x in eng_lines]
    return [int(l) for a in range(int(max(area_of_line)) + 1) for l, q in zip(eng_lines, area_of_line) if q == a]


@pytest.mark.parametrize("tag", ["wcci118", "case14"])
def test_replay_of_the_recorded_episodes(tag):
    """every launch of the recorded run on 3 lanes (the replay of tests/test_gpu_opponent_area.py with the alerts on top): state rows,
    reward and the seven attributes of the observation vector equal the recording, game-over launches included"""
    from grid2op_amd.chronics import chronics_table
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from grid2op_amd.obs_spec import ObsSpec
    from test_opponent_area_cpu import fixture_config
    fx = dict(np.load(golden_path(f"alert_{tag}.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    n, A = 3, len(fx["lines"])
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    tab = chronics_table({k[len("chron_"):]: fx[k] for k in fx if k.startswith("chron_")})
    eng.upload_chronics(tab)
    T = tab.shape[1]
    eng.set_thermal_limits(fx["thermal_limit"])
    p = [int(x) for x in fx["params"]]
    eng.set_topo_rules(legal_rules=True, max_sub_changed=p[0], max_line_status_changed=p[1], cooldown_sub=p[2], cooldown_line=p[3])
    acts = []
    for l in range(m.n_line):                      # entry 2 l: reconnect line l, entry 2 l + 1: open it
        acts += [{"set_line_status": [(l, 1)]}, {"set_line_status": [(l, -1)]}]
    assert not eng.upload_topo_actions(acts).any()
    cfg, aol = fixture_config(fx)
    eng.set_opponent(R.GEOMETRIC, **cfg)
    eng.set_opponent_areas(aol)
    eng.upload_opponent_draws(np.tile(fx["draws"], (n, 1)))
    c = [float(x) for x in fx["reward_constants"]]
    eng.set_alerts(int(fx["time_window"]), c[0], c[1], c[2], c[3])
    spec = ObsSpec(m, list(AR.OBS_ATTRS), dim_alerts=A)
    eng.set_obs_spec(spec)
    used = [int(x) for x in fx["scenarios_used"]]
    where, resets, scored, game_over = None, 0, 0, 0
    for i in range(len(fx["is_reset"])):
        want = (used.index(int(fx["scenario"][i])), (int(fx["row"][i]) - i) % T)
        if want != where:
            eng.set_lane_chronics(lane_table=np.full(n, want[0]), lane_offset=np.full(n, want[1]))
            where = want
        if fx["is_reset"][i]:
            eng.upload_opponent_area_schedule(fx["schedule"][resets], fx["schedule_count"][resets])
            resets += 1
            assert (eng.episode()[1] == 0).all(), i
        a = int(fx["agent_line"][i])
        eng.set_lane_topo_actions(None if a < 0 else np.full(n, 2 * a + (0 if fx["agent_value"][i] > 0 else 1)))
        eng.set_lane_alerts(np.tile(fx["alert_mask"][i], (n, 1)) if fx["alert_mask"][i].any() or i % 2 else None)
        eng.step(i, cascade=False, nb_ts_reco=p[4], auto_reset=True)
        # what the alerts take as input is what was recorded ...
        assert (eng.opponent_attack_lines() == fx["info_lines"][i]).all(), i
        assert (eng.episode()[0] == bool(fx["done"][i])).all(), i
        if a >= 0:
            assert (eng.topo_action_flags()[0] == bool(fx["is_illegal"][i])).all(), i
        # ... and so is what they make of it
        rows, want_row = eng.alert_state(), AR.fixture_row(fx, i)
        assert (rows == want_row).all(), (i, np.argwhere(rows != want_row)[:6])
        rew = eng.alert_reward()
        assert rew.tobytes() == np.full(n, fx["alert_reward"][i], np.float32).tobytes(), (i, rew, fx["alert_reward"][i])
        vec = eng.observation_vector_host()
        for k in AR.OBS_ATTRS:
            # (a game-over observation of the reference leaves attack_under_alert uninitialised, baseObservation.py:1687: the environment's value)
            rec = fx["env_attack_under_alert"][i] if fx["done"][i] and k == "attack_under_alert" else fx["obs_" + k][i]
            assert (vec[:, spec.offsets[k]] == np.asarray(rec, np.float32).reshape(1, -1)).all(), (i, k, vec[:, spec.offsets[k]], rec)
        scored += int(fx["alert_reward"][i] != 0)
        game_over += int(fx["done"][i])
    assert scored >= 10 and resets == 1 + game_over and game_over == int(fx["done"].sum())
    eng.close()


def _device_masks(eng, masks, A, rng):
    """the masks through the device buffer, with bits at or above A set at random: outside the feature's domain, dropped by the kernel"""
    import torch
    v = eng.device_views()
    junk = (rng.integers(0, 2 ** 62, len(masks), dtype=np.uint64) << np.uint64(A)) if A < 64 else np.zeros(len(masks), np.uint64)
    with torch.cuda.stream(v["stream"]):
        v["act_alert"].copy_(torch.from_numpy((masks | junk).view(np.int64)).to(v["act_alert"].device))
    v["stream"].synchronize()
    eng.alerts_on_device(True)


SHAPES = [("l2rpn_case14_sandbox", [7], None, 62),                                         # A = 1, the largest window
          ("l2rpn_wcci_2022_dev", 22, np.repeat([0, 1, 2], [6, 10, 6]), 12),               # idf's shape: 22 lines in three areas
          ("l2rpn_wcci_2022_dev", 64, np.arange(64) % 16, 1),                              # A = 64 (bit 63 in every mask), a ring of three rows
          ("l2rpn_case14_sandbox", 20, np.arange(20) % 5, 4)]


@pytest.mark.parametrize("name,lines,aol,W", SHAPES, ids=["A1_W62", "A22_3areas_W12", "A64_W1", "A20_W4"])
def test_device_equals_restatement_on_its_own_attacks_and_game_overs(name, lines, aol, W):
    """65 lanes (one past a block of four wavefronts and past a wavefront's worth) x 60 steps: a Philox Geometric opponent attacks, every
    29th chronics row is unservable (game over, then the reset launch under auto_reset), the alerts are random; the restatement gets the
    device's own attack vector, done flags and steps survived.  Odd steps hand the masks over from the host, even steps write them on
    the device: both must give what the restatement gives."""
    n, steps = 65, 60
    offsets = 3 * np.arange(n)
    m, eng, T = _engine(name, n, offsets, bad_rows=True)
    rng = np.random.default_rng(7 + W)
    if isinstance(lines, int):
        lines = [int(x) for x in rng.permutation(m.n_line)[:lines]]
    A = len(lines)
    bad = _bad_steps(offsets, T, steps)
    assert bad.sum() >= n and (bad.sum(axis=0) >= 1).all()             # chosen beforehand: every lane meets an unservable row
    cfg = dict(GEO, lines=lines, attack_cooldown=0 if aol is not None else 1, seed=0xA1E47 + A)
    eng.set_opponent(**cfg)
    if aol is not None:
        eng.set_opponent_areas(aol)
    order = _alertable(lines, aol)
    consts = (-1.0, -10.0, 1.0, 2.0) if W != 4 else (-0.5, -3.0, 0.25, 7.0)
    eng.set_alerts(W, *consts)
    refs = [AR.AlertRef(A, W, consts) for _ in range(n)]
    seen = dict(attacked=0, game_over=0, scored=0, blackout_scored=0, reset_launches=0)
    for t in range(steps):
        done0, survived, _ = eng.episode()
        raise_ = rng.random((n, A)) < 0.35
        if A == 64:
            raise_[:, 63] = True
        masks = np.array([AR.mask_of(x) for x in raise_], np.uint64)
        if t % 2:
            eng.set_lane_alerts(masks)
        else:
            _device_masks(eng, masks, A, rng)
        eng.step(t, **STEP)
        att = eng.opponent_attack_lines()[:, order]
        done1 = eng.episode()[0]
        assert done1[bad[t]].all(), (t, np.flatnonzero(bad[t] & ~done1))      # (an attack may end an episode too)
        for k in range(n):
            refs[k].prestep(int(survived[k]), bool(done0[k]), raise_[k], att[k])
            refs[k].poststep(bool(done1[k]))
        rows, want = eng.alert_state(), np.array([r.row() for r in refs])
        assert np.array_equal(rows, want), (t, np.argwhere(rows != want)[:6])
        rew = eng.alert_reward()
        assert rew.tobytes() == np.array([r.reward for r in refs], np.float32).tobytes(), t
        ran = np.array([r.ran for r in refs])
        seen["attacked"] += int((att.any(axis=1) & ran).sum())
        seen["game_over"] += int((done1 & ran).sum())
        seen["scored"] += int((ran & ~done1 & (rew != 0)).sum())
        seen["blackout_scored"] += int((ran & done1 & (rew != 0)).sum())
        seen["reset_launches"] += int((survived == 0).sum())
    print(name, A, W, seen)
    assert seen["attacked"] >= n and seen["game_over"] >= n // 2 and seen["reset_launches"] >= n + n // 2, seen
    assert seen["blackout_scored"] >= 1 and (W > 12 or seen["scored"] >= 10), seen
    eng.close()


def test_state_round_trip_copy_reset_and_views():
    from grid2op_amd.engine import GridPFError
    n, A, W = 8, 5, 3
    m, eng, _ = _engine("l2rpn_case14_sandbox", n, np.arange(n))
    keys_off = set(eng.device_views())
    eng.set_opponent(**dict(GEO, lines=[0, 3, 7, 11, 15], attack_cooldown=1, seed=11))
    with pytest.raises(GridPFError, match="alerts are off"):
        eng.alert_state()
    eng.set_alerts(W)
    v = eng.device_views()
    assert set(v) - keys_off == {"act_alert", "alert_reward", "alert_obs"}
    assert tuple(v["act_alert"].shape) == (n,) and tuple(v["alert_reward"].shape) == (n,) and tuple(v["alert_obs"].shape) == (n, 6 * A + 1)
    rows = eng.alert_state()
    fresh = AR.AlertRef(A, W).row()
    assert rows.shape == (n, AR.state_ints(A, W)) and (rows == fresh).all()
    rng = np.random.default_rng(3)
    for t in range(2):                               # (past the reset launch: the lanes have completed steps)
        eng.step(t, **STEP)
    assert (eng.episode()[1] > 0).all()
    refs = [AR.AlertRef(A, W) for _ in range(n)]
    for r in refs:                                   # arbitrary states
        r.last_alert, r.is_already_attacked = rng.random(A) < 0.5, rng.random(A) < 0.5
        r.time_since_last_alert, r.alert_duration = rng.integers(-1, 9, A).astype(np.int32), rng.integers(0, 9, A).astype(np.int32)
        r.time_since_last_attack, r.attack_under_alert = rng.integers(-1, 9, A).astype(np.int32), rng.integers(-1, 2, A).astype(np.int32)
        r.was_alert_used_after_attack, r.total_number_of_alert = rng.integers(-1, 2, A).astype(np.int32), int(rng.integers(0, 99))
        r.current_id, r.ran = int(rng.integers(0, W + 2)), bool(rng.integers(0, 2))
        r.currently_attacked, r.ts_attack, r.alert_launched = rng.random(A) < 0.5, rng.random((W + 2, A)) < 0.3, rng.random((W + 2, A)) < 0.5
    want = np.array([r.row() for r in refs])
    eng.set_alert_state(want)
    assert np.array_equal(eng.alert_state(), want)
    f = eng.alert_state_fields(eng.alert_state())
    assert np.array_equal(f["ts_attack"][2], refs[2].ts_attack) and f["current_id"][5] == refs[5].current_id
    obs = v["alert_obs"].cpu().numpy()
    assert np.array_equal(obs[:, 3 * A:4 * A], want[:, 4 * A:5 * A]) and np.array_equal(obs[:, 6 * A], want[:, 7 * A])      # the time_since_last_attack section, the total
    eng.copy_lanes(0, 4, 3)
    got = eng.alert_state()
    assert np.array_equal(got[4:7], want[0:3]) and np.array_equal(got[7], want[7]) and np.array_equal(got[:4], want[:4])
    # ... and the lanes go on from the written state as the restatement does
    eng.set_alert_state(want)
    for t in range(2, 8):
        done0, survived, _ = eng.episode()
        raise_ = rng.random((n, A)) < 0.4
        eng.set_lane_alerts(raise_)
        eng.step(t, **STEP)
        att, done1 = eng.opponent_attack_lines()[:, [0, 3, 7, 11, 15]], eng.episode()[0]
        for k in range(n):
            refs[k].prestep(int(survived[k]), bool(done0[k]), raise_[k], att[k])
            refs[k].poststep(bool(done1[k]))
        assert np.array_equal(eng.alert_state(), np.array([r.row() for r in refs])), t
        assert eng.alert_reward().tobytes() == np.array([r.reward for r in refs], np.float32).tobytes(), t
    eng.reset(2, 3)
    got = eng.alert_state()
    assert (got[2:5] == fresh).all() and np.array_equal(got[5], refs[5].row()) and (eng.alert_reward(2, 3) == 0).all()
    for col, value, reason in ((0, 2, "last_alert is not 0 / 1"), (2 * A, -2, "below -1"), (3 * A, -1, "negative alert_duration"),
                               (5 * A, 2, r"outside \{-1, 0, 1\}"), (7 * A + 1, W + 2, "_current_id is outside"), (8 * A + 3, 3, "is not 0 / 1")):
        bad = want[:1].copy()
        bad[0, col] = value
        with pytest.raises(GridPFError, match=reason):
            eng.set_alert_state(bad)
    with pytest.raises(GridPFError, match="at or above the 5 alertable lines"):
        eng.set_lane_alerts(np.full(n, 1 << 5, np.uint64))
    eng.set_opponent(**dict(GEO, lines=[1, 2], attack_cooldown=1, seed=1))        # a new opponent: alerts off, the views as before
    assert set(eng.device_views()) == keys_off
    with pytest.raises(GridPFError, match="alerts are off"):
        eng.alert_reward()
    eng.close()


def test_two_shards_equal_one_engine():
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.sharding import ShardedEngine
    n, steps, W = 64, 25, 2
    offsets = 2 * np.arange(n)
    m, one, _ = _engine("l2rpn_case14_sandbox", n, offsets, bad_rows=True)
    _, two, _ = _engine("l2rpn_case14_sandbox", n, offsets, bad_rows=True, factory=lambda mm, nn: ShardedEngine(
        mm, nn, devices=[0, 0], engine_factory=lambda m_, n_, dev, nbb: PowerFlowEngine(m_, n_lanes=n_, device=0, n_busbar=nbb)))
    cfg = dict(GEO, lines=[0, 2, 4, 9, 13, 17], attack_cooldown=0, seed=77)
    for eng in (one, two):
        eng.set_opponent(**cfg)
        eng.set_opponent_areas([0, 0, 0, 1, 1, 2])
        eng.set_alerts(W)
    rng = np.random.default_rng(12)
    scored = 0
    for t in range(steps):
        raise_ = rng.random((n, 6)) < 0.4
        for eng in (one, two):
            eng.set_lane_alerts(raise_)
            eng.step(t, **STEP)
        assert np.array_equal(one.alert_state(), two.alert_state()), t
        ra, rb = one.alert_reward(), two.alert_reward()
        assert ra.tobytes() == rb.tobytes(), t
        scored += int((ra != 0).sum())
    assert scored > n
    one.close()
    two.close()


def test_alerts_change_nothing_else():
    """the same run with alerts on and off: byte-identical results, step outputs, opponent state, cooldowns, episodes and step counters"""
    n = 16
    m, a, _ = _engine("l2rpn_case14_sandbox", n, np.arange(n), bad_rows=True)
    _, b, _ = _engine("l2rpn_case14_sandbox", n, np.arange(n), bad_rows=True)
    cfg = dict(GEO, lines=[1, 2, 3, 8, 12], attack_cooldown=0, seed=5)
    for eng in (a, b):
        eng.set_opponent(**cfg)
        eng.set_opponent_areas([0, 0, 1, 1, 2])
    views_off = set(b.device_views())
    a.set_alerts(3)
    rng = np.random.default_rng(1)
    for t in range(30):
        a.set_lane_alerts(rng.random((n, 5)) < 0.5)
        a.step(t, **STEP)
        b.step(t, **STEP)
        sa, sb = a.opponent_state(), b.opponent_state()
        assert np.array_equal(sa.rows(), sb.rows()) and np.array_equal(sa.budget, sb.budget), t
        assert np.array_equal(a.opponent_area_state().rows(), b.opponent_area_state().rows()), t
        for x, y in zip(a.step_outputs(), b.step_outputs()):
            assert np.array_equal(x, y, equal_nan=True), t
        assert np.array_equal(a.cooldown(), b.cooldown()), t
    ra, rb = a.results(), b.results()
    for f in ("out", "topo_vect", "shunt_bus", "line_status", "status", "bus_vm", "bus_va"):
        assert np.array_equal(getattr(ra, f), getattr(rb, f), equal_nan=True), f
    assert all(np.array_equal(x, y) for x, y in zip(a.episode(), b.episode())) and a.episode()[2].sum() > 0
    assert a.counters() == b.counters()                                # the step's own dispatches: the same launches
    assert (a.alert_state()[:, 7 * 5] > 0).any() and set(b.device_views()) == views_off
    a.set_alerts(None)                                                 # off again: the views and the launches are what they were
    assert set(a.device_views()) == views_off
    a.step(30, **STEP)
    b.step(30, **STEP)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a.step_outputs(), b.step_outputs()))
    a.close()
    b.close()
