"""The opponent of the batched acting path on the device (include/gridpf.h gpf_set_opponent, grid2op_amd/csrc/gridpf_opponent.hpp):
episodes recorded from the unmodified reference replayed launch by launch (tests/golden/opponent_*.npz), the kernel against the Python
restatement (tests/opponent_ref.py) on states nobody recorded, state round trips, the refusals, sharding, and off means off."""
import numpy as np
import pytest

import opponent_ref as R
from conftest import golden_path

pytestmark = pytest.mark.gpu

STEP = dict(cascade=False, nb_ts_reco=10, auto_reset=True)


def _engine(name, n, offsets, factory=None):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path(f"{name}.grid.npz"))
    ch = dict(np.load(golden_path(f"{name}.chronics.npz")))
    if "prod_v" not in ch:
        ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
    eng = factory(m, n) if factory else PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    eng.set_lane_chronics(lane_offset=offsets)
    eng.set_thermal_limits(ch["thermal_limits"])
    return m, eng


@pytest.mark.parametrize("tag", ["neurips36", "wcci118", "case14"])
def test_replay_of_the_recorded_episodes(tag):
    """every launch of the recorded run on 3 lanes: table source, the agent's actions through an uploaded table, one launch per env.step
    and one per env.reset() (the game over of the case14 run restarts its lanes with a reset opponent under auto_reset)"""
    from grid2op_amd.chronics import chronics_table
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from test_opponent_cpu import COLS, STATE_KEYS, fixture_config
    fx = dict(np.load(golden_path(f"opponent_{tag}.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    n = 3
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
    cfg = fixture_config(fx)
    eng.set_opponent(**cfg)
    eng.upload_opponent_draws(np.tile(fx["draws"], (n, 1)))
    used = [int(x) for x in fx["scenarios_used"]]
    where, resets, attacked_steps, worst_rho = None, 0, 0, 0.0
    for i in range(len(fx["is_reset"])):
        want = (used.index(int(fx["scenario"][i])), (int(fx["row"][i]) - i) % T)
        if want != where:
            eng.set_lane_chronics(lane_table=np.full(n, want[0]), lane_offset=np.full(n, want[1]))
            where = want
        if fx["is_reset"][i]:
            if cfg["kind"] == R.GEOMETRIC:
                k = int(fx["schedule_count"][resets])
                eng.upload_opponent_schedule(np.tile(fx["schedule"][resets, :k], (n, 1, 1)), k)
            resets += 1
            assert (eng.episode()[1] == 0).all(), i
        a = int(fx["agent_line"][i])
        eng.set_lane_topo_actions(None if a < 0 else np.full(n, 2 * a + (0 if fx["agent_value"][i] > 0 else 1)))
        eng.step(i, cascade=False, nb_ts_reco=p[4], auto_reset=True)
        st = eng.opponent_state()
        rows = st.rows()
        for k in STATE_KEYS + ("n_draws", "info_line", "info_duration"):
            assert (rows[:, COLS[k]] == int(fx[k][i])).all(), (i, k, rows[:, COLS[k]], int(fx[k][i]))
        assert (st.budget == float(fx["budget"][i])).all(), (i, st.budget, float(fx["budget"][i]))
        failed = eng.episode()[0]
        assert (failed == bool(fx["done"][i])).all(), i
        if a >= 0:
            assert (eng.topo_action_flags()[0] == bool(fx["is_illegal"][i])).all(), i
        if not fx["done"][i]:
            assert (eng.results(with_bus=False).line_status == fx["line_status"][i]).all(), i
            assert (eng.cooldown() == fx["cooldown_line"][i]).all(), i
            worst_rho = max(worst_rho, float(np.abs(eng.step_outputs()[0] - fx["rho"][i]).max()))
        attacked_steps += int(fx["info_line"][i] >= 0)
    print(f"{tag}: max |rho - recorded rho| over the run = {worst_rho:.3e}")      # (reported, not a bar: the step's parity is pinned elsewhere)
    assert (st.flags == 0).all() and attacked_steps >= 20 and resets == 1 + int(fx["done"].sum())
    eng.close()


KINDS = {
    "random_line": dict(kind=R.RANDOM_LINE),
    "weighted_random": dict(kind=R.WEIGHTED_RANDOM, attack_period=3),
    "geometric": dict(kind=R.GEOMETRIC, attack_hazard_rate=0.3, recovery_rate=0.5, recovery_minimum_duration=1, pmax_pmin_ratio=4.0,
                      episode_max_time=100, schedule_cap=6),
}
SPACE = dict(init_budget=3.0, budget_per_ts=0.5, attack_duration=3, attack_cooldown=5)


def _config(m, kind_name, lines, seed, **extra):
    cfg = dict(KINDS[kind_name], lines=lines, draw_source=R.PHILOX, seed=seed, **SPACE)
    if kind_name == "weighted_random":
        cfg["rho_normalization"] = 0.5 + (np.arange(len(lines)) % 7) / 7.0
    cfg.update(extra)
    return cfg


def _refs(cfg, n, base=0):
    kw = {k: v for k, v in cfg.items() if k not in ("kind", "lines", "lane_base")}
    return [R.OpponentRef(cfg["kind"], cfg["lines"], global_lane=base + k, **kw) for k in range(n)]


def _run_against_restatement(eng, m, cfg, n, steps, refs=None, reconnect=True):
    """launch by launch: the restatement is fed the device's own rho / line status / episode counters of before the launch"""
    refs = refs or _refs(cfg, n)
    lo, le = np.asarray(m.line_or_pos_topo_vect), np.asarray(m.line_ex_pos_topo_vect)
    attacks = 0
    for t in range(steps):
        rho = eng.step_outputs()[0]
        status = eng.results(with_bus=False).line_status
        done, survived, _ = eng.episode()
        cd0 = eng.cooldown()
        want = [refs[k].prestep(int(survived[k]), bool(done[k]), rho[k], status[k]) for k in range(n)]
        eng.step(t, **STEP)
        st = eng.opponent_state()
        rows = np.array([r.row() for r in refs], dtype=np.int32)
        assert np.array_equal(st.rows()[:, :13], rows[:, :13]), (t, np.argwhere(st.rows()[:, :13] != rows[:, :13])[:5])
        assert np.array_equal(st.budget, np.array([float(r.budget) for r in refs])), t
        failed, _, _ = eng.episode()
        ls, cd1 = eng.results(with_bus=False).line_status, eng.cooldown()
        for k, (line, dur) in enumerate(want):
            assert st.opponent_attack_line[k] == line and st.opponent_attack_duration[k] == dur
            if line >= 0 and survived[k] > 0 and not done[k] and not failed[k]:
                attacks += 1
                assert not ls[k, line] and cd1[k, line] == max(cd0[k, line], dur) - 1, (t, k)
        if reconnect:                          # a host agent: every line whose cooldown ran out goes back in
            topo = eng.get_topology()[0]
            back = (cd1 == 0) & ((topo[:, lo] < 0) | (topo[:, le] < 0))
            if back.any():
                kk, ll = np.nonzero(back)
                topo[kk, lo[ll]] = 1
                topo[kk, le[ll]] = 1
                eng.set_topology(topo)
    return refs, attacks


@pytest.mark.parametrize("kind_name", list(KINDS))
@pytest.mark.parametrize("name,one_line", [("l2rpn_wcci_2022_dev", False), ("l2rpn_case14_sandbox", True)])
def test_device_equals_restatement_on_its_own_observations(name, one_line, kind_name):
    """65 lanes x 40 steps, Philox source: all 186 lines of the 118-substation grid attackable (three strides of the wavefront), or exactly
    one line of the 14-substation grid (the Geometric opponent then never draws a line)"""
    n, steps = 65, 40
    m, eng = _engine(name, n, 3 * np.arange(n))
    lines = [3] if one_line else list(np.random.default_rng(5).permutation(m.n_line))
    cfg = _config(m, kind_name, lines, seed=0x5EED0000ABCD + len(lines))
    eng.set_opponent(**cfg)
    refs, attacks = _run_against_restatement(eng, m, cfg, n, steps)
    # the fixed seed keeps every u away from a decision boundary (the device sums in another order than numpy)
    assert min(r.margin for r in refs) > 1e-9
    assert attacks >= n, attacks
    if kind_name == "geometric":
        assert any(r.flags & R.FLAG_SCHEDULE_CAPPED for r in refs) and all(len(r.waits) <= 6 for r in refs)
    eng.close()


def test_state_round_trip_and_copy_lanes():
    from grid2op_amd.engine import OPP_TIME_NONE
    n = 8
    m, eng = _engine("l2rpn_case14_sandbox", n, np.arange(n))
    cfg = _config(m, "weighted_random", [0, 3, 7, 11, 15], seed=11)
    eng.set_opponent(**cfg)
    for t in range(3):
        eng.step(t, **STEP)
    st = eng.opponent_state()
    assert (st.episode == 1).all() and (st.next_attack_time != OPP_TIME_NONE).any()
    st.budget[:] = np.linspace(0.25, 9.0, n)
    st.budget_is_f32[:] = [0, 1] * (n // 2)
    st.attack_duration[:], st.attack_cooldown[:], st.attack_line[:] = 2, np.arange(n), [-1, 0, 3, 7, 11, 15, 19, 2]
    st.previous_fails[:], st.next_attack_time[:], st.cursor[:] = 1, [OPP_TIME_NONE, -3, 0, 1, 2, 3, 4, 5], 100 + np.arange(n)
    eng.set_opponent_state(st)
    got = eng.opponent_state()
    assert np.array_equal(got.rows(), st.rows()) and np.array_equal(got.budget, st.budget)
    eng.copy_lanes(0, 4, 3)
    got = eng.opponent_state()
    assert np.array_equal(got.rows()[4:7], st.rows()[0:3]) and np.array_equal(got.budget[4:7], st.budget[0:3])
    assert np.array_equal(got.rows()[7], st.rows()[7])
    # ... and the copied lanes go on as their sources do (same state, same observation; other Philox lane: decisions that draw may differ)
    refs = _refs(cfg, n)
    for k in range(n):
        refs[k].set_row(got.budget[k], got.rows()[k])
    _run_against_restatement(eng, m, cfg, n, 6, refs=refs)
    with pytest.raises(Exception, match="outside"):
        st.attack_line[0] = m.n_line
        eng.set_opponent_state(st)
    eng.close()


def test_refusals():
    from grid2op_amd.engine import GridPFError
    m, eng = _engine("l2rpn_case14_sandbox", 4, np.arange(4))
    eng.set_opponent(**_config(m, "random_line", [1, 2], seed=1))
    with pytest.raises(GridPFError, match="one-step launch"):
        eng.step(0, n_steps=2, nb_ts_reco=10)
    with pytest.raises(GridPFError, match="track_cooldown"):
        eng.step(0, nb_ts_reco=-1)
    eng.step(0, **STEP)
    eng.set_opponent(None)
    eng.step(1, n_steps=2, nb_ts_reco=-1)                    # off: nothing to refuse
    with pytest.raises(GridPFError, match="no opponent"):
        eng.opponent_state()
    eng.close()


@pytest.mark.parametrize("kind_name", ["weighted_random", "geometric"])
def test_two_shards_draw_what_one_engine_draws(kind_name):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.sharding import ShardedEngine
    n, steps = 64, 25
    offsets = 2 * np.arange(n)
    m, one = _engine("l2rpn_case14_sandbox", n, offsets)
    _, two = _engine("l2rpn_case14_sandbox", n, offsets, factory=lambda mm, nn: ShardedEngine(
        mm, nn, devices=[0, 0], engine_factory=lambda m_, n_, dev, nbb: PowerFlowEngine(m_, n_lanes=n_, device=0, n_busbar=nbb)))
    cfg = _config(m, kind_name, [0, 2, 4, 9, 13, 17], seed=77)
    one.set_opponent(**cfg)
    two.set_opponent(**cfg)
    assert [e.n_lanes for e in two.engines] == [32, 32]
    seen = 0
    for t in range(steps):
        one.step(t, **STEP)
        two.step(t, **STEP)
        a, b = one.opponent_state(), two.opponent_state()
        assert np.array_equal(a.rows(), b.rows()) and np.array_equal(a.budget, b.budget), t
        seen += int((a.opponent_attack_line >= 0).sum())
    assert seen > n and len(set(one.opponent_state().cursor)) > 1
    assert np.array_equal(one.results(with_bus=False).line_status, two.results(with_bus=False).line_status)
    one.close()
    two.close()


def test_off_means_off():
    """after set_opponent(None) a one-step launch is bit-identical, in every result row, to the launch of an engine that never had one"""
    n = 16
    m, a = _engine("l2rpn_case14_sandbox", n, np.arange(n))
    _, b = _engine("l2rpn_case14_sandbox", n, np.arange(n))
    a.set_opponent(**_config(m, "random_line", [1, 2, 3], seed=5))
    a.set_opponent(None)
    for t in range(3):
        a.step(t, **STEP)
        b.step(t, **STEP)
    ra, rb = a.results(), b.results()
    for f in ("out", "topo_vect", "shunt_bus", "line_status", "status", "bus_vm", "bus_va"):
        assert np.array_equal(getattr(ra, f), getattr(rb, f), equal_nan=True), f
    for x, y in zip(a.step_outputs(), b.step_outputs()):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(a.cooldown(), b.cooldown()) and np.array_equal(a.get_topology()[0], b.get_topology()[0])
    assert all(np.array_equal(x, y) for x, y in zip(a.episode(), b.episode()))
    a.close()
    b.close()
