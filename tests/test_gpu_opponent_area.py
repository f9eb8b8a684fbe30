"""The multi-area opponent of the batched acting path on the device (include/gridpf.h gpf_set_opponent_areas,
grid2op_amd/csrc/gridpf_opponent.hpp opponent_area_prestep_kernel): episodes recorded from the unmodified reference's
GeometricOpponentMultiArea replayed launch by launch (tests/golden/opponent_area_*.npz), the kernel against the Python restatement
(tests/opponent_area_ref.py) on states nobody recorded, state round trips, the launch-time refusals, sharding, and off means single-area."""
import numpy as np
import pytest

import opponent_area_ref as A
import opponent_ref as R
from conftest import golden_path

pytestmark = pytest.mark.gpu

STEP = dict(cascade=False, nb_ts_reco=10, auto_reset=True)
GEO = dict(kind=R.GEOMETRIC, attack_hazard_rate=0.3, recovery_rate=0.5, recovery_minimum_duration=1, pmax_pmin_ratio=4.0, episode_max_time=100,
           schedule_cap=6, init_budget=3.0, budget_per_ts=0.7, attack_duration=3, draw_source=R.PHILOX)


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


@pytest.mark.parametrize("tag", ["wcci118", "case14"])
def test_replay_of_the_recorded_episodes(tag):
    """every launch of the recorded run on 3 lanes: table source, the agent's actions through an uploaded table, one launch per env.step
    and one per env.reset() (the game over of the case14 run restarts its lanes with a reset opponent under auto_reset)"""
    from grid2op_amd.chronics import chronics_table
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from test_opponent_area_cpu import AREA_COLS, SPACE_COLS, area_info_lines, fixture_config
    fx = dict(np.load(golden_path(f"opponent_area_{tag}.npz")))
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
    cfg, aol = fixture_config(fx)
    eng.set_opponent(R.GEOMETRIC, **cfg)
    eng.set_opponent_areas(aol)
    eng.upload_opponent_draws(np.tile(fx["draws"], (n, 1)))
    used = [int(x) for x in fx["scenarios_used"]]
    where, resets, attacked_steps, worst_rho = None, 0, 0, 0.0
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
        eng.step(i, cascade=False, nb_ts_reco=p[4], auto_reset=True)
        st, ar = eng.opponent_state(), eng.opponent_area_state().rows()
        rows = st.rows()
        for k, col in SPACE_COLS.items():
            assert (rows[:, col] == int(fx[k][i])).all(), (i, k, rows[:, col], int(fx[k][i]))
        assert (st.budget == float(fx["budget"][i])).all(), (i, st.budget, float(fx["budget"][i]))
        for k, col in AREA_COLS.items():
            assert (ar[:, :, col] == fx[k][i]).all(), (i, k, ar[:, :, col], fx[k][i])
        assert (ar[:, :, A.A_N_SCHED] == fx["schedule_count"][resets - 1]).all() and (ar[:, :, 6:] == 0).all(), i
        assert (ar[:, :, A.A_INFO_LINE] == area_info_lines(fx, i)).all(), i
        assert (eng.opponent_attack_lines() == fx["info_lines"][i]).all(), i
        failed = eng.episode()[0]
        assert (failed == bool(fx["done"][i])).all(), i
        if a >= 0:
            assert (eng.topo_action_flags()[0] == bool(fx["is_illegal"][i])).all(), i
        if not fx["done"][i]:
            assert (eng.results(with_bus=False).line_status == fx["line_status"][i]).all(), i
            assert (eng.cooldown() == fx["cooldown_line"][i]).all(), i
            worst_rho = max(worst_rho, float(np.abs(eng.step_outputs()[0] - fx["rho"][i]).max()))
        attacked_steps += int(fx["info_lines"][i].any())
    print(f"{tag}: max |rho - recorded rho| over the run = {worst_rho:.3e}")      # (reported, not a bar: the step's parity is pinned elsewhere)
    assert (st.flags == 0).all() and attacked_steps >= 20 and resets == 1 + int(fx["done"].sum())
    eng.close()


def _refs(cfg, aol, n, base=0):
    kw = {k: v for k, v in cfg.items() if k not in ("kind", "lines", "lane_base")}
    return [A.OpponentAreaRef(cfg["lines"], aol, global_lane=base + k, **kw) for k in range(n)]


def _run_against_restatement(eng, m, refs, n, steps, reconnect=True):
    """launch by launch: the restatement is fed the device's own rho / line status / episode counters of before the launch"""
    lo, le = np.asarray(m.line_or_pos_topo_vect), np.asarray(m.line_ex_pos_topo_vect)
    attacks, several = 0, 0
    for t in range(steps):
        rho = eng.step_outputs()[0]
        status = eng.results(with_bus=False).line_status
        done, survived, _ = eng.episode()
        cd0 = eng.cooldown()
        want = [refs[k].prestep(int(survived[k]), bool(done[k]), rho[k], status[k]) for k in range(n)]
        eng.step(t, **STEP)
        st, ar = eng.opponent_state(), eng.opponent_area_state().rows()
        rows = np.array([r.row() for r in refs], dtype=np.int32)
        assert np.array_equal(st.rows()[:, :13], rows[:, :13]), (t, np.argwhere(st.rows()[:, :13] != rows[:, :13])[:5])
        area_rows = np.array([r.area_rows() for r in refs], dtype=np.int32)
        assert np.array_equal(ar, area_rows), (t, np.argwhere(ar != area_rows)[:5])
        assert np.array_equal(st.budget, np.array([float(r.budget) for r in refs])), t
        failed, _, _ = eng.episode()
        ls, cd1, al = eng.results(with_bus=False).line_status, eng.cooldown(), eng.opponent_attack_lines()
        for k, (out, dur) in enumerate(want):
            assert sorted(np.flatnonzero(al[k])) == out and st.opponent_attack_duration[k] == dur
            if out and survived[k] > 0 and not done[k] and not failed[k]:
                attacks += 1
                several += int(len(out) >= 2)
                for line in out:                   # every accepted line is out, its cooldown max(before, 1) - 1
                    assert not ls[k, line] and cd1[k, line] == max(cd0[k, line], 1) - 1, (t, k, line)
        if reconnect:                              # a host agent: every line whose cooldown ran out goes back in
            topo = eng.get_topology()[0]
            back = (cd1 == 0) & ((topo[:, lo] < 0) | (topo[:, le] < 0))
            if back.any():
                kk, ll = np.nonzero(back)
                topo[kk, lo[ll]] = 1
                topo[kk, le[ll]] = 1
                eng.set_topology(topo)
    return attacks, several


@pytest.mark.parametrize("name,cooldown", [("l2rpn_wcci_2022_dev", 0), ("l2rpn_case14_sandbox", 1)])
def test_device_equals_restatement_on_its_own_observations(name, cooldown):
    """65 lanes x 40 steps (blocks of 4 wavefronts and a ragged last block), Philox source: all 186 lines of the 118-substation grid,
    permuted, in areas of 120 / 65 / 1 (two strides of the wavefront, one stride plus one line, an area that never draws), or the 20 lines
    of the 14-substation grid in 16 areas"""
    n, steps = 65, 40
    m, eng = _engine(name, n, 3 * np.arange(n))
    rng = np.random.default_rng(5)
    lines = list(rng.permutation(m.n_line))
    aol = np.repeat([0, 1, 2], [120, 65, 1]) if m.n_line == 186 else np.arange(20) % 16
    assert len(aol) == m.n_line
    cfg = dict(GEO, lines=lines, attack_cooldown=cooldown, seed=0x5EED0000ABCD + m.n_line)
    eng.set_opponent(**cfg)
    eng.set_opponent_areas(aol)
    refs = _refs(cfg, aol, n)
    attacks, several = _run_against_restatement(eng, m, refs, n, steps)
    # the fixed seed keeps every u away from a decision boundary (the device sums in another order than numpy)
    assert min(r.margin for r in refs) > 1e-9
    assert attacks >= n and several >= 1, (attacks, several)
    assert all(len(s.waits) <= 6 for r in refs for s in r.areas)
    eng.close()


def test_area_state_round_trip_copy_lanes_and_continuation():
    from grid2op_amd.engine import OPP_TIME_NONE, GridPFError
    n = 8
    m, eng = _engine("l2rpn_case14_sandbox", n, np.arange(n))
    lines, aol = [0, 3, 7, 11, 15, 2], [0, 0, 1, 1, 1, 2]
    cfg = dict(GEO, lines=lines, attack_cooldown=1, seed=11)
    eng.set_opponent(**cfg)
    eng.set_opponent_areas(aol)
    for t in range(3):
        eng.step(t, **STEP)
    st, ar = eng.opponent_state(), eng.opponent_area_state()
    assert (st.episode == 1).all() and ar.counter.shape == (n, 3) and (ar.n_schedule > 0).all()
    ar.counter[:] = [[-1, 0, 2]] * n
    ar.line[:] = np.array([[0, 7, 2], [3, 11, -1], [-1, 15, 2], [3, -1, -1]] * 2)
    ar.next_attack_time[:] = [[OPP_TIME_NONE, -3, 2]] * n
    ar.attack_counter[:] = np.minimum(np.arange(n)[:, None] % 3, ar.n_schedule)
    ar.opponent_attack_line[:] = np.where(np.arange(n)[:, None] % 2 == 0, ar.line, -1)
    st.budget[:] = np.linspace(0.25, 9.0, n)
    st.budget_is_f32[:] = [0, 1] * (n // 2)
    st.attack_duration[:], st.attack_cooldown[:], st.previous_fails[:] = [0, 1] * (n // 2), [0, 1, 3, 1] * 2, [1, 0, 0, 1] * 2
    eng.set_opponent_state(st)
    eng.set_opponent_area_state(ar)
    got, gar = eng.opponent_state(), eng.opponent_area_state()
    assert np.array_equal(got.rows(), st.rows()) and np.array_equal(got.budget, st.budget) and np.array_equal(gar.rows(), ar.rows())
    assert np.array_equal(eng.opponent_attack_lines().sum(axis=1), (ar.opponent_attack_line >= 0).sum(axis=1))
    eng.copy_lanes(0, 4, 3)
    got, gar = eng.opponent_state(), eng.opponent_area_state()
    assert np.array_equal(gar.rows()[4:7], ar.rows()[0:3]) and np.array_equal(got.rows()[4:7], st.rows()[0:3]) and np.array_equal(gar.rows()[7], ar.rows()[7])
    # ... and the lanes go on from the written state as the restatement does: the schedules are those the kernel sampled at the reset,
    # which the restatement samples from the same stream (lanes 4-6 were copied from 0-2: their schedules too)
    refs = _refs(cfg, aol, n)
    for k, r in enumerate(refs):
        r.prestep(0, False, None, None)
    for k, r in enumerate(refs):
        src = refs[k - 4] if 4 <= k < 7 else r
        sched = [np.stack([s.waits, s.durs], axis=1).reshape(-1, 2) for s in src.areas]
        assert [len(s) for s in sched] == list(gar.n_schedule[k])
        r.set_rows(got.budget[k], got.rows()[k], gar.rows()[k], schedules=sched)
    _run_against_restatement(eng, m, refs, n, 8)
    with pytest.raises(GridPFError, match="outside the area's list"):
        ar.line[0, 0] = 7
        eng.set_opponent_area_state(ar)
    with pytest.raises(GridPFError, match="attack duration is 0 or 1"):
        st.attack_duration[0] = 2
        eng.set_opponent_state(st)
    eng.close()


def test_launch_time_refusals_with_areas_set():
    from grid2op_amd.engine import GridPFError
    m, eng = _engine("l2rpn_case14_sandbox", 4, np.arange(4))
    eng.set_opponent(**dict(GEO, lines=[1, 2, 5], attack_cooldown=0, seed=1))
    eng.set_opponent_areas([0, 1, 1])
    with pytest.raises(GridPFError, match="one-step launch"):
        eng.step(0, n_steps=2, nb_ts_reco=10)
    with pytest.raises(GridPFError, match="track_cooldown"):
        eng.step(0, nb_ts_reco=-1)
    eng.step(0, **STEP)
    assert eng.opponent_area_state().counter.shape == (4, 2)
    with pytest.raises(GridPFError, match="cannot be played"):
        eng.set_opponent(**dict(GEO, lines=[1, 2, 5], attack_cooldown=2, seed=1))
        eng.set_opponent_areas([0, 1, 1])
    eng.set_opponent(None)
    eng.step(1, n_steps=2, nb_ts_reco=-1)                    # off: nothing to refuse
    with pytest.raises(GridPFError, match="no areas"):
        eng.opponent_area_state()
    eng.close()


def test_two_shards_draw_what_one_engine_draws():
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.sharding import ShardedEngine
    n, steps = 64, 25
    offsets = 2 * np.arange(n)
    m, one = _engine("l2rpn_case14_sandbox", n, offsets)
    _, two = _engine("l2rpn_case14_sandbox", n, offsets, factory=lambda mm, nn: ShardedEngine(
        mm, nn, devices=[0, 0], engine_factory=lambda m_, n_, dev, nbb: PowerFlowEngine(m_, n_lanes=n_, device=0, n_busbar=nbb)))
    cfg = dict(GEO, lines=[0, 2, 4, 9, 13, 17], attack_cooldown=0, seed=77)
    for eng in (one, two):
        eng.set_opponent(**cfg)
        eng.set_opponent_areas([0, 0, 0, 1, 1, 2])
    assert [e.n_lanes for e in two.engines] == [32, 32]
    seen = 0
    for t in range(steps):
        one.step(t, **STEP)
        two.step(t, **STEP)
        a, b = one.opponent_state(), two.opponent_state()
        assert np.array_equal(a.rows(), b.rows()) and np.array_equal(a.budget, b.budget), t
        assert np.array_equal(one.opponent_area_state().rows(), two.opponent_area_state().rows()), t
        al = one.opponent_attack_lines()
        assert np.array_equal(al, two.opponent_attack_lines()), t
        seen += int(al.any(axis=1).sum())
    assert seen > n and len(set(one.opponent_state().cursor)) > 1
    assert np.array_equal(one.results(with_bus=False).line_status, two.results(with_bus=False).line_status)
    one.close()
    two.close()


def test_areas_off_means_the_single_area_opponent():
    """after set_opponent_areas(None) a Geometric Philox opponent equals, in every result row and every state row, an engine on which
    areas were never set"""
    from grid2op_amd.engine import GridPFError
    n = 16
    m, a = _engine("l2rpn_case14_sandbox", n, np.arange(n))
    _, b = _engine("l2rpn_case14_sandbox", n, np.arange(n))
    cfg = dict(GEO, lines=[1, 2, 3, 8, 12], attack_cooldown=1, seed=5)
    a.set_opponent(**cfg)
    a.set_opponent_areas([0, 0, 1, 1, 2])
    a.set_opponent_areas(None)
    b.set_opponent(**cfg)
    with pytest.raises(GridPFError, match="no areas"):
        a.opponent_area_state()
    attacked = 0
    for t in range(10):
        a.step(t, **STEP)
        b.step(t, **STEP)
        sa, sb = a.opponent_state(), b.opponent_state()
        assert np.array_equal(sa.rows(), sb.rows()) and np.array_equal(sa.budget, sb.budget), t
        assert np.array_equal(a.opponent_attack_lines(), b.opponent_attack_lines()), t
        attacked += int((sa.opponent_attack_line >= 0).sum())
    assert attacked > 0
    ra, rb = a.results(), b.results()
    for f in ("out", "topo_vect", "shunt_bus", "line_status", "status", "bus_vm", "bus_va"):
        assert np.array_equal(getattr(ra, f), getattr(rb, f), equal_nan=True), f
    for x, y in zip(a.step_outputs(), b.step_outputs()):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(a.cooldown(), b.cooldown()) and np.array_equal(a.get_topology()[0], b.get_topology()[0])
    assert all(np.array_equal(x, y) for x, y in zip(a.episode(), b.episode()))
    a.close()
    b.close()
