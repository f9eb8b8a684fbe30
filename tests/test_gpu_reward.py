"""The environment's rewards of the batched acting path on the device (include/gridpf.h gpf_set_rewards, grid2op_amd/csrc/gridpf_reward.hpp
reward_kernel): the three episodes recorded from the unmodified reference environment replayed launch by launch on 65 lanes
(tests/golden/reward_*.npz), the kernel against the float64 restatement (tests/reward_ref.py) on seeded rows at the element counts around
one and two strides, bit-equality under permutation / between runs / between the launch and `rewards_eval` / through two shards, the
stale topology flag, and rewards that change nothing else.

Tolerance: a slot is within ONE float32 spacing of the restatement's value on the same float32 inputs (both accumulate in float64, their
orders differ by about 1e-16 relative, so only the final rounding can differ); the constant branches are bit-equal."""
import numpy as np
import pytest

import reward_ref as R
from conftest import golden_path

pytestmark = pytest.mark.gpu

N_LANES, STAGGER = 65, 4


def _slots_for_engine(slots):
    return [(k, list(p)) for k, p in slots]


def _snapshot(eng, dispatch):
    """the lanes' state as reward_kernel reads it, on the host.  dispatch: "env" (the dynamics' actual dispatch), an array, or None"""
    r = eng.results(with_bus=False)
    sl = eng.out_slices
    inj = eng.get_injections()
    rho = eng.step_outputs()[0]
    return dict(gen_p=r.out[:, sl["gen_p"]], load_p=r.out[:, sl["load_p"]], a_or=r.out[:, sl["a_or"]], rho=rho, line_status=r.line_status,
                storage=inj[:, eng.inj_slices["storage_p"]].astype(np.float32),
                dispatch=eng.env_state()["actual"] if isinstance(dispatch, str) else dispatch)


def _lane_row(snap, k, thermal, cost):
    return dict(gen_p=snap["gen_p"][k], load_p=snap["load_p"][k], a_or=snap["a_or"][k], rho=snap["rho"][k], line_status=snap["line_status"][k],
                thermal=thermal, dispatch=None if snap["dispatch"] is None else snap["dispatch"][k], storage=snap["storage"][k], cost=cost)


def _check(got, slots, row, failed, illegal, ambiguous, what):
    want = R.lane_values(slots, **row, failed=failed, illegal=illegal, ambiguous=ambiguous)
    assert R.spacing_ok(got, want).all(), (what, got, want)
    for s, (kind, _) in enumerate(slots):
        if R.constant_branch(kind, failed, illegal, ambiguous):
            assert got[s].tobytes() == want[s].tobytes(), (what, s, got[s], want[s])


def _check_groups(eng, got, slots, snap, thermal, cost, failed, illegal, ambiguous, what):
    """lanes of one stagger group play the same step: one restatement per group, the group's lanes bit-identical"""
    for g in range(STAGGER):
        lanes = np.arange(g, N_LANES, STAGGER)
        k = int(lanes[0])
        assert all(got[q].tobytes() == got[k].tobytes() for q in lanes), (what, g)
        _check(got[k], slots, _lane_row(snap, k, thermal, cost), bool(failed[k]), bool(illegal[k]), bool(ambiguous[k]), (what, g))


def test_replay_of_the_recorded_topology_episodes():
    """reward_case14_topo.npz: every lane of a 65-lane batch plays the recorded launches, lane k starting k mod 4 launches late.  done and
    the flags agree with the recording; every slot of every lane at every launch is held to the restatement on the device's own inputs."""
    from grid2op_amd.chronics import chronics_table
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    import sys
    import os
    sys.path.insert(0, os.path.dirname(golden_path("x")))
    from make_reward_fixtures import topo_table
    fx = dict(np.load(golden_path("reward_case14_topo.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    eng = PowerFlowEngine(m, n_lanes=N_LANES, device=0)
    tab = chronics_table({k[len("chron_"):]: fx[k] for k in fx if k.startswith("chron_")})
    eng.upload_chronics(tab)
    T = tab.shape[1]
    eng.set_thermal_limits(fx["thermal_limit"])
    p = [int(x) for x in fx["params"]]
    eng.set_topo_rules(legal_rules=True, max_sub_changed=p[0], max_line_status_changed=p[1], cooldown_sub=p[2], cooldown_line=p[3])
    table, n0 = topo_table(m, int(fx["table_seed"]))
    off, items = eng.pack_actions(table)
    assert n0 == int(fx["n_table"]) and np.array_equal(off, fx["off"]) and np.array_equal(np.asarray(items).reshape(-1, 3), fx["items"].reshape(-1, 3))
    eng.upload_topo_actions(table)
    slots = R.fixture_slots(fx)
    eng.set_rewards(_slots_for_engine(slots), fx["gen_cost_per_MW"])
    used = [int(x) for x in fx["scenarios_used"]]
    N = len(fx["done"])
    group = np.arange(N_LANES) % STAGGER
    seen = dict(illegal=0, ambiguous=0, game_over=0, plain=0)
    for L in range(N + STAGGER - 1):
        j = L - group                                                   # the recorded launch every lane plays (outside [0, N): idle)
        act = (j >= 0) & (j < N)
        jj = np.clip(j, 0, N - 1)
        for k in np.flatnonzero(act & (j == 0)):
            eng.reset(int(k), 1)
        table_of = np.where(act, [used.index(int(s)) for s in fx["scenario"][jj]], 0)
        offset = np.where(act, (fx["row"][jj] - L) % T, 0)
        eng.set_lane_chronics(lane_table=table_of, lane_offset=offset)
        eng.set_lane_topo_actions(np.where(act, fx["played"][jj], -1))
        eng.step(L, cascade=False, nb_ts_reco=p[4], auto_reset=True)
        done = eng.episode()[0]
        ill, amb = eng.topo_action_flags()
        want_done = np.where(act, fx["done"][jj], 0).astype(bool)
        want_ill, want_amb = np.where(act, fx["is_illegal"][jj], 0).astype(bool), np.where(act, fx["is_ambiguous"][jj], 0).astype(bool)
        assert np.array_equal(done[act], want_done[act]), (L, np.flatnonzero(done != want_done))
        assert not done[~act].any(), L
        assert np.array_equal(ill, want_ill) and np.array_equal(amb, want_amb), (L, np.flatnonzero(ill != want_ill), np.flatnonzero(amb != want_amb))
        _check_groups(eng, eng.rewards(), slots, _snapshot(eng, None), fx["thermal_limit"], fx["gen_cost_per_MW"], done, ill, amb, L)
        k0 = int(np.flatnonzero(group == 0)[0])
        if act[k0] and not fx["is_reset"][jj[k0]]:
            seen["illegal"] += int(ill[k0] and not done[k0]); seen["ambiguous"] += int(amb[k0] and not done[k0]); seen["game_over"] += int(done[k0])
            seen["plain"] += int(not (ill[k0] or amb[k0] or done[k0]))
    assert seen["illegal"] >= 10 and seen["ambiguous"] >= 5 and seen["game_over"] >= 3 and seen["plain"] >= 40, seen
    eng.close()


@pytest.mark.parametrize("tag", ["case14_storage", "wcci2022"])
def test_replay_of_the_recorded_dynamics_episodes(tag):
    """reward_case14_storage.npz / reward_wcci2022.npz through one-step launches with the dynamics on, lane k starting k mod 4 launches
    late: no game over, the per-step "a redispatch was cancelled" bit equals info's failed_redispatching, every slot is held to the
    restatement on the device's own results, actual dispatch and clamped storage power."""
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    fx = dict(np.load(golden_path(f"reward_{tag}.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    eng = PowerFlowEngine(m, n_lanes=N_LANES, device=0)
    eng.upload_chronics(eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"]))
    T = fx["ch_load_p"].shape[0]
    eng.set_thermal_limits(fx["thermal_limit"])
    eng.set_gen_limits(fx["pmin"], fx["pmax"], fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], eps_poly=float(fx["eps_poly"]))
    eng.set_storage_params(fx["storage_Emax"], fx["storage_Emin"], fx["storage_loss"], fx["storage_charging_efficiency"],
                           fx["storage_discharging_efficiency"], fx["storage_charge0"], float(fx["delta_time_seconds"]), bool(fx["activate_storage_loss"]))
    eng.set_env_dynamics(True, tol_poly=float(fx["tol_poly"]))
    eng.set_gen_renewable(fx["renewable"])
    slots = R.fixture_slots(fx)
    eng.set_rewards(_slots_for_engine(slots), fx["gen_cost_per_MW"])
    N, row0 = len(fx["done"]), int(fx["row"][0])
    group = np.arange(N_LANES) % STAGGER
    eng.set_lane_chronics(lane_offset=(row0 - group) % T)
    count = np.zeros(N_LANES, np.int64)
    cancelled = clamped = 0
    for L in range(N + STAGGER - 1):
        j = L - group
        act = (j >= 0) & (j < N)
        jj = np.clip(j, 0, N - 1)
        for k in np.flatnonzero(act & (j == 0)):
            eng.reset(int(k), 1)                                        # the reset left _gen_activeprod_t_redisp = the row before the first step
            eng.set_env_state(int(k), prev_p=fx["ch_prod_p"][row0 - 1][None])
            count[k] = 0
        red = np.where(act[:, None], fx["act_redisp"][jj], 0.0).astype(np.float32)
        sto = np.where(act[:, None], fx["act_storage"][jj], 0.0).astype(np.float32)
        cur = np.where(act[:, None], fx["act_curtail"][jj], -1.0).astype(np.float32)
        eng.set_lane_actions(red, sto)
        if (cur != -1).any():
            eng.set_lane_curtailment(cur)
        eng.step(L)
        done = eng.episode()[0]
        assert not done.any(), (L, np.flatnonzero(done))
        now = eng.env_state()["illegal"].astype(np.int64)
        bit = now != count
        count = now
        want_bit = np.where(act, fx["failed_redisp"][jj], 0).astype(bool)
        assert np.array_equal(bit, want_bit), (L, np.flatnonzero(bit != want_bit))
        snap = _snapshot(eng, "env")
        _check_groups(eng, eng.rewards(), slots, snap, fx["thermal_limit"], fx["gen_cost_per_MW"], done, bit, np.zeros(N_LANES, bool), L)
        k0 = 0
        if act[k0]:
            cancelled += int(bit[k0])
            clamped += int(np.abs(snap["storage"][k0] - sto[k0]).max() > 0.5 and not bit[k0])
            if not bit[k0]:                                             # the device's inputs are the recorded step's (the projection is exact here,
                assert np.abs(snap["storage"][k0] - fx["storage_power"][jj[k0]]).max() < 1e-3, L       # SLSQP's there: the dispatch may differ)
    assert cancelled == int(fx["failed_redisp"].sum()) and (clamped >= 1 or tag != "case14_storage"), (cancelled, clamped)
    eng.close()


def _seeded_engine(m, n, seed, with_storage=True):
    """an engine whose lanes hold seeded rows (no power flow is run): returns what was written, for the restatement"""
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    rng = np.random.default_rng(seed)
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    v = eng.device_views()
    out = rng.uniform(-5.0, 80.0, (n, eng.n_out)).astype(np.float32)
    out[:, eng.out_slices["load_p"]] = rng.uniform(1.0, 60.0, (n, m.n_load))
    out[:, eng.out_slices["a_or"]] = rng.uniform(0.0, 900.0, (n, m.n_line))
    out[:, eng.out_slices["gen_p"].start] = 10.0                         # (a generator that produces: inside the reference's domain)
    rho = rng.uniform(0.0, 1.4, (n, m.n_line)).astype(np.float32)
    ls = (rng.random((n, m.n_line)) > 0.2).astype(np.uint8)
    done = np.zeros(n, np.uint8)
    done[n - 1] = 1                                                      # the failed lane
    delta = rng.uniform(-10.0, 10.0, (n, m.n_gen)).astype(np.float32)
    thermal = rng.uniform(100.0, 800.0, m.n_line).astype(np.float32)
    cost = rng.uniform(0.0, 90.0, m.n_gen).astype(np.float32)
    inj = eng.get_injections()
    if m.n_storage and with_storage:
        inj[:, eng.inj_slices["storage_p"]] = rng.uniform(-4.0, 4.0, (n, m.n_storage)).astype(np.float32)
        eng.set_injections(inj)
    eng.set_thermal_limits(thermal)
    eng.set_lane_redispatch(delta)
    with torch.cuda.stream(v["stream"]):
        for key, a in (("out", out), ("rho", rho), ("line_status", ls), ("done", done[:, None]), ("status", np.zeros((n, 4), np.int32))):
            v[key].copy_(torch.from_numpy(a).to(v[key].device))
    v["stream"].synchronize()
    sl = eng.out_slices
    snap = dict(gen_p=out[:, sl["gen_p"]], load_p=out[:, sl["load_p"]], a_or=out[:, sl["a_or"]], rho=rho, line_status=ls, dispatch=delta,
                storage=inj[:, eng.inj_slices["storage_p"]].astype(np.float32))
    return eng, snap, thermal, cost, done


FLAGS5 = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [0, 0]], np.uint8)        # the four combinations, then the failed lane


def _eval_and_check(eng, snap, thermal, cost, done, slots, what):
    import torch
    n = len(done)
    eng.set_rewards(_slots_for_engine(slots), cost)
    flags = torch.from_numpy(np.resize(FLAGS5, (n, 2)).copy()).to(f"cuda:{eng.device}")
    got = eng.rewards_eval(flags=flags)
    eng.sync()
    got = got.cpu().numpy()
    fl = np.resize(FLAGS5, (n, 2))
    for k in range(n):
        _check(got[k], slots, _lane_row(snap, k, thermal, cost), bool(done[k]), bool(fl[k, 0]), bool(fl[k, 1]), (what, k))
    return got


SLOTS = [(R.REDISP, [5.0, 1.0e5, -10.0, 0.25, 300.0 / 3600.0]), (R.L2RPN, []), (R.LINES_CAPACITY, []),
         (R.ECONOMIC, [5.0e4, -0.5, 1.5, 300.0 / 3600.0]), (R.GAMEPLAY, [-1.0, 1.0])]


@pytest.mark.parametrize("n_gen", [1, 63, 64, 65, 129])
def test_element_counts_through_the_generator_count(n_gen, load_model):
    """copies of the 5-substation grid with 1 .. 129 generators, 5 lanes of seeded rows: all five kinds against the restatement, all four flag
    combinations and a failed lane; every kind's reduction goes through the one strided helper whose boundaries these counts cross"""
    from redispatch_cases import BASE_GRID, resized_model
    m = resized_model(load_model(BASE_GRID), n_gen)
    eng, snap, thermal, cost, done = _seeded_engine(m, 5, 900 + n_gen)
    got = _eval_and_check(eng, snap, thermal, cost, done, SLOTS, n_gen)
    assert np.isfinite(got).all()
    # the same through a caller's tensor with a wider row, slots in another order; and without a dispatch delta
    import torch
    eng.set_rewards(_slots_for_engine(SLOTS[::-1]), cost)
    wide = torch.full((5, 8), 7.0, dtype=torch.float32, device="cuda:0")
    eng.rewards_eval(flags=torch.from_numpy(FLAGS5.copy()).to("cuda:0"), out=wide)
    eng.sync()
    w = wide.cpu().numpy()
    assert w[:, :5][:, ::-1].tobytes() == got.tobytes() and (w[:, 5:] == 7.0).all()
    eng.set_lane_redispatch(None)
    _eval_and_check(eng, dict(snap, dispatch=None), thermal, cost, done, SLOTS, (n_gen, "no delta"))
    eng.close()


@pytest.mark.parametrize("name", ["l2rpn_neurips_2020_track1", "l2rpn_wcci_2022_dev"])
def test_element_counts_through_the_line_count(name, load_model):
    """59 lines (below one stride) and 186 lines (above two): 22 / 62 generators, 37 / 91 loads, 0 / 7 storage units"""
    m = load_model(name)
    eng, snap, thermal, cost, done = _seeded_engine(m, 5, 77)
    _eval_and_check(eng, snap, thermal, cost, done, SLOTS, name)
    eng.close()


def _chronics_engine(name, n, offsets, factory=None):
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


def _case14_slots(m):
    from grid2op_amd.engine import reward_config
    cost = np.linspace(10.0, 60.0, m.n_gen).astype(np.float32)
    pmax = np.full(m.n_gen, 120.0, np.float32)
    names = ("RedispReward", "L2RPNReward", "LinesCapacityReward", "EconomicReward", "GameplayReward")
    return [reward_config(k, gen_cost_per_MW=cost, gen_pmax=pmax) if k in names[::3] else reward_config(k) for k in names], cost


TWO_LINES = [{"set_line_status": [(0, -1), (1, -1)]}, {"set_line_status": [(2, -1)]}, {"set_line_status": [(2, 1)], "change_line_status": [2]}]
RULES = dict(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=3)


def test_bit_equality_under_permutation_between_runs_eval_and_shards():
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.sharding import ShardedEngine
    n = N_LANES
    rng = np.random.default_rng(21)
    offsets = 3 * np.arange(n)
    perm = rng.permutation(n)
    idx = rng.integers(-1, len(TWO_LINES), n).astype(np.int32)
    m, a = _chronics_engine("l2rpn_case14_sandbox", n, offsets)
    _, b = _chronics_engine("l2rpn_case14_sandbox", n, offsets)                 # a second run
    _, c = _chronics_engine("l2rpn_case14_sandbox", n, offsets[perm])           # the lanes in another order
    _, d = _chronics_engine("l2rpn_case14_sandbox", n, offsets, factory=lambda mm, nn: ShardedEngine(
        mm, nn, devices=[0, 0], engine_factory=lambda m_, n_, dev, nbb: PowerFlowEngine(m_, n_lanes=n_, device=0, n_busbar=nbb)))
    slots, cost = _case14_slots(m)
    for eng in (a, b, c, d):
        eng.set_rewards(slots, cost)
        eng.upload_topo_actions(TWO_LINES)
        eng.set_topo_rules(**RULES)
    for t in range(1, 4):
        for eng, ix in ((a, idx), (b, idx), (c, idx[perm]), (d, idx)):
            eng.set_lane_topo_actions(ix)
            eng.step(t, nb_ts_reco=10)
        ra = a.rewards()
        assert ra.tobytes() == b.rewards().tobytes(), t
        assert ra[perm].tobytes() == c.rewards().tobytes(), t
        assert ra.tobytes() == d.rewards().tobytes(), t
        ill, amb = a.topo_action_flags()
        assert ill.any() and amb.any() and np.isfinite(ra).all() and len(np.unique(ra[:, 0])) > n // 4
        # the launch's rewards and rewards_eval on the same state with the same flags
        flags = a.device_views()["topo_flags"].clone()
        out = torch.zeros((n, 5), dtype=torch.float32, device="cuda:0")
        a.rewards_eval(flags=flags, out=out)
        a.sync()
        assert out.cpu().numpy().tobytes() == ra.tobytes(), t
        parts = d.rewards_eval(flags=[flags[b0:b0 + bn].contiguous() for b0, bn in d.blocks])
        d.sync()
        assert np.concatenate([x.cpu().numpy() for x in parts]).tobytes() == ra.tobytes(), t
    a.reset(3, 2)                                                               # reset lanes read 0
    rr = a.rewards()
    assert (rr[3:5] == 0).all() and rr[:3].tobytes() == ra[:3].tobytes() and rr[5:].tobytes() == ra[5:].tobytes()
    for eng in (a, b, c, d):
        eng.close()


def test_a_launch_without_actions_does_not_read_the_stale_topology_flag():
    n = 5
    m, eng = _chronics_engine("l2rpn_case14_sandbox", n, np.arange(n))
    slots, cost = _case14_slots(m)
    eng.set_rewards(slots, cost)
    eng.upload_topo_actions(TWO_LINES)
    eng.set_topo_rules(**RULES)
    eng.set_lane_topo_actions(np.array([0, 2, -1, 0, 1], np.int32))            # illegal (two lines), ambiguous, nothing, illegal, legal
    eng.step(1, nb_ts_reco=10)
    r1 = eng.rewards()
    assert [float(x) for x in r1[:, 4]] == [-0.5, -0.5, 1.0, -0.5, 1.0] and [float(x) for x in r1[:, 2] > 0] == [0.0, 0.0, 1.0, 0.0, 1.0]
    assert (r1[[0, 1, 3], 0] == 0).all() and (r1[[2, 4], 0] > 0).all()
    eng.step(2, nb_ts_reco=10)                                                  # no actions: legal, whatever gpf_get_topo_flags still holds
    ill, amb = eng.topo_action_flags()
    assert list(ill) == [True, False, False, True, False] and list(amb) == [False, True, False, False, False]
    r2 = eng.rewards()
    assert (r2[:, 4] == 1.0).all() and (r2[:, 0] > 0).all() and (r2[:, 2] > 0).all()
    eng.close()


def test_multi_step_launch_and_rewards_off_change_nothing():
    from grid2op_amd.engine import GridPFError
    n = 16
    m, a = _chronics_engine("l2rpn_case14_sandbox", n, np.arange(n))
    _, b = _chronics_engine("l2rpn_case14_sandbox", n, np.arange(n))
    slots, cost = _case14_slots(m)
    a.set_rewards(slots, cost)
    views_off = set(b.device_views())

    def same():
        ra, rb = a.results(), b.results()
        for f in ("out", "topo_vect", "shunt_bus", "line_status", "status", "bus_vm", "bus_va"):
            assert np.array_equal(getattr(ra, f), getattr(rb, f), equal_nan=True), f
        for x, y in zip(a.step_outputs(), b.step_outputs()):
            assert np.array_equal(x, y, equal_nan=True)
        assert all(np.array_equal(x, y) for x, y in zip(a.episode(), b.episode()))
    a.step(1, cascade=True)
    b.step(1, cascade=True)
    same()
    assert np.isfinite(a.rewards()).all()
    a.step(2, n_steps=3, cascade=True)                                          # a multi-step launch queues nothing for rewards
    b.step(2, n_steps=3, cascade=True)
    same()
    assert a.counters() == b.counters()
    with pytest.raises(GridPFError, match="multi-step launch"):
        a.rewards()
    a.step(5, cascade=True)
    b.step(5, cascade=True)
    same()
    assert a.counters() == b.counters() and np.isfinite(a.rewards()).all()      # the step's own dispatches: the same launches
    a.set_rewards(None)                                                         # off: the parent's path
    with pytest.raises(GridPFError, match="rewards are off"):
        a.rewards()
    assert set(a.device_views()) == views_off
    a.step(6, cascade=True)
    b.step(6, cascade=True)
    same()
    assert a.counters() == b.counters()
    a.close()
    b.close()
