"""Episode time limits of the batched acting path on the device (include/gridpf.h gpf_set_episode_limit, grid2op_amd/csrc/gridpf_episode.hpp
episode_kernel, the `truncated` flag in reward_kernel and alert_poststep_kernel): the three episodes recorded from the unmodified reference
replayed through one-step launches with auto_reset, the in-launch reset of a truncated lane against a twin engine reset from the host,
the float64 returns against a sequential numpy sum, the flags' corner cases, and a feature that changes nothing while it is off.

Shapes: 1, 5 and 6 lanes (none a multiple of the four lanes of a block: one and two blocks), 1 and 8 reward slots, the 14-substation
grids and 3 lanes of the 118-substation grid (dim_topo 532, 186 lines, 118 substations: every stride-64 row loop takes several passes).
Tolerances are those of tests/test_episode_limit_cpu.py: flags, lengths and the alert bonus exact, EpisodeDurationReward at one float32
spacing of the recording (bit-equal to the restatement), rewards at one float32 spacing of the restatement on the device's own inputs."""
import os
import sys

import numpy as np
import pytest

import alert_ref as AR
import episode_ref as E
import opponent_ref as OR
import reward_ref as R
from conftest import golden_path

pytestmark = pytest.mark.gpu

SLOTS8 = [(R.L2RPN, []), (R.GAMEPLAY, [-1.0, 1.0]), (R.LINES_CAPACITY, []), (R.L2RPN, []), (R.GAMEPLAY, [-2.0, 3.0]), (R.LINES_CAPACITY, []),
          (R.L2RPN, []), (R.GAMEPLAY, [-0.5, 0.25])]


def _snapshot(eng, dispatch):
    r = eng.results(with_bus=False)
    sl = eng.out_slices
    inj = eng.get_injections()
    return dict(gen_p=r.out[:, sl["gen_p"]], load_p=r.out[:, sl["load_p"]], a_or=r.out[:, sl["a_or"]], rho=eng.step_outputs()[0],
                line_status=r.line_status, storage=inj[:, eng.inj_slices["storage_p"]].astype(np.float32),
                dispatch=eng.env_state()["actual"] if dispatch else None)


def _check_rewards(got, slots, snap, k, thermal, cost, failed, illegal, ambiguous, trunc, what):
    row = dict(gen_p=snap["gen_p"][k], load_p=snap["load_p"][k], a_or=snap["a_or"][k], rho=snap["rho"][k], line_status=snap["line_status"][k],
               thermal=thermal, dispatch=None if snap["dispatch"] is None else snap["dispatch"][k], storage=snap["storage"][k], cost=cost,
               failed=failed, illegal=illegal, ambiguous=ambiguous)
    want = E.lane_values(slots, trunc=trunc, **row)
    assert R.spacing_ok(got, want).all(), (what, got, want)
    for s, (kind, _) in enumerate(slots):
        if E.constant_branch(kind, failed, illegal, ambiguous, trunc):
            assert got[s].tobytes() == want[s].tobytes(), (what, s, got[s], want[s])


def _check_ends(ends, k, fx, i, limit, what):
    """flags and length exactly; EpisodeDurationReward bit-equal to the restatement and within one float32 spacing of the recording"""
    done = bool(fx["done"][i])
    assert bool(ends["terminated"][k]) == bool(fx["terminated"][i]) and bool(ends["truncated"][k]) == bool(fx["truncated"][i]), what
    assert int(ends["length"][k]) == (int(fx["nb_time_step"][i]) if done else 0), (what, ends["length"][k])
    want = E.duration_reward(done, int(fx["nb_time_step"][i]), limit)
    assert ends["duration_reward"][k].tobytes() == want.tobytes(), (what, ends["duration_reward"][k], want)
    rec = np.float32(fx["reward_episode_duration"][i])
    assert abs(float(rec) - float(want)) <= float(np.spacing(np.float32(abs(want)))), (what, rec, want)


def test_replay_of_the_recorded_topology_episodes():
    """episode_limit_case14.npz on 5 lanes, one launch per recorded env.step (the reset observation takes none, so the limit is the
    reference's max step).  Lanes 0-3 carry the recorded limit.  Lane 4 plays the same actions with another limit: the recorded one plus
    100 in every other episode, where it must NOT be truncated (its rewards are those of a step that goes on, and the host resets it)."""
    from grid2op_amd.chronics import chronics_table
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    sys.path.insert(0, os.path.dirname(golden_path("x")))
    from make_episode_limit_fixtures import episode_table
    fx = dict(np.load(golden_path("episode_limit_case14.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    n = 5
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    tab = chronics_table({k[len("chron_"):]: fx[k] for k in fx if k.startswith("chron_")})
    eng.upload_chronics(tab)
    T = tab.shape[1]
    eng.set_thermal_limits(fx["thermal_limit"])
    p = [int(x) for x in fx["params"]]
    eng.set_topo_rules(legal_rules=True, max_sub_changed=p[0], max_line_status_changed=p[1], cooldown_sub=p[2], cooldown_line=p[3])
    table, n0, n_two = episode_table(m, int(fx["table_seed"]))
    off, items = eng.pack_actions(table)
    assert n0 == int(fx["n_table"]) and n_two == int(fx["two_lines_entry"]) and np.array_equal(off, fx["off"])
    assert np.array_equal(np.asarray(items).reshape(-1, 3), fx["items"].reshape(-1, 3))
    eng.upload_topo_actions(table)
    slots = R.fixture_slots(fx)
    eng.set_rewards([(k, list(q)) for k, q in slots], fx["gen_cost_per_MW"])
    used = [int(x) for x in fx["scenarios_used"]]
    L, episode, seen = 0, -1, dict(trunc=0, term=0, other_not_truncated=0)
    limits = np.zeros(n, np.int32)
    for i in range(len(fx["done"])):
        if fx["is_reset"][i]:
            episode += 1
            limits[:] = int(fx["max_step"][i])
            if episode % 2:
                limits[4] += 100
            eng.set_episode_limit(limits)
            assert (eng.episode()[1][:4] == 0).all(), i               # the lanes restarted inside the launch that ended their episode
            continue
        N = int(fx["max_step"][i])
        eng.set_lane_chronics(lane_table=np.full(n, used.index(int(fx["scenario"][i]))), lane_offset=np.full(n, (int(fx["row"][i]) - L) % T))
        eng.set_lane_topo_actions(np.full(n, int(fx["played"][i])))
        eng.step(L, cascade=False, nb_ts_reco=p[4], auto_reset=True)
        L += 1
        done, ends = eng.episode()[0], eng.episode_ends()
        ill, amb = eng.topo_action_flags()
        assert (done == bool(fx["terminated"][i])).all() and (ill == bool(fx["is_illegal"][i])).all() and (amb == bool(fx["is_ambiguous"][i])).all(), i
        rew, snap = eng.rewards(), _snapshot(eng, False)
        for k in range(n):
            other = k == 4 and episode % 2 == 1
            if other:                                                   # the lane with the far limit goes on where the others are truncated
                assert not ends["truncated"][k] and bool(ends["terminated"][k]) == bool(fx["terminated"][i]), i
                assert int(ends["length"][k]) == (int(fx["nb_time_step"][i]) if fx["terminated"][i] else 0)
                seen["other_not_truncated"] += int(fx["truncated"][i])
            else:
                _check_ends(ends, k, fx, i, N, (i, k))
            trunc = bool(fx["truncated"][i]) and not other
            _check_rewards(rew[k], slots, snap, k, fx["thermal_limit"], fx["gen_cost_per_MW"], bool(done[k]), bool(ill[k]), bool(amb[k]), trunc, (i, k))
        assert all(rew[k].tobytes() == rew[0].tobytes() for k in range(4)), i
        seen["trunc"] += int(fx["truncated"][i]); seen["term"] += int(fx["terminated"][i])
        if fx["truncated"][i] and episode % 2 == 1:
            eng.reset(4, 1)
    st = eng.episode_stats()
    assert (st["n_episodes"][:4] == seen["trunc"] + seen["term"]).all() and seen["trunc"] >= 5 and seen["term"] == 2 and seen["other_not_truncated"] >= 2
    eng.close()


def _dyn_engine(fx, n):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"]))
    eng.set_thermal_limits(fx["thermal_limit"])
    eng.set_gen_limits(fx["pmin"], fx["pmax"], fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], eps_poly=float(fx["eps_poly"]))
    eng.set_storage_params(fx["storage_Emax"], fx["storage_Emin"], fx["storage_loss"], fx["storage_charging_efficiency"],
                           fx["storage_discharging_efficiency"], fx["storage_charge0"], float(fx["delta_time_seconds"]), bool(fx["activate_storage_loss"]))
    eng.set_env_dynamics(True, tol_poly=float(fx["tol_poly"]))
    eng.set_gen_renewable(fx["renewable"])
    return m, eng


def test_replay_of_the_recorded_storage_episodes():
    """episode_limit_storage.npz on 6 lanes with the dynamics on: two episodes of six steps on the same chronics rows.  The truncated
    launch leaves dispatch and charge as env.reset() does, and the second episode (other actions on the same rows) follows the recording
    from there.  A twin engine without a limit, reset from the host between the episodes, plays the same launches: it still holds the
    final step's dispatch, which the truncated lanes' rewards saw before their reset, and equals the lanes in every other input."""
    fx = dict(np.load(golden_path("episode_limit_storage.npz")))
    n, N = 6, int(fx["max_step"][0])
    m, eng = _dyn_engine(fx, n)
    _, twin = _dyn_engine(fx, n)
    T, row0 = fx["ch_load_p"].shape[0], int(fx["row"][0])
    slots = R.fixture_slots(fx)
    for e in (eng, twin):
        e.set_rewards([(k, list(q)) for k, q in slots], fx["gen_cost_per_MW"])
    eng.set_episode_limit(N)
    for i in range(len(fx["done"])):
        t = i % N
        for e in (eng, twin):
            if t == 0:
                if e is twin:
                    e.reset()
                e.set_lane_chronics(lane_offset=np.full(n, (row0 - i) % T))
                e.set_env_state(0, prev_p=np.tile(fx["ch_prod_p"][row0 - 1], (n, 1)))    # (the reset left _gen_activeprod_t_redisp = the row before)
            e.set_lane_actions(np.tile(fx["act_redisp"][i], (n, 1)), np.tile(fx["act_storage"][i], (n, 1)))
            e.step(i, auto_reset=True)
        ends, rew, snap = eng.episode_ends(), eng.rewards(), _snapshot(eng, True)
        assert not eng.episode()[0].any() and not twin.episode()[0].any()
        trunc = bool(fx["truncated"][i])
        if trunc:                                                       # (the lanes' own dispatch is reset by now)
            snap["dispatch"] = twin.env_state()["actual"]
            assert np.abs(snap["dispatch"]).sum() > 0
        assert snap["dispatch"].tobytes() == twin.env_state()["actual"].tobytes() and snap["gen_p"].tobytes() == _snapshot(twin, True)["gen_p"].tobytes(), i
        for k in range(n):
            _check_ends(ends, k, fx, i, N, (i, k))
            _check_rewards(rew[k], slots, snap, k, fx["thermal_limit"], fx["gen_cost_per_MW"], False, bool(fx["failed_redisp"][i]), False, trunc, (i, k))
        others = [s for s, (kind, _) in enumerate(slots) if kind != R.L2RPN]
        assert rew[:, others].tobytes() == twin.rewards()[:, others].tobytes(), i          # a legal truncated step changes L2RPNReward alone
        assert (rew[:, 1] == 0).all() == trunc and (twin.rewards()[:, 1] > 0).all()
        st = eng.env_state()
        if trunc:                                                       # what env.reset() leaves
            assert not st["target"].any() and not st["actual"].any() and not st["already_modified"].any() and not st["illegal"].any()
            assert np.array_equal(st["charge"], np.tile(fx["storage_charge0"].astype(np.float32), (n, 1))) and (st["curtail_limit"] == 1).all()
            assert (eng.episode()[1] == 0).all() and (eng.episode()[2] == i // N + 1).all()
        else:
            assert np.abs(st["charge"] - fx["storage_charge"][i]).max() < 1e-3, i
    st = eng.episode_stats()
    assert (st["n_episodes"] == 2).all() and (st["length_last"] == N).all()
    eng.close(); twin.close()


def test_replay_of_the_recorded_alert_episodes():
    """episode_limit_alert_case14.npz on 5 lanes: the replay of tests/test_gpu_alert.py, where the reset observation takes a launch (the
    opponent and the alerts expect one), so the limit is max step + 1 and a length counts that launch.  The alert reward equals the
    recording on every launch -- reward_end_episode_bonus on the two truncated ones -- and so do the seven alert attributes."""
    from grid2op_amd.chronics import chronics_table
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from grid2op_amd.obs_spec import ObsSpec
    from test_opponent_area_cpu import fixture_config
    fx = dict(np.load(golden_path("episode_limit_alert_case14.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    n, A = 5, len(fx["lines"])
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    tab = chronics_table({k[len("chron_"):]: fx[k] for k in fx if k.startswith("chron_")})
    eng.upload_chronics(tab)
    T = tab.shape[1]
    eng.set_thermal_limits(fx["thermal_limit"])
    p = [int(x) for x in fx["params"]]
    eng.set_topo_rules(legal_rules=True, max_sub_changed=p[0], max_line_status_changed=p[1], cooldown_sub=p[2], cooldown_line=p[3])
    acts = []
    for l in range(m.n_line):
        acts += [{"set_line_status": [(l, 1)]}, {"set_line_status": [(l, -1)]}]
    assert not eng.upload_topo_actions(acts).any()
    cfg, aol = fixture_config(fx)
    eng.set_opponent(OR.GEOMETRIC, **cfg)
    eng.set_opponent_areas(aol)
    eng.upload_opponent_draws(np.tile(fx["draws"], (n, 1)))
    c = [float(x) for x in fx["reward_constants"]]
    eng.set_alerts(int(fx["time_window"]), c[0], c[1], c[2], c[3])
    spec = ObsSpec(m, list(AR.OBS_ATTRS), dim_alerts=A)
    eng.set_obs_spec(spec)
    bonus = float(fx["reward_end_episode_bonus"])
    used = [int(x) for x in fx["scenarios_used"]]
    resets, n_trunc, kept = 0, 0, 0
    for i in range(len(fx["is_reset"])):
        eng.set_lane_chronics(lane_table=np.full(n, used.index(int(fx["scenario"][i]))), lane_offset=np.full(n, (int(fx["row"][i]) - i) % T))
        if fx["is_reset"][i]:
            eng.upload_opponent_area_schedule(fx["schedule"][resets], fx["schedule_count"][resets])
            resets += 1
            assert (eng.episode()[1] == 0).all(), i                     # every episode's end restarted the lanes inside its launch
            eng.set_episode_limit(int(fx["max_step"][i]) + 1, alert_end_bonus=bonus)
        a = int(fx["agent_line"][i])
        eng.set_lane_topo_actions(None if a < 0 else np.full(n, 2 * a + (0 if fx["agent_value"][i] > 0 else 1)))
        eng.set_lane_alerts(np.tile(fx["alert_mask"][i], (n, 1)) if fx["alert_mask"][i].any() else None)
        eng.step(i, cascade=False, nb_ts_reco=p[4], auto_reset=True)
        assert (eng.opponent_attack_lines() == fx["info_lines"][i]).all(), i
        ends = eng.episode_ends()
        assert (ends["terminated"] == bool(fx["terminated"][i])).all() and (ends["truncated"] == bool(fx["truncated"][i])).all(), i
        assert (ends["length"] == (int(fx["nb_time_step"][i]) + 1 if fx["done"][i] else 0)).all(), i
        rew = eng.alert_reward()
        assert rew.tobytes() == np.full(n, fx["alert_reward"][i], np.float32).tobytes(), (i, rew, fx["alert_reward"][i])
        vec = eng.observation_vector_host()
        for k in AR.OBS_ATTRS:
            rec = fx["env_attack_under_alert"][i] if fx["terminated"][i] and k == "attack_under_alert" else fx["obs_" + k][i]
            assert (vec[:, spec.offsets[k]] == np.asarray(rec, np.float32).reshape(1, -1)).all(), (i, k, vec[:, spec.offsets[k]], rec)
        if fx["truncated"][i]:
            assert float(rew[0]) == bonus
            n_trunc += 1
            kept += int(np.any(fx["obs_was_alert_used_after_attack"][i] != 0))
    assert n_trunc == 2 and kept >= 1 and resets == 3
    eng.close()


def _sandbox(n, offsets, factory=None):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path("l2rpn_case14_sandbox.grid.npz"))
    ch = dict(np.load(golden_path("l2rpn_case14_sandbox.chronics.npz")))
    eng = factory(m, n) if factory else PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    eng.set_lane_chronics(lane_offset=np.asarray(offsets))
    eng.set_thermal_limits(ch["thermal_limits"])
    return m, eng, ch


def _reset_rows(eng, dyn):
    """every row the reset of a lane touches"""
    _, oc, _ = eng.step_outputs()
    out = dict(topo=eng.get_topology()[0], overflow=oc, cooldown=eng.cooldown(), sub_cooldown=eng.sub_cooldown(), last_bus=eng.last_bus(),
               steps=eng.episode()[1])
    if dyn:
        out.update({"env_" + k: v for k, v in eng.env_state().items()})
    return out


def _results(eng):
    r = eng.results(with_bus=False)
    rho, oc, _ = eng.step_outputs()
    return dict(out=r.out, topo_vect=r.topo_vect, line_status=r.line_status, status=r.status, rho=rho, overflow=oc, cooldown=eng.cooldown(),
                sub_cooldown=eng.sub_cooldown())


def _twin_run(make, launches_before, launches_after, limit, dyn):
    """engine A truncates at launch `limit` under auto_reset; its twin B plays the same launches without a limit and is reset from the host"""
    a, b = make(), make()
    a.set_episode_limit(limit)
    for L, play in enumerate(launches_before):
        for e in (a, b):
            play(e)
            e.step(L, cascade=False, nb_ts_reco=10, auto_reset=True)
        if L < limit - 1:
            assert not a.episode_ends()["truncated"].any() and not a.episode()[0].any() and not b.episode()[0].any(), L
    assert len(launches_before) == limit and a.episode_ends()["truncated"].all() and (a.episode_ends()["length"] == limit).all()
    a.set_episode_limit(1000)                                           # (a new limit on a running feature: no second truncation below)
    before_b = _reset_rows(b, dyn)
    b.reset()
    ra, rb = _reset_rows(a, dyn), _reset_rows(b, dyn)
    changed = [k for k in rb if not np.array_equal(before_b[k], rb[k])]
    for k in rb:
        assert np.array_equal(ra[k], rb[k]), (k, np.argwhere(ra[k] != rb[k])[:5])
    for L, play in enumerate(launches_after, len(launches_before)):
        for e in (a, b):
            play(e)
            e.step(L, cascade=False, nb_ts_reco=10, auto_reset=True)
        xa, xb = _results(a), _results(b)
        for k in xa:
            assert xa[k].tobytes() == xb[k].tobytes(), (L, k)
        assert not a.episode()[0].any()
    a.close(); b.close()
    return changed


def test_truncated_lane_equals_a_host_reset_on_a_moved_topology_class():
    """14 substations, 5 lanes: the lanes split a substation (another topology class: the host must re-key them when they truncate), open a
    line (line cooldown, last_bus) and run over a thermal limit; then four more launches equal the twin's bit for bit"""
    n, limit = 5, 4
    split = {"set_bus": {36: 2, 37: 2, 38: 1, 39: 1, 40: 1}}

    def make():
        m, eng, ch = _sandbox(n, 5 * np.arange(n))
        th = ch["thermal_limits"].copy()
        th[[0, 4]] *= 0.05                                              # two lines above their limit at every step: overflow counters count
        eng.set_thermal_limits(th)
        eng.set_topo_rules(legal_rules=True, max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=3)
        eng.upload_topo_actions([split, {"set_line_status": [(7, -1)]}, {"set_line_status": [(7, 1)]}])
        return eng

    def act(k):
        return lambda e: e.set_lane_topo_actions(None if k < 0 else np.full(n, k))
    probe = make()
    act(0)(probe)
    probe.step(0, cascade=False, nb_ts_reco=10, auto_reset=True)
    assert not probe.episode()[0].any() and not probe.topo_action_flags()[0].any() and (probe.plan()["topology_classes"] or probe.plan()["busbars_per_block"] > 1), "the split must move the lanes"
    probe.close()
    changed = _twin_run(make, [act(-1), act(0), act(1), act(-1)], [act(-1), act(0), act(-1), act(2)], limit, False)
    assert {"topo", "overflow", "cooldown", "sub_cooldown", "last_bus", "steps"} <= set(changed), changed


def test_truncated_lane_equals_a_host_reset_on_the_118_substation_grid():
    """118 substations, 3 lanes, the dynamics on: redispatch, storage and curtailment actions of the recorded wcci episode, a line opened
    by an action; the truncated lanes must equal the twin in every dynamics row too"""
    fx = dict(np.load(golden_path("reward_wcci2022.npz")))
    n, limit = 3, 3
    T, row0 = fx["ch_load_p"].shape[0], int(fx["row"][0])

    def make():
        m, eng = _dyn_engine(fx, n)
        assert m.n_sub == 118 and m.dim_topo > 64 and m.n_line > 64
        eng.set_lane_chronics(lane_offset=np.full(n, row0 % T))
        th = fx["thermal_limit"].copy()
        th[[3, 100, 185]] *= 0.05
        eng.set_thermal_limits(th)
        eng.set_topo_rules(legal_rules=True, max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=3)
        eng.upload_topo_actions([{"set_line_status": [(120, -1)]}])
        return eng

    def dyn(i):
        def play(e):
            e.set_lane_actions(np.tile(fx["act_redisp"][i], (n, 1)), np.tile(fx["act_storage"][i], (n, 1)))
            if (fx["act_curtail"][i] != -1).any():
                e.set_lane_curtailment(np.tile(fx["act_curtail"][i], (n, 1)))
        return play

    def line(e):
        e.set_lane_topo_actions(np.zeros(n, np.int64))
    changed = _twin_run(make, [dyn(0), line, dyn(2)], [dyn(0), dyn(1), line, dyn(3)], limit, True)
    # (last_bus is not among them: an opened line keeps its last known busbars)
    assert {"topo", "overflow", "cooldown", "steps", "env_target", "env_actual", "env_charge", "env_curtail_limit"} <= set(changed), changed


def _returns_run(eng, n, limits, steps, perm=None):
    """`steps` launches with every 29th chronics row unservable; returns (rewards [steps, n, slots], stats, ends per launch)"""
    rews, ends = [], []
    for t in range(steps):
        eng.step(t, cascade=False, nb_ts_reco=10, auto_reset=True)
        rews.append(eng.rewards())
        ends.append(eng.episode_ends())
    return np.array(rews), eng.episode_stats(), ends


@pytest.mark.parametrize("n,n_slot", [(1, 1), (6, 8)])
def test_returns_equal_a_sequential_float64_sum(n, n_slot):
    """return_running / return_last against a sequential numpy float64 sum of the engine's own float32 rewards, bit for bit, across three
    episodes and more (per-lane limits 3 .. 8, a game over where a lane reads an unservable chronics row); with 6 lanes the same bits under
    a lane permutation and through two shards"""
    from grid2op_amd.sharding import ShardedEngine
    from test_gpu_alert import BAD_AT, BAD_EVERY, BAD_SCALE
    steps = 26
    offsets = 11 + 2 * np.arange(n)
    limits = (3 + np.arange(n)).astype(np.int32)
    slots = SLOTS8[:n_slot]

    def run(order, factory=None):
        m, eng, ch = _sandbox(n, offsets[order], factory)
        for key in ("load_p", "load_q"):
            ch[key] = ch[key].copy()
            ch[key][BAD_AT::BAD_EVERY] *= BAD_SCALE
        eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
        eng.set_rewards([(k, list(q)) for k, q in slots])
        eng.set_episode_limit(limits[order])
        out = _returns_run(eng, n, limits[order], steps)
        eng.close()
        return out
    ident = np.arange(n)
    rews, st, ends = run(ident)
    run_ref, last_ref = np.zeros((n, n_slot)), np.zeros((n, n_slot))
    n_ep, len_last, n_term = np.zeros(n, int), np.zeros(n, int), 0
    for t in range(steps):
        for k in range(n):
            for s in range(n_slot):
                run_ref[k, s] = run_ref[k, s] + np.float64(rews[t, k, s])
            if ends[t]["terminated"][k] or ends[t]["truncated"][k]:
                last_ref[k], run_ref[k] = run_ref[k].copy(), 0.0
                n_ep[k] += 1
                len_last[k] = ends[t]["length"][k]
                n_term += int(ends[t]["terminated"][k])
                assert ends[t]["length"][k] == (limits[k] if ends[t]["truncated"][k] else ends[t]["length"][k]) and ends[t]["length"][k] >= 1
    assert st["return_running"].tobytes() == run_ref.tobytes() and st["return_last"].tobytes() == last_ref.tobytes()
    assert np.array_equal(st["n_episodes"], n_ep) and np.array_equal(st["length_last"], len_last) and (n_ep >= 3).all()
    assert n_term >= 1 and np.abs(last_ref).sum() > 0
    if n == 1:
        return
    perm = np.random.default_rng(5).permutation(n)
    _, st_p, _ = run(perm)
    for key in st:
        assert st_p[key].tobytes() == st[key][perm].tobytes(), key
    from grid2op_amd.engine import PowerFlowEngine
    _, st_s, _ = run(ident, factory=lambda mm, k: ShardedEngine(mm, k, devices=[0, 0], engine_factory=lambda m_, n_, dev, nbb: PowerFlowEngine(
        m_, n_lanes=n_, device=0, n_busbar=nbb)))
    for key in st:
        assert np.asarray(st_s[key]).tobytes() == st[key].tobytes(), key


def test_flags_corner_cases_reset_and_copy():
    """6 lanes: a step that fails AT the limit is terminated, not truncated; without auto_reset a truncated lane stays as it is and
    re-flags while its statistics roll over once; reset zeroes the buffers, copy_lanes copies them; the views alias them"""
    from test_gpu_alert import BAD_AT, BAD_EVERY, BAD_SCALE
    n = 6
    m, eng, ch = _sandbox(n, np.zeros(n, int))
    for key in ("load_p", "load_q"):
        ch[key] = ch[key].copy()
        ch[key][BAD_AT::BAD_EVERY] *= BAD_SCALE
    eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    # lane k reads row t + off[k]: lanes 0-2 meet the unservable row at their 4th launch, lanes 3-5 never
    off = np.array([BAD_AT - 3] * 3 + [BAD_AT + 1] * 3)
    eng.set_lane_chronics(lane_offset=off)
    eng.set_rewards([R.L2RPN, (R.GAMEPLAY, [-1.0, 1.0])])
    limits = np.array([4, 3, 0, 4, 3, 0], np.int32)                       # lane 0 fails AT its limit, lane 1 after a truncation, lane 2 without a limit
    eng.set_episode_limit(limits, per_timestep=2.0)
    hist = []
    for t in range(6):
        eng.step(t, cascade=False, nb_ts_reco=10, auto_reset=False)
        hist.append((eng.episode_ends(), eng.episode(), eng.rewards(), eng.episode_stats()))
    e4, ep4 = hist[3][0], hist[3][1]
    assert ep4[0][:3].all() and not ep4[0][3:].any()                      # the 4th launch failed on lanes 0-2
    assert e4["terminated"][0] and not e4["truncated"][0] and e4["length"][0] == 4 and e4["duration_reward"][0] == np.float32(4 / (4 * 2.0))
    assert e4["terminated"][2] and e4["length"][2] == 4 and e4["duration_reward"][2] == np.float32(4.0)      # no limit: the length itself
    assert e4["truncated"][3] and not e4["terminated"][3] and e4["length"][3] == 4 and e4["duration_reward"][3] == np.float32(0.5)
    assert hist[3][2][3, 0] == 0.0 and hist[2][2][3, 0] > 0.0               # L2RPNReward is 0 on the truncated step
    for t in (2, 3, 4, 5):                                                # lane 4 (limit 3, left alone) re-flags at every later launch ...
        assert hist[t][0]["truncated"][4] and hist[t][0]["length"][4] == t + 1 and hist[t][1][1][4] == t + 1
        assert hist[t][3]["n_episodes"][4] == 1 and hist[t][3]["length_last"][4] == 3      # ... and rolled over once
    assert not any(hist[t][0]["truncated"][5] or hist[t][0]["terminated"][5] for t in range(6)) and hist[5][3]["n_episodes"][5] == 0
    want = np.float64(0.0)
    for t in range(3):
        want = want + np.float64(hist[t][2][4, 0])
    assert hist[5][3]["return_last"][4, 0] == want
    # copy and reset
    st = eng.episode_stats()
    eng.copy_lanes(4, 5, 1)
    st2, ends2 = eng.episode_stats(), eng.episode_ends()
    for key in st:
        assert st2[key][5].tobytes() == st[key][4].tobytes(), key
    assert ends2["truncated"][5] and ends2["length"][5] == ends2["length"][4]
    v = eng.episode_views()
    eng.sync()
    assert v["limit"].cpu().numpy().tolist() == [4, 3, 0, 4, 3, 3] and v["truncated"].cpu().numpy().astype(bool).tolist() == ends2["truncated"].tolist()
    assert v["return_last"].cpu().numpy().tobytes() == st2["return_last"].tobytes() and v["n_episodes"].cpu().numpy().tolist() == st2["n_episodes"].tolist()
    eng.reset(3, 3)
    st3, ends3 = eng.episode_stats(), eng.episode_ends()
    for key in st3:
        assert not st3[key][3:].any() and st3[key][:3].tobytes() == st2[key][:3].tobytes(), key
    for key in ends3:
        assert not ends3[key][3:].any(), key
    eng.step(6, cascade=False, nb_ts_reco=10, auto_reset=False)          # the reset lanes count from 0 again
    assert (eng.episode_ends()["length"][3:] == 0).all() and not eng.episode_ends()["truncated"][3:].any()
    eng.close()


def test_off_means_off():
    """never enabled / enabled with far limits then switched off / far limits left on: a 6-step sequence with opponent, alerts and rewards
    gives bit-identical outputs, rewards and alert rewards; a multi-step launch is refused while on and accepted after off"""
    from grid2op_amd.engine import GridPFError
    from test_gpu_alert import GEO
    n = 5

    def run(mode):
        m, eng, _ = _sandbox(n, 3 * np.arange(n))
        eng.set_opponent(**dict(GEO, lines=[0, 3, 7, 11, 15], attack_cooldown=1, seed=11))
        eng.set_alerts(3)
        eng.set_rewards([R.L2RPN, R.LINES_CAPACITY, (R.GAMEPLAY, [-1.0, 1.0])])
        if mode != "never":
            eng.set_episode_limit(1000, alert_end_bonus=5.0)
            with pytest.raises(GridPFError, match="with an episode limit set"):
                eng.step(0, n_steps=2, nb_ts_reco=10)
        if mode == "on_off":
            eng.set_episode_limit(None)
            with pytest.raises(GridPFError, match="episode limits are off"):
                eng.episode_ends()
        got = []
        for t in range(6):
            eng.set_lane_alerts(np.full(n, (t * 5) % 32, np.uint64))
            eng.step(t, cascade=False, nb_ts_reco=10, auto_reset=True)
            r = eng.results(with_bus=False)
            got.append((r.out.tobytes(), r.topo_vect.tobytes(), eng.rewards().tobytes(), eng.alert_reward().tobytes(), eng.alert_state().tobytes()))
        if mode == "on_off":
            eng.set_opponent()
            eng.step(6, n_steps=2)                                      # accepted again
        eng.close()
        return got
    never = run("never")
    assert run("on_off") == never and run("far") == never
