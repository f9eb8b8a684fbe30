"""The N-1 screen of the batched acting path on the device (include/gridpf.h gpf_set_n1_screen, grid2op_amd/csrc/gridpf_n1.hpp): the three
recordings of the unmodified reference's N1Reward replayed on 65 environment lanes (tests/golden/n1_*.npz), the screen against the long
way round (`fanout_n1` per environment and `runpf` on a twin engine), environment lanes that the screen leaves alone, contingency lanes
that follow their environment's topology class, the constants and the summary, the GPF_RW_N1 reward slot, two shards, stability and the
off path.

Bounds (tests/n1_ref.py): a value against the restatement on the device's OWN contingency-lane results row, and the constants 0 and -1,
bit for bit; a finite value against the recording within max_l tol(a_or_l) / max(th_l, 1) + one float32 spacing, tol the float32 output
tolerance tests/test_gpu_parity.py applies to a_or.

Shapes: 14 substations with 1, 5 and 65 environments x 1, 3 and 20 watched lines (an odd n_env misaligns the contingency range with the
instance groups, n_env x K not a multiple of 4 leaves a partial last block of the reduce kernel), 3 x 59 on 36 substations, 3 x 186 on 118
(three trips of the strided loop, two wavefronts per instance)."""
import dataclasses
import os
import sys

import numpy as np
import pytest

import n1_ref as N
from conftest import golden_path

pytestmark = pytest.mark.gpu

N_ENV, STAGGER = 65, 4
GRIDS = {14: "l2rpn_case14_sandbox", 36: "l2rpn_neurips_2020_track1", 118: "l2rpn_wcci_2022_dev"}


def _engine(grid, n_lanes, offsets=None):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path(f"{grid}.grid.npz"))
    ch = dict(np.load(golden_path(f"{grid}.chronics.npz")))
    if "prod_v" not in ch:                                              # (the 118-substation tables hold no voltage set-points)
        ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
    eng = PowerFlowEngine(m, n_lanes=n_lanes, device=0)
    eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    eng.set_lane_chronics(lane_offset=7 * np.arange(n_lanes) if offsets is None else np.asarray(offsets))
    eng.set_thermal_limits(ch["thermal_limits"])
    return m, eng, ch


def _same(a, b):
    """two LaneResults, every array bit for bit"""
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray):
            assert x.tobytes() == y.tobytes(), f.name


def _restated(eng, n_env, K, thermal, done):
    """the restatement on the device's own contingency-lane rows: [n_env, K]"""
    r = eng.results(n_env, n_env * K, with_bus=False)
    return np.array([N.values(r.a_or[i * K:(i + 1) * K], thermal, bool(done[i]), r.converged[i * K:(i + 1) * K]) for i in range(n_env)], np.float32)


def _long_way(twin, eng, n_env, lines):
    """today's API on a twin engine: the environments' inputs, `fanout_n1` per environment, one `runpf` of the contingency lanes"""
    K = len(lines)
    topo, sb = eng.get_topology(0, n_env)
    twin.set_injections(eng.get_injections(0, n_env))
    twin.set_topology(topo, sb)
    for i in range(n_env):
        twin.fanout_n1(i, n_env + i * K, lines)
    twin.runpf(n_env, n_env * K)
    return twin.results(n_env, n_env * K)


SHAPES = [(14, n, k) for n in (1, 5, 65) for k in (1, 3, 20)] + [(36, 3, 59), (118, 3, 186)]


@pytest.mark.parametrize("n_sub,n_env,K", SHAPES)
def test_same_result_as_the_long_way_round(n_sub, n_env, K):
    """One launch with the screen on against `fanout_n1` + `runpf(n_env, n_env * K)` on a twin that holds the same lane numbers: the whole
    results rows of the contingency lanes and the K values of every environment are bit-equal, and a value is the restatement's on its row."""
    n = n_env * (1 + K)
    m, eng, ch = _engine(GRIDS[n_sub], n)
    _, twin, _ = _engine(GRIDS[n_sub], n)
    lines = (np.arange(K) * 7 + 2) % m.n_line if K < m.n_line else np.arange(m.n_line)
    eng.set_n1_screen(lines, n_env)
    eng.step(1)
    got = eng.results(n_env, n_env * K)
    _same(got, _long_way(twin, eng, n_env, lines))
    done = eng.episode()[0]
    vals = eng.n1_values()
    assert vals.shape == (n_env, K) and vals.tobytes() == _restated(eng, n_env, K, ch["thermal_limits"], done).tobytes()
    # the contingency lane is the environment with the line out: its topology row says so
    tv = eng.results(0, n_env, with_bus=False).topo_vect
    for i in (0, n_env - 1):
        for k in (0, K - 1):
            want = tv[i].copy()
            want[[m.line_or_pos_topo_vect[lines[k]], m.line_ex_pos_topo_vect[lines[k]]]] = -1
            assert np.array_equal(got.topo_vect[i * K + k], want), (i, k)
    s = eng.n1_summary()
    for i in range(n_env):
        w, a, ni, nd = N.summary(vals[i])
        assert (s["worst"][i].tobytes(), s["arg_worst"][i], s["n_insecure"][i], s["n_diverged"][i]) == (w.tobytes(), a, ni, nd), i
    v = eng.n1_views()
    eng.sync()
    assert np.array_equal(v["values"].cpu().numpy(), vals) and np.array_equal(v["lines"].cpu().numpy(), lines) and np.array_equal(v["arg_worst"].cpu().numpy(), s["arg_worst"])
    eng.close(); twin.close()


def _acting_engine(n_lanes, n_env, screen_lines):
    """topology actions with rules, the opponent, alerts, rewards and an episode limit; the screen when lines are given"""
    import opponent_ref as OR
    import reward_ref as R
    sys.path.insert(0, os.path.dirname(golden_path("x")))
    from make_reward_fixtures import topo_table
    m, eng, ch = _engine(GRIDS[14], n_lanes, 3 * np.arange(n_lanes))
    table, n0 = topo_table(m, 3)
    eng.set_topo_rules(legal_rules=True, max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=3)
    eng.upload_topo_actions(table)
    eng.set_opponent(kind=OR.GEOMETRIC, attack_hazard_rate=0.3, recovery_rate=0.5, recovery_minimum_duration=1, pmax_pmin_ratio=4.0, episode_max_time=100,
                     schedule_cap=6, init_budget=3.0, budget_per_ts=0.7, attack_duration=3, draw_source=OR.PHILOX, lines=[0, 3, 7, 11, 15], attack_cooldown=1, seed=11)
    eng.set_alerts(3)
    eng.set_rewards([R.L2RPN, R.LINES_CAPACITY, (R.GAMEPLAY, [-1.0, 1.0])])
    lim = np.zeros(n_lanes, np.int32)
    lim[:n_env] = 3 + np.arange(n_env) % 3
    eng.set_episode_limit(lim)
    if screen_lines is not None:
        eng.set_n1_screen(screen_lines, n_env)
    return m, eng, ch, table, n0


@pytest.mark.parametrize("n_env", [8, 7, 5])
def test_environment_lanes_are_undisturbed(n_env):
    """Screen on against screen off on twin engines of the same lanes: five launches with device topology actions, the opponent, alerts,
    rewards and an episode limit under auto_reset.  Every result, reward, flag, state and observation vector of the environment lanes is
    bit-identical -- also at an odd n_env, where the environment range does not end on an instance group (two lanes per wavefront on
    this grid) and runs from a ghost-padded lane list on the groups of the whole batch."""
    import torch
    from grid2op_amd.obs_spec import ObsSpec
    lines = [2, 9, 18]
    n = n_env * (1 + len(lines))
    got = {}
    for mode in ("on", "off"):
        m, eng, ch, table, n0 = _acting_engine(n, n_env, lines if mode == "on" else None)
        eng.set_obs_spec(ObsSpec(m, ["rho", "line_status", "topo_vect", "gen_p", "load_p", "a_or", "time_before_cooldown_line"]))
        views = eng.device_views()
        seen = []
        for t in range(5):
            act = np.full(n, -1, np.int32)
            act[:n_env] = (np.arange(n_env) * 5 + t * 3) % n0 if t != 3 else -1
            with torch.cuda.stream(views["stream"]):
                views["act_topo"].copy_(torch.from_numpy(act.reshape(-1, 1)).to(views["act_topo"].device))
            eng.topo_actions_on_device()
            eng.set_lane_alerts(np.where(np.arange(n) < n_env, (t * 5) % 32, 0).astype(np.uint64))
            eng.step(t, cascade=False, nb_ts_reco=10, auto_reset=True)
            r = eng.results(0, n_env)
            ill, amb = eng.topo_action_flags(0, n_env)
            ends = eng.episode_ends(0, n_env)
            seen.append(tuple(x.tobytes() for x in (r.out, r.topo_vect, r.status, r.line_status, r.bus_vm, r.bus_va, eng.rewards(0, n_env), eng.alert_reward(0, n_env),
                                                   eng.alert_state(0, n_env), ill, amb, ends["terminated"], ends["truncated"], ends["length"], eng.episode(0, n_env)[1],
                                                   eng.cooldown(0, n_env), eng.sub_cooldown(0, n_env), eng.get_topology(0, n_env)[0], eng.opponent_attack_lines(0, n_env),
                                                   eng.episode_stats(0, n_env)["return_running"], eng.observation_vector_host(0, n_env)) + eng.step_outputs(0, n_env)))
        got[mode] = seen
        if mode == "on":
            assert np.isfinite(eng.n1_values()).all()
        eng.close()
    for t, (a, b) in enumerate(zip(got["on"], got["off"])):
        assert a == b, (t, [i for i, (x, y) in enumerate(zip(a, b)) if x != y])


def test_contingency_lanes_follow_their_environments_topology_class():
    """Lane 1 moves to a split topology by a device-side action, holds it three steps, then fails on a line it opens itself and auto-resets;
    lane 0 (another class) sits in the same launches, and an episode limit is set.  At every step the K values equal the twin's, which is keyed by `set_topology`."""
    sys.path.insert(0, os.path.dirname(golden_path("x")))
    from make_reward_fixtures import topo_table
    n_env, n_steps = 3, 7
    m, eng, ch = _engine(GRIDS[14], n_env * 21, 5 * np.arange(n_env * 21))
    K = m.n_line
    lines = np.arange(K)
    _, twin, _ = _engine(GRIDS[14], n_env * 21)
    table, n0 = topo_table(m, 3)
    eng.set_topo_rules(legal_rules=False)
    eng.upload_topo_actions(table)
    eng.set_n1_screen(lines, n_env)
    eng.set_episode_limit(1000)                                     # (the re-keying read-back of the reset then also runs behind episode_kernel)
    split_seen, reset_seen, kill = 0, 0, -1
    for t in range(n_steps):
        act = np.full(n_env * 21, -1, np.int32)
        if t == 1:
            act[1] = 0                                              # the table's first entry: a substation split
        if kill >= 0 and t == 5:
            act[1] = n0 + kill                                      # open a line whose loss does not converge: game over, auto-reset
        eng.set_lane_topo_actions(act)
        eng.step(t, cascade=False, nb_ts_reco=10, auto_reset=True)
        done = eng.episode()[0][:n_env]
        vals = eng.n1_values()
        if not done[1]:
            want = _long_way(twin, eng, n_env, lines)
            _same(eng.results(n_env, n_env * K), want)
        assert vals.tobytes() == _restated(eng, n_env, K, ch["thermal_limits"], done).tobytes(), t
        split = bool((eng.get_topology(1, 1)[0] == 2).any())
        split_seen += int(split)
        if done[1]:
            reset_seen += 1
            assert (vals[1] == 0).all() and not split                 # the failed lane: 0 everywhere, back on its reset topology
        if t == 4:
            ls = eng.results(1, 1, with_bus=False).line_status[0]
            cand = [k for k in range(K) if vals[1][k] == -1 and ls[k]]
            assert cand, "no diverging contingency in the split state"
            kill = cand[0]
    assert split_seen >= 3 and reset_seen == 1, (split_seen, reset_seen)
    eng.close(); twin.close()


def test_plans_follow_a_host_side_class_change_behind_a_whole_batch_plan():
    """`set_topology` moves an environment lane to a split topology, then `runpf()` / `plan()` over all lanes re-make the batch's plan
    before the next launch: the screen's own plans are re-made with it (the lane steps on its new class, its contingency lanes take the
    class over).  Against the twin, keyed by `set_topology`, at every launch."""
    sys.path.insert(0, os.path.dirname(golden_path("x")))
    from make_reward_fixtures import topo_table
    n_env, K = 5, 20
    n = n_env * (1 + K)
    m, eng, ch = _engine(GRIDS[14], n)
    _, twin, _ = _engine(GRIDS[14], n)
    lines = np.arange(K)
    table, _ = topo_table(m, 3)
    eng.set_n1_screen(lines, n_env)
    eng.step(1)
    base = eng.get_topology(0, n_env)[0]
    for t, (lane, how) in enumerate([(1, "runpf"), (3, "plan"), (1, "runpf")], start=2):
        row = eng.candidate_topologies(base[lane], [table[0]])[0] if t < 4 else base[lane]     # split, split, merged again
        assert (row == 2).any() == (t < 4)
        eng.set_topology(row[None], lane0=lane)
        if how == "runpf":
            eng.runpf()                                              # a whole-batch plan between the class change and the launch
        else:
            eng.plan()
        eng.step(t)
        assert eng.results(0, n_env, with_bus=False).converged.all(), t
        assert np.array_equal(eng.get_topology(lane, 1)[0][0], row), t
        _same(eng.results(n_env, n_env * K), _long_way(twin, eng, n_env, lines))
        assert eng.n1_values().tobytes() == _restated(eng, n_env, K, ch["thermal_limits"], eng.episode()[0]).tobytes(), t
    eng.close(); twin.close()


@pytest.mark.parametrize("cursor_first", [True, False])
def test_contingency_lanes_start_no_scenario(cursor_first):
    """the chronics cursor and the screen together, in either order, and `set_lane_chronics` after both (it clears every lane's skip byte:
    the screen puts its contingency lanes' back): the environments start scenarios, the contingency lanes never do"""
    n_env, lines = 3, [1, 6]
    n = n_env * 3
    m, eng, ch = _engine(GRIDS[14], n)
    for what in (("cursor", "screen") if cursor_first else ("screen", "cursor")):
        if what == "cursor":
            eng.set_chronics_cursor(first_row=1)
        else:
            eng.set_n1_screen(lines, n_env)
    for t in range(3):
        if t == 1:
            eng.set_lane_chronics(lane_offset=np.zeros(n, np.int64))
        eng.step(t)
        st = eng.chronics_cursor_state()
        assert (st.n_started[:n_env] >= 1).all() and (st.n_started[n_env:] == 0).all(), (t, st.n_started)
    eng.set_n1_screen(None)                                           # off: the lanes are ordinary lanes again
    eng.step(3)
    assert (eng.chronics_cursor_state().n_started >= 1).all()
    eng.close()


def test_replay_of_the_recorded_opponent_attacks():
    """n1_case14_attack.npz on 65 environment lanes in step: a RandomLineOpponent on the recorded draws attacks, the agent reconnects.
    The attacked line is out in the row the step leaves (never in a row the agent sent): the attack is the recorded one at every launch,
    the attacked line's own contingency is the base case, and all 20 values hold the recording's bound."""
    from grid2op_amd.chronics import chronics_table
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from test_opponent_cpu import fixture_config
    fx = dict(np.load(golden_path("n1_case14_attack.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    K = m.n_line
    n = N_ENV * (1 + K)
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    tab = chronics_table({k[len("chron_"):]: fx[k] for k in fx if k.startswith("chron_")})
    eng.upload_chronics(tab)
    T = tab.shape[1]
    th = fx["thermal_limit"]
    eng.set_thermal_limits(th)
    p = [int(x) for x in fx["params"]]
    eng.set_topo_rules(legal_rules=True, max_sub_changed=p[0], max_line_status_changed=p[1], cooldown_sub=p[2], cooldown_line=p[3])
    acts = []
    for l in range(K):                                                  # entry 2 l: reconnect line l, entry 2 l + 1: open it
        acts += [{"set_line_status": [(l, 1)]}, {"set_line_status": [(l, -1)]}]
    assert not eng.upload_topo_actions(acts).any()
    eng.set_opponent(**fixture_config(fx))
    eng.upload_opponent_draws(np.tile(fx["draws"], (n, 1)))
    eng.set_n1_screen(np.arange(K), N_ENV)
    used = [int(x) for x in fx["scenarios_used"]]
    attacked, checked = 0, 0
    for i in range(len(fx["is_reset"])):
        eng.set_lane_chronics(lane_table=np.full(n, used.index(int(fx["scenario"][i]))), lane_offset=np.full(n, (int(fx["row"][i]) - i) % T))
        a = int(fx["agent_line"][i])
        act = np.full(n, -1, np.int32)
        if a >= 0:
            act[:N_ENV] = 2 * a + (0 if fx["agent_value"][i] > 0 else 1)
        eng.set_lane_topo_actions(act)
        eng.step(i, cascade=False, nb_ts_reco=p[4], auto_reset=True)
        if fx["is_reset"][i]:
            continue
        hit = eng.opponent_attack_lines(0, N_ENV)
        want_hit = np.zeros(K, bool)
        if fx["info_line"][i] >= 0:
            want_hit[fx["info_line"][i]] = True
        assert (hit == want_hit).all(), i
        r_env = eng.results(0, N_ENV, with_bus=False)
        assert (r_env.line_status == fx["line_status"][i]).all() and not eng.episode()[0][:N_ENV].any(), i
        vals = eng.n1_values()
        assert all(vals[q].tobytes() == vals[0].tobytes() for q in range(N_ENV)), i
        r = eng.results(N_ENV, K, with_bus=False)
        assert vals[0].tobytes() == N.values(r.a_or, th, False, r.converged).tobytes(), i
        for k in range(K):
            rec = fx["n1"][i][k]
            if rec == N.DIVERGED or vals[0][k] == N.DIVERGED:
                assert vals[0][k].tobytes() == rec.tobytes(), (i, k, vals[0][k], rec)
            else:
                assert abs(float(vals[0][k]) - float(rec)) <= N.bound(r.a_or[k], th, rec), (i, k, vals[0][k], rec)
            checked += 1
        if fx["info_line"][i] >= 0:                                     # the attacked line's own contingency: the step's own max(a_or / th)
            attacked += 1
            assert vals[0][fx["info_line"][i]].tobytes() == N.value(r_env.a_or[0], th).tobytes(), i
    assert attacked >= 8 and checked == K * int((fx["is_reset"] == 0).sum()), (attacked, checked)
    eng.close()


def test_constants_and_summary():
    """A failed lane and a truncated lane give 0 in all K entries; a line whose loss does not converge gives -1, n_diverged counts it and
    worst / arg_worst follow the rule; a watched line that is already out gives the base case's own max(a_or / th)."""
    n_env, K = 5, 20
    m, eng, ch = _engine(GRIDS[14], n_env * (1 + K))
    th = ch["thermal_limits"]
    eng.set_n1_screen(np.arange(K), n_env)
    lim = np.zeros(n_env * (1 + K), np.int32)
    lim[2] = 2                                                          # lane 2 is truncated by the second launch
    eng.set_episode_limit(lim)
    eng.disconnect_line(3, 4)                                           # lane 3: watched line 4 is out already
    eng.step(1)
    vals, s = eng.n1_values(), eng.n1_summary()
    assert (vals == -1).any(), "the sandbox has a line whose loss does not converge"
    for i in range(n_env):
        assert s["n_diverged"][i] == (vals[i] == -1).sum() and s["n_insecure"][i] == ((vals[i] == -1) | (vals[i] > 1)).sum()
        if s["n_diverged"][i]:
            assert s["arg_worst"][i] == np.flatnonzero(vals[i] == -1)[0] and s["worst"][i] == -1
        else:
            assert s["arg_worst"][i] == np.argmax(vals[i]) and s["worst"][i] == vals[i].max()
    base = eng.results(3, 1, with_bus=False)
    assert not base.line_status[0][4] and vals[3][4].tobytes() == N.value(base.a_or[0], th).tobytes()
    # a failed lane: lane 4 loses a line whose loss does not converge, by the host
    k_bad = int(np.flatnonzero(vals[4] == -1)[0])
    eng.disconnect_line(4, k_bad)
    eng.step(2)
    vals, done, ends = eng.n1_values(), eng.episode()[0], eng.episode_ends()
    assert done[4] and ends["truncated"][2] and not done[2]
    for i in (2, 4):
        assert vals[i].tobytes() == np.zeros(K, np.float32).tobytes(), i
    s = eng.n1_summary()
    assert s["worst"][4] == 0 and s["arg_worst"][4] == 0 and s["n_insecure"][4] == 0 and s["n_diverged"][4] == 0
    assert (vals[0] != 0).all()
    eng.close()


def test_reward_slot_returns_and_rewards_eval():
    """GPF_RW_N1 equals its table entry, the float64 episode return is the sequential sum of the slot, `rewards_eval` returns the entry."""
    import reward_ref as R
    from grid2op_amd.engine import RW_N1, GridPFError
    n_env, lines = 5, [2, 9, 13]
    n = n_env * 4
    m, eng, ch = _engine(GRIDS[14], n)
    with pytest.raises(GridPFError, match="needs the N-1 screen"):
        eng.set_rewards([(RW_N1, [0])])
    eng.set_n1_screen(lines, n_env)
    with pytest.raises(GridPFError, match="index into the 3 watched lines"):
        eng.set_rewards([(RW_N1, [3])])
    eng.set_rewards([R.L2RPN, (RW_N1, [2]), (RW_N1, [0])])
    with pytest.raises(GridPFError, match="set the rewards anew"):
        eng.set_n1_screen(None)
    eng.set_episode_limit(100)
    total = np.zeros((n_env, 2), np.float64)
    for t in range(4):
        eng.step(t)
        vals, rew = eng.n1_values(), eng.rewards()
        assert rew[:n_env, 1].tobytes() == vals[:, 2].tobytes() and rew[:n_env, 2].tobytes() == vals[:, 0].tobytes(), t
        assert (rew[n_env:, 1:] == 0).all()
        total += rew[:n_env, 1:].astype(np.float64)
        assert eng.episode_stats(0, n_env)["return_running"][:, 1:].tobytes() == total.tobytes(), t
    ev = eng.rewards_eval(0, n).cpu().numpy()
    assert ev[:n_env, 1].tobytes() == vals[:, 2].tobytes() and ev[:n_env, 2].tobytes() == vals[:, 0].tobytes() and ev[:, 0].tobytes() == rew[:, 0].tobytes()
    with pytest.raises(GridPFError, match="one-step launch"):
        eng.step(5, n_steps=2)
    eng.close()


def test_two_shards_on_one_device_equal_one_engine_per_shard():
    from grid2op_amd.sharding import ShardedEngine
    n_env, lines = 4, [1, 6, 18]
    n = n_env * 4
    m, a, ch = _engine(GRIDS[14], n, 7 * np.arange(n))
    _, b, _ = _engine(GRIDS[14], n, 7 * (n + np.arange(n)))
    se = ShardedEngine(m, 2 * n, devices=[0, 0])
    se.upload_chronics(a.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    se.set_lane_chronics(lane_offset=7 * np.arange(2 * n))
    se.set_thermal_limits(ch["thermal_limits"])
    for e in (a, b, se):
        e.set_n1_screen(lines, n_env)
        e.step(2)
    want = np.concatenate([a.n1_values(), b.n1_values()])
    assert se.n1_values().tobytes() == want.tobytes() and se.n1_values(n, n).tobytes() == b.n1_values().tobytes()
    assert se.n1_summary()["arg_worst"].tobytes() == np.concatenate([a.n1_summary()["arg_worst"], b.n1_summary()["arg_worst"]]).tobytes()
    assert [tuple(v["values"].shape) for v in se.n1_views()] == [(n_env, 3)] * 2
    a.close(); b.close(); se.close()


def test_two_runs_and_a_permutation_of_the_environments():
    n_env, K = 6, 20
    n = n_env * (1 + K)
    perm = np.array([4, 0, 5, 2, 1, 3])
    runs = []
    for order in (np.arange(n_env), np.arange(n_env), perm):
        off = np.zeros(n, np.int64)
        off[:n_env] = 11 * order
        m, eng, _ = _engine(GRIDS[14], n, off)
        eng.set_n1_screen(np.arange(K), n_env)
        eng.step(1)
        eng.step(2)
        runs.append(eng.n1_values())
        eng.close()
    assert runs[0].tobytes() == runs[1].tobytes()
    assert runs[2].tobytes() == runs[0][perm].tobytes()


def test_off_path_is_bit_identical_to_an_engine_without_a_screen():
    n = 24
    out = []
    for touched in (False, True):
        m, eng, _ = _engine(GRIDS[14], n)
        if touched:
            eng.set_n1_screen([3, 5], 8)
            eng.set_n1_screen([], None)
        eng.step(1)
        eng.step(2, n_steps=2)
        r = eng.results()
        out.append((r.out.tobytes(), r.status.tobytes(), r.topo_vect.tobytes(), tuple(sorted(eng.counters().items()))))
        if touched:
            from grid2op_amd.engine import GridPFError
            with pytest.raises(GridPFError, match="the N-1 screen is off"):
                eng.n1_values()
        eng.close()
    assert out[0] == out[1]


# ---- the recordings ------------------------------------------------------------------------------------------------------------------
def _check_recorded(eng, K, thermal, vals, done, act, jj, fx, what):
    """one launch of a staggered replay: the lanes of a stagger group are bit-identical; the group's first lane against the recording"""
    r = eng.results(N_ENV, N_ENV * K, with_bus=False)
    assert vals.tobytes() == np.array([N.values(r.a_or[i * K:(i + 1) * K], thermal, bool(done[i]), r.converged[i * K:(i + 1) * K])
                                       for i in range(N_ENV)], np.float32).tobytes(), what
    n_checked = 0
    for g in range(STAGGER):
        lanes = np.arange(g, N_ENV, STAGGER)
        k0 = int(lanes[0])
        if not act[k0]:
            continue
        assert all(vals[q].tobytes() == vals[k0].tobytes() for q in lanes), (what, g)
        rec = fx["n1"][jj[k0]]
        for k in range(K):
            if rec[k] in (N.DONE, N.DIVERGED) or vals[k0][k] in (N.DONE, N.DIVERGED):
                assert vals[k0][k].tobytes() == rec[k].tobytes(), (what, g, k, vals[k0][k], rec[k])
            else:
                b = N.bound(r.a_or[k0 * K + k], thermal, rec[k])
                assert abs(float(vals[k0][k]) - float(rec[k])) <= b, (what, g, k, vals[k0][k], rec[k], b)
            n_checked += 1
    return n_checked


def test_replay_of_the_recorded_topology_episodes():
    """n1_case14.npz: 65 environment lanes play the recorded launches, lane k starting k mod 4 launches late, all 20 lines watched."""
    from grid2op_amd.chronics import chronics_table
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    sys.path.insert(0, os.path.dirname(golden_path("x")))
    from make_reward_fixtures import topo_table
    fx = dict(np.load(golden_path("n1_case14.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    K = m.n_line
    n = N_ENV * (1 + K)
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    tab = chronics_table({k[len("chron_"):]: fx[k] for k in fx if k.startswith("chron_")})
    eng.upload_chronics(tab)
    T = tab.shape[1]
    eng.set_thermal_limits(fx["thermal_limit"])
    p = [int(x) for x in fx["params"]]
    eng.set_topo_rules(legal_rules=True, max_sub_changed=p[0], max_line_status_changed=p[1], cooldown_sub=p[2], cooldown_line=p[3])
    table, n0 = topo_table(m, int(fx["table_seed"]))
    assert n0 == int(fx["n_table"]) and np.array_equal(eng.pack_actions(table)[0], fx["off"])
    eng.upload_topo_actions(table)
    eng.set_n1_screen(np.arange(K), N_ENV)
    used = [int(x) for x in fx["scenarios_used"]]
    n_rec = len(fx["done"])
    group = np.arange(N_ENV) % STAGGER
    checked = dict(values=0, game_over=0)

    def lanes_of(v, fill):
        full = np.full(n, fill, np.asarray(v).dtype)
        full[:N_ENV] = v
        return full
    for L in range(n_rec + STAGGER - 1):
        j = L - group
        act = (j >= 0) & (j < n_rec)
        jj = np.clip(j, 0, n_rec - 1)
        for k in np.flatnonzero(act & (j == 0)):
            eng.reset(int(k), 1)
        table_of = np.where(act, [used.index(int(s)) for s in fx["scenario"][jj]], 0)
        eng.set_lane_chronics(lane_table=lanes_of(table_of, 0), lane_offset=lanes_of(np.where(act, (fx["row"][jj] - L) % T, 0), 0))
        eng.set_lane_topo_actions(lanes_of(np.where(act, fx["played"][jj], -1).astype(np.int32), -1))
        eng.step(L, cascade=False, nb_ts_reco=p[4], auto_reset=True)
        done = eng.episode()[0][:N_ENV]
        want_done = np.where(act, fx["done"][jj], 0).astype(bool)
        assert np.array_equal(done[act], want_done[act]), (L, np.flatnonzero(done != want_done))
        is_step = act & (fx["is_reset"][jj] == 0)
        checked["values"] += _check_recorded(eng, K, fx["thermal_limit"], eng.n1_values(), done, is_step, jj, fx, L)
        checked["game_over"] += int(is_step[0] and done[0])
    assert checked["values"] >= STAGGER * K * 50 and checked["game_over"] >= 2, checked
    eng.close()


@pytest.mark.parametrize("tag", ["neurips36", "wcci2022"])
def test_replay_of_the_recorded_injection_episodes(tag):
    """n1_neurips36.npz (do-nothing steps, one thermal limit below 1 A) and n1_wcci2022.npz (redispatch and storage acting under the
    environment's dynamics), every line watched, on 65 environment lanes at staggered offsets.

    The acting episode is replayed by its recorded STATE, not by its actions: every step gets the reference's own actual dispatch
    (`set_lane_redispatch`) and storage power (the storage set-points of the injection row), with the engine's dynamics off.  Sent as
    actions through the dynamics the same steps leave another dispatch -- the engine projects a redispatch exactly where the reference's
    SLSQP stops short (tests/test_gpu_envdyn.py) --, so the environment's own flows differ from the recording before any line is out:
    `test_screen_under_the_dynamics_against_the_recorded_actions` measures that and holds the screen to its own rows there."""
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    fx = dict(np.load(golden_path(f"n1_{tag}.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    K = m.n_line
    n = N_ENV * (1 + K)
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"]))
    T = fx["ch_load_p"].shape[0]
    eng.set_thermal_limits(fx["thermal_limit"])
    acting = bool(fx["acting"])
    sto_cols = eng.inj_slices["storage_p"]
    eng.set_n1_screen(np.arange(K), N_ENV)
    n_rec, row0 = len(fx["done"]), int(fx["row"][0])
    group = np.arange(N_ENV) % STAGGER
    off = np.zeros(n, np.int64)
    off[:N_ENV] = (row0 - group) % T
    eng.set_lane_chronics(lane_offset=off)
    checked = 0
    for L in range(n_rec + STAGGER - 1):
        j = L - group
        act = (j >= 0) & (j < n_rec)
        jj = np.clip(j, 0, n_rec - 1)
        for k in np.flatnonzero(act & (j == 0)):
            eng.reset(int(k), 1)
        if acting:                                                      # the reference's dispatch and storage power of the step every lane plays
            delta = np.zeros((n, m.n_gen), np.float32)
            delta[:N_ENV] = np.where(act[:, None], fx["actual_dispatch"][jj], 0.0)
            eng.set_lane_redispatch(delta)
            inj = eng.get_injections(0, N_ENV)
            inj[:, sto_cols] = np.where(act[:, None], fx["storage_power"][jj], 0.0)
            eng.set_injections(inj, 0)
        eng.step(L)
        done = eng.episode()[0][:N_ENV]
        assert not done.any(), (L, np.flatnonzero(done))
        if acting:                                                      # the lanes hold the recorded storage power, and the contingency lanes took it over
            r0 = eng.results(0, 1, with_bus=False).out[0][eng.out_slices["storage_p"]]
            rc = eng.results(N_ENV, 1, with_bus=False).out[0][eng.out_slices["storage_p"]]
            want = fx["storage_power"][jj[0]] if act[0] else np.zeros_like(r0)
            assert np.abs(r0 - want).max() < 1e-3 and np.array_equal(r0, rc), L
        checked += _check_recorded(eng, K, fx["thermal_limit"], eng.n1_values(), done, act, jj, fx, L)
    assert checked == STAGGER * K * n_rec, checked
    if acting:
        assert np.abs(fx["actual_dispatch"]).max() > 5.0 and np.abs(fx["storage_power"]).sum(1).min() > 50.0      # (MW: both really act)
    eng.close()


def test_screen_under_the_dynamics_against_the_recorded_actions():
    """n1_wcci2022.npz sent as ACTIONS through the engine's dynamics on 4 environment lanes: the screen runs behind a step with the
    dynamics on, every value is bit-equal to the restatement on the device's own contingency rows and the contingency lanes hold the
    environment's storage power.  The dispatch the dynamics leave is NOT the reference's (exact projection against SLSQP; measured on an
    MI355X and printed here: 1.8 MW apart at the first launch, 7.1 MW at the sixth, values moved by up to 5e-2), which is why the recorded values are pinned by the state replay."""
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    fx = dict(np.load(golden_path("n1_wcci2022.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    K, n_env = m.n_line, 4
    n = n_env * (1 + K)
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"]))
    eng.set_thermal_limits(fx["thermal_limit"])
    eng.set_gen_limits(fx["pmin"], fx["pmax"], fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], eps_poly=float(fx["eps_poly"]))
    eng.set_storage_params(fx["storage_Emax"], fx["storage_Emin"], fx["storage_loss"], fx["storage_charging_efficiency"],
                           fx["storage_discharging_efficiency"], fx["storage_charge0"], float(fx["delta_time_seconds"]), bool(fx["activate_storage_loss"]))
    eng.set_env_dynamics(True, tol_poly=float(fx["tol_poly"]))
    eng.set_gen_renewable(fx["renewable"])
    eng.set_n1_screen(np.arange(K), n_env)
    row0 = int(fx["row"][0])
    off = np.zeros(n, np.int64)
    off[:n_env] = row0
    eng.set_lane_chronics(lane_offset=off)
    eng.reset(0, n_env)
    eng.set_env_state(0, prev_p=np.tile(fx["ch_prod_p"][row0 - 1], (n_env, 1)))
    for L in range(len(fx["done"])):
        red = np.zeros((n, m.n_gen), np.float32)
        sto = np.zeros((n, fx["act_storage"].shape[1]), np.float32)
        red[:n_env], sto[:n_env] = fx["act_redisp"][L], fx["act_storage"][L]
        eng.set_lane_actions(red, sto)
        eng.step(L)
        done = eng.episode()[0][:n_env]
        assert not done.any(), L
        vals = eng.n1_values()
        assert vals.tobytes() == _restated(eng, n_env, K, fx["thermal_limit"], done).tobytes(), L
        actual = eng.env_state()["actual"][:n_env]
        gap = float(np.abs(actual - fx["actual_dispatch"][L]).max())
        moved = float(np.nanmax(np.where((vals[0] > 0) & (fx["n1"][L] > 0), np.abs(vals[0] - fx["n1"][L]), np.nan)))
        print(f"launch {L}: |actual dispatch - recorded| max {gap:.3f} MW, values move by up to {moved:.2e}")
        sp = eng.out_slices["storage_p"]                                  # the contingency lanes took the dynamics' storage power over
        assert np.array_equal(eng.results(n_env, 1, with_bus=False).out[0][sp], eng.results(0, 1, with_bus=False).out[0][sp]), L
        assert np.abs(eng.results(0, 1, with_bus=False).out[0][sp] - fx["storage_power"][L]).max() < 1e-3, L
    eng.close()
