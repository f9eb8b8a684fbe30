#!/usr/bin/env python
"""Record episodes of the unmodified reference environment that end at a TIME LIMIT (build container only, never on a GPU box).

    python tests/golden/make_episode_limit_fixtures.py /path/to/reference [case14 storage alert]   # -> tests/golden/episode_limit_*.npz

Every episode starts with ``env.reset(options={"max step": N})``; the environments, rewards and scripted agents are those of
make_reward_fixtures.py and make_alert_fixtures.py, with ``EpisodeDurationReward`` added to the other rewards:

  episode_limit_case14.npz        l2rpn_case14_sandbox, DefaultRules with cooldowns 3 / 3, the action table of make_reward_fixtures.py:
                                  consecutive episodes with N in {1, 2, 5, 12} that end truncated on a legal, an illegal and an ambiguous
                                  step, by a game over exactly at step N and by one before N
  episode_limit_storage.npz       educ_case14_storage, the redispatch + storage script: two episodes with N = 6 on the same chronics rows
                                  (the second shows that dispatch and charge restart)
  episode_limit_alert_case14.npz  the case14 alert scenario: a truncation with an attack inside the alert window, one without, a game over

Per step: what a replay needs, the rewards, ``done`` split into terminated (info has an exception) and truncated, ``env.nb_time_step``.
The recorder asserts its coverage and that every recorded reward lies within HALF the bound tests/reward_ref.py derives.  Data only."""
import json
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
EXTRA = ("terminated", "truncated", "nb_time_step", "max_step", "reward_episode_duration")


def make_env(env_name, param, **kw):
    import grid2op
    from grid2op.Reward import EconomicReward, EpisodeDurationReward, GameplayReward, L2RPNReward, LinesCapacityReward, RedispReward
    from conformance_backend import OracleHipBackend
    return grid2op.make(env_name, test=True, backend=OracleHipBackend(), param=param, reward_class=RedispReward,
                        other_rewards=dict(l2rpn=L2RPNReward, lines_capacity=LinesCapacityReward, economic=EconomicReward, gameplay=GameplayReward,
                                           episode_duration=EpisodeDurationReward), **kw)


def has_error(info):
    """the step failed: an exception that is not the agent's illegal or ambiguous action (those are listed too, and end nothing)"""
    from grid2op.Exceptions import AmbiguousAction, IllegalAction
    return any(not isinstance(e, (AmbiguousAction, IllegalAction)) for e in info.get("exception", []) or [])


def step_row(env, obs, reward, info, done, max_step, is_reset=False):
    """make_reward_fixtures.step_row with the two meanings of done apart: a truncated step still has a backend state to read"""
    import make_reward_fixtures as MR
    cls = type(env)
    failed = bool(done) and has_error(info)
    if failed or is_reset:
        gen_p, load_p, a_or = np.zeros(cls.n_gen), np.zeros(cls.n_load), np.zeros(cls.n_line)
    else:
        gen_p, load_p, a_or = env.backend.generators_info()[0], env.backend.loads_info()[0], env.backend.get_line_flow()
    row = dict(is_reset=int(is_reset), done=int(done), is_illegal=int(bool(info.get("is_illegal", False))),
               is_ambiguous=int(bool(info.get("is_ambiguous", False))), failed_redisp=int(bool(info.get("failed_redispatching", False))),
               gen_p=np.array(gen_p, np.float32), load_p=np.array(load_p, np.float32), a_or=np.array(a_or, np.float32),
               rho=np.array(obs.rho, np.float32), line_status=np.array(obs.line_status, bool),
               actual_dispatch=np.array(env._actual_dispatch, np.float32), storage_power=np.array(env._storage_power, np.float32),
               terminated=int(failed), truncated=int(bool(done) and not failed), nb_time_step=int(env.nb_time_step), max_step=int(max_step))
    if is_reset:
        row.update({"reward_" + k: np.float32(np.nan) for k in MR.NAMES + ("episode_duration",)})
    else:
        row["reward_redisp"] = np.float32(reward)
        for k in MR.NAMES[1:] + ("episode_duration",):
            row["reward_" + k] = np.float32(info["rewards"][k])
    return row


def finish(tag, out, rec, keys):
    """dtypes, the half-bound check of every recorded reward against the restatement with is_done = failed or truncated, the file"""
    import episode_ref as E
    import make_reward_fixtures as MR
    import reward_ref as R
    for k in keys:
        out[k] = np.asarray(rec[k], dtype=bool if k == "line_status" else np.int8 if k in MR.STEP_KEYS[:5] + ("terminated", "truncated") else
                            np.int32 if k in ("nb_time_step", "max_step") else np.float32)
    slots = R.fixture_slots(out)
    worst = 0.0
    for i in range(len(out["done"])):
        if out["is_reset"][i]:
            continue
        row, tr = E.fixture_row(out, i), bool(out["truncated"][i])
        got = R.fixture_rewards(out, i)
        for s, (kind, p) in enumerate(slots):
            want = E.value(kind, p, trunc=tr, **row)
            if E.constant_branch(kind, row["failed"], row["illegal"], row["ambiguous"], tr):
                assert want == got[s], (tag, i, s, want, got[s])
                continue
            b = R.bound(kind, p, **row)
            err = abs(float(got[s]) - float(want))
            assert err <= 0.5 * b, (tag, i, s, float(got[s]), float(want), err, b)
            worst = max(worst, err / b)
        ended = bool(out["done"][i])
        want = E.duration_reward(ended, int(out["nb_time_step"][i]), int(out["max_step"][i]))
        assert abs(float(out["reward_episode_duration"][i]) - float(want)) <= float(np.spacing(np.float32(max(abs(float(want)), 1e-30)))), (tag, i)
    path = os.path.join(HERE, f"episode_limit_{tag}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{tag}: {len(out['done'])} rows, worst reference error / bound {worst:.4f}, {size} bytes", flush=True)
    assert size <= MR.MAX_BYTES, "cut steps"


# ---- fixture 1: topology actions under DefaultRules, episodes of 1 / 2 / 5 / 12 steps ----
# (N, how the episode's last step goes)
PLAN = [(1, "legal"), (2, "ambiguous"), (5, "illegal"), (12, "legal"), (5, "kill_at_limit"), (12, "kill_early"), (2, "legal"), (1, "illegal")]


def episode_table(model, seed=3):
    """the table of make_reward_fixtures.py (its own entries, then one per line that opens it) plus ONE entry that opens two lines at once:
    illegal at any step (MAX_LINE_STATUS_CHANGED = 1), the illegal action of an episode of one step.  Returns (table, n0, that entry)."""
    import make_reward_fixtures as MR
    table, n0 = MR.topo_table(model, seed)
    return table + [{"set_line_status": [(0, -1), (1, -1)]}], n0, len(table)


def record_case14(reference, seed=3):
    from grid2op.Parameters import Parameters
    from grid2op_amd.chronics import load_chronics_multifolder
    from grid2op_amd.grid_model import GridModel
    import make_reward_fixtures as MR
    from make_topo_mask_fixtures import PARAMS, to_reference
    from topo_rules_ref import pack_actions
    env_name = "l2rpn_case14_sandbox"
    model = GridModel.load_npz(os.path.join(HERE, env_name + ".grid.npz"))
    p = Parameters()
    p.NO_OVERFLOW_DISCONNECTION = True
    for k, v in PARAMS.items():
        setattr(p, k, v)
    env = make_env(env_name, p)
    cls = type(env)
    table, n0, n_two = episode_table(model, seed)
    off, items = pack_actions(table)
    ambiguous = [k for k in range(n0) if to_reference(env.action_space, table[k], cls.dim_topo).is_ambiguous()[0]]
    order = np.random.default_rng(seed).permutation(n0)
    env.seed(seed)
    chron_dir = os.path.join(reference, "grid2op", "data", env_name, "chronics")
    charac = os.path.join(reference, "grid2op", "data", env_name, "prods_charac.csv")
    names, _ = load_chronics_multifolder(chron_dir, model, prods_charac=charac, max_rows=2, truncate=True)
    keys = MR.STEP_KEYS + ("reward_episode_duration",) + EXTRA[:4]
    rec = {k: [] for k in keys + ("played", "scenario", "row")}

    def note(row, played):
        row.update(played=played, scenario=names.index(os.path.basename(env.chronics_handler.get_id())), row=int(env.nb_time_step))
        for k in rec:
            rec[k].append(row[k])

    def act_of(k):
        return env.action_space({}) if k < 0 else to_reference(env.action_space, table[k], cls.dim_topo)

    def killer(obs):
        for l in range(cls.n_line):                 # the first line whose loss ends the episode right now
            if obs.line_status[l] and obs.time_before_cooldown_line[l] == 0:
                sim_env = env.copy()
                _, _, d_, i_ = sim_env.step(env.action_space({"set_line_status": [(l, -1)]}))
                sim_env.close()
                if d_ and has_error(i_):
                    return n0 + l
        raise AssertionError("no line ends the episode")

    def legal_entry(obs, walk):
        """the next entry of the walk that is legal right now and moves something"""
        for q in range(n0):
            k = int(order[(walk + q) % n0])
            if k in ambiguous:
                continue
            sim_env = env.copy()
            o2, _, d_, i_ = sim_env.step(act_of(k))
            sim_env.close()
            if not has_error(i_) and not i_["is_illegal"] and not i_["is_ambiguous"] and (np.any(o2.time_before_cooldown_sub > 0) or np.any(o2.time_before_cooldown_line > 0)):
                return k, walk + q + 1
        raise AssertionError("no legal entry")

    cover = dict(trunc_legal=0, trunc_illegal=0, trunc_ambiguous=0, fail_at_limit=0, fail_before=0, n1=0)
    walk = 0
    for N, how in PLAN:
        env.set_id(0)
        obs = env.reset(options={"max step": N})
        assert env.max_episode_duration() == N
        note(step_row(env, obs, 0.0, {}, False, N, is_reset=True), -1)
        last = -1
        for t in range(1, N + 1):
            final = t == N
            if how == "kill_early" and t == 3 or how == "kill_at_limit" and final:
                k = killer(obs)
            elif how == "illegal" and final and N > 1:
                k = last                            # again: into the cooldown the entry just started
            elif how == "illegal" and final:
                k = n_two                           # N = 1: two lines at once are over MAX_LINE_STATUS_CHANGED
            elif how == "ambiguous" and final:
                k = ambiguous[N % len(ambiguous)]
            elif how == "illegal" and t == N - 1:
                k, walk = legal_entry(obs, walk)
            elif t % 4 == 2:
                k = -1
            else:
                k, walk = legal_entry(obs, walk)
            last = k
            obs, reward, done, info = env.step(act_of(k))
            note(step_row(env, obs, reward, info, done, N), k)
            r = rec
            if done:
                tr, ill, amb = r["truncated"][-1], r["is_illegal"][-1], r["is_ambiguous"][-1]
                cover["trunc_legal"] += int(tr and not ill and not amb); cover["trunc_illegal"] += int(tr and ill); cover["trunc_ambiguous"] += int(tr and amb)
                cover["fail_at_limit"] += int(not tr and t == N); cover["fail_before"] += int(not tr and t < N); cover["n1"] += int(N == 1)
                assert (how.startswith("kill")) == (not tr) and r["nb_time_step"][-1] == t, (N, how, t)
                break
        assert done, (N, how)
    return env, rec, keys, cover, dict(n_two=n_two, names=names, model=model, chron_dir=chron_dir, charac=charac, off=off, items=items, n0=n0, seed=seed, env_name=env_name)


def case14(reference):
    import make_reward_fixtures as MR
    from grid2op_amd.chronics import load_chronics_multifolder
    env, rec, keys, cover, ctx = record_case14(reference)
    n_two = ctx["n_two"]
    env.reset()                                     # (the last episode is over: the metadata is read from an initialised environment)
    meta = MR.reward_meta(env)
    pr = env.parameters
    env.close()
    print("case14:", cover, flush=True)
    assert cover["trunc_legal"] >= 2 and cover["trunc_illegal"] >= 2 and cover["trunc_ambiguous"] >= 1 and cover["fail_at_limit"] >= 1 \
        and cover["fail_before"] >= 1 and cover["n1"] >= 2, cover
    used = sorted(set(rec["scenario"]))
    n_rows = max(rec["row"]) + 2
    _, ch = load_chronics_multifolder(ctx["chron_dir"], ctx["model"], prods_charac=ctx["charac"], max_rows=n_rows, truncate=True)
    out = dict(meta, grid=np.array(ctx["env_name"]), off=ctx["off"], items=ctx["items"], table_seed=np.int32(ctx["seed"]), n_table=np.int32(ctx["n0"]),
               two_lines_entry=np.int32(n_two), scenarios_used=np.array(used, np.int32),
               params=np.array([pr.MAX_SUB_CHANGED, pr.MAX_LINE_STATUS_CHANGED, pr.NB_TIMESTEP_COOLDOWN_SUB, pr.NB_TIMESTEP_COOLDOWN_LINE,
                                pr.NB_TIMESTEP_RECONNECTION], np.int32),
               played=np.asarray(rec["played"], np.int32), scenario=np.asarray(rec["scenario"], np.int32), row=np.asarray(rec["row"], np.int32))
    for k, v in ch.items():
        if k in ("load_p", "load_q", "prod_p", "prod_v"):
            out["chron_" + k] = v[used].astype(np.float32)
        elif k == "maintenance":
            assert not v[used][:, :n_rows].any(), "a maintenance in the recorded window: choose another seed"
    finish("case14", out, rec, keys)


# ---- fixture 2: redispatch + storage, two episodes of six steps on the same rows ----
def storage(reference, N=6, seed=5):
    from grid2op.Action import DontAct
    from grid2op.Opponent import BaseOpponent
    from grid2op.Parameters import Parameters
    from grid2op_amd.chronics import load_chronics_folder
    from grid2op_amd.grid_model import GridModel
    import make_reward_fixtures as MR
    env_name = "educ_case14_storage"
    p = Parameters()
    p.NO_OVERFLOW_DISCONNECTION = True
    env = make_env(env_name, p, opponent_class=BaseOpponent, opponent_action_class=DontAct, opponent_init_budget=0.0, opponent_budget_per_ts=0.0)
    cls = type(env)
    env.seed(seed)
    rng = np.random.default_rng(seed)
    disp = np.nonzero(cls.gen_redispatchable)[0]
    keys = MR.STEP_KEYS + ("reward_episode_duration",) + EXTRA[:4]
    rec = {k: [] for k in keys + ("row", "act_redisp", "act_storage", "act_curtail", "target_dispatch", "storage_charge")}
    charge0 = None
    for ep in range(2):
        env.set_id(0)
        env.reset(options={"max step": N})
        data = env.chronics_handler.real_data.data
        if charge0 is None:
            charge0 = np.array(env._storage_current_charge, np.float64)
        assert np.array_equal(charge0, np.array(env._storage_current_charge, np.float64)) and not np.any(env._actual_dispatch)
        for t in range(N):
            red, sto = np.zeros(cls.n_gen, np.float32), np.zeros(cls.n_storage, np.float32)
            k = rng.choice(disp, size=2, replace=False)
            red[k] = cls.gen_max_ramp_up[k] * rng.uniform(0.2, 0.7, 2) * np.array([1.0, -1.0])
            sto[:] = rng.uniform(-4.0, 4.0, cls.n_storage)
            act = {"redispatch": [(int(g), float(red[g])) for g in np.nonzero(red)[0]], "set_storage": [(int(i), float(sto[i])) for i in np.nonzero(sto)[0]]}
            obs, reward, done, info = env.step(env.action_space(act))
            row = step_row(env, obs, reward, info, done, N)
            row.update(row=int(data.current_index), act_redisp=red, act_storage=sto, act_curtail=np.full(cls.n_gen, -1.0, np.float32),
                       target_dispatch=np.array(env._target_dispatch, np.float32), storage_charge=np.array(env._storage_current_charge, np.float32))
            for q in rec:
                rec[q].append(row[q])
            assert done == (t == N - 1) and not has_error(info), (ep, t, info["exception"])
        assert rec["truncated"][-1] and np.abs(rec["actual_dispatch"][-1]).sum() > 0 and np.abs(rec["storage_charge"][-1] - charge0).max() > 0
    env.set_id(0)
    env.reset()
    out = MR.reward_meta(env)
    out.update(grid=np.array(env_name), storage_charge0=charge0, row=np.asarray(rec["row"], np.int32), act_redisp=np.asarray(rec["act_redisp"], np.float32),
               act_storage=np.asarray(rec["act_storage"], np.float32), act_curtail=np.asarray(rec["act_curtail"], np.float32),
               target_dispatch=np.asarray(rec["target_dispatch"], np.float32), storage_charge=np.asarray(rec["storage_charge"], np.float32),
               pmin=cls.gen_pmin.astype(np.float64), pmax=cls.gen_pmax.astype(np.float64), ramp_up=cls.gen_max_ramp_up.astype(np.float64),
               ramp_down=cls.gen_max_ramp_down.astype(np.float64), redispatchable=cls.gen_redispatchable.astype(bool),
               renewable=cls.gen_renewable.astype(bool), eps_poly=np.float64(env._epsilon_poly), tol_poly=np.float64(env._tol_poly),
               activate_storage_loss=np.bool_(env.parameters.ACTIVATE_STORAGE_LOSS),
               storage_Emax=cls.storage_Emax.astype(np.float64), storage_Emin=cls.storage_Emin.astype(np.float64),
               storage_loss=cls.storage_loss.astype(np.float64), storage_charging_efficiency=cls.storage_charging_efficiency.astype(np.float64),
               storage_discharging_efficiency=cls.storage_discharging_efficiency.astype(np.float64))
    m = GridModel.load_npz(os.path.join(HERE, f"{env_name}.grid.npz"))
    ch = load_chronics_folder(env.chronics_handler.get_id(), m, max_rows=N + 4)
    for k in ("load_p", "load_q", "prod_p", "prod_v"):
        out["ch_" + k] = ch[k]
    env.close()
    assert rec["row"][:N] == rec["row"][N:], "the two episodes must read the same chronics rows"
    finish("storage", out, rec, keys)


# ---- fixture 3: the case14 alert scenario ----
ALERT_PLAN = [(8, "truncate_attack"), (19, "truncate"), (30, "kill")]


def alert(reference):
    import grid2op
    from grid2op.Action import PlayableAction, PowerlineSetAction
    from grid2op.Observation import CompleteObservation
    from grid2op.Opponent import BaseActionBudget, GeometricOpponentMultiArea
    from grid2op.Parameters import Parameters
    from grid2op.Reward import AlertReward
    from conformance_backend import OracleHipBackend
    from grid2op_amd.chronics import load_chronics_multifolder
    from grid2op_amd.grid_model import GridModel
    import make_alert_fixtures as MA
    from make_opponent_area_fixtures import SCENARIOS, space_state
    from make_opponent_fixtures import RecordingPrng
    tag = "case14"
    sc, al = SCENARIOS[tag], MA.ALERT[tag]
    env_name = sc["env"]
    model = GridModel.load_npz(os.path.join(HERE, env_name + ".grid.npz"))
    p = Parameters()
    p.NO_OVERFLOW_DISCONNECTION = True
    p.ALERT_TIME_WINDOW = al["window"]
    p.NB_TIMESTEP_COOLDOWN_LINE = MA.COOLDOWN_LINE
    tmp = tempfile.mkdtemp(prefix="episode_limit_fixture_")
    try:
        data = os.path.join(tmp, env_name)
        shutil.copytree(os.path.join(reference, "grid2op", "data", env_name), data)
        with open(os.path.join(data, "alerts_info.json"), "w") as f:
            json.dump({"by_line": "opponent"}, f)
        env = grid2op.make(data, backend=OracleHipBackend(), param=p, action_class=PlayableAction, observation_class=CompleteObservation,
                           opponent_class=GeometricOpponentMultiArea, opponent_action_class=PowerlineSetAction,
                           opponent_budget_class=BaseActionBudget, kwargs_opponent=dict(sc["kwargs_opponent"]), other_rewards={"alert": AlertReward},
                           **sc["make"])
        out, cover = _alert_run(env, sc, model, reference, env_name, RecordingPrng, space_state, load_chronics_multifolder, MA)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("alert:", cover, flush=True)
    assert cover["truncated_with_attack_in_window"] >= 1 and cover["truncated_without_attack"] >= 1 and cover["game_over"] >= 1, cover
    assert cover["used_kept"] >= 1, "no truncated step shows a was_alert_used_after_attack left by the step before: move the limits"
    path = os.path.join(HERE, "episode_limit_alert_case14.npz")
    np.savez_compressed(path, **out)
    import make_reward_fixtures as MR
    print(f"alert: {len(out['is_reset'])} launches, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) <= MR.MAX_BYTES


def _alert_run(env, sc, model, reference, env_name, RecordingPrng, space_state, load_chronics_multifolder, MA):
    cls = type(env)
    opp = env._opponent
    subs = opp.list_opponents
    area_ids = [[int(x) for x in o._lines_ids] for o in subs]
    lines = [l for ids in area_ids for l in ids]
    A = cls.dim_alerts
    assert A == len(lines) and [int(x) for x in cls.alertable_line_ids] == lines, (A, lines, cls.alertable_line_ids)
    W = int(env.parameters.ALERT_TIME_WINDOW)
    helper = env.other_rewards["alert"]
    rew = helper.template_reward if hasattr(helper, "template_reward") else helper
    env.seed(sc["seed"])
    draws = []
    for o in subs:
        pr = RecordingPrng(o.space_prng)
        pr.draws = draws
        o.space_prng = pr
    chron_dir = os.path.join(reference, "grid2op", "data", env_name, "chronics")
    charac = os.path.join(reference, "grid2op", "data", env_name, "prods_charac.csv")
    names, _ = load_chronics_multifolder(chron_dir, model, prods_charac=charac, max_rows=2, truncate=True)
    keys = ("is_reset", "agent_line", "agent_value", "info_line", "info_duration", "info_lines", "n_draws", "scenario", "row", "rho", "line_status",
            "cooldown_line", "topo_vect", "done", "terminated", "truncated", "nb_time_step", "max_step", "is_illegal", "budget", "budget_is_f32",
            "attack_duration", "attack_cooldown", "attack_line", "previous_fails", "next_attack_time", "attack_counter", "area_counter", "area_line",
            "area_next_attack_time", "area_attack_counter", "alert_mask", "has_attack", "alert_reward", "total_number_of_alert", "ts_attack",
            "alert_launched", "current_id", "currently_attacked") + tuple("env" + k for k in MA.ENV_ARRAYS) + tuple("obs_" + k for k in MA.OBS_ATTRS)
    rec = {k: [] for k in keys}
    schedules = []
    cover = dict(truncated_with_attack_in_window=0, truncated_without_attack=0, game_over=0, used_kept=0)

    def note(obs, is_reset, agent, info, done, mask, N):
        st, out = space_state(env)
        failed = bool(done) and has_error(info)
        row = dict(is_reset=is_reset, agent_line=agent[0], agent_value=agent[1], n_draws=len(draws),
                   scenario=names.index(os.path.basename(env.chronics_handler.get_id())), row=int(env.nb_time_step),
                   rho=obs.rho.astype(np.float32), line_status=obs.line_status.copy(), cooldown_line=obs.time_before_cooldown_line.astype(np.int32),
                   topo_vect=obs.topo_vect.astype(np.int32), done=int(done), terminated=int(failed), truncated=int(bool(done) and not failed),
                   nb_time_step=int(env.nb_time_step), max_step=int(N), is_illegal=int(bool(info.get("is_illegal", False))), **st)
        atk = info.get("opponent_attack_line")
        vec = np.zeros(cls.n_line, bool) if atk is None else np.asarray(atk, bool)
        assert sorted(int(x) for x in np.flatnonzero(vec)) == out
        row.update(info_lines=vec, info_line=st["attack_line"], info_duration=int(info.get("opponent_attack_duration", 0)), alert_mask=mask.copy(),
                   has_attack=int(atk is not None), alert_reward=np.float32(info["rewards"]["alert"]) if "rewards" in info else np.float32(0.0),
                   total_number_of_alert=int(env._total_number_of_alert), ts_attack=rew._ts_attack.copy(), alert_launched=rew._alert_launched.copy(),
                   current_id=int(rew._current_id), currently_attacked=rew._lines_currently_attacked.copy())
        for k in MA.ENV_ARRAYS:
            row["env" + k] = np.asarray(getattr(env, k)).copy()
        for k in MA.OBS_ATTRS:
            row["obs_" + k] = np.asarray(getattr(obs, k)).copy()
        for k in keys:
            rec[k].append(row[k])

    t_all = 0
    for N, how in ALERT_PLAN:
        env.set_id(sc.get("chronic", 0))
        obs = env.reset(options={"max step": N})
        schedules.append([np.stack([o._attack_waiting_times, o._attack_durations], axis=1).astype(np.int32).reshape(-1, 2) for o in subs])
        note(obs, 1, (-1, 0), {}, False, np.zeros(A, bool), N)
        for t in range(1, N + 1):
            agent = (-1, 0)
            if how == "kill" and t >= 14:
                killer = None
                for l in range(cls.n_line):
                    if obs.line_status[l] and obs.time_before_cooldown_line[l] == 0:
                        sim_env = env.copy()
                        _, _, d_, i_ = sim_env.step(env.action_space({"set_line_status": [(l, -1)]}))
                        sim_env.close()
                        if d_ and has_error(i_):
                            killer = l
                            break
                assert killer is not None
                agent = (killer, -1)
            elif t % sc["agent_every"] == 0:
                cand = np.flatnonzero(~obs.line_status & (obs.time_before_cooldown_line == 0))
                if len(cand):
                    agent = (int(cand[0]), 1)
            mask = MA.alert_pattern(t_all, A)
            t_all += 1
            d = {"raise_alert": [int(i) for i in np.flatnonzero(mask)]} if mask.any() else {}
            if agent[0] >= 0:
                d["set_line_status"] = [(agent[0], agent[1])]
            before = {k: np.asarray(getattr(env, k)).copy() for k in MA.ENV_ARRAYS}
            obs, _, done, info = env.step(env.action_space(d))
            note(obs, 0, agent, info, done, mask, N)
            if not done and np.any(rec["env_was_alert_used_after_attack"][-1] != 0):
                cover.setdefault("scored_steps", []).append((N, t))
            if done:
                if rec["truncated"][-1]:
                    assert t == N and float(rec["alert_reward"][-1]) == float(rew.reward_end_episode_bonus)
                    in_window = bool((np.asarray(env._time_since_last_attack) >= 0).any() and
                                     (np.asarray(env._time_since_last_attack)[np.asarray(env._time_since_last_attack) >= 0] <= W).any())
                    cover["truncated_with_attack_in_window"] += int(in_window)
                    cover["truncated_without_attack"] += int(not in_window)
                    # the bonus is returned before _update_state: was_alert_used_after_attack is the step before's
                    assert np.array_equal(rec["env_was_alert_used_after_attack"][-1], before["_was_alert_used_after_attack"])
                    cover["used_kept"] += int(np.any(before["_was_alert_used_after_attack"] != 0))
                    assert rec["current_id"][-1] == rec["current_id"][-2], "the rings moved on a truncated step"
                else:
                    cover["game_over"] += 1
                break
        assert done and (how == "kill") == bool(rec["terminated"][-1]), (N, how)
    env.reset()
    thermal = env.get_thermal_limit().astype(np.float32)
    pr = env.parameters
    consts = np.array([rew.reward_min_no_blackout, rew.reward_min_blackout, rew.reward_max_no_blackout, rew.reward_max_blackout], np.float32)
    bonus = np.float32(rew.reward_end_episode_bonus)
    env.close()
    used_sc = sorted(set(rec["scenario"]))
    n_rows = max(rec["row"]) + 2
    _, ch = load_chronics_multifolder(chron_dir, model, prods_charac=charac, max_rows=n_rows, truncate=True)
    out = {"grid": np.array(env_name), "kind": np.int32(3), "lines": np.array(lines, np.int32),
           "area_of_line": np.array([a for a, ids in enumerate(area_ids) for _ in ids], np.int32), "scenarios_used": np.array(used_sc, np.int32),
           "draws": np.array(draws, np.float64), "thermal_limit": thermal, "time_window": np.int32(W), "reward_constants": consts,
           "reward_end_episode_bonus": bonus}
    for k, v in ch.items():
        if k in ("load_p", "load_q", "prod_p", "prod_v"):
            out["chron_" + k] = v[used_sc].astype(np.float32)
        elif k == "maintenance":
            assert not v[used_sc][:, :n_rows].any(), "a maintenance in the recorded window: choose another scenario"
    sp_kw = sc["make"]
    out["space"] = np.array([sp_kw["opponent_init_budget"], sp_kw["opponent_budget_per_ts"]], np.float32)
    out["space_int"] = np.array([sp_kw["opponent_attack_duration"], sp_kw["opponent_attack_cooldown"]], np.int32)
    o0 = subs[0]
    out["geometric"] = np.array([o0._attack_hazard_rate, o0._recovery_rate, o0._pmax_pmin_ratio], np.float64)
    out["geometric_int"] = np.array([o0._recovery_minimum_duration, o0._episode_max_time], np.int64)
    cap = max(len(s) for per in schedules for s in per)
    out["schedule_count"] = np.array([[len(s) for s in per] for per in schedules], np.int32)
    out["schedule"] = np.stack([np.stack([np.concatenate([s, np.zeros((cap - len(s), 2), np.int32)]) for s in per]) for per in schedules])
    out["params"] = np.array([pr.MAX_SUB_CHANGED, pr.MAX_LINE_STATUS_CHANGED, pr.NB_TIMESTEP_COOLDOWN_SUB, pr.NB_TIMESTEP_COOLDOWN_LINE,
                              pr.NB_TIMESTEP_RECONNECTION], np.int32)
    small = ("topo_vect", "cooldown_line") + tuple("env" + k for k in MA.ENV_ARRAYS) + tuple("obs_" + k for k in MA.OBS_ATTRS if k != "total_number_of_alert")
    bools = ("line_status", "info_lines", "alert_mask", "ts_attack", "alert_launched", "currently_attacked", "env_last_alert", "env_is_already_attacked",
             "obs_active_alert")
    for k in keys:
        out[k] = np.asarray(rec[k], dtype=np.float32 if k in ("rho", "alert_reward") else bool if k in bools else np.float64 if k == "budget" else
                            np.int8 if k in small and int(np.abs(np.asarray(rec[k])).max()) < 127 else np.int32)
    return out, cover


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    reference = os.path.abspath(sys.argv[1])
    for q in (ROOT, os.path.join(ROOT, "tests"), HERE, reference, os.path.join(ROOT, "tests", "_refshim")):
        if q not in sys.path:
            sys.path.insert(0, q)
    os.environ.setdefault("_GRID2OP_FORCE_TEST", "1")
    warnings.filterwarnings("ignore")
    only = sys.argv[2:]
    if not only:                                    # one process per fixture: the reference caches an environment's class by its name
        import subprocess
        for tag in ("case14", "storage", "alert"):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), reference, tag])
        return
    if not only or "case14" in only:
        case14(reference)
    if not only or "storage" in only:
        storage(reference)
    if not only or "alert" in only:
        alert(reference)


if __name__ == "__main__":
    main()
