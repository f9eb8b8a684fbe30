#!/usr/bin/env python
"""Record episodes of the reference environment WITH alerts and AlertReward (build container only, never on a GPU box).

    python tests/golden/make_alert_fixtures.py /path/to/reference [tag ...]      # writes tests/golden/alert_{wcci118,case14}.npz

The scenarios of make_opponent_area_fixtures.py (the UNMODIFIED reference Environment on `OracleHipBackend` with
``GeometricOpponentMultiArea``), extended: those two datasets have no ``alerts_info.json``, so the recorder makes a temporary copy of the
dataset folder, adds ``{"by_line": "opponent"}`` to it and calls ``grid2op.make`` on that path (the copy is deleted afterwards);
``other_rewards={"alert": AlertReward}``; ``ALERT_TIME_WINDOW`` 12 (the default) on wcci118 and 4 on case14; the scripted agent raises
alerts on a fixed pattern, tries an illegal reconnection now and then, and on case14 ends several episodes.

Per launch the fixture holds everything the opponent-area fixtures hold (so that the same replay applies) plus: the alert mask, the eight
``_..alert/attack..`` arrays of the environment, ``info["rewards"]["alert"]``, AlertReward's rings, ``_current_id`` and
``_lines_currently_attacked``, the seven observation attributes; per scenario one full ``obs.to_vect()``.  Data only;
tests/test_alert_cpu.py and tests/test_gpu_alert.py read it.  The recorder asserts its coverage (`check`)."""
import json
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
N_STEPS = 150
ENV_ARRAYS = ("_last_alert", "_is_already_attacked", "_time_since_last_alert", "_alert_duration", "_time_since_last_attack", "_attack_under_alert",
              "_was_alert_used_after_attack")
OBS_ATTRS = ("active_alert", "time_since_last_alert", "alert_duration", "total_number_of_alert", "time_since_last_attack", "attack_under_alert",
             "was_alert_used_after_attack")
ALERT = {"wcci118": dict(window=12, max_game_over=0), "case14": dict(window=4, max_game_over=6)}
COOLDOWN_LINE = 3          # NB_TIMESTEP_COOLDOWN_LINE: an agent that acts again on the line it just moved is illegal


def window_kinds(rew, W):
    """what a blackout at the NEXT step would find in the ring rows that are still in its window: {True} a line whose first noted row
    carries an alert, {False} one without, empty: no attack"""
    seen, kinds = set(), set()
    for i in range(W):
        r = (rew._current_id - W + 1 + i) % (W + 2)
        for l in np.flatnonzero(rew._ts_attack[r]):
            if l not in seen:
                seen.add(l)
                kinds.add(bool(rew._alert_launched[r, l]))
    return kinds


def alert_pattern(t, n):
    """the scripted agent's alerts at its step t: every third alertable line, shifting by one per step, none at every fifth step"""
    return np.array([(t + i) % 3 == 0 and t % 5 != 4 for i in range(n)], bool)


def record(tag, reference):
    import grid2op
    from grid2op.Action import PlayableAction, PowerlineSetAction
    from grid2op.Observation import CompleteObservation
    from grid2op.Opponent import BaseActionBudget, GeometricOpponentMultiArea
    from grid2op.Parameters import Parameters
    from grid2op.Reward import AlertReward
    from conformance_backend import OracleHipBackend
    from grid2op_amd.chronics import load_chronics_multifolder
    from grid2op_amd.grid_model import GridModel
    from make_opponent_area_fixtures import SCENARIOS, space_state
    from make_opponent_fixtures import RecordingPrng

    sc, al = SCENARIOS[tag], ALERT[tag]
    env_name = sc["env"]
    model = GridModel.load_npz(os.path.join(HERE, env_name + ".grid.npz"))
    p = Parameters()
    p.NO_OVERFLOW_DISCONNECTION = True
    p.ALERT_TIME_WINDOW = al["window"]
    p.NB_TIMESTEP_COOLDOWN_LINE = COOLDOWN_LINE
    kwo = dict(sc["kwargs_opponent"])
    if "areas_from" in sc:
        from importlib import import_module
        cfg = import_module(f"grid2op.data.{sc['areas_from']}.config")
        kwo["lines_attacked"] = [[x for x in area if x not in sc["drop_lines"]][:sc["keep_lines"]] for area in cfg.lines_attacked]
    tmp = tempfile.mkdtemp(prefix="alert_fixture_")
    try:
        data = os.path.join(tmp, env_name)
        shutil.copytree(os.path.join(reference, "grid2op", "data", env_name), data)
        with open(os.path.join(data, "alerts_info.json"), "w") as f:
            json.dump({"by_line": "opponent"}, f)
        env = grid2op.make(data, backend=OracleHipBackend(), param=p, action_class=PlayableAction,
                           observation_class=CompleteObservation, opponent_class=GeometricOpponentMultiArea,
                           opponent_action_class=PowerlineSetAction, opponent_budget_class=BaseActionBudget, kwargs_opponent=kwo,
                           other_rewards={"alert": AlertReward}, **sc["make"])
        return _run(env, tag, sc, al, model, reference, env_name, RecordingPrng, space_state, load_chronics_multifolder)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _run(env, tag, sc, al, model, reference, env_name, RecordingPrng, space_state, load_chronics_multifolder):
    cls = type(env)
    assert np.array_equal(cls.line_or_pos_topo_vect, model.line_or_pos_topo_vect) and list(cls.name_line) == [str(x) for x in model.name_line]
    opp = env._opponent
    subs = opp.list_opponents
    area_ids = [[int(x) for x in o._lines_ids] for o in subs]
    lines = [l for ids in area_ids for l in ids]
    A = cls.dim_alerts
    assert A == len(lines) and [int(x) for x in cls.alertable_line_ids] == lines, "the alertable lines are not the opponent's flattened list"
    W = int(env.parameters.ALERT_TIME_WINDOW)
    rew = env.other_rewards["alert"].template_reward if hasattr(env.other_rewards["alert"], "template_reward") else env.other_rewards["alert"]
    env.seed(sc["seed"])
    draws = []
    for o in subs:
        pr = RecordingPrng(o.space_prng)
        pr.draws = draws
        o.space_prng = pr
    env.set_id(sc.get("chronic", 0))
    chron_dir = os.path.join(reference, "grid2op", "data", env_name, "chronics")
    charac = os.path.join(reference, "grid2op", "data", env_name, "prods_charac.csv")
    names, _ = load_chronics_multifolder(chron_dir, model, prods_charac=charac, max_rows=2, truncate=True)
    keys = ("is_reset", "agent_line", "agent_value", "info_line", "info_duration", "info_lines", "n_draws", "scenario", "row", "rho", "line_status",
            "cooldown_line", "topo_vect", "done", "is_illegal", "budget", "budget_is_f32", "attack_duration", "attack_cooldown", "attack_line",
            "previous_fails", "next_attack_time", "attack_counter", "area_counter", "area_line", "area_next_attack_time", "area_attack_counter",
            "alert_mask", "has_attack", "alert_reward", "total_number_of_alert", "ts_attack", "alert_launched", "current_id", "currently_attacked") \
        + tuple("env" + k for k in ENV_ARRAYS) + tuple("obs_" + k for k in OBS_ATTRS)
    rec = {k: [] for k in keys}
    schedules, vect = [], None
    cover = dict(scored_without_alert=0, scored_with_alert=0, blackout_line_alerted=0, blackout_line_not_alerted=0, blackout_no_attack=0, quirk=0,
                 too_old=0, alert_with_illegal=0, resets=0, attacked_steps=0)

    def note(obs, is_reset, agent, info, done, mask):
        st, out = space_state(env)
        row = dict(is_reset=is_reset, agent_line=agent[0], agent_value=agent[1], n_draws=len(draws),
                   scenario=names.index(os.path.basename(env.chronics_handler.get_id())), row=int(env.nb_time_step),
                   rho=obs.rho.astype(np.float32), line_status=obs.line_status.copy(), cooldown_line=obs.time_before_cooldown_line.astype(np.int32),
                   topo_vect=obs.topo_vect.astype(np.int32), done=int(done), is_illegal=int(bool(info.get("is_illegal", False))), **st)
        atk = info.get("opponent_attack_line")
        vec = np.zeros(cls.n_line, bool) if atk is None else np.asarray(atk, bool)
        assert sorted(int(x) for x in np.flatnonzero(vec)) == out
        row.update(info_lines=vec, info_line=st["attack_line"], info_duration=int(info.get("opponent_attack_duration", 0)), alert_mask=mask.copy(),
                   has_attack=int(atk is not None), alert_reward=np.float32(info["rewards"]["alert"]) if "rewards" in info else np.float32(0.0),
                   total_number_of_alert=int(env._total_number_of_alert), ts_attack=rew._ts_attack.copy(), alert_launched=rew._alert_launched.copy(),
                   current_id=int(rew._current_id), currently_attacked=rew._lines_currently_attacked.copy())
        assert atk is None or vec.any()
        for k in ENV_ARRAYS:
            row["env" + k] = np.asarray(getattr(env, k)).copy()
        for k in OBS_ATTRS:
            row["obs_" + k] = np.asarray(getattr(obs, k)).copy()
        for k in keys:
            rec[k].append(row[k])

    def reset():
        obs = env.reset()
        mt = getattr(env.chronics_handler.real_data.data, "maintenance", None)
        assert mt is None or not np.asarray(mt)[:N_STEPS + 2].any(), "a maintenance in the recorded window: choose another scenario or seed"
        schedules.append([np.stack([o._attack_waiting_times, o._attack_durations], axis=1).astype(np.int32).reshape(-1, 2) for o in subs])
        note(obs, 1, (-1, 0), {}, False, np.zeros(A, bool))
        cover["resets"] += 1
        return obs

    obs = reset()
    since_reset, kills = 0, 0
    for t in range(N_STEPS):
        agent = (-1, 0)
        since_reset += 1
        kinds = window_kinds(rew, W)
        # the agent ends an episode when that would cover a blackout case nobody has seen yet (decided from the rings alone)
        wanted = (True in kinds and not cover["blackout_line_alerted"]) or (False in kinds and not cover["blackout_line_not_alerted"]) or \
            (not kinds and not cover["blackout_no_attack"])
        if since_reset >= 12 and kills < al["max_game_over"] and wanted:
            kills += 1
            killer = None
            for l in range(cls.n_line):             # the first line whose loss ends the episode right now
                if obs.line_status[l] and obs.time_before_cooldown_line[l] == 0:
                    sim_env = env.copy()
                    _, _, d_, _ = sim_env.step(env.action_space({"set_line_status": [(l, -1)]}))
                    sim_env.close()
                    if d_:
                        killer = l
                        break
            assert killer is not None
            agent = (killer, -1)
        elif t % 7 >= 4 and (obs.time_before_cooldown_line > 0).any():
            l = int(np.flatnonzero(obs.time_before_cooldown_line > 0)[0])                                 # illegal: the line is in cooldown
            agent = (l, -1 if obs.line_status[l] else 1)
        elif t % sc["agent_every"] == 0:
            cand = np.flatnonzero(~obs.line_status & (obs.time_before_cooldown_line == 0))
            if len(cand):
                agent = (int(cand[0]), 1)
        mask = alert_pattern(t, A)
        d = {"raise_alert": [int(i) for i in np.flatnonzero(mask)]} if mask.any() else {}
        if agent[0] >= 0:
            d["set_line_status"] = [(agent[0], agent[1])]
        prev_att = rec["info_lines"][-1][lines] if not rec["is_reset"][-1] else np.zeros(A, bool)
        obs, _, done, info = env.step(env.action_space(d))
        note(obs, 0, agent, info, done, mask)
        r = float(rec["alert_reward"][-1])
        att = rec["info_lines"][-1][lines]
        cover["attacked_steps"] += int(att.any())
        cover["alert_with_illegal"] += int(bool(info["is_illegal"]) and mask.any())
        cover["quirk"] += int(att.any() and (prev_att & ~att & rec["env_is_already_attacked"][-1]).any())
        cover["too_old"] += int((rec["env_time_since_last_attack"][-1] > int(env.parameters.ALERT_TIME_WINDOW)).any())
        used = rec["env_was_alert_used_after_attack"][-1]
        if done:
            assert info["exception"], "a done without error: the end-of-episode bonus is out of scope"
            cover["blackout_line_alerted"] += int((used == 1).sum())
            cover["blackout_line_not_alerted"] += int((used == -1).sum())
            cover["blackout_no_attack"] += int(not (used != 0).any() and r == 0.0)
            obs = reset()
            since_reset = 0
        else:
            cover["scored_with_alert"] += int((used == -1).sum())
            cover["scored_without_alert"] += int((used == 1).sum())
            if vect is None and (used != 0).any():
                vect = (len(rec["is_reset"]) - 1, obs.to_vect().astype(np.float32))
    assert vect is not None
    thermal = env.get_thermal_limit().astype(np.float32)
    pr = env.parameters
    consts = np.array([rew.reward_min_no_blackout, rew.reward_min_blackout, rew.reward_max_no_blackout, rew.reward_max_blackout], np.float32)
    attr_vect = [(a, int(getattr(obs, a).size if hasattr(getattr(obs, a), "size") else 1)) for a in type(obs).attr_list_vect]
    env.close()

    used_sc = sorted(set(rec["scenario"]))
    n_rows = max(rec["row"]) + 2
    _, ch = load_chronics_multifolder(chron_dir, model, prods_charac=charac, max_rows=n_rows, truncate=True)
    out = {"grid": np.array(env_name), "kind": np.int32(3), "lines": np.array(lines, np.int32),
           "area_of_line": np.array([a for a, ids in enumerate(area_ids) for _ in ids], np.int32), "scenarios_used": np.array(used_sc, np.int32),
           "draws": np.array(draws, np.float64), "thermal_limit": thermal, "time_window": np.int32(W), "reward_constants": consts,
           "vect_launch": np.int32(vect[0]), "vect": vect[1], "vect_names": np.array([a for a, _ in attr_vect]),
           "vect_sizes": np.array([s for _, s in attr_vect], np.int32)}
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
    small = ("topo_vect", "cooldown_line") + tuple("env" + k for k in ENV_ARRAYS) + tuple("obs_" + k for k in OBS_ATTRS if k != "total_number_of_alert")
    bools = ("line_status", "info_lines", "alert_mask", "ts_attack", "alert_launched", "currently_attacked", "env_last_alert", "env_is_already_attacked",
             "obs_active_alert")
    for k in keys:
        out[k] = np.asarray(rec[k], dtype=np.float32 if k in ("rho", "alert_reward") else bool if k in bools else np.float64 if k == "budget" else
                            np.int8 if k in small and int(np.abs(np.asarray(rec[k])).max()) < 127 else np.int32)
    return out, cover


def check(tag, cover):
    assert cover["attacked_steps"] >= 20 and cover["scored_without_alert"] >= 1 and cover["scored_with_alert"] >= 1, cover
    assert cover["too_old"] >= 1 and cover["alert_with_illegal"] >= 1, cover
    if tag == "wcci118":
        assert cover["quirk"] >= 1 and cover["resets"] == 1, cover
    if tag == "case14":
        assert cover["blackout_line_alerted"] >= 1 and cover["blackout_line_not_alerted"] >= 1 and cover["blackout_no_attack"] >= 1, cover
        assert cover["resets"] >= 3, cover


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    reference = os.path.abspath(sys.argv[1])
    for q in (ROOT, os.path.join(ROOT, "tests"), HERE, reference, os.path.join(ROOT, "tests", "_refshim")):
        if q not in sys.path:
            sys.path.insert(0, q)
    os.environ.setdefault("_GRID2OP_FORCE_TEST", "1")
    warnings.filterwarnings("ignore")
    for tag in ALERT:
        if len(sys.argv) > 2 and tag not in sys.argv[2:]:
            continue
        out, cover = record(tag, reference)
        print(f"{tag}: {len(out['is_reset'])} launches, {cover}", flush=True)
        check(tag, cover)
        path = os.path.join(HERE, f"alert_{tag}.npz")
        np.savez_compressed(path, **out)
        print(f"{tag}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
