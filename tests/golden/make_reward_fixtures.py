#!/usr/bin/env python
"""Record the REWARDS of the unmodified reference environment (build container only, never on a GPU box).

    python tests/golden/make_reward_fixtures.py /path/to/reference [topo storage wcci]    # -> tests/golden/reward_*.npz

The environment -- façade over the CPU oracle (tests/conformance_backend.py), ``reward_class=RedispReward`` and L2RPNReward,
LinesCapacityReward, EconomicReward, GameplayReward as ``other_rewards`` -- is driven by scripted agents:

  reward_case14_topo.npz     l2rpn_case14_sandbox, DefaultRules with cooldowns 3 / 3 (the parameters of make_topo_mask_fixtures.py): the
                             agent walks that recorder's action table (legal, illegal and ambiguous entries), repeats entries into their
                             cooldown, and ends episodes by opening the line whose loss is a game over (the search of make_alert_fixtures.py)
  reward_case14_storage.npz  educ_case14_storage: redispatch + storage actions as make_envdyn_fixtures.py plays them, the second unit charged
                             until _compute_storage clamps it, then that recorder's ``push`` recipe, which makes _prepare_redisp cancel actions
  reward_wcci2022.npz        l2rpn_wcci_2022_dev (62 generators, 91 loads, 186 lines, 7 storage units): redispatch + storage + curtailment

Per step: what a replay needs (the actions, the chronics rows), the five rewards, info's illegal / ambiguous / failed-redispatch flags and
the inputs of the formulas (gen_p, load_p, a_or, rho, line_status, _actual_dispatch, _storage_power) with what the rewards' ``initialize``
left (max_regret, worst_cost, ...).  The recorder asserts its coverage and that every recorded value lies within HALF the bound that
tests/reward_ref.py derives for the reference's float32 evaluation.  Data only."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
MAX_BYTES = 195216                     # the largest alert fixture
PUSH = (5, 1, 0)                       # make_envdyn_fixtures.py: generator pushed up by its ramp, the two that go down
NAMES = ("redisp", "l2rpn", "lines_capacity", "economic", "gameplay")


def make_env(env_name, param, **kw):
    import grid2op
    from grid2op.Reward import EconomicReward, GameplayReward, L2RPNReward, LinesCapacityReward, RedispReward
    from conformance_backend import OracleHipBackend
    return grid2op.make(env_name, test=True, backend=OracleHipBackend(), param=param, reward_class=RedispReward,
                        other_rewards=dict(l2rpn=L2RPNReward, lines_capacity=LinesCapacityReward, economic=EconomicReward, gameplay=GameplayReward), **kw)


def template(helper):
    return helper.template_reward if hasattr(helper, "template_reward") else helper


def reward_meta(env):
    cls = type(env)
    rd, ec, gp = template(env._reward_helper), template(env.other_rewards["economic"]), template(env.other_rewards["gameplay"])
    return dict(redisp_alpha=np.float64(rd._alpha_redisp), redisp_max_regret=np.float64(rd.max_regret), redisp_min_reward=np.float64(rd.reward_min),
                redisp_reward_max=np.float64(rd.reward_max), redisp_illegal_ambiguous=np.float64(rd._reward_illegal_ambiguous),
                economic_worst_cost=np.float64(ec.worst_cost), economic_reward_min=np.float64(ec.reward_min), economic_reward_max=np.float64(ec.reward_max),
                gameplay_reward_min=np.float64(gp.reward_min), gameplay_reward_max=np.float64(gp.reward_max),
                gen_cost_per_MW=np.asarray(cls.gen_cost_per_MW, np.float32), gen_pmax=np.asarray(cls.gen_pmax, np.float32),
                delta_time_seconds=np.float64(env.delta_time_seconds), thermal_limit=np.asarray(env.get_thermal_limit(), np.float32))


STEP_KEYS = ("is_reset", "done", "is_illegal", "is_ambiguous", "failed_redisp", "gen_p", "load_p", "a_or", "rho", "line_status", "actual_dispatch",
             "storage_power") + tuple("reward_" + k for k in NAMES)


def step_row(env, obs, reward, info, done, is_reset=False):
    """the rewards of the step and the inputs of their formulas, read where the reward classes read them"""
    cls = type(env)
    if done or is_reset:                 # (a game over leaves no backend state to read; the branches that apply are constants)
        gen_p, load_p, a_or = np.zeros(cls.n_gen), np.zeros(cls.n_load), np.zeros(cls.n_line)
    else:
        gen_p, load_p, a_or = env.backend.generators_info()[0], env.backend.loads_info()[0], env.backend.get_line_flow()
        assert np.array_equal((np.asarray(env._gen_activeprod_t) > 0), np.asarray(gen_p, np.float32) > 0), "marginal cost: _gen_activeprod_t vs gen_p"
    row = dict(is_reset=int(is_reset), done=int(done), is_illegal=int(bool(info.get("is_illegal", False))),
               is_ambiguous=int(bool(info.get("is_ambiguous", False))), failed_redisp=int(bool(info.get("failed_redispatching", False))),
               gen_p=np.array(gen_p, np.float32), load_p=np.array(load_p, np.float32), a_or=np.array(a_or, np.float32),
               rho=np.array(obs.rho, np.float32), line_status=np.array(obs.line_status, bool),
               actual_dispatch=np.array(env._actual_dispatch, np.float32), storage_power=np.array(env._storage_power, np.float32))
    if is_reset:
        row.update({"reward_" + k: np.float32(np.nan) for k in NAMES})
    else:
        assert not done or info["exception"], "a done without an error is outside the engine's domain"
        row["reward_redisp"] = np.float32(reward)
        for k in NAMES[1:]:
            row["reward_" + k] = np.float32(info["rewards"][k])
    return row


def finish(tag, out, rec):
    import reward_ref as R
    for k in STEP_KEYS:
        out[k] = np.asarray(rec[k], dtype=bool if k == "line_status" else np.int8 if k in STEP_KEYS[:5] else np.float32)
    slots = R.fixture_slots(out)
    worst = {k: 0.0 for k in NAMES}
    for i in range(len(out["done"])):
        if out["is_reset"][i]:
            continue
        row = R.fixture_row(out, i)
        got = R.fixture_rewards(out, i)
        for s, (kind, p) in enumerate(slots):
            want = R.value(kind, p, **row)
            if R.constant_branch(kind, row["failed"], row["illegal"], row["ambiguous"]):
                assert want == got[s], (tag, i, NAMES[s], want, got[s])
                continue
            b = R.bound(kind, p, **row)
            err = abs(float(got[s]) - float(want))
            assert err <= 0.5 * b, (tag, i, NAMES[s], float(got[s]), float(want), err, b)
            worst[NAMES[s]] = max(worst[NAMES[s]], err / b)
    path = os.path.join(HERE, f"reward_{tag}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{tag}: {len(out['done'])} rows, worst reference error / bound {({k: round(v, 4) for k, v in worst.items()})}, {size} bytes", flush=True)
    assert size <= MAX_BYTES, "cut steps"


# ---- fixture 1: topology actions under DefaultRules, game overs by the agent's own disconnections ----
def topo_table(model, seed):
    """the table of make_topo_mask_fixtures.py, then one entry per line that opens it (the agent's way to end an episode)"""
    from make_topo_mask_fixtures import build_table
    table = build_table(model, np.random.default_rng(seed))
    n0 = len(table)
    table += [{"set_line_status": [(l, -1)]} for l in range(model.n_line)]
    return table, n0


def record_topo(reference, n_steps=96, seed=3):
    from grid2op.Parameters import Parameters
    from grid2op_amd.chronics import load_chronics_multifolder
    from grid2op_amd.grid_model import GridModel
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
    table, n0 = topo_table(model, seed)
    off, items = pack_actions(table)
    ambiguous = [k for k in range(n0) if to_reference(env.action_space, table[k], cls.dim_topo).is_ambiguous()[0]]
    rng = np.random.default_rng(seed)
    order = rng.permutation(n0)
    env.seed(seed)
    env.set_id(0)
    chron_dir = os.path.join(reference, "grid2op", "data", env_name, "chronics")
    charac = os.path.join(reference, "grid2op", "data", env_name, "prods_charac.csv")
    names, _ = load_chronics_multifolder(chron_dir, model, prods_charac=charac, max_rows=2, truncate=True)
    rec = {k: [] for k in STEP_KEYS + ("played", "scenario", "row")}

    def note(row, played):
        row.update(played=played, scenario=names.index(os.path.basename(env.chronics_handler.get_id())), row=int(env.nb_time_step))
        for k in rec:
            rec[k].append(row[k])

    def reset():
        obs = env.reset()
        note(step_row(env, obs, 0.0, {}, False, is_reset=True), -1)
        return obs

    obs = reset()
    since, kills, walk, last = 0, 0, 0, -1
    for t in range(n_steps):
        since += 1
        if since >= 16 and kills < 4:
            k = None
            for l in range(cls.n_line):             # the first line whose loss ends the episode right now
                if obs.line_status[l] and obs.time_before_cooldown_line[l] == 0:
                    sim_env = env.copy()
                    _, _, d_, _ = sim_env.step(env.action_space({"set_line_status": [(l, -1)]}))
                    sim_env.close()
                    if d_:
                        k = n0 + l
                        break
            assert k is not None
            kills += 1
        elif t % 5 == 3 and last >= 0:
            k = last                                # again: into the cooldown the entry just started
        elif t % 9 == 7:
            k = ambiguous[(t // 9) % len(ambiguous)]
        elif t % 4 == 1:
            k = -1                                  # do nothing
        else:
            k = int(order[walk % n0])
            walk += 1
        last = k
        act = env.action_space({}) if k < 0 else to_reference(env.action_space, table[k], cls.dim_topo)
        obs, reward, done, info = env.step(act)
        note(step_row(env, obs, reward, info, done), k)
        if done:
            obs = reset()
            since, last = 0, -1
    meta = reward_meta(env)
    pr = env.parameters
    env.close()
    step = np.asarray(rec["is_reset"]) == 0
    ill, amb, dn = (np.asarray(rec[k]).astype(bool) for k in ("is_illegal", "is_ambiguous", "done"))
    cover = dict(illegal=int((ill & ~dn).sum()), ambiguous=int((amb & ~dn).sum()), game_over=int(dn.sum()), plain=int((step & ~ill & ~amb & ~dn).sum()))
    print("topo:", cover, flush=True)
    assert cover["illegal"] >= 10 and cover["ambiguous"] >= 5 and cover["game_over"] >= 3 and cover["plain"] >= 40, cover
    used = sorted(set(rec["scenario"]))
    n_rows = max(rec["row"]) + 2
    _, ch = load_chronics_multifolder(chron_dir, model, prods_charac=charac, max_rows=n_rows, truncate=True)
    out = dict(meta, grid=np.array(env_name), off=off, items=items, table_seed=np.int32(seed), n_table=np.int32(n0), scenarios_used=np.array(used, np.int32),
               params=np.array([pr.MAX_SUB_CHANGED, pr.MAX_LINE_STATUS_CHANGED, pr.NB_TIMESTEP_COOLDOWN_SUB, pr.NB_TIMESTEP_COOLDOWN_LINE,
                                pr.NB_TIMESTEP_RECONNECTION], np.int32),
               played=np.asarray(rec["played"], np.int32), scenario=np.asarray(rec["scenario"], np.int32), row=np.asarray(rec["row"], np.int32))
    for k, v in ch.items():
        if k in ("load_p", "load_q", "prod_p", "prod_v"):
            out["chron_" + k] = v[used].astype(np.float32)
        elif k == "maintenance":
            assert not v[used][:, :n_rows].any(), "a maintenance in the recorded window: choose another seed"
    finish("case14_topo", out, rec)


# ---- fixtures 2 and 3: redispatch / storage / curtailment under the environment's dynamics ----
def record_dyn(tag, env_name, n_steps, seed, every, charge_unit, curtail, push_from=None, n_move=2, amp=(0.2, 0.7), sto_amp=None):
    """the actions of make_envdyn_fixtures.record: every `every` steps `n_move` redispatchable generators move against each other and every
    storage unit gets a set-point, unit `charge_unit` close to its largest absorption until _compute_storage clamps it at Emax and from
    the middle of the episode the opposite; with `curtail` two renewable generators are curtailed and released; from step `push_from`
    on that recorder's push recipe (every step asks for +ramp on PUSH[0], storage every third step).  `sto_amp` (the large grid, where
    the storage term must weigh 100 bounds of a reward dominated by max_regret): every unit at that fraction of its largest power, its sign
    turning every five steps, so that no unit reaches Emax or Emin: with 84 MW of storage in all, no step of that grid can show both the
    storage term AND the difference between requested and clamped power at 100 bounds; the clamped steps are the small grid's."""
    from grid2op.Action import DontAct
    from grid2op.Opponent import BaseOpponent
    from grid2op.Parameters import Parameters
    from grid2op_amd.chronics import load_chronics_folder
    from grid2op_amd.grid_model import GridModel
    p = Parameters()
    p.NO_OVERFLOW_DISCONNECTION = True
    env = make_env(env_name, p, opponent_class=BaseOpponent, opponent_action_class=DontAct, opponent_init_budget=0.0, opponent_budget_per_ts=0.0)
    cls = type(env)
    env.seed(seed)
    env.set_id(0)
    env.reset()
    rng = np.random.default_rng(seed)
    disp = np.nonzero(cls.gen_redispatchable)[0]
    rec = {k: [] for k in STEP_KEYS + ("row", "act_redisp", "act_storage", "act_curtail")}
    data = env.chronics_handler.real_data.data
    charge0 = np.array(env._storage_current_charge, np.float64)
    n_push = n_steps if push_from is None else push_from
    for t in range(n_steps):
        red = np.zeros(cls.n_gen, np.float32)
        sto = np.zeros(cls.n_storage, np.float32)
        cur = np.full(cls.n_gen, -1.0, np.float32)
        if curtail and t % 8 == 2:
            ren = np.nonzero(cls.gen_renewable)[0]
            ratio = np.asarray(data.prod_p[data.current_index + 1])[ren] / cls.gen_pmax[ren]
            k = ren[np.argsort(-ratio)[(t // 8) % 2 * 2:(t // 8) % 2 * 2 + 2]]
            cur[k] = 1.0 if t >= 24 else (ratio[np.isin(ren, k)] * rng.uniform(0.85, 0.95, 2)).astype(np.float32)
        if t >= n_push:
            up, d1, d2 = PUSH
            red[up] = cls.gen_max_ramp_up[up]
            red[d1] = -min(cls.gen_max_ramp_down[d1], cls.gen_max_ramp_up[up])
            red[d2] = -(cls.gen_max_ramp_up[up] + red[d1])
            if t % 3 == 1:
                sto[:] = rng.uniform(-3.0, 3.0, cls.n_storage)
        elif t % every == 0:
            k = rng.choice(disp, size=min(len(disp), n_move), replace=False)
            red[k] = cls.gen_max_ramp_up[k] * rng.uniform(amp[0], amp[1], len(k)) * np.tile([1.0, -1.0], n_move)[:len(k)]
            if sto_amp is None:
                sto[:] = rng.uniform(-4.0, 4.0, cls.n_storage)
                sto[charge_unit] = (0.9 if t < n_push // 2 else -0.9) * cls.storage_max_p_absorb[charge_unit]
            else:
                sto[:] = sto_amp * cls.storage_max_p_absorb * np.where(((t + np.arange(cls.n_storage)) // 5) % 2 == 0, 1.0, -1.0)
        act = {}
        if (red != 0).any():
            act["redispatch"] = [(int(g), float(red[g])) for g in np.nonzero(red)[0]]
        if (sto != 0).any():
            act["set_storage"] = [(int(i), float(sto[i])) for i in np.nonzero(sto)[0]]
        if (cur != -1).any():
            act["curtail"] = [(int(g), float(cur[g])) for g in np.nonzero(cur != -1)[0]]
        obs, reward, done, info = env.step(env.action_space(act))
        assert not done, (t, info["exception"])
        row = step_row(env, obs, reward, info, done)
        row.update(row=int(data.current_index), act_redisp=red, act_storage=sto, act_curtail=cur)
        for k in rec:
            rec[k].append(row[k])
    out = reward_meta(env)
    out.update(grid=np.array(env_name), storage_charge0=charge0, row=np.asarray(rec["row"], np.int32), act_redisp=np.asarray(rec["act_redisp"], np.float32),
               act_storage=np.asarray(rec["act_storage"], np.float32), act_curtail=np.asarray(rec["act_curtail"], np.float32),
               pmin=cls.gen_pmin.astype(np.float64), pmax=cls.gen_pmax.astype(np.float64), ramp_up=cls.gen_max_ramp_up.astype(np.float64),
               ramp_down=cls.gen_max_ramp_down.astype(np.float64), redispatchable=cls.gen_redispatchable.astype(bool),
               renewable=cls.gen_renewable.astype(bool), eps_poly=np.float64(env._epsilon_poly), tol_poly=np.float64(env._tol_poly),
               activate_storage_loss=np.bool_(env.parameters.ACTIVATE_STORAGE_LOSS),
               storage_Emax=cls.storage_Emax.astype(np.float64), storage_Emin=cls.storage_Emin.astype(np.float64),
               storage_loss=cls.storage_loss.astype(np.float64), storage_charging_efficiency=cls.storage_charging_efficiency.astype(np.float64),
               storage_discharging_efficiency=cls.storage_discharging_efficiency.astype(np.float64))
    m = GridModel.load_npz(os.path.join(HERE, f"{env_name}.grid.npz"))
    ch = load_chronics_folder(env.chronics_handler.get_id(), m, max_rows=n_steps + 4)
    for k in ("load_p", "load_q", "prod_p", "prod_v"):
        out["ch_" + k] = ch[k]
    env.close()
    ok = ~(np.asarray(rec["is_illegal"]).astype(bool) | np.asarray(rec["failed_redisp"]).astype(bool))
    both = ok & (np.abs(np.asarray(rec["actual_dispatch"])).sum(1) > 0) & (np.abs(np.asarray(rec["storage_power"])).sum(1) > 0)
    clamped = both & (np.abs(np.asarray(rec["storage_power"]) - np.asarray(rec["act_storage"])).max(1) > 0.5)
    cover = dict(cancelled=int(np.asarray(rec["failed_redisp"]).sum()), dispatch_and_storage=int(both.sum()), clamped=int(clamped.sum()))
    print(f"{tag}:", cover, flush=True)
    assert cover["dispatch_and_storage"] >= 1 and (cover["clamped"] >= 1) == (sto_amp is None) and (push_from is None or cover["cancelled"] >= 3), cover
    finish(tag, out, rec)


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
    if not only or "topo" in only:
        record_topo(reference)
    if not only or "storage" in only:
        record_dyn("case14_storage", "educ_case14_storage", 36, 5, 2, 1, False, push_from=24)
    if not only or "wcci" in only:
        record_dyn("wcci2022", "l2rpn_wcci_2022_dev", 40, 6, 1, 1, True, n_move=8, amp=(0.5, 0.9), sto_amp=0.98)


if __name__ == "__main__":
    main()
