"""Combined topology + injection actions of the batched acting path on the device (include/gridpf.h gpf_set_combined_actions,
grid2op_amd/csrc/gridpf_combined.hpp): an engine in combined mode against a TWIN with the mode off that the host steers from the
restatement (tests/combined_ref.py) -- per launch the twin gets the surviving topology through set_topology / set_cooldown /
set_sub_cooldown / set_last_bus and the surviving injection rows through set_lane_actions / set_lane_curtailment --, bit for bit; the mode
with one kind of action only against an engine without it; permutation, shards, auto-reset, episode limits and rewards; the refusals.

Every test calls `set_combined_actions`."""
import numpy as np
import pytest

import combined_ref as CR
from conftest import golden_path
from topo_rules_ref import TopoRules

pytestmark = pytest.mark.gpu

RULES = dict(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=3)
CASES = ("both_legal", "look_param", "reconnection", "topo_ambiguous", "fixed_gen", "ramp_up", "ramp_down", "storage_power", "curtail_range",
         "curtail_fixed", "disco_storage", "disco_reconnects", "illegal_redisp", "game_over")
N_LAUNCH = 3


def _load(name):
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path(f"{name}.grid.npz"))
    fx = dict(np.load(golden_path(f"envdyn_{name}.npz")))
    return m, fx


def _table(m):
    """line switches, a substation split, an entry that disconnects storage unit 0 and one that reconnects it, two lines at once (illegal by
    LookParam), an ambiguous entry; returns (table, names -> index)"""
    from topo_rules_ref import topo_pos_sub
    ps = topo_pos_sub(m)
    sub = max(range(m.n_sub), key=lambda s: (ps == s).sum())
    pos = np.flatnonzero(ps == sub)
    split = {int(p): 1 + (i % 2) for i, p in enumerate(pos)}
    table = [{"set_line_status": [(l, -1)]} for l in range(4)]                       # 0..3
    table += [{"change_line_status": [4]}, {"set_bus": split}]                       # 4, 5
    idx = dict(line=0, line2=1, change=4, split=5)
    if m.n_storage:
        p0 = int(m.storage_pos_topo_vect[0])
        table += [{"set_bus": {p0: -1}}, {"set_bus": {p0: 1}}]                       # 6, 7
        idx.update(sto_off=6, sto_on=7)
    idx["two_lines"] = len(table)
    table.append({"set_line_status": [(5, -1), (6, -1)]})
    idx["ambiguous"] = len(table)
    table.append({"set_bus": {int(pos[0]): 2}, "change_bus": [int(pos[0])]})
    return table, idx


def _engine(m, fx, n, combined=True, check_values=True, factory=None, table=None):
    from grid2op_amd.engine import PowerFlowEngine
    eng = factory(m, n) if factory else PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"]))
    eng.set_thermal_limits(fx["thermal_limit"])
    eng.set_gen_limits(fx["pmin"], fx["pmax"], fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], eps_poly=float(fx["eps_poly"]))
    if m.n_storage:
        eng.set_storage_params(fx["storage_Emax"], fx["storage_Emin"], fx["storage_loss"], fx["storage_charging_efficiency"],
                               fx["storage_discharging_efficiency"], fx["storage_charge0"], float(fx["delta_time_seconds"]), bool(fx["activate_storage_loss"]))
    eng.set_env_dynamics(True, tol_poly=float(fx["tol_poly"]))
    if "renewable" in fx:
        eng.set_gen_renewable(fx["renewable"])
    eng.set_topo_rules(**RULES)
    eng.upload_topo_actions(table if table is not None else _table(m)[0])
    if combined:
        eng.set_combined_actions(True, check_values=check_values, storage_max_p_prod=fx.get("storage_max_p_prod") if m.n_storage else None,
                                 storage_max_p_absorb=fx.get("storage_max_p_absorb") if m.n_storage else None)
    return eng


def _limits(m, fx):
    return CR.Limits(fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], fx.get("renewable"), fx.get("storage_max_p_prod") if m.n_storage else None,
                     fx.get("storage_max_p_absorb") if m.n_storage else None, m.storage_pos_topo_vect if m.n_storage else ())


def _script(m, fx, idx, n, seed, all_cases=CASES):
    """Per-lane actions of N_LAUNCH launches, lane k playing coverage case k mod len(cases) (a case that needs a prepared state gets it in
    `prep`), the launches around the case's own drawn from the seed.  -> (cases, act[launch] = (index, redisp, storage, curtail), prep)"""
    rng = np.random.default_rng(seed)
    ng, ns = m.n_gen, m.n_storage
    ren = np.flatnonzero(fx["renewable"]) if "renewable" in fx else np.zeros(0, int)
    disp = np.flatnonzero(fx["redispatchable"])
    fixed = np.flatnonzero(~np.asarray(fx["redispatchable"], bool))
    cases = [c for c in all_cases if (ns or c not in ("storage_power", "disco_storage", "disco_reconnects")) and (len(fixed) or c != "fixed_gen")]
    T = fx["ch_load_p"].shape[0]
    case_of = [cases[k % len(cases)] for k in range(n)]
    acts = [(np.full(n, -1, np.int32), np.zeros((n, ng), np.float32), np.zeros((n, ns), np.float32), np.full((n, ng), -1.0, np.float32))
            for _ in range(N_LAUNCH)]
    prep = dict(sto_off=[], target={}, far=[], offset=np.zeros(n, np.int32))

    def legal_pair(k, a, scale=0.3):
        g = rng.choice(disp, 2, replace=False)
        amp = np.float32(min(fx["ramp_up"][g[0]], fx["ramp_down"][g[1]]) * scale)
        a[1][k, g[0]], a[1][k, g[1]] = amp, -amp
        if ns:
            a[2][k] = rng.uniform(-0.5, 0.5, ns).astype(np.float32) * np.minimum(fx["storage_max_p_prod"], fx["storage_max_p_absorb"]).astype(np.float32)

    for k, c in enumerate(case_of):
        prep["offset"][k] = int(rng.integers(0, T - 8))
        a0, a1, a2 = acts
        # launch 0: a legal line switch for the lanes whose case needs a cooldown (and the game over); launch 1: the case
        a0[0][k] = idx["line"] if c in ("reconnection", "game_over") else -1
        if rng.random() < 0.5:
            legal_pair(k, a0, 0.1)
        a1[0][k] = idx["split"]
        legal_pair(k, a1)
        if c == "both_legal":
            pass
        elif c == "look_param":
            a1[0][k] = idx["two_lines"]
        elif c == "reconnection":
            a1[0][k] = idx["line"]
        elif c == "topo_ambiguous":
            a1[0][k] = idx["ambiguous"] if k % 2 else 10 ** 6
        elif c == "fixed_gen":
            a1[1][k, fixed[0]] = 1e-3
        elif c == "ramp_up":
            g = disp[0]
            a1[1][k, g] = np.nextafter(np.float32(fx["ramp_up"][g]), np.float32(np.inf))
        elif c == "ramp_down":
            g = disp[-1]
            a1[1][k, g] = -np.nextafter(np.float32(fx["ramp_down"][g]), np.float32(np.inf))
        elif c == "storage_power":
            a1[2][k, ns - 1] = np.nextafter(np.float32(fx["storage_max_p_absorb"][ns - 1]), np.float32(np.inf))
        elif c == "curtail_range":
            a1[3][k, ren[0] if len(ren) else 0] = 1.5 if k % 2 else -0.5
        elif c == "curtail_fixed":
            a1[3][k, np.flatnonzero(~np.asarray(fx.get("renewable", np.zeros(ng)), bool))[0]] = 0.5
        elif c == "disco_storage":
            prep["sto_off"].append(k)
            a1[0][k] = idx["line"]
            a1[2][k, 0] = 1.0
        elif c == "disco_reconnects":
            prep["sto_off"].append(k)
            a1[0][k] = idx["sto_on"]
            a1[2][k, 0] = 1.0
        elif c == "illegal_redisp":
            g = disp[0]
            prep["target"][k] = g
            a1[1][k] = 0.0
            a1[1][k, g] = np.float32(fx["ramp_up"][g] * 0.9)
            a1[0][k] = idx["line"]
        elif c == "game_over":                                             # at launch 0: no projection meets set-points 200 MW away
            prep["far"].append(k)
            legal_pair(k, a0, 0.2)
        a2[0][k] = int(rng.choice([-1, idx["line"], idx["split"], idx["change"]]))
        if rng.random() < 0.6:
            legal_pair(k, a2, 0.2)
    return case_of, acts, prep


def _prepare(eng, m, fx, prep):
    eng.set_lane_chronics(lane_offset=prep["offset"])
    if prep["sto_off"]:
        topo, sb = eng.get_topology()
        for k in prep["sto_off"]:
            topo[k, m.storage_pos_topo_vect[0]] = -1
            eng.set_topology(topo[k:k + 1], sb[k:k + 1] if m.n_shunt else None, lane0=k)
    for k in prep["far"]:
        eng.set_env_state(k, prev_p=(fx["ch_prod_p"][prep["offset"][k]] + 200.0)[None])
    span = (fx["pmax"] - fx["pmin"]).astype(np.float32)
    for k, g in prep["target"].items():
        st = eng.env_state(k, 1)
        st["target"][0, g] = span[g] - np.float32(0.5 * fx["ramp_up"][g])
        st["already_modified"][0, g] = True
        eng.set_env_state(k, target=st["target"], already_modified=st["already_modified"])


def _prep_take(prep, order):
    """the preparation of an engine whose lane j is lane order[j] of the script"""
    order = np.asarray(order)
    at = {int(k): j for j, k in enumerate(order)}
    return dict(sto_off=[at[k] for k in prep["sto_off"] if k in at], far=[at[k] for k in prep["far"] if k in at],
                target={at[k]: g for k, g in prep["target"].items() if k in at}, offset=prep["offset"][order])


def _state(eng):
    r = eng.results(with_bus=False)
    rho = eng.step_outputs()[0]
    return dict(out=r.out, status=r.status, rho=rho, topo=eng.get_topology()[0], line_cd=eng.cooldown(), sub_cd=eng.sub_cooldown(), last=eng.last_bus(),
                done=eng.episode()[0], **{"env_" + k: v for k, v in eng.env_state().items()})


def _assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, np.argwhere(np.asarray(a[k]) != np.asarray(b[k]))[:5])


def _hand_over(eng, on_device, ix, red, sto, cur, with_cur):
    import torch
    if not on_device:
        eng.set_lane_topo_actions(ix)
        eng.set_lane_actions(red, sto if sto.shape[1] else None)
        if with_cur:
            eng.set_lane_curtailment(cur)
        return
    v = eng.device_views()
    with torch.cuda.stream(v["stream"]):
        v["act_topo"].copy_(torch.from_numpy(ix.reshape(-1, 1)).to(v["act_topo"].device))
        v["act_redispatch"].copy_(torch.from_numpy(red).to(v["act_redispatch"].device))
        if sto.shape[1]:
            v["act_storage"].copy_(torch.from_numpy(sto).to(v["act_storage"].device))
        v["act_curtail"].copy_(torch.from_numpy(cur).to(v["act_curtail"].device))
    eng.topo_actions_on_device(True)
    eng.lane_actions_on_device(redispatch=True, storage_power=bool(sto.shape[1]), curtailment=True)


def _twin_run(name, n, on_device, seed=11):
    m, fx = _load(name)
    table, idx = _table(m)
    comb, twin = _engine(m, fx, n, table=table), _engine(m, fx, n, combined=False, table=table)
    off, items = comb.pack_actions(table)
    rules = TopoRules(m, off, np.asarray(items).reshape(-1, 3), legal_rules=True, max_sub=1, max_line=1, cd_sub=3, cd_line=3)
    lane = CR.CombinedLane(rules, _limits(m, fx))
    if n >= len(CASES):
        _twin_play(m, fx, idx, comb, twin, lane, n, on_device, seed, CASES, name)
    else:                                                                   # fewer lanes than cases: the cases one after the other
        for s, c in enumerate(CASES):
            for e in (comb, twin):
                e.set_lane_topo_actions(None)
                e.reset()
            _twin_play(m, fx, idx, comb, twin, lane, n, on_device, seed + s, (c,), name)
    comb.close()
    twin.close()


def _twin_play(m, fx, idx, comb, twin, lane, n, on_device, seed, all_cases, name):
    case_of, acts, prep = _script(m, fx, idx, n, seed, all_cases)
    for e in (comb, twin):
        _prepare(e, m, fx, prep)
    seen = {c: 0 for c in set(case_of)}
    with_cur = "renewable" in fx and bool(np.any(fx["renewable"]))
    for L, (ix, red, sto, cur) in enumerate(acts):
        # host-written curtailment is range-checked at the call: the two curtailment value rules are device-written cases
        if not on_device:
            cur = np.where((cur == -1) | ((cur >= 0) & (cur <= 1)), cur, -1.0).astype(np.float32)
        before = _state(twin)
        _hand_over(comb, on_device, ix, red, sto, cur, with_cur)
        comb.step(L, nb_ts_reco=10)
        # the twin, steered from the restatement
        pre = [lane.pre(before["topo"][k], before["line_cd"][k], before["sub_cd"][k], before["last"][k], int(ix[k]), red[k],
                        sto[k] if m.n_storage else None, cur[k] if (with_cur or on_device) else None) for k in range(n)]
        rows = np.stack([p["row"] for p in pre]).astype(np.int32)
        for k in np.flatnonzero((rows != before["topo"]).any(1)):
            twin.set_topology(rows[k:k + 1], lane0=int(k))
        twin.set_lane_actions(np.stack([p["redisp"] for p in pre]), np.stack([p["storage"] for p in pre]) if m.n_storage else None)
        if with_cur or on_device:
            c_surv = np.stack([p["curtail"] for p in pre])
            if (c_surv != -1).any() and with_cur:
                twin.set_lane_curtailment(c_surv)
        twin.step(L, nb_ts_reco=10)
        mid = _state(twin)
        ill_redisp = mid["env_illegal"] != before["env_illegal"]
        post = [lane.post(pre[k], mid["topo"][k], mid["line_cd"][k], before["sub_cd"][k], before["last"][k], bool(mid["done"][k]), bool(ill_redisp[k]))
                for k in range(n)]
        twin.set_cooldown(np.stack([p[0] for p in post]).astype(np.int32))
        twin.set_sub_cooldown(np.stack([p[1] for p in post]).astype(np.int32))
        twin.set_last_bus(np.stack([p[2] for p in post]).astype(np.int32))
        _assert_same(_state(comb), _state(twin), (name, n, L))
        fl = comb.action_flags()
        want = np.stack([p[3] for p in post])
        got = np.stack([fl["is_illegal"], fl["is_ambiguous"], fl["is_illegal_redisp"], fl["reason"]], 1).astype(np.uint8)
        assert np.array_equal(got, want), (name, n, L, np.argwhere(got != want)[:5])
        t_ill, t_amb = comb.topo_action_flags()
        assert np.array_equal(t_ill, [p["topo_flags"][0] for p in pre]) and np.array_equal(t_amb, [p["topo_flags"][1] for p in pre]), (name, n, L)
        for k, c in enumerate(case_of):                                     # every coverage case happened, on the restatement
            if L == (0 if c == "game_over" else 1):
                p, f = pre[k], post[k][3]
                applied = (rows[k] != before["topo"][k]).any()
                inj_void = not p["redisp"].any()
                hit = dict(both_legal=applied and not inj_void and not f[:3].any(), look_param=f[0] and f[3] == CR.TOPO_RULES and inj_void and not applied,
                           reconnection=f[0] and f[3] == CR.TOPO_RULES and inj_void and before["line_cd"][k].any(),
                           topo_ambiguous=f[1] and f[3] == CR.TOPO_AMBIGUOUS and inj_void, fixed_gen=f[1] and f[3] == CR.REDISP_FIXED_GEN and not applied,
                           ramp_up=f[1] and f[3] == CR.REDISP_RAMP_UP and not applied, ramp_down=f[1] and f[3] == CR.REDISP_RAMP_DOWN and not applied,
                           storage_power=f[1] and f[3] == CR.STORAGE_POWER and not applied,
                           curtail_range=(f[1] and f[3] == CR.CURTAIL_RANGE and not applied) or not on_device,
                           curtail_fixed=(f[1] and f[3] == CR.CURTAIL_FIXED_GEN and not applied) or not on_device,
                           disco_storage=f[0] and f[3] == CR.DISCO_STORAGE and not applied and inj_void,
                           disco_reconnects=not f[:3].any() and applied and rows[k][m.storage_pos_topo_vect[0]] == 1 if m.n_storage else True,
                           illegal_redisp=f[2] and not f[0] and applied and not mid["done"][k] and np.array_equal(post[k][1], np.maximum(before["sub_cd"][k] - 1, 0))
                           and np.array_equal(post[k][0], mid["line_cd"][k]),
                           game_over=bool(mid["done"][k]) and applied)[c]
                seen[c] += int(bool(hit))
    want_cases = set(case_of)
    assert all(seen[c] >= 1 for c in want_cases), (name, n, {c: seen[c] for c in sorted(want_cases)})


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("on_device", [False, True])
def test_against_a_twin_steered_from_the_restatement_14_substations(n, on_device):
    _twin_run("educ_case14_storage", n, on_device)


@pytest.mark.parametrize("on_device", [False, True])
def test_against_a_twin_steered_from_the_restatement_118_substations(on_device):
    _twin_run("l2rpn_wcci_2022_dev", 65, on_device)


def _plain_pair(n, check_values=True):
    m, fx = _load("educ_case14_storage")
    return m, fx, _engine(m, fx, n, check_values=check_values), _engine(m, fx, n, combined=False)


def test_one_kind_of_action_equals_the_mode_off():
    """only topology actions, and only injection actions with check_values off: bit for bit the launch of an engine without the mode"""
    n = 65
    m, fx, a, b = _plain_pair(n, check_values=False)
    _, idx = _table(m)
    rng = np.random.default_rng(3)
    for e in (a, b):
        e.set_lane_chronics(lane_offset=(np.arange(n) % 8).astype(np.int32))
    for L in range(4):
        ix = rng.choice([-1, idx["line"], idx["split"], idx["two_lines"], idx["ambiguous"], idx["change"]], n).astype(np.int32)
        red = np.zeros((n, m.n_gen), np.float32)
        disp = np.flatnonzero(fx["redispatchable"])
        red[:, disp[0]], red[:, disp[1]] = 0.5, -0.5
        sto = rng.uniform(-1, 1, (n, m.n_storage)).astype(np.float32)
        for e in (a, b):
            if L % 2 == 0:
                e.set_lane_topo_actions(ix)
            else:
                e.set_lane_actions(red, sto)
            e.step(L, nb_ts_reco=10)
        _assert_same(_state(a), _state(b), L)
        fl = a.action_flags()
        t_ill, t_amb = a.topo_action_flags()
        if L % 2 == 0:
            assert np.array_equal(fl["is_illegal"], t_ill) and np.array_equal(fl["is_ambiguous"], t_amb) and t_ill.any() and t_amb.any()
        else:
            assert not fl["is_illegal"].any() and not fl["is_ambiguous"].any()
    a.close()
    b.close()


def test_permutation_and_two_shards():
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.sharding import ShardedEngine
    n = 65
    m, fx = _load("educ_case14_storage")
    table, idx = _table(m)
    case_of, acts, prep = _script(m, fx, idx, n, 5)
    perm = np.random.default_rng(9).permutation(n)
    a = _engine(m, fx, n, table=table)
    c = _engine(m, fx, n, table=table)
    d = _engine(m, fx, n, table=table, factory=lambda mm, nn: ShardedEngine(
        mm, nn, devices=[0, 0], engine_factory=lambda m_, n_, dev, nbb: PowerFlowEngine(m_, n_lanes=n_, device=0, n_busbar=nbb)))
    _prepare(a, m, fx, prep)
    _prepare(c, m, fx, _prep_take(prep, perm))
    for e, (l0, bn) in zip(d.engines, d.blocks):
        _prepare(e, m, fx, _prep_take(prep, np.arange(l0, l0 + bn)))
    for L, (ix, red, sto, cur) in enumerate(acts):
        cur = np.full_like(cur, -1.0)
        for e, p in ((a, slice(None)), (c, perm), (d, slice(None))):
            e.set_lane_topo_actions(ix[p])
            e.set_lane_actions(red[p], sto[p])
            e.step(L, nb_ts_reco=10)
        sa, sc, sd = _state(a), _state(c), _state(d)
        _assert_same({k: v[perm] for k, v in sa.items()}, sc, ("perm", L))
        _assert_same(sa, sd, ("shards", L))
        fa, fc, fd = a.action_flags(), c.action_flags(), d.action_flags()
        for k in fa:
            assert np.array_equal(fa[k][perm], fc[k]) and np.array_equal(fa[k], fd[k]), (L, k)
    assert fa["is_illegal"].any() or fa["is_ambiguous"].any()
    views = d.combined_views()
    assert len(views) == 2 and sum(v["flags"].shape[0] for v in views) == n
    for e in (a, c, d):
        e.close()


def test_auto_reset_episode_limit_and_rewards():
    """a lane whose combined step ends its episode restarts; with a limit and rewards on, the rewards read the flags of the whole step"""
    from grid2op_amd.engine import reward_config
    n = 28
    m, fx = _load("educ_case14_storage")
    table, idx = _table(m)
    case_of, acts, prep = _script(m, fx, idx, n, 7)
    eng = _engine(m, fx, n, table=table)
    _prepare(eng, m, fx, prep)
    eng.set_rewards([reward_config("GameplayReward")])
    eng.set_episode_limit(2)
    resets0 = eng.episode()[2].copy()
    over = [k for k, c in enumerate(case_of) if c == "game_over"]
    for L, (ix, red, sto, cur) in enumerate(acts[:2]):
        eng.set_lane_topo_actions(ix)
        eng.set_lane_actions(red, sto)
        eng.step(L, nb_ts_reco=10, auto_reset=True)
        fl, ends, rw = eng.action_flags(), eng.episode_ends(), eng.rewards()[:, 0]
        bad = fl["is_illegal"] | fl["is_ambiguous"] | fl["is_illegal_redisp"]
        if L == 0:                                                          # the game over of a combined step: the lane restarts
            assert over and ends["terminated"][over].all() and not ends["terminated"].all()
            assert (eng.episode()[2][over] == resets0[over] + 1).all() and (eng.sub_cooldown()[over] == 0).all() and (eng.cooldown()[over] == 0).all()
            assert (rw[over] == -1.0).all()
        else:                                                               # the limit, and the rewards on the flags of the whole step
            alive = ~ends["terminated"]
            assert ends["truncated"][[k for k in range(n) if k not in over]].all() and not ends["truncated"][over].any()
            assert bad[alive].any() and (~bad[alive]).any()
            assert (rw[alive & bad] == -0.5).all() and (rw[alive & ~bad] == 1.0).all()
            assert fl["is_ambiguous"].any() and fl["is_illegal"].any() and fl["is_illegal_redisp"].any()
    eng.reset(0, 2)
    assert not np.stack(list(eng.action_flags(0, 2).values())).any()
    eng.copy_lanes(3, 0, 1)
    assert all(v[0] == v[3] for v in eng.action_flags().values())
    eng.sync()
    fv, fh = eng.combined_views()["flags"].cpu().numpy(), eng.action_flags()                 # the view aliases what the getter copies
    assert np.array_equal(fv[:, 0].astype(bool), fh["is_illegal"]) and np.array_equal(fv[:, 1].astype(bool), fh["is_ambiguous"]) and np.array_equal(fv[:, 3], fh["reason"])
    eng.close()


def test_refusals_and_off_against_never_on():
    from grid2op_amd.engine import GridPFError, PowerFlowEngine
    n = 8
    m, fx, a, b = _plain_pair(n)
    _, idx = _table(m)
    ix = np.full(n, idx["line"], np.int32)
    red, sto = np.zeros((n, m.n_gen), np.float32), np.full((n, m.n_storage), 0.5, np.float32)
    a.set_lane_topo_actions(ix)
    a.set_lane_actions(red, sto, hold_storage=True)
    with pytest.raises(GridPFError, match="held storage"):
        a.step(0, nb_ts_reco=10)
    a.set_lane_actions(red, sto)
    a.set_lane_topo_actions(ix)
    with pytest.raises(GridPFError, match="one-step"):
        a.step(0, n_steps=2, nb_ts_reco=10)
    a.set_lane_topo_actions(None)
    a.set_lane_actions(red, sto)
    with pytest.raises(GridPFError, match="combined mode"):
        a.step(0, n_steps=2, nb_ts_reco=10)
    bare = PowerFlowEngine(m, n_lanes=2, device=0)
    bare.set_topo_rules(**RULES)
    with pytest.raises(GridPFError, match="dynamics are off"):
        bare.set_combined_actions(True)
    bare.close()
    # off: the old refusal is back, and a run queues what an engine that never enabled the mode queues
    a.set_lane_topo_actions(None)
    a.reset()
    a.set_combined_actions(False)
    with pytest.raises(GridPFError, match="combined actions are off"):
        a.action_flags()
    a.set_lane_topo_actions(ix)
    a.set_lane_actions(red, sto)
    with pytest.raises(GridPFError, match="combined"):
        a.step(0, nb_ts_reco=10)
    a.set_lane_topo_actions(None)
    a.reset()
    b.reset()
    c0 = (a.counters(), b.counters())
    for L in range(3):
        for e in (a, b):
            if L == 1:
                e.set_lane_topo_actions(ix)
            else:
                e.set_lane_actions(red, sto)
            e.step(L, nb_ts_reco=10)
    _assert_same(_state(a), _state(b), "off")
    ca, cb = a.counters(), b.counters()
    assert {k: ca[k] - c0[0][k] for k in ca if isinstance(ca[k], (int, np.integer))} == {k: cb[k] - c0[1][k] for k in cb if isinstance(cb[k], (int, np.integer))}
    a.close()
    b.close()


# ---- the recordings of the unmodified reference environment, replayed through one-step launches ---------------------------------
N_LANES, STAGGER = 65, 4


@pytest.mark.parametrize("tag", ["case14_storage", "wcci118"])
def test_replay_of_the_recordings(tag):
    """tests/golden/combined_*.npz: every lane of a 65-lane batch plays the recorded steps, lane k starting k mod 4 launches late (a lane
    restarts where the recording resets).  Flags, topo_vect, line and substation cooldowns exact at every step.  The dynamics state with the
    two-fold tolerance of tests/test_gpu_envdyn.py: dispatch targets within 1e-4 MW of the restatement run with the EXACT minimiser of the
    projection (what the device computes) and within that file's 2.5 MW of the recording (SLSQP stops short of the minimiser, and a
    generator redispatched for the first time inherits the gap of `actual`), charge within 1e-4 MWh of both.  Every reward slot within one
    float32 spacing of the restatement (tests/reward_ref.py) on the device's own inputs, constant branches bit-equal."""
    import torch
    import reward_ref as R
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from test_gpu_reward import _check, _lane_row, _snapshot
    fx = dict(np.load(golden_path(f"combined_{tag}.npz")))
    m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
    n = N_LANES
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"]))
    T = fx["ch_load_p"].shape[0]
    eng.set_thermal_limits(fx["thermal_limit"])
    eng.set_gen_limits(fx["pmin"], fx["pmax"], fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], eps_poly=float(fx["eps_poly"]))
    eng.set_storage_params(fx["storage_Emax"], fx["storage_Emin"], fx["storage_loss"], fx["storage_charging_efficiency"],
                           fx["storage_discharging_efficiency"], fx["storage_charge0"], float(fx["delta_time_seconds"]), bool(fx["activate_storage_loss"]))
    eng.set_env_dynamics(True, tol_poly=float(fx["tol_poly"]))
    eng.set_gen_renewable(fx["renewable"])
    p = [int(x) for x in fx["params"]]
    eng.set_topo_rules(legal_rules=True, max_sub_changed=p[0], max_line_status_changed=p[1], cooldown_sub=p[2], cooldown_line=p[3])
    import os
    import sys
    sys.path.insert(0, os.path.dirname(golden_path("x")))
    from make_combined_fixtures import build_table
    table = build_table(m)[0]
    off, items = eng.pack_actions(table)
    assert np.array_equal(off, fx["off"]) and np.array_equal(np.asarray(items).reshape(-1, 3), fx["items"].reshape(-1, 3))
    eng.upload_topo_actions(table)
    eng.set_combined_actions(True, check_values=True, storage_max_p_prod=fx["storage_max_p_prod"], storage_max_p_absorb=fx["storage_max_p_absorb"])
    slots = R.fixture_slots(fx)
    eng.set_rewards([(k, list(q)) for k, q in slots], fx["gen_cost_per_MW"])
    v = eng.device_views()
    N = len(fx["done"])
    # the restatement with the exact minimiser through the recorded steps, once: the dispatch targets and the charge the device must show
    from test_oracle_envdyn import dyn_from_fixture
    rules = TopoRules(m, off, np.asarray(items).reshape(-1, 3), legal_rules=True, max_sub=p[0], max_line=p[1], cd_sub=p[2], cd_line=p[3])
    lane = CR.CombinedLane(rules, _limits(m, fx))
    ex_target, ex_charge = np.zeros((N, m.n_gen), np.float32), np.zeros((N, m.n_storage), np.float32)
    for i in range(N):
        if fx["is_reset"][i]:
            topo, ex = fx["topo_vect"][i], dyn_from_fixture(fx, exact=True)
            ex.prev_p[:] = fx["ch_prod_p"][fx["row"][i]]
            continue
        cd_l, cd_s = fx["cooldown_line"][i - 1], fx["cooldown_sub"][i - 1]
        pre = lane.pre(topo, cd_l, cd_s, np.maximum(topo, 1), int(fx["played"][i]), fx["act_redisp"][i], fx["act_storage"][i], fx["act_curtail"][i])
        ok, _, _ = ex.step(fx["ch_prod_p"][fx["row"][i]], pre["redisp"], pre["storage"], pre["curtail"])
        assert ok != bool(fx["done"][i]) and ex.illegal == bool(fx["failed_redisp"][i]) or fx["done"][i], i
        ex_target[i], ex_charge[i], topo = ex.target, ex.charge, fx["topo_vect"][i]
    group = np.arange(n) % STAGGER
    first = np.r_[False, fx["is_reset"][:-1].astype(bool)]                    # the first step of an episode: the lane starts from a reset
    seen = {str(c): 0 for c in fx["cases"]}
    for L in range(N + STAGGER - 1):
        j = L - group
        act = (j >= 0) & (j < N)
        jj = np.clip(j, 0, N - 1)
        act &= ~fx["is_reset"][jj].astype(bool)                               # (a lane idles while the recording resets)
        for k in np.flatnonzero(act & first[jj]):
            eng.reset(int(k), 1)
            eng.set_env_state(int(k), prev_p=fx["ch_prod_p"][fx["row"][jj[k] - 1]][None])
        eng.set_lane_chronics(lane_offset=np.where(act, (fx["row"][jj] - L) % T, 0).astype(np.int32))
        eng.set_lane_topo_actions(np.where(act, fx["played"][jj], -1).astype(np.int32))
        red = np.where(act[:, None], fx["act_redisp"][jj], 0.0).astype(np.float32)
        sto = np.where(act[:, None], fx["act_storage"][jj], 0.0).astype(np.float32)
        cur = np.where(act[:, None], fx["act_curtail"][jj], -1.0).astype(np.float32)
        with torch.cuda.stream(v["stream"]):                                 # device-written: the host call refuses curtailments out of range
            v["act_redispatch"].copy_(torch.from_numpy(red).to(v["act_redispatch"].device))
            v["act_storage"].copy_(torch.from_numpy(sto).to(v["act_storage"].device))
            v["act_curtail"].copy_(torch.from_numpy(cur).to(v["act_curtail"].device))
        eng.lane_actions_on_device(redispatch=True, storage_power=True, curtailment=True)
        eng.step(L, nb_ts_reco=p[4])
        fl, done, st = eng.action_flags(), eng.episode()[0], eng.env_state()
        a = np.flatnonzero(act)
        for key, got in (("is_illegal", fl["is_illegal"]), ("is_ambiguous", fl["is_ambiguous"]), ("done", done)):
            assert np.array_equal(got[a], fx[key][jj[a]].astype(bool)), (tag, L, key, a[got[a] != fx[key][jj[a]].astype(bool)][:5])
        live = a[~done[a]]
        assert np.array_equal(fl["is_illegal_redisp"][live], fx["failed_redisp"][jj[live]].astype(bool)), (tag, L)
        assert np.array_equal(eng.get_topology()[0][live], fx["topo_vect"][jj[live]]), (tag, L)
        assert np.array_equal(eng.cooldown()[live], fx["cooldown_line"][jj[live]]) and np.array_equal(eng.sub_cooldown()[live], fx["cooldown_sub"][jj[live]]), (tag, L)
        assert np.abs(st["target"][live] - ex_target[jj[live]]).max(initial=0) < 1e-4, (tag, L)
        assert np.abs(st["target"][live] - fx["target_dispatch"][jj[live]]).max(initial=0) < 2.5, (tag, L)
        assert np.abs(st["charge"][live] - ex_charge[jj[live]]).max(initial=0) < 1e-4, (tag, L)
        assert np.abs(st["charge"][live] - fx["storage_charge"][jj[live]]).max(initial=0) < 1e-4, (tag, L)
        assert np.abs(st["curtail_limit"][live] - fx["limit_curtailment"][jj[live]]).max(initial=0) < 1e-6, (tag, L)
        rw, snap = eng.rewards(), _snapshot(eng, "env")
        for g in range(STAGGER):
            lanes = np.arange(g, n, STAGGER)
            k = int(lanes[0])
            if not act[k]:
                continue
            assert all(rw[q].tobytes() == rw[k].tobytes() for q in lanes), (tag, L, g)
            _check(rw[k], slots, _lane_row(snap, k, fx["thermal_limit"], fx["gen_cost_per_MW"]), bool(done[k]),
                   bool(fl["is_illegal"][k] or fl["is_illegal_redisp"][k]), bool(fl["is_ambiguous"][k]), (tag, L, g))
        if act[0] and fx["case"][jj[0]] >= 0:
            seen[str(fx["cases"][fx["case"][jj[0]]])] += 1
    assert all(c >= 2 for c in seen.values()), seen
    eng.close()


def test_a_launch_without_topology_actions_is_screened_too():
    """check_values on, injection actions only: a lane that breaks a value rule, or gives power to a disconnected storage unit, is ambiguous /
    illegal and plays nothing; the others equal an engine without the mode that was handed the surviving rows"""
    n = 65
    m, fx, a, b = _plain_pair(n)
    rng = np.random.default_rng(23)
    off = (np.arange(n) % 8).astype(np.int32)
    topo, sb = a.get_topology()
    p0 = m.storage_pos_topo_vect[0]
    disco = np.arange(5, n, 13)
    for e in (a, b):
        e.set_lane_chronics(lane_offset=off)
        for k in disco:
            row = topo[k:k + 1].copy()
            row[0, p0] = -1
            e.set_topology(row, sb[k:k + 1] if m.n_shunt else None, lane0=int(k))
    disp = np.flatnonzero(fx["redispatchable"])
    lim = _limits(m, fx)
    for L in range(3):
        red = np.zeros((n, m.n_gen), np.float32)
        red[:, disp[0]], red[:, disp[1]] = 0.4, -0.4
        red[3::11, disp[0]] = np.nextafter(np.float32(fx["ramp_up"][disp[0]]), np.float32(np.inf))
        sto = rng.uniform(-1, 1, (n, m.n_storage)).astype(np.float32)
        sto[7::17, 1] = -np.nextafter(np.float32(fx["storage_max_p_prod"][1]), np.float32(np.inf))
        rows = a.get_topology()[0]
        scr = [CR.screen(lim, red[k], sto[k], None, rows[k]) for k in range(n)]
        void = np.array([s[0] or s[1] for s in scr])
        a.set_lane_actions(red, sto)
        a.step(L, nb_ts_reco=10)
        b.set_lane_actions(np.where(void[:, None], 0, red).astype(np.float32), np.where(void[:, None], 0, sto).astype(np.float32))
        b.step(L, nb_ts_reco=10)
        _assert_same(_state(a), _state(b), L)
        fl = a.action_flags()
        assert np.array_equal(fl["is_ambiguous"], [s[0] for s in scr]) and np.array_equal(fl["is_illegal"], [s[1] for s in scr]), L
        assert np.array_equal(fl["reason"], [s[2] for s in scr]) and not fl["is_illegal_redisp"].any()
        assert {CR.REDISP_RAMP_UP, CR.STORAGE_POWER, CR.DISCO_STORAGE, CR.NONE} <= set(int(x) for x in fl["reason"])
    a.close()
    b.close()
