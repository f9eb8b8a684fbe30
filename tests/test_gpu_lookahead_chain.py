"""The look-ahead chain on the device (include/gridpf.h gpf_set_lookahead_chain / gpf_lookahead_chain, grid2op_amd/csrc/gridpf_lookahead.hpp):
the recordings of the unmodified reference's obs.get_forecast_env() (tests/golden/lookahead_chain_*.npz, one environment lane per recorded
state), n_steps = 1 against `lookahead`, the scratch lanes against a twin engine that steps the same rows one launch at a time, the
chain's outputs against the host emulator on the device's own rows, `play` against an engine whose host writes the same indices, and a
`ShardedEngine` over one device.

Bounds: flags, topology rows, line status and survived steps against the recording exactly; rho per step within 3e-5 (tests/lookahead_ref.RHO_TOL:
what tests/test_gpu_simulate.py holds this step kernel to -- every step is a power flow of its own, nothing accumulates); everything else
bit for bit."""
import json

import numpy as np
import pytest

import lookahead_chain_ref as LC
from conftest import golden_path

pytestmark = pytest.mark.gpu

FC_H = 4
SCALE = {"l2rpn_case14_sandbox": 0.8, "rte_case5_example": 0.75}      # thermal limits lowered: some lanes lose lines and fail inside the horizon, some survive it
CASE5_LIMITS = np.array([600., 220., 160., 160., 600., 300., 300., 160.])     # (rte_case5_example ships none with its chronics)


def _table(m):
    lines = [{"set_line_status": [(l, -1)]} for l in range(min(m.n_line, 6))]
    return lines + [{"change_line_status": [1]}, {"set_line_status": [(0, +1)], "change_line_status": [0]},
                    {"set_bus": {int(m.line_or_pos_topo_vect[2]): 2, int(m.load_pos_topo_vect[0]): 2}}]


def _forecasts(tab, horizons):
    """horizon h of row r: the chronics of row r + h scaled up a little more at every horizon (loads and productions alike)"""
    T = tab.shape[0]
    return np.stack([tab[(np.arange(T) + h + 1) % T] * np.float32(1.0 + 0.02 * (h + 1)) for h in range(horizons)], axis=1)


def _engine(grid, n_lanes, offsets=None, horizons=FC_H, limit_scale=1.0):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path(f"{grid}.grid.npz"))
    ch = dict(np.load(golden_path(f"{grid}.chronics.npz")))
    if "prod_v" not in ch:
        ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
    eng = PowerFlowEngine(m, n_lanes=n_lanes, device=0)
    tab = eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"])[:48]
    eng.upload_chronics(tab)
    fc = _forecasts(tab, horizons)
    eng.upload_forecasts(fc[None])
    eng.set_lane_chronics(lane_offset=7 * np.arange(n_lanes) if offsets is None else np.asarray(offsets))
    eng.set_thermal_limits(eng_limits(grid) * limit_scale)
    return m, eng, fc


def _chain_state(eng, n_env, K):
    """what a chain leaves: the look-ahead's outputs, the chain's, and the scratch lanes' own rows"""
    out = dict(eng.lookahead_values())
    out.update(eng.lookahead_chain_values())
    rho, ovc, _ = eng.step_outputs(n_env, n_env * K)
    out["rho"], out["ovc"] = rho.reshape(n_env, K, -1), ovc.reshape(n_env, K, -1)
    out["done"] = eng.episode(n_env, n_env * K)[0].reshape(n_env, K)
    return out


def _check_against_the_emulator(eng, n_env, K, H, t, cand, **kw):
    """chains of 1 .. H steps from the same observation: the chain of h steps leaves the scratch lanes as step h of the chain of H steps
    does (the environments are only read), so the device's own rho rows and done bytes of every step are on the host -- value_h, value,
    peak, survived, flags, best and fallback of the chain of H steps are the emulator's on them, bit for bit; the views are the getters."""
    rho, done = [], []
    for h in range(1, H + 1):
        eng.lookahead_chain(t, h, cand, **kw)
        st = _chain_state(eng, n_env, K)
        rho.append(st["rho"]); done.append(st["done"])
        assert (st["survived"] <= h).all()
    rho, done = np.stack(rho, axis=2), np.stack(done, axis=2)              # [n_env, K, H, L], [n_env, K, H]
    flags1 = None
    eng.lookahead(t, 1, cand, **kw)
    flags1 = eng.lookahead_values()["flags"] & 3
    eng.lookahead_chain(t, H, cand, **kw)
    st = _chain_state(eng, n_env, K)
    assert st["value_h"].shape[:2] == (n_env, K) and st["value_h"].shape[2] >= H
    for i in range(n_env):
        lanes = [LC.emul_lane(rho[i, k], done[i, k]) for k in range(K)]
        for k, want in enumerate(lanes):
            got = dict(survived=int(st["survived"][i, k]), peak=st["peak"][i, k], value=st["value"][i, k], value_h=st["value_h"][i, k, :H],
                       failed=bool(st["flags"][i, k] & LC.DONE))
            assert LC.same_lane(want, got), (i, k, want, got)
        flags = LC.chain_flags(flags1[i], [l["failed"] for l in lanes])
        assert np.array_equal(st["flags"][i], flags), i
        best, bv, n_ok, n_done = LC.summary(st["value"][i], flags)
        assert (st["best"][i], st["best_value"][i].tobytes(), st["n_playable"][i], st["n_done"][i]) == (best, bv.tobytes(), n_ok, n_done), i
        fb = LC.emul_fallback(st["survived"][i], st["peak"][i], flags)
        assert (int(st["fallback"][i]), int(st["fallback_steps"][i])) == fb == LC.fallback(st["survived"][i], st["peak"][i], flags), i
    v = eng.lookahead_chain_views()
    eng.sync()
    for key in ("survived", "peak", "value_h", "fallback", "fallback_steps"):
        assert np.array_equal(v[key].cpu().numpy(), eng.lookahead_chain_values()[key]), key
    return st, rho, done


@pytest.mark.parametrize("grid,n_env,K", [("l2rpn_case14_sandbox", 1, 1), ("l2rpn_case14_sandbox", 3, 5), ("rte_case5_example", 2, 64),
                                          ("rte_case5_example", 2, 65), ("rte_case5_example", 65, 2)])
def test_shapes_one_step_is_the_look_ahead_and_every_output_is_the_emulators(grid, n_env, K):
    """(n_env, K) at which the kernels' loops and blocks end differently: one lane, n_env K = 15 and 130 (no multiple of the four
    wavefronts of a block), K = 64 / 65 (one / two trips of the summary's strided loop), 65 environments (17 blocks of the summary).
    n_steps = 1 is `lookahead(t, 1)` bit for bit; H = 2 and H = the uploaded horizons against the emulator; thermal limits lowered so
    that lines run above 1, the protections trip some of them on the way and some lanes end their episode."""
    n = n_env * (1 + K)
    m, eng, _ = _engine(grid, n, offsets=(3 * np.arange(n)) % 40, limit_scale=SCALE[grid])
    table = _table(m)
    eng.set_topo_rules(max_sub_changed=1, max_line_status_changed=1)
    eng.upload_topo_actions(table)
    eng.set_lookahead(K, n_env)
    eng.set_lookahead_chain(FC_H)
    cand = ((np.arange(n_env * K).reshape(n_env, K) * 5 + 1) % (len(table) + 2) - 1).astype(np.int32)       # -1 .. len(table): one past the table too
    kw = dict(cascade=True, nb_ts_allowed=2, hard_overflow=2.0)
    eng.set_overflow_count(np.ones((n_env, m.n_line), np.int32), lane0=0)                                      # counters already running
    eng.lookahead(2, 1, cand, **kw)
    want = eng.lookahead_values()
    want_rows = eng.results(n_env, n_env * K).out.tobytes()
    eng.lookahead_chain(2, 1, cand, **kw)
    got = eng.lookahead_values()
    for key in ("value", "flags", "best", "best_value", "n_playable", "n_done"):
        assert got[key].tobytes() == want[key].tobytes(), key
    assert eng.results(n_env, n_env * K).out.tobytes() == want_rows
    ch = eng.lookahead_chain_values()
    assert np.array_equal(ch["survived"], ((got["flags"] & LC.DONE) == 0).astype(np.int32)) and ch["value_h"][:, :, 0].tobytes() == got["value"].tobytes()
    seen = set()
    for H in (2, FC_H):
        st, rho, done = _check_against_the_emulator(eng, n_env, K, H, 2, cand, **kw)
        seen |= set(np.unique(st["survived"]).tolist())
    if n_env * K >= 15:
        assert len(seen) >= 2 and (st["flags"] & 3).any() and (cand == -1).any(), seen          # lanes that fail at different steps, flagged slots
    with pytest.raises(Exception, match="exceeds max_steps"):
        eng.lookahead_chain(2, FC_H + 1, cand)
    eng.close()


def _twin_steps(eng, twin, n_env, K, H, t, fc_h, idx, cand, step_kw, with_env=False):
    """the twin's lanes take the scratch lanes' state after step 1 and are stepped do-nothing, one launch per forecast row"""
    nc = n_env * K
    eng.lookahead_chain(t, 1, cand, **step_kw)
    topo, shb = eng.get_topology(n_env, nc)
    twin.set_topology(topo, shb if eng.model.n_shunt else None, lane0=0)
    twin.set_overflow_count(eng.step_outputs(n_env, nc)[1], lane0=0)
    twin.set_cooldown(eng.cooldown(n_env, nc), lane0=0)
    if with_env:
        twin.set_env_state(0, **eng.env_state(n_env, nc))
    twin.set_lane_chronics(lane_offset=np.repeat(fc_h * np.asarray(idx), K))
    seen = []
    for h in range(2, H + 1):
        twin.step(h - 1, nb_ts_reco=-1, **step_kw)                        # row fc_h idx + (h - 1)
        eng.lookahead_chain(t, h, cand, **step_kw)
        a, b = eng.results(n_env, nc), twin.results(0, nc)
        for f in ("out", "topo_vect", "shunt_bus", "line_status", "status"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (h, f)
        sa, sb = eng.step_outputs(n_env, nc), twin.step_outputs(0, nc)
        assert sa[0].tobytes() == sb[0].tobytes() and sa[1].tobytes() == sb[1].tobytes(), h
        assert eng.get_topology(n_env, nc)[0].tobytes() == twin.get_topology(0, nc)[0].tobytes(), h
        assert np.array_equal(eng.episode(n_env, nc)[0], twin.episode(0, nc)[0]), h
        if with_env:
            ea, eb = eng.env_state(n_env, nc), twin.env_state(0, nc)
            for key in ea:
                assert np.asarray(ea[key]).tobytes() == np.asarray(eb[key]).tobytes(), (h, key)
        seen.append((a.line_status.copy(), eng.episode(n_env, nc)[0].copy()))
    return seen


@pytest.mark.parametrize("grid,is_dc", [("rte_case5_example", False), ("rte_case5_example", True), ("l2rpn_case14_sandbox", False), ("l2rpn_case14_sandbox", True)])
def test_scratch_lanes_equal_a_twin_engine_stepped_one_launch_at_a_time(grid, is_dc):
    """A twin of n_env K lanes whose chronics table is the forecast table as [T n_h] rows: results rows, rho, topology rows, overflow
    counters and done flags of the chain's scratch lanes after step h are the twin's after its launch on row n_h idx + (h - 1)."""
    from grid2op_amd.engine import PowerFlowEngine
    n_env, K, t = 3, 5, 3
    n = n_env * (1 + K)
    offsets = 7 * np.arange(n)
    m, eng, fc = _engine(grid, n, offsets, limit_scale=0.7)
    twin = PowerFlowEngine(m, n_lanes=n_env * K, device=0)
    twin.upload_chronics(fc.reshape(-1, fc.shape[-1]))
    twin.set_thermal_limits(eng_limits(grid) * 0.7)
    table = _table(m)
    eng.set_topo_rules(legal_rules=False)
    eng.upload_topo_actions(table)
    eng.set_lookahead(K, n_env)
    eng.set_lookahead_chain(FC_H)
    eng.set_overflow_count(np.ones((n_env, m.n_line), np.int32), lane0=0)
    cand = np.tile(np.array([0, 3, -1, 6, 8], np.int32), (n_env, 1))
    idx = (t + offsets[:n_env]) % 48
    seen = _twin_steps(eng, twin, n_env, K, FC_H, t, FC_H, idx, cand, dict(cascade=True, is_dc=is_dc))
    assert any((~ls).any() for ls, _ in seen)                             # lines did go out on the way
    eng.close(); twin.close()


def eng_limits(grid):
    return dict(np.load(golden_path(f"{grid}.chronics.npz"))).get("thermal_limits", CASE5_LIMITS)


def test_large_rows_with_env_dynamics_equal_the_twin(load_model, load_npz):
    """118 substations, 186 lines (three trips of the strided maximum), the injection dynamics on: every step of the chain is one more
    do-nothing step of the dynamics, on the state the scratch lanes took over from their environments."""
    from grid2op_amd.engine import PowerFlowEngine
    name = "l2rpn_wcci_2022_dev"
    m, fx = load_model(name), load_npz(f"envdyn_{name}.npz")
    n_env, K, H = 2, 3, 3
    n = n_env * (1 + K)
    table = [{"set_line_status": [(5, -1)]}, {"set_line_status": [(100, -1)]}, {"change_line_status": [185]}, {"set_line_status": [(64, -1)]}]
    row = int(fx["row"][0])
    engs = []
    for lanes in (n, n_env * K):
        eng = PowerFlowEngine(m, n_lanes=lanes, device=0)
        tab = eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"])
        fc = _forecasts(tab, H)
        if lanes == n:
            eng.upload_chronics(tab)
            eng.upload_forecasts(fc[None])
        else:
            eng.upload_chronics(fc.reshape(-1, fc.shape[-1]))
        eng.set_thermal_limits(fx["thermal_limit"])
        eng.set_gen_limits(fx["pmin"], fx["pmax"], fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], eps_poly=float(fx["eps_poly"]))
        if m.n_storage:
            eng.set_storage_params(fx["storage_Emax"], fx["storage_Emin"], fx["storage_loss"], fx["storage_charging_efficiency"],
                                   fx["storage_discharging_efficiency"], fx["storage_charge0"], float(fx["delta_time_seconds"]), bool(fx["activate_storage_loss"]))
        eng.set_env_dynamics(True, tol_poly=float(fx["tol_poly"]))
        engs.append((eng, tab.shape[0]))
    (eng, T), (twin, _) = engs
    off = np.zeros(n, np.int32)
    off[:n_env] = (row, row + 2)
    eng.set_lane_chronics(lane_offset=off)
    eng.set_env_state(0, prev_p=np.tile(fx["ch_prod_p"][row - 1], (n, 1)))
    eng.set_topo_rules(legal_rules=False)
    eng.upload_topo_actions(table)
    eng.set_lookahead(K, n_env)
    eng.set_lookahead_chain(H)
    eng.step(0)
    eng.step(1)                                                            # two environment steps first: a dynamics state to take over
    idx = (2 + off[:n_env]) % T
    _twin_steps(eng, twin, n_env, K, H, 2, H, idx, np.tile(np.array([3, 0, -1], np.int32), (n_env, 1)), dict(), with_env=True)
    st = eng.lookahead_chain_values()
    assert (st["survived"] == H).all() and (eng.lookahead_values()["best"] >= 0).all()
    eng.close(); twin.close()


def test_play_writes_the_choice_and_play_0_leaves_the_acting_path_alone():
    """Ten acting steps with `lookahead_chain(play=2)` in front of each: the environment lanes are, bit for bit, those of an engine whose
    host writes table[cand[i][best[i]]] (else the fall-back's entry, else -1) with `set_lane_topo_actions`.  play = 0 touches nothing."""
    n_env, K, H = 5, 4, 3
    n = n_env * (1 + K)
    seen, picks = {}, []
    for mode in ("play", "host"):
        m, eng, _ = _engine("l2rpn_case14_sandbox", n, 5 * np.arange(n), limit_scale=0.75)
        table = _table(m)
        eng.set_topo_rules(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=3)
        eng.upload_topo_actions(table)
        eng.set_lookahead(K, n_env)
        eng.set_lookahead_chain(H)
        kw = dict(cascade=True)
        rows = []
        for t in range(10):
            cand = ((np.arange(n_env * K).reshape(n_env, K) * 3 + t) % (len(table) + 1) - 1).astype(np.int32)
            if mode == "play":
                if t == 0:                                                 # play = 0: the action buffer and the pending actions stay as they are
                    before = eng.device_views()["act_topo"].cpu().numpy().copy()
                    eng.lookahead_chain(t, H, cand, play=0, **kw)
                    eng.sync()
                    assert np.array_equal(eng.device_views()["act_topo"].cpu().numpy(), before)
                eng.lookahead_chain(t, H, cand, play=2, **kw)
                la, lc = eng.lookahead_values(), eng.lookahead_chain_values()
                slot = np.where(la["best"] >= 0, la["best"], lc["fallback"])
                pick = np.where(slot >= 0, cand[np.arange(n_env), np.maximum(slot, 0)], -1).astype(np.int32)
                assert np.array_equal(eng.device_views()["act_topo"].cpu().numpy()[:n_env, 0], pick), t
                picks.append(pick)
            else:
                act = np.full(n, -1, np.int32)
                act[:n_env] = picks[t]
                eng.set_lane_topo_actions(act)
            eng.step(t, cascade=True, nb_ts_reco=10)
            r = eng.results(0, n_env)
            ill, amb = eng.topo_action_flags(0, n_env)
            rows.append(tuple(x.tobytes() for x in (r.out, r.topo_vect, r.status, r.line_status, ill, amb, eng.cooldown(0, n_env), eng.sub_cooldown(0, n_env),
                                                   eng.last_bus(0, n_env), eng.get_topology(0, n_env)[0]) + eng.episode(0, n_env) + eng.step_outputs(0, n_env)))
        seen[mode] = rows
        eng.close()
    for t, (a, b) in enumerate(zip(seen["play"], seen["host"])):
        assert a == b, (t, [i for i, (x, y) in enumerate(zip(a, b)) if x != y])
    assert any((p >= 0).any() for p in picks) and len({row[1] for row in seen["host"]}) >= 3      # choices were played and changed the topology


def test_play_0_leaves_a_pending_action_to_the_next_step():
    """a pending host action survives a chain with play = 0 and is played by the next step as without the chain"""
    n_env, K = 3, 2
    n = n_env * (1 + K)
    rows = []
    for chain in (True, False):
        m, eng, _ = _engine("l2rpn_case14_sandbox", n)
        eng.set_topo_rules(max_sub_changed=1, max_line_status_changed=1)
        eng.upload_topo_actions(_table(m))
        eng.set_lookahead(K, n_env)
        eng.set_lookahead_chain(2)
        act = np.full(n, -1, np.int32)
        act[:n_env] = [0, 8, 3]
        eng.set_lane_topo_actions(act)
        if chain:
            eng.lookahead_chain(0, 2, np.array([[1, 2], [3, -1], [4, 5]], np.int32))
        eng.step(0)
        rows.append((eng.results(0, n_env).out.tobytes(), eng.get_topology(0, n_env)[0].tobytes()))
        assert (eng.get_topology(0, n_env)[0] != m.initial_topo_vect()).any()
        eng.close()
    assert rows[0] == rows[1]


def test_a_sharded_engine_over_one_device_agrees_with_the_plain_engine():
    from grid2op_amd.grid_model import GridModel
    from grid2op_amd.sharding import ShardedEngine
    n_env, K, H = 3, 4, 3
    n = n_env * (1 + K)
    m, eng, fc = _engine("l2rpn_case14_sandbox", n, limit_scale=0.8)
    se = ShardedEngine(GridModel.load_npz(golden_path("l2rpn_case14_sandbox.grid.npz")), n, devices=[0])
    ch = dict(np.load(golden_path("l2rpn_case14_sandbox.chronics.npz")))
    tab = eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"])[:48]
    se.upload_chronics(tab)
    se.upload_forecasts(fc[None])
    se.set_lane_chronics(lane_offset=7 * np.arange(n))
    se.set_thermal_limits(ch["thermal_limits"] * 0.8)
    table = _table(m)
    cand = ((np.arange(n_env * K).reshape(n_env, K) * 2) % (len(table) + 1) - 1).astype(np.int32)
    for e in (eng, se):
        e.set_topo_rules(max_sub_changed=1, max_line_status_changed=1)
        e.upload_topo_actions(table)
        e.set_lookahead(K, n_env)
        e.set_lookahead_chain(H)
        e.lookahead_chain(1, H, cand, cascade=True)
    for a, b in ((eng.lookahead_values(), se.lookahead_values()), (eng.lookahead_chain_values(), se.lookahead_chain_values())):
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), key
    assert len(se.lookahead_chain_views()) == 1 and np.array_equal(se.lookahead_chain_views()[0]["survived"].cpu().numpy(), eng.lookahead_chain_values()["survived"])
    eng.close(); se.close()


def _fx_table(fx):
    return [{k: ({int(p): int(b) for p, b in v.items()} if isinstance(v, dict) else v) for k, v in a.items()} for a in json.loads(str(fx["table_json"]))]


@pytest.mark.parametrize("fixture", ["lookahead_chain_5bus.npz", "lookahead_chain_5bus_maintenance.npz"])
def test_recorded_forecast_environments_on_staggered_lanes(fixture, load_model, load_npz):
    """State s of the recording is environment lane s (its own chronics row, topology, counters and cooldowns), its K candidates are held
    over the H recorded forecast steps.  Second file: a maintenance begins inside the horizon."""
    from grid2op_amd.engine import PowerFlowEngine
    m, fx = load_model("rte_case5_example"), load_npz(fixture)
    S, K, H, L = fx["sim_rho"].shape
    row0 = int(fx["row0"])
    eng = PowerFlowEngine(m, n_lanes=S * (1 + K), device=0)
    eng.upload_chronics(eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"]))
    T = fx["ch_load_p"].shape[0]
    fc = np.stack([eng.pack_chronics(fx["fc_load_p"][:, h], fx["fc_load_q"][:, h], fx["fc_prod_p"][:, h], fx["fc_prod_v"][:, h]) for h in range(fx["fc_load_p"].shape[1])], axis=1)
    assert fc.shape[:2] == (T, H)
    eng.upload_forecasts(fc[None])
    if "maintenance" in fx:
        eng.upload_maintenance(fx["maintenance"])
    eng.set_thermal_limits(fx["thermal_limit"])
    off = np.zeros(S * (1 + K), np.int32)
    off[:S] = fx["row"] - row0
    eng.set_lane_chronics(lane_offset=off)
    max_sub, max_line, cd_sub, cd_line = (int(v) for v in fx["params"])
    eng.set_topo_rules(max_sub_changed=max_sub, max_line_status_changed=max_line, cooldown_sub=cd_sub, cooldown_line=cd_line)
    eng.upload_topo_actions(_fx_table(fx))
    eng.set_topology(fx["topo_vect"].astype(np.int32), lane0=0)
    eng.set_last_bus(np.maximum(fx["last_bus"].astype(np.int32), 1), lane0=0)
    eng.set_overflow_count(fx["timestep_overflow"].astype(np.int32), lane0=0)
    eng.set_cooldown(fx["cooldown_line"].astype(np.int32), lane0=0)
    eng.set_sub_cooldown(fx["cooldown_sub"].astype(np.int32), lane0=0)
    eng.set_lookahead(K, S)
    eng.set_lookahead_chain(H)
    kw = dict(cascade=True, hard_overflow=float(fx["hard_overflow"]), nb_ts_allowed=int(fx["nb_ts_allowed"]))
    worst = 0.0
    for h in range(1, H + 1):                                              # the chain of h steps leaves the scratch lanes as step h does
        eng.lookahead_chain(0, h, fx["cand"], **kw)
        r = eng.results(S, S * K, with_bus=False)
        rho, ovc = (x.reshape(S, K, L) for x in eng.step_outputs(S, S * K)[:2])
        ch, la = eng.lookahead_chain_values(), eng.lookahead_values()
        assert np.array_equal(ch["survived"], np.minimum(fx["sim_steps"], h)), h
        assert np.array_equal(la["flags"], LC.chain_flags(fx["sim_flags"], fx["sim_steps"] < h)), h
        for s in range(S):
            for k in range(K):
                if fx["sim_steps"][s, k] < h:                              # failed before or at this step: solved and ignored
                    assert np.isinf(ch["value_h"][s, k, h - 1])
                    continue
                q = s * K + k
                assert np.array_equal(r.topo_vect[q], fx["sim_topo_vect"][s, k, h - 1]), (h, s, k)
                assert np.array_equal(r.line_status[q], fx["sim_line_status"][s, k, h - 1]), (h, s, k)
                assert np.array_equal(ovc[s, k], fx["sim_timestep_overflow"][s, k, h - 1]), (h, s, k)       # the protection counters ran on
                err = float(np.abs(rho[s, k] - fx["sim_rho"][s, k, h - 1]).max())
                worst = max(worst, err)
                assert err < LC.RHO_TOL, (h, s, k, err)
                assert ch["value_h"][s, k, h - 1].tobytes() == rho[s, k].max().tobytes()
    print(f"{fixture}: max |rho - recorded| over every step = {worst:.2e}")
    pinned = 0
    for s in range(S):
        if int(fx["best"][s]) != -2:
            assert la["best"][s] == fx["best"][s], s
        if int(fx["fallback"][s]) != -2:
            assert ch["fallback"][s] == fx["fallback"][s], s
        pinned += int(fx["best"][s]) != -2 and int(fx["fallback"][s]) != -2
    assert pinned >= 0.75 * S
    # the environments were only read
    assert np.array_equal(eng.get_topology(0, S)[0], fx["topo_vect"])
    assert np.array_equal(eng.cooldown(0, S), fx["cooldown_line"]) and np.array_equal(eng.sub_cooldown(0, S), fx["cooldown_sub"])
    eng.close()
