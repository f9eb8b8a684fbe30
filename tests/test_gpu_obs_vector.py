"""Observation vectors assembled on the device (include/gridpf.h: gpf_set_obs_spec / gpf_obs_vector; grid2op_amd/csrc/gridpf_obs.hpp)
against the numpy restatement tests/obs_ref.py fed from the engine's existing getters -- bit for bit: the kernel is a cast and an affine
map in float32 --, against the vectors the reference recorded on rte_case5_example, and the refusals."""
import datetime as dt

import numpy as np
import pytest

import obs_ref
from conftest import golden_path
from test_obs_spec import CASE5_LIMITS, CASE5_RENEWABLE
from topo_rules_ref import random_topo_table

pytestmark = pytest.mark.gpu

START = [dt.datetime(2019, 1, 6, 0, 0), dt.datetime(2012, 2, 28, 23, 40)]     # (the second one crosses a leap day within a few rows)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _engine(name, n, offsets, wcci_dynamics=False):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path(f"{name}.grid.npz"))
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    extra = {}
    if wcci_dynamics:
        fx = np.load(golden_path(f"envdyn_{name}.npz"))
        eng.upload_chronics(eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"]))
        eng.set_thermal_limits(fx["thermal_limit"])
        eng.set_gen_limits(fx["pmin"], fx["pmax"], fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], eps_poly=float(fx["eps_poly"]))
        if m.n_storage:
            eng.set_storage_params(fx["storage_Emax"], fx["storage_Emin"], fx["storage_loss"], fx["storage_charging_efficiency"],
                                   fx["storage_discharging_efficiency"], fx["storage_charge0"], float(fx["delta_time_seconds"]),
                                   bool(fx["activate_storage_loss"]))
        eng.set_env_dynamics(True, tol_poly=float(fx["tol_poly"]))
        if "renewable" in fx.files:
            eng.set_gen_renewable(fx["renewable"])
            extra["renewable"] = fx["renewable"]
        extra["gen_limits"] = (fx["pmin"], fx["pmax"], fx["ramp_up"], fx["ramp_down"])
        extra["thermal"] = np.asarray(fx["thermal_limit"], np.float32)
    else:
        ch = dict(np.load(golden_path(f"{name}.chronics.npz")))
        if "prod_v" not in ch:
            ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
        eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
        eng.set_thermal_limits(ch["thermal_limits"])
        extra["thermal"] = np.asarray(ch["thermal_limits"], np.float32)
    eng.set_lane_chronics(lane_offset=offsets)
    return m, eng, extra


def _custom_spec(m, rng):
    """A shuffled subset with per-element subtract / divide (one attribute left at the defaults: its segment must stay a plain cast)."""
    from grid2op_amd.obs_spec import ObsSpec
    attrs = ["rho", "topo_vect", "gen_p", "line_status", "p_or", "a_ex", "load_q", "time_before_cooldown_line", "time_before_cooldown_sub",
             "timestep_overflow", "minute_of_hour", "day", "gen_margin_up", "actual_dispatch", "thermal_limit", "current_step", ("const", 5, -3.25),
             "time_next_maintenance", "v_or"]
    attrs = [attrs[i] for i in rng.permutation(len(attrs))]
    size = lambda a: ObsSpec(m, [a]).dim  # noqa: E731
    sub = {a: rng.normal(size=size(a)).astype(np.float32) for a in attrs if isinstance(a, str) and a not in ("v_or", "day")}
    div = {a: (1.0 + rng.random(size(a))).astype(np.float32) for a in attrs if isinstance(a, str) and a not in ("v_or", "rho")}
    sub["day"], div["const0"] = 1.0, 4.0
    return ObsSpec(m, attrs, subtract=sub, divide=div)


@pytest.mark.parametrize("name,n,steps", [("l2rpn_case14_sandbox", 4096, 32), ("l2rpn_wcci_2022_dev", 1024, 32)])
def test_vector_equals_numpy_restatement_bitwise(name, n, steps):
    from grid2op_amd.obs_spec import ObsSpec
    rng = np.random.default_rng(11)
    wcci = name == "l2rpn_wcci_2022_dev"
    offsets = (3 * np.arange(n)).astype(np.int32)
    m, eng, extra = _engine(name, n, offsets, wcci_dynamics=wcci)
    acts = random_topo_table(m, rng)
    eng.upload_topo_actions(acts)
    eng.set_topo_rules(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=3)
    clock = ([START[0]], 5, 2016)
    eng.set_obs_clock(START[0], step_minutes=5, max_step=2016)
    full, custom = ObsSpec.complete(m, fill=True), _custom_spec(m, rng)
    kw = dict(clock=clock, gen_limits=extra.get("gen_limits"), renewable=extra.get("renewable"), lane_offset=offsets, acting=True)
    for t in range(1, steps + 1):
        eng.set_lane_topo_actions(rng.integers(-1, len(acts), size=n).astype(np.int32))
        eng.step(t, cascade=True, nb_ts_reco=10)
        # every launch is compared: the whole batch at every 4th step and the last, a window of n / 8 lanes that moves through the batch at
        # the others (the host restatement is the slow side)
        whole = t % 4 == 0 or t == steps
        l0, nl = (0, n) if whole else (((t * 5) % 8) * (n // 8), n // 8)
        for spec in (full, custom):
            eng.set_obs_spec(spec)
            got = eng.observation_vector_host(l0, nl)
            st = obs_ref.engine_state(eng, spec, t=t, lane0=l0, n=nl, **kw)
            st["thermal_limit"] = np.tile(extra["thermal"], (nl, 1))
            want = obs_ref.compose(spec, st)
            bad = np.nonzero(_bits(got) != _bits(want))
            assert bad[0].size == 0, (t, spec is full, l0 + bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5])
        if not whole:
            continue
        # a spec with game_over_fill off hands the failed lanes' rows through as they are
        eng.set_obs_spec(full, game_over_fill=False)
        st = obs_ref.engine_state(eng, full, t=t, **kw)
        assert np.array_equal(eng.observation_vector_host(), obs_ref.compose(full, st, game_over_fill=False), equal_nan=True)
    assert eng.cooldown().any() and eng.sub_cooldown().any()
    # device tensor, caller-owned strided output, lane sub-range
    import torch
    eng.set_obs_spec(custom)
    want = eng.observation_vector_host()
    views = eng.device_views()
    o = eng.observation_vector()
    views["stream"].synchronize()
    assert o.shape == (n, custom.dim) and o.data_ptr() == views["obs"].data_ptr()
    assert np.array_equal(_bits(o.cpu().numpy()), _bits(want))
    pad = torch.full((100, custom.dim + 7), 123.5, dtype=torch.float32, device=o.device)
    torch.cuda.synchronize()
    r = eng.observation_vector(17, 100, out=pad)
    views["stream"].synchronize()
    assert np.array_equal(_bits(r.cpu().numpy()), _bits(want[17:117]))
    assert (pad[:, custom.dim:] == 123.5).all().item()
    with pytest.raises(ValueError):
        eng.observation_vector(0, 100, out=pad[:, :custom.dim - 1])
    with pytest.raises(ValueError):
        eng.observation_vector(0, 99, out=pad)
    eng.close()


def test_maintenance_lookahead_and_trajectory_on_the_36_substation_grid():
    from grid2op_amd.engine import GridPFError, PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from grid2op_amd.obs_spec import ObsSpec
    name = "l2rpn_neurips_2020_track1"
    m = GridModel.load_npz(golden_path(f"{name}.grid.npz"))
    fx = np.load(golden_path(f"rollout_{name}.npz"))
    n = 256
    T = fx["chron_load_p"].shape[1]
    rng = np.random.default_rng(5)
    table = (np.arange(n) % 2).astype(np.int32)
    offsets = rng.integers(0, T, size=n).astype(np.int32)

    def make():
        eng = PowerFlowEngine(m, n_lanes=n, device=0)
        eng.upload_chronics(eng.pack_chronics(fx["chron_load_p"], fx["chron_load_q"], fx["chron_prod_p"], fx["chron_prod_v"]))
        eng.upload_maintenance(fx["chron_maintenance"])
        eng.set_thermal_limits(fx["thermal_limit"])
        eng.set_lane_chronics(lane_table=table, lane_offset=offsets)
        eng.set_obs_clock(START, step_minutes=5, max_step=T - 1)
        return eng
    assert fx["chron_maintenance"].any()
    spec = ObsSpec(m, ["time_next_maintenance", "duration_next_maintenance", "year", "month", "day", "hour_of_day", "minute_of_hour",
                       "day_of_week", "rho", "line_status", "topo_vect", "time_before_cooldown_line", "gen_p", "a_or", "max_step", "delta_time"],
                   divide={"rho": 0.5, "time_before_cooldown_line": 3.0}, subtract={"year": 2000})
    a, b = make(), make()
    a.set_obs_spec(spec); b.set_obs_spec(spec)
    K = 16
    a.set_trajectory(K, a.TRAJ_OBS)
    a.step(1, n_steps=K, cascade=True, nb_ts_reco=int(fx["nb_ts_reco"]))
    traj = a.observation_trajectory(K)
    a.sync()
    traj = traj.cpu().numpy()
    look = [obs_ref.maintenance_lookahead(tb) for tb in fx["chron_maintenance"]]
    seen_outage = 0
    for k in range(K):
        b.step(1 + k, cascade=True, nb_ts_reco=int(fx["nb_ts_reco"]))
        one = b.observation_vector_host()
        assert np.array_equal(_bits(traj[k]), _bits(one)), k                       # multi-step = single steps, bit for bit
        rows = (1 + k + offsets) % T
        done = b.episode()[0]
        nxt = np.stack([look[tb][0][r] for tb, r in zip(table, rows)]).astype(np.float32)
        dur = np.stack([look[tb][1][r] for tb, r in zip(table, rows)]).astype(np.float32)
        nxt[done], dur[done] = -1.0, 0.0
        assert np.array_equal(one[:, spec.offsets["time_next_maintenance"]], nxt), k
        assert np.array_equal(one[:, spec.offsets["duration_next_maintenance"]], dur), k
        seen_outage += int(((nxt == 0) & ~done[:, None]).sum())
        cal = np.stack([obs_ref.calendar(START[tb], 5, [r])[0] for tb, r in zip(table, rows)]).astype(np.float32)
        cal[:, 0] -= 2000
        assert np.array_equal(one[:, spec.offsets["year"].start:spec.offsets["day_of_week"].stop], cal), k
    assert seen_outage > 0
    # the last step of the launch is also what the lanes' own rows give
    assert np.array_equal(_bits(a.observation_vector_host()), _bits(traj[K - 1]))
    # attributes without a per-step copy are refused by name in trajectory mode; so is a launch without TRAJ_OBS
    a.set_obs_spec(ObsSpec(m, ["rho", "timestep_overflow"]))
    with pytest.raises(GridPFError, match="timestep_overflow"):
        a.observation_trajectory(K)
    a.set_obs_spec(ObsSpec(m, ["rho", "current_step"]))
    with pytest.raises(GridPFError, match="current_step"):
        a.observation_trajectory(K)
    b.set_trajectory(K, b.TRAJ_RHO)
    b.step(40, n_steps=2)
    with pytest.raises(GridPFError, match="TRAJ_OBS"):
        b.observation_trajectory(2)
    a.close(); b.close()


def test_trajectory_line_cooldowns_without_a_per_step_copy():
    """The int16 per-step copy of the line cooldowns is written by converged steps of launches that maintain them: a launch that does not
    leaves the lanes' own counters standing, and they are what every step of it reads; a failed step has no copy, so with game_over_fill
    off the attribute is refused in trajectory mode."""
    from grid2op_amd.engine import GridPFError
    from grid2op_amd.obs_spec import ObsSpec
    n = 64
    m, eng, _ = _engine("l2rpn_case14_sandbox", n, np.arange(n, dtype=np.int32))
    spec = ObsSpec(m, ["time_before_cooldown_line", "rho"])
    eng.set_obs_spec(spec)
    eng.set_trajectory(4, eng.TRAJ_OBS)
    cd = np.zeros((n, m.n_line), np.int32); cd[:, 3] = 7; cd[5, 0] = 2
    eng.step(1, n_steps=4, cascade=True, nb_ts_reco=10)             # a tracking launch fills the per-step copy
    eng.set_cooldown(cd)
    eng.step(5, n_steps=4, nb_ts_reco=-1)                           # not tracked: the counters stand
    traj = eng.observation_trajectory(4)
    eng.sync()
    traj = traj.cpu().numpy()
    assert np.array_equal(eng.cooldown(), cd)
    live = ~eng.episode()[0]                                        # (a finished lane writes the game-over zeros)
    assert live.sum() > n // 2
    for k in range(4):
        assert np.array_equal(traj[k][live][:, spec.offsets["time_before_cooldown_line"]], cd[live].astype(np.float32)), k
    eng.step(9, n_steps=4, cascade=True, nb_ts_reco=10)
    eng.set_obs_spec(spec, game_over_fill=False)
    with pytest.raises(GridPFError, match="time_before_cooldown_line"):
        eng.observation_trajectory(4)
    eng.close()


def test_refusals_without_spec_or_clock_and_bad_segments():
    import ctypes as C
    from grid2op_amd._capi import ptr
    from grid2op_amd.engine import GridPFError
    from grid2op_amd.obs_spec import ObsSpec
    m, eng, _ = _engine("l2rpn_case14_sandbox", 8, np.zeros(8, np.int32))
    with pytest.raises(GridPFError, match="no observation spec"):
        eng.observation_vector_host()
    assert eng.device_views()["obs"] is None
    eng.set_obs_spec(ObsSpec(m, ["rho", "hour_of_day"]))
    with pytest.raises(GridPFError, match="no clock"):
        eng.observation_vector_host()
    eng.set_obs_spec(ObsSpec(m, ["rho"]))
    eng.step(1)
    assert np.array_equal(eng.observation_vector_host(), eng.step_outputs()[0])
    good = ObsSpec(m, ["rho", "gen_p"])

    def raw(seg, dim, sub=None, div=None):
        seg = np.ascontiguousarray(seg, np.int32)
        return eng._lib.gpf_set_obs_spec(eng._h, seg.shape[0], ptr(seg, C.c_int32), dim, ptr(sub, C.c_float), ptr(div, C.c_float), 1)
    s = good.segments.copy(); s[1, 3] -= 1
    assert raw(s, good.dim) < 0 and b"overlap" in eng._lib.gpf_last_error()
    s = good.segments.copy(); s[1, 3] += 1
    assert raw(s, good.dim + 1) < 0 and b"gap" in eng._lib.gpf_last_error()
    s = good.segments.copy(); s[0, 2] = m.n_line + 1; s[1, 3] += 1
    assert raw(s, good.dim + 1) < 0 and b"source range" in eng._lib.gpf_last_error()
    s = good.segments.copy(); s[0, 0] = 99
    assert raw(s, good.dim) < 0 and b"unknown source kind" in eng._lib.gpf_last_error()
    dv = np.ones(good.dim, np.float32); dv[3] = 0
    assert raw(good.segments, good.dim, None, dv) < 0 and b"zero" in eng._lib.gpf_last_error()
    assert np.array_equal(eng.observation_vector_host(), eng.step_outputs()[0])      # a refused spec leaves the one in place untouched
    eng.close()


def test_sharded_halves_equal_one_engine():
    from grid2op_amd.obs_spec import ObsSpec
    from grid2op_amd.sharding import ShardedEngine
    n = 128
    offsets = (7 * np.arange(n)).astype(np.int32)
    m, one, _ = _engine("l2rpn_case14_sandbox", n, offsets)
    ch = dict(np.load(golden_path("l2rpn_case14_sandbox.chronics.npz")))
    sh = ShardedEngine(m, n, devices=[0, 0])
    sh.upload_chronics(sh.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    sh.set_thermal_limits(ch["thermal_limits"])
    sh.set_lane_chronics(lane_offset=offsets)
    spec = ObsSpec.complete(m, fill=True)
    for e in (one, sh):
        e.set_obs_clock(START[0], 5, 100)
        e.set_obs_spec(spec)
        e.step(3, n_steps=2, cascade=True)
    want = one.observation_vector_host()
    assert np.array_equal(_bits(sh.observation_vector_host()), _bits(want))
    parts = sh.observation_vector()
    sh.sync()
    assert len(parts) == 2 and np.array_equal(_bits(np.concatenate([p.cpu().numpy() for p in parts])), _bits(want))
    assert np.array_equal(_bits(sh.observation_vector_host(60, 10)), _bits(want[60:70]))
    one.close(); sh.close()


def test_recorded_reference_vectors_of_case5():
    """The complete 192-wide vector against the rows the reference's Runner recorded (tests/golden/obsvec_runner_case5.npz): per episode one
    lane, whose chronics table holds the injections of the recorded rows and whose topology is the row's, one launch per row (t = 1 .. for
    the played steps; `played` is the reference's nb_timestep_played, which counts the step that ended the episode, so rows
    0 .. played - 1 are live and row `played` is the game-over observation: a lane that took k steps has current_step k, as the reference after k env.step), the protection counters and cooldowns
    the row states restored through the setters, the clock at the episode's start.  Copied / derived integer, bool, calendar and const
    columns must be exactly equal, power-flow columns within the float32 parity bar 2e-4 + 5e-6 |x|; a game-over row
    (a lane whose launch failed: `done`) must equal the recorded row exactly.  The reset observation (row 0) is produced by a launch at
    t = 0 on a second engine -- the engine counts that launch as a step, so its current_step column reads 1 where the reference has 0;
    every other column of that row is held to the same bars."""
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from grid2op_amd.obs_spec import ObsSpec
    m = GridModel.load_npz(golden_path("rte_case5_example.grid.npz"))
    fx = np.load(golden_path("obsvec_runner_case5.npz"))
    vec, ep, played = fx["vectors"], fx["episode"], fx["played"]
    spec = ObsSpec.complete(m, fill=True)
    off = spec.offsets
    n_ep = len(played)
    rows_of = [vec[ep == e] for e in range(n_ep)]
    T = max(len(r) for r in rows_of) + 1
    tab = np.zeros((n_ep, T, 2 * m.n_load + 2 * m.n_gen), np.float32)
    for e, rows in enumerate(rows_of):
        for k in range(T):
            r = rows[min(k, int(played[e]) - 1)]                 # (from the failing step on the last live row repeats: that launch needs inputs too)
            tab[e, k] = np.concatenate([r[off["load_p"]], r[off["load_q"]], r[off["gen_p"]] - r[off["gen_p_delta"]], r[off["gen_v"]]])
    starts = [dt.datetime(*[int(x) for x in s]) for s in fx["start"]]
    flow = np.zeros(192, bool)
    for name in ("gen_p", "gen_q", "gen_v", "load_p", "load_q", "load_v", "p_or", "q_or", "v_or", "a_or", "p_ex", "q_ex", "v_ex", "a_ex", "rho",
                 "gen_margin_up", "gen_margin_down", "gen_p_delta", "gen_p_before_curtail"):
        flow[off[name]] = True

    def make():
        eng = PowerFlowEngine(m, n_lanes=n_ep, device=0)
        eng.upload_chronics(tab)
        eng.set_lane_chronics(lane_table=np.arange(n_ep, dtype=np.int32))
        eng.set_thermal_limits(m.thermal_limit_a)
        eng.set_gen_limits(*CASE5_LIMITS, [False, True])
        eng.set_gen_renewable(CASE5_RENEWABLE)
        eng.set_obs_clock(starts, step_minutes=5, max_step=100)
        eng.set_obs_spec(spec)
        return eng

    def check(got, want, what, skip=()):
        keep = np.ones(192, bool)
        for name in skip:
            keep[off[name]] = False
        ex = keep & ~flow
        assert np.array_equal(got[ex], want[ex]), (what, np.nonzero(got[ex] != want[ex])[0], got[ex][got[ex] != want[ex]], want[ex][got[ex] != want[ex]])
        err = np.abs(got[flow].astype(np.float64) - want[flow])
        print(what, "worst power-flow column deviation", float(err.max()))
        assert np.all(err <= 2e-4 + 5e-6 * np.abs(want[flow])), (what, float(err.max()))

    def restore(eng, e, row):
        eng.set_overflow_count(row[off["timestep_overflow"]].astype(np.int32)[None, :], lane0=e)
        eng.set_cooldown(row[off["time_before_cooldown_line"]].astype(np.int32)[None, :], lane0=e)

    n_checked = n_over = 0
    first = make()
    for e in range(n_ep):
        first.set_topology(rows_of[e][0][off["topo_vect"]].astype(np.int32)[None, :], lane0=e)
    first.step(0)
    for e in range(n_ep):
        restore(first, e, rows_of[e][0])
    got = first.observation_vector_host()
    for e in range(n_ep):
        check(got[e], rows_of[e][0], (str(fx["names"][e]), 0), skip=("current_step",))
        assert got[e][off["current_step"]] == 1.0
        n_checked += 1
    first.close()
    eng = make()
    for t in range(1, T):
        live = [e for e in range(n_ep) if t < len(rows_of[e])]
        if not live:
            break
        for e in live:
            over = t >= int(played[e])
            topo = np.full(m.dim_topo, -1, np.int32) if over else rows_of[e][t][off["topo_vect"]].astype(np.int32)
            eng.set_topology(topo[None, :], lane0=e)             # (a game over: every element disconnected, the launch fails)
        eng.step(t)
        done = eng.episode()[0]
        for e in live:
            if t < int(played[e]):
                restore(eng, e, rows_of[e][t])
        got = eng.observation_vector_host()
        for e in live:
            want = rows_of[e][t]
            if t >= int(played[e]):
                assert done[e]
                assert np.array_equal(got[e], want), (str(fx["names"][e]), t, "game over", np.nonzero(got[e] != want)[0])
                n_over += 1
            else:
                assert not done[e], (str(fx["names"][e]), t)
                check(got[e], want, (str(fx["names"][e]), t))
            n_checked += 1
    eng.close()
    assert n_checked == len(vec) and n_over >= 2
