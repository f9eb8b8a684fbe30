"""The look-ahead screen (include/gridpf.h gpf_set_lookahead / gpf_lookahead), the parts that need no GPU: the recordings of the unmodified
reference's obs.simulate on per-step candidate lists (tests/golden/lookahead_*.npz) against the numpy restatement (tests/lookahead_ref.py)
and the library's rule core compiled with g++ (tests/native/lookahead_emul.cpp), every refusal through a header-only handle, the exported
symbols, the constants and the routing of `ShardedEngine`."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import lookahead_ref as LA
from conftest import golden_path
from topo_rules_ref import TopoRules

FIXTURES = {"case14": ("lookahead_case14.npz", "l2rpn_case14_sandbox"), "neurips36": ("lookahead_maintenance_neurips36.npz", "l2rpn_neurips_2020_track1")}


@pytest.fixture(scope="module")
def recorded():
    return {tag: dict(np.load(golden_path(f))) for tag, (f, _) in FIXTURES.items()}


def _restated_flags(fx, model, s, ts):
    rules = TopoRules(model, fx["off"], fx["items"], True, *[int(v) for v in fx["params"]])
    out = None
    if "maintenance" in fx:
        idx = int(fx["row"][s]) - int(fx["row0"])
        out = LA.maintenance_ahead(fx["maintenance"], idx, ts)
        assert np.array_equal(out, LA.emul_maintenance(fx["maintenance"], idx, ts))
    return LA.verdicts(rules, fx["topo_vect"][s], fx["cooldown_line"][s], fx["cooldown_sub"][s], fx["last_bus"][s], fx["cand"][s], out)


@pytest.mark.parametrize("tag", list(FIXTURES))
def test_restatement_and_emulator_against_the_recording(recorded, load_model, tag):
    """Flags: the restated verdict of every (state, horizon, slot) equals sim_info's is_illegal / is_ambiguous exactly, with the
    maintenance ahead taken out before the action.  Rows: where the simulated step tripped no further line, the restated row is the
    recorded topo_vect.  Values and ranking: restatement and emulator agree bit for bit on the recorded rho rows."""
    fx, model = recorded[tag], load_model(FIXTURES[tag][1])
    S, K = fx["cand"].shape
    assert K == 6 and S >= 8 and len({tuple(c) for c in fx["cand"]}) == S            # a different list after every step
    n_rows = n_flagged = 0
    for s in range(S):
        for ts in (0, 1):
            rec_flags = fx[f"sim{ts}_flags"][s]
            flags, rows = _restated_flags(fx, model, s, ts)
            assert np.array_equal(flags, rec_flags & 3), (tag, s, ts, flags, rec_flags)
            n_flagged += int((flags != 0).sum())
            done = (rec_flags & LA.DONE) != 0
            assert np.array_equal(done, fx[f"sim{ts}_done"][s])
            for k in np.flatnonzero(~done):
                tv = fx[f"sim{ts}_topo_vect"][s][k]
                on = (rows[k][model.line_or_pos_topo_vect] > 0) & (rows[k][model.line_ex_pos_topo_vect] > 0)
                if np.array_equal(on, fx[f"sim{ts}_line_status"][s][k]):        # (no line tripped in the simulated step)
                    assert np.array_equal(rows[k], tv), (tag, s, ts, k)
                    n_rows += 1
            vals = np.array([LA.value(r, d) for r, d in zip(fx[f"sim{ts}_rho"][s], done)], np.float32)
            for k in range(K):
                assert LA.emul_value(fx[f"sim{ts}_rho"][s][k], done[k]).tobytes() == vals[k].tobytes()
                assert np.isinf(vals[k]) == bool(done[k])
                if not done[k]:
                    assert abs(float(vals[k]) - float(fx[f"sim{ts}_rho"][s][k].max())) <= LA.RHO_TOL
            got, want = LA.emul_summary(vals, rec_flags), LA.summary(vals, rec_flags)
            assert (got[0], got[1].tobytes(), got[2], got[3]) == (want[0], want[1].tobytes(), want[2], want[3]), (tag, s, ts)
    assert n_rows >= S * K and n_flagged >= 6


def test_what_the_recordings_hold(recorded):
    fx = recorded["case14"]
    fl = np.concatenate([fx["sim0_flags"].ravel(), fx["sim1_flags"].ravel()])
    assert (fl & LA.ILLEGAL).any() and (fl & LA.AMBIGUOUS).any() and (fl & LA.DONE).any() and (fx["cand"] == -1).any()
    assert (fx["topo_vect"] == 2).any() and (fx["last_bus"] == 2).any() and (fx["cooldown_line"] > 0).any() and (fx["cooldown_sub"] > 0).any()
    close = sum(LA.margin(np.where(fx[f"sim{ts}_flags"][s] & LA.DONE, np.inf, fx[f"sim{ts}_rho"][s].max(1)), fx[f"sim{ts}_flags"][s]) <= LA.MARGIN
                for s in range(len(fx["row"])) for ts in (0, 1))
    assert close <= 0.1 * 2 * len(fx["row"])
    fm = recorded["neurips36"]
    m = int(fm["maintained"])
    starts = np.flatnonzero(fm["time_next_maintenance"][:, m] == 1)
    assert len(starts) == 1 and fm["line_status"][starts[0]][m]
    s = int(starts[0])
    k = list(fm["cand"][s]).index(-1)
    assert fm["sim0_line_status"][s][k][m] and not fm["sim1_line_status"][s][k][m]      # out in the forecast one step ahead only


@pytest.mark.parametrize("K,n_line", [(1, 20), (6, 59), (64, 64), (70, 187), (129, 65)])
def test_emulator_equals_the_restatement_on_seeded_tables(K, n_line):
    rng = np.random.default_rng(1000 * K + n_line)
    for rep in range(8):
        rho = rng.uniform(0, 1.9, (K, n_line)).astype(np.float32)
        flags = np.where(rng.random(K) < 0.3, rng.integers(1, 8, K), 0).astype(np.uint8)
        if rep == 1:
            flags[:] = rng.integers(1, 8, K)                              # no playable slot
        if rep == 2:
            flags[:] = 0
        if rep >= 3 and K > 2:
            rho[K // 2] = rho[K // 3]                                     # a tie: the lower slot
            flags[K // 2] = flags[K // 3] = 0
        done = (flags & LA.DONE) != 0
        vals = np.array([LA.value(r, d) for r, d in zip(rho, done)], np.float32)
        assert np.isinf(vals[done]).all() and np.isfinite(vals[~done]).all()
        for k in range(K):
            assert LA.emul_value(rho[k], done[k]).tobytes() == vals[k].tobytes()
        if rep == 4:
            vals[0] = np.inf                                              # +inf on a playable slot never wins against a finite one
        got, want = LA.emul_summary(vals, flags), LA.summary(vals, flags)
        assert (got[0], got[1].tobytes(), got[2], got[3]) == (want[0], want[1].tobytes(), want[2], want[3]), (K, rep)
        if rep == 1:
            assert got[0] == -1 and np.isinf(got[1]) and got[2] == 0
        if rep >= 3 and K > 2 and got[0] == K // 2:
            raise AssertionError("a tie went to the higher slot")
    L = LA.emulator()
    assert L.la_emul_outranks(0.5, 3, 0.5, 4) == 1 and L.la_emul_outranks(0.5, 4, 0.5, 3) == 0 and L.la_emul_outranks(0.4, 9, 0.5, 0) == 1
    assert L.la_emul_outranks(0.4, -1, 0.5, 0) == 0 and L.la_emul_outranks(float("inf"), 2, 0.1, -1) == 1 and L.la_emul_outranks(0.1, -1, 0.1, -1) == 0


def test_maintenance_ahead_emulator_equals_the_restatement():
    rng = np.random.default_rng(5)
    for rep in range(20):
        T, L = int(rng.integers(3, 12)), int(rng.integers(1, 7))
        M = (rng.random((T, L)) < 0.35).astype(np.uint8)
        for idx in range(T):
            for ts in range(4):
                assert np.array_equal(LA.emul_maintenance(M, idx, ts), LA.maintenance_ahead(M, idx, ts)), (rep, idx, ts)
    M = np.array([[0], [0], [1], [1], [0], [1]], np.uint8)
    assert [bool(LA.emul_maintenance(M, i, 1)[0]) for i in range(6)] == [False, True, True, False, True, False]   # begins there / under way / over / past the table
    assert not LA.emul_maintenance(M, 1, 0)[0] and LA.emul_maintenance(M, 1, 2)[0] and not LA.emul_maintenance(M, 1, 3)[0]


def test_every_refusal_on_a_header_only_handle(load_model):
    from grid2op_amd import _capi
    from grid2op_amd.engine import GridPFError, PowerFlowEngine
    m = load_model("l2rpn_case14_sandbox")
    eng = PowerFlowEngine(m, n_lanes=14, device=-1)
    L = eng._lib
    opts = _capi.GpfStepOpts(max_iter=10, tol_mva=1e-4)
    for fn in (eng.lookahead_values, eng.lookahead_views):
        with pytest.raises(GridPFError, match="the look-ahead is off"):
            fn()
    with pytest.raises(GridPFError, match="the look-ahead is off"):
        eng.lookahead(0)
    for rc in (L.gpf_get_lookahead(eng._h, 0, 1, None, None, None, None, None),
               L.gpf_lookahead_device_pointers(eng._h, (C.c_void_p * _capi.N_LOOKAHEAD_POINTERS)(), _capi.N_LOOKAHEAD_POINTERS),
               L.gpf_lookahead(eng._h, 0, 1, None, C.byref(opts))):
        assert rc != 0 and b"the look-ahead is off" in L.gpf_last_error()
    with pytest.raises(GridPFError, match=r"no action table \(gpf_upload_topo_actions\)"):
        eng.set_lookahead(3, 2)
    eng.upload_topo_actions([{"set_line_status": [(3, -1)]}, {"set_line_status": [(3, +1)]}, {"change_line_status": [5]}])
    for bad in (0, -3):
        with pytest.raises(GridPFError, match="n_env must be positive"):
            eng.set_lookahead(3, bad)
    with pytest.raises(GridPFError, match=r"4 environments x \(1 \+ 3 candidates\) need 16 lanes, the engine has 14"):
        eng.set_lookahead(3, 4)
    assert L.gpf_set_lookahead(eng._h, 2, -1) != 0 and b"negative n_cand" in L.gpf_last_error()
    # composite slots and areas, with their reason
    eng.set_topo_slots(2)
    with pytest.raises(GridPFError, match=r"composite actions \(gpf_set_topo_slots > 1\) are not supported"):
        eng.set_lookahead(3, 2)
    eng.set_topo_slots(1)
    eng.set_topo_areas(np.arange(m.n_sub) % 2)
    with pytest.raises(GridPFError, match=r"rules by area \(gpf_set_topo_areas\) are not supported"):
        eng.set_lookahead(3, 2)
    eng.set_topo_areas(None)
    # the N-1 screen and the look-ahead claim the same lanes
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_n1_screen([3, 5], 2)
    with pytest.raises(GridPFError, match=r"the N-1 screen \(gpf_set_n1_screen\) is on"):
        eng.set_lookahead(3, 2)
    eng.set_n1_screen(None)
    eng.set_lookahead(0)                                                  # off is always possible
    eng.set_lookahead(None)
    assert L.gpf_step_n(eng._h, 0, 3, C.byref(opts)) != 0 and b"look-ahead" not in L.gpf_last_error()     # off: another refusal
    with pytest.raises(GridPFError, match="no HIP device"):               # a good call gets as far as the missing device
        eng.set_lookahead(3, 3)
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_lookahead(3)                                              # n_env by default: as many as fit
    with pytest.raises(GridPFError, match=r"the look-ahead \(gpf_set_lookahead\) is set"):
        eng.set_n1_screen([3, 5], 2)
    eng.set_n1_screen(None)                                               # (off stays possible)
    # a horizon without forecasts, with gpf_simulate_batch's reason
    with pytest.raises(GridPFError, match=r"no forecast for that horizon \(gpf_upload_forecasts; NoForecastAvailable in the reference\)"):
        eng.lookahead(0, time_step=1)
    with pytest.raises(GridPFError, match="no forecast for that horizon"):
        eng.lookahead(0, time_step=-1)
    with pytest.raises(GridPFError, match="no HIP device"):               # the observation's own injections need none
        eng.lookahead(0, time_step=0)
    # candidates of the wrong shape
    for bad in (np.zeros((3, 2), np.int32), np.zeros(9, np.int32), np.zeros((4, 3), np.int32)):
        with pytest.raises(ValueError, match=r"candidates must be \[n_env, K\] = \[3, 3\]"):
            eng.lookahead(0, time_step=0, candidates=bad)
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.lookahead(0, time_step=0, candidates=np.full((3, 3), -1))
    # composite slots / areas set AFTER the look-ahead are refused at the call
    eng.set_topo_slots(2)
    with pytest.raises(GridPFError, match="composite actions"):
        eng.lookahead(0, time_step=0)
    eng.set_topo_slots(1)
    # a multi-step launch while the look-ahead is set: the message has the form of the other one-step features
    assert L.gpf_step_n(eng._h, 0, 3, C.byref(opts)) != 0
    msg = L.gpf_last_error().decode()
    assert msg.startswith("gpf_step_n: with the look-ahead set (gpf_set_lookahead) a launch must be a one-step launch") and msg.endswith("use n_steps = 1")
    with pytest.raises(GridPFError, match="the look-ahead is off"):       # the getters: nothing was set on a device
        eng.lookahead_values()
    eng.set_lookahead(0)
    assert L.gpf_step_n(eng._h, 0, 3, C.byref(opts)) != 0 and b"look-ahead" not in L.gpf_last_error()
    with pytest.raises(GridPFError, match="the look-ahead is off"):
        eng.lookahead(0, time_step=0, candidates=np.full((3, 3), -1))
    eng.close()


def test_exported_symbols_constants_and_routes():
    from grid2op_amd import _capi, engine
    from grid2op_amd.sharding import ROUTES, every, gather, per_device
    names = ("gpf_set_lookahead", "gpf_lookahead", "gpf_get_lookahead", "gpf_lookahead_device_pointers")
    assert all(n in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), n) for n in names)
    sig = list(_capi.SIGNATURES)
    assert [sig.index(n) for n in names] == list(range(sig.index("gpf_n1_device_pointers") + 1, sig.index("gpf_n1_device_pointers") + 5))
    hdr = open(golden_path("../../include/gridpf.h")).read()
    assert [hdr.index(f"int {n}(") for n in names] == sorted(hdr.index(f"int {n}(") for n in names) and hdr.index("int gpf_n1_device_pointers(") < hdr.index("int gpf_set_lookahead(")
    for text in ("#define GPF_N_LOOKAHEAD_POINTERS 6", "#define GPF_LA_ILLEGAL 1", "#define GPF_LA_AMBIGUOUS 2", "#define GPF_LA_DONE 4",
                 "#define GPF_ABI_VERSION 326", "#define GPF_N_DEVICE_POINTERS 34"):
        assert text in hdr, text
    assert (engine.LA_ILLEGAL, engine.LA_AMBIGUOUS, engine.LA_DONE) == (LA.ILLEGAL, LA.AMBIGUOUS, LA.DONE) == (1, 2, 4)
    assert _capi.N_LOOKAHEAD_POINTERS == 6 and _capi.ABI_VERSION == 326 and _capi.N_DEVICE_POINTERS == 34
    assert "set_lookahead" in ROUTES[every] and "lookahead" in ROUTES[every] and "lookahead_values" in ROUTES[gather] and "lookahead_views" in ROUTES[per_device]


def test_sharded_engine_forwards_the_look_ahead(load_model):
    from stub_engine import StubEngine
    from grid2op_amd.sharding import ShardedEngine

    class Stub(StubEngine):
        def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
            super().__init__(model, n_lanes, device, n_busbar)
            self.calls, self.n_lanes_ = [], n_lanes

        def set_lookahead(self, n_cand, n_env=None):
            self.calls.append(("set", n_cand, n_env))

        def lookahead(self, t_obs, time_step=1, candidates=None, **kw):
            self.calls.append(("look", t_obs, time_step, candidates, kw))

        def lookahead_values(self, lane0=0, n=None):                         # two environments per shard, inside the range asked for
            n = self.n_lanes_ - lane0 if n is None else n
            envs = [i for i in range(2) if lane0 <= i < lane0 + n]
            return dict(value=np.array([[1000 * self.device + i] * 3 for i in envs], np.float32).reshape(-1, 3), best=np.array(envs, np.int32))

        def lookahead_views(self):
            return {"cand": self.device}

    m = load_model("l2rpn_case14_sandbox")
    se = ShardedEngine(m, 24, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: Stub(mm, n, dev, nbb))
    se.set_lookahead(3, 2)
    se.lookahead(5, time_step=0, cascade=True)
    assert all(e.calls == [("set", 3, 2), ("look", 5, 0, None, {"cascade": True})] for e in se.engines)
    assert se.lookahead_values()["value"][:, 0].tolist() == [0, 1, 1000, 1001, 2000, 2001]         # each shard's environments, in shard order
    assert se.lookahead_values(9, 7)["best"].tolist() == [1]                                       # lanes 9..15: lane 1 of the second shard
    assert se.lookahead_views() == [{"cand": e.device} for e in se.engines]


def test_sanitized_stand_alone_emulator_runs_clean():
    p = subprocess.run([LA.sanitized_program()], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK") and not p.stderr, (p.stdout, p.stderr[-2000:])
