"""The look-ahead chain (include/gridpf.h gpf_set_lookahead_chain / gpf_lookahead_chain), the parts that need no GPU: the recordings of the
unmodified reference's obs.get_forecast_env() (tests/golden/lookahead_chain_*.npz) against the numpy restatement
(tests/lookahead_chain_ref.py) and the library's rule functions compiled with g++ (tests/native/lookahead_chain_emul.cpp), every refusal
through a header-only handle, the exported symbols, the constants and the routing of `ShardedEngine`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lookahead_chain_ref as LC
from conftest import golden_path

FIXTURES = ("lookahead_chain_5bus.npz", "lookahead_chain_5bus_maintenance.npz")


@pytest.fixture(scope="module")
def recorded():
    return {f: dict(np.load(golden_path(f))) for f in FIXTURES}


@pytest.mark.parametrize("fixture", FIXTURES)
def test_restatement_and_emulator_against_the_recording(recorded, fixture):
    """Per (state, slot): the restated record of the recorded rho rows and done flags is the emulator's bit for bit, survived is the number
    of forecast-env steps the reference completed, the chain's flags are step 1's verdict plus "done anywhere"; per state: best and
    fall-back of restatement and emulator agree on the recorded values."""
    fx = recorded[fixture]
    S, K, H, L = fx["sim_rho"].shape
    assert H >= 4 and fx["sim_done"].shape == (S, K, H)
    for s in range(S):
        lanes = []
        for k in range(K):
            want, got = LC.lane(fx["sim_rho"][s, k], fx["sim_done"][s, k]), LC.emul_lane(fx["sim_rho"][s, k], fx["sim_done"][s, k])
            assert LC.same_lane(want, got), (s, k, want, got)
            assert want["survived"] == int(fx["sim_steps"][s, k]) and want["failed"] == bool(fx["sim_done"][s, k].any())
            if want["survived"]:
                assert abs(float(want["peak"]) - float(fx["sim_rho"][s, k, :want["survived"]].max())) == 0.0
            lanes.append(want)
        flags = LC.chain_flags(fx["sim_flags"][s], [l["failed"] for l in lanes])
        value, sv, pk = np.array([l["value"] for l in lanes], np.float32), [l["survived"] for l in lanes], np.array([l["peak"] for l in lanes], np.float32)
        from lookahead_ref import emul_summary
        a, b = LC.summary(value, flags), emul_summary(value, flags)
        assert (a[0], a[1].tobytes(), a[2], a[3]) == (b[0], b[1].tobytes(), b[2], b[3]), s
        assert LC.fallback(sv, pk, flags) == LC.emul_fallback(sv, pk, flags), s
        assert a[0] == int(fx["best"][s]) or int(fx["best"][s]) == -2                    # (-2: not pinned, the runner-up is within the margin)
        assert LC.fallback(sv, pk, flags)[0] == int(fx["fallback"][s]) or int(fx["fallback"][s]) == -2


def test_what_the_recordings_hold(recorded):
    """what the maker asserted, once more on the files themselves"""
    seen = dict(late_trip=0, late_done=0, illegal=0, ambiguous=0, minus_one=0, none_survives=0, late_maintenance=0)
    pinned = total = 0
    for f, fx in recorded.items():
        S, K, H, L = fx["sim_rho"].shape
        hard = float(fx["hard_overflow"])
        rho = fx["sim_rho"][np.isfinite(fx["sim_rho"]) & (fx["sim_valid"][..., None] != 0)]
        assert (np.abs(rho - 1.0) > LC.MARGIN).all() and (np.abs(rho - hard) > LC.MARGIN).all()
        for s in range(S):
            total += 1
            pinned += int(fx["best"][s]) != -2 and int(fx["fallback"][s]) != -2
            all_fail = True
            for k in range(K):
                done, ls = fx["sim_done"][s, k], fx["sim_line_status"][s, k]
                seen["illegal"] += bool(fx["sim_flags"][s, k] & LC.ILLEGAL)
                seen["ambiguous"] += bool(fx["sim_flags"][s, k] & LC.AMBIGUOUS)
                seen["minus_one"] += int(fx["cand"][s, k]) == -1
                seen["late_done"] += bool(done.any() and not done[0])
                all_fail &= bool(done.any()) or bool(fx["sim_flags"][s, k] & 3)
                for h in range(1, int(fx["sim_steps"][s, k])):
                    tripped = ls[h - 1] & ~ls[h] & ~fx["sim_maint_out"][s, h]
                    seen["late_trip"] += bool(tripped.any() and (fx["timestep_overflow"][s][tripped] >= 1).any())
                    seen["late_maintenance"] += bool((fx["sim_maint_out"][s, h] & ~fx["sim_maint_out"][s, h - 1] & ls[h - 1]).any())
            seen["none_survives"] += all_fail
    assert seen["late_trip"] and seen["late_done"] and seen["illegal"] and seen["ambiguous"] and seen["minus_one"] and seen["none_survives"], seen
    assert seen["late_maintenance"], seen
    assert pinned >= 0.75 * total, (pinned, total)


@pytest.mark.parametrize("K,n_line,H", [(1, 20, 1), (6, 59, 4), (64, 64, 2), (65, 187, 12), (129, 8, 3)])
def test_emulator_equals_the_restatement_on_seeded_tables(K, n_line, H):
    rng = np.random.default_rng(1000 * K + n_line + H)
    L = LC.emulator()
    for rep in range(6):
        rho = rng.uniform(0, 1.9, (K, H, n_line)).astype(np.float32)
        done = rng.random((K, H)) < (0.0 if rep == 0 else 1.0 if rep == 1 else 0.25)
        lanes = []
        for k in range(K):
            want, got = LC.lane(rho[k], done[k]), LC.emul_lane(rho[k], done[k])
            assert LC.same_lane(want, got), (k, want, got)
            first = int(np.argmax(done[k])) if done[k].any() else H
            assert want["survived"] == first and np.isinf(want["value"]) == bool(done[k].any()) and np.isinf(want["value_h"][first:]).all()
            assert want["peak"] == (rho[k, :first].max() if first else -np.inf)             # later steps of a failed lane are ignored
            lanes.append(want)
        sv, pk = np.array([l["survived"] for l in lanes]), np.array([l["peak"] for l in lanes], np.float32)
        flags = np.where(rng.random(K) < 0.3, rng.integers(1, 4, K), 0).astype(np.uint8)
        if rep == 2:
            flags[:] = rng.integers(1, 4, K)                                                # no eligible slot
        if rep >= 3 and K > 2:
            sv[K // 2], pk[K // 2], flags[K // 2], flags[K // 3] = sv[K // 3], pk[K // 3], 0, 0   # a tie: the lower slot
        flags = LC.chain_flags(flags, sv < H)
        got, want = LC.emul_fallback(sv, pk, flags), LC.fallback(sv, pk, flags)
        assert got == want, (rep, got, want)
        if rep == 2:
            assert got == (-1, 0)
        elif got[0] >= 0:
            ok = np.flatnonzero((flags & 3) == 0)
            assert got[1] == sv[ok].max() and pk[got[0]] == pk[ok][sv[ok] == got[1]].min() and got[0] == ok[(sv[ok] == got[1]) & (pk[ok] == pk[got[0]])][0]
    inf = float("inf")
    assert L.la_chain_emul_outranks(3, 0.9, 5, 2, 0.1, 0) == 1 and L.la_chain_emul_outranks(2, 0.1, 0, 3, 0.9, 5) == 0      # more steps first
    assert L.la_chain_emul_outranks(3, 0.5, 5, 3, 0.6, 0) == 1 and L.la_chain_emul_outranks(3, 0.5, 5, 3, 0.5, 4) == 0      # then the peak, then the slot
    assert L.la_chain_emul_outranks(0, -inf, 1, 0, -inf, 2) == 1 and L.la_chain_emul_outranks(4, 0.1, -1, 0, -inf, 2) == 0 and L.la_chain_emul_outranks(0, -inf, 2, 9, 0.1, -1) == 1
    assert [L.la_chain_emul_pick(p, b, f) for p, b, f in ((1, 3, 5), (1, -1, 5), (2, -1, 5), (2, -1, -1), (2, 0, 5))] == [3, -1, 5, -1, 0]
    assert [LC.pick(p, b, f) for p, b, f in ((1, 3, 5), (1, -1, 5), (2, -1, 5), (2, -1, -1), (2, 0, 5))] == [3, -1, 5, -1, 0]
    assert [L.la_chain_emul_row(12, 7, h) for h in (1, 2, 12)] == [84, 85, 95] and L.la_chain_emul_row(1, 7, 1) == 7


def test_every_refusal_on_a_header_only_handle(load_model):
    from grid2op_amd import _capi
    from grid2op_amd.engine import GridPFError, PowerFlowEngine
    m = load_model("l2rpn_case14_sandbox")
    eng = PowerFlowEngine(m, n_lanes=14, device=-1)
    L = eng._lib
    opts = _capi.GpfStepOpts(max_iter=10, tol_mva=1e-4)
    for fn in (eng.lookahead_chain_values, eng.lookahead_chain_views):
        with pytest.raises(GridPFError, match="the chain is off"):
            fn()
    # the look-ahead is off: the chain cannot be set, and a call says so first
    with pytest.raises(GridPFError, match=r"the look-ahead is off \(gpf_set_lookahead\)"):
        eng.set_lookahead_chain(4)
    with pytest.raises(GridPFError, match=r"gpf_lookahead_chain: the look-ahead is off \(gpf_set_lookahead\)"):
        eng.lookahead_chain(0, 2)
    for rc in (L.gpf_get_lookahead_chain(eng._h, 0, 1, None, None, None, None, None),
               L.gpf_lookahead_chain_device_pointers(eng._h, (C.c_void_p * _capi.N_LOOKAHEAD_CHAIN_POINTERS)(), _capi.N_LOOKAHEAD_CHAIN_POINTERS)):
        assert rc != 0 and b"the chain is off" in L.gpf_last_error()
    assert L.gpf_lookahead_chain_device_pointers(eng._h, (C.c_void_p * 6)(), 6) != 0 and b"GPF_N_LOOKAHEAD_CHAIN_POINTERS" in L.gpf_last_error()
    eng.set_lookahead_chain(0)                                            # off is always possible
    eng.upload_topo_actions([{"set_line_status": [(3, -1)]}, {"set_line_status": [(3, +1)]}, {"change_line_status": [5]}])
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_lookahead(3, 3)
    # the look-ahead is set, the chain is not
    with pytest.raises(GridPFError, match=r"gpf_lookahead_chain: the chain is off \(gpf_set_lookahead_chain\)"):
        eng.lookahead_chain(0, 2)
    assert L.gpf_set_lookahead_chain(eng._h, -2) != 0 and b"negative max_steps" in L.gpf_last_error()
    with pytest.raises(GridPFError, match="no HIP device"):               # a good call gets as far as the missing device
        eng.set_lookahead_chain(4)
    # n_steps: below 1, above max_steps, above the uploaded forecast horizons (none here)
    for bad in (0, -1):
        with pytest.raises(GridPFError, match="n_steps must be at least 1"):
            eng.lookahead_chain(0, bad)
    with pytest.raises(GridPFError, match=r"n_steps = 5 exceeds max_steps = 4 of gpf_set_lookahead_chain"):
        eng.lookahead_chain(0, 5)
    with pytest.raises(GridPFError, match=r"gpf_lookahead_chain: no forecast for that horizon \(gpf_upload_forecasts; NoForecastAvailable in the reference\)"):
        eng.lookahead_chain(0, 2)
    # play: its range, and one action slot per lane
    for bad in (-1, 3):
        with pytest.raises(GridPFError, match="play must be 0"):
            eng.lookahead_chain(0, 2, play=bad)
    eng.set_topo_slots(2)
    with pytest.raises(GridPFError, match=r"play needs one action slot per lane \(gpf_set_topo_slots is 2\)"):
        eng.lookahead_chain(0, 2, play=1)
    with pytest.raises(GridPFError, match=r"gpf_lookahead_chain: composite actions \(gpf_set_topo_slots > 1\) are not supported"):   # gpf_lookahead's refusals
        eng.lookahead_chain(0, 2)
    eng.set_topo_slots(1)
    eng.set_topo_areas(np.arange(m.n_sub) % 2)
    with pytest.raises(GridPFError, match=r"gpf_lookahead_chain: rules by area \(gpf_set_topo_areas\) are not supported"):
        eng.lookahead_chain(0, 2)
    eng.set_topo_areas(None)
    # candidates of the wrong shape
    for bad in (np.zeros((3, 2), np.int32), np.zeros(9, np.int32)):
        with pytest.raises(ValueError, match=r"candidates must be \[n_env, K\] = \[3, 3\]"):
            eng.lookahead_chain(0, 2, candidates=bad)
    # the one-step look-ahead is refused as before
    with pytest.raises(GridPFError, match=r"gpf_lookahead: no forecast for that horizon"):
        eng.lookahead(0, time_step=1)
    with pytest.raises(GridPFError, match="the chain is off"):            # the getters: nothing was set on a device
        eng.lookahead_chain_values()
    # switching the look-ahead off releases the chain
    eng.set_lookahead(0)
    with pytest.raises(GridPFError, match="the look-ahead is off"):
        eng.lookahead_chain(0, 2)
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_lookahead(3, 3)
    with pytest.raises(GridPFError, match="the chain is off"):
        eng.lookahead_chain(0, 2)
    eng.close()


def test_exported_symbols_constants_and_routes():
    from grid2op_amd import _capi
    from grid2op_amd.sharding import ROUTES, every, gather, per_device
    names = ("gpf_set_lookahead_chain", "gpf_lookahead_chain", "gpf_get_lookahead_chain", "gpf_lookahead_chain_device_pointers")
    assert all(n in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), n) for n in names)
    sig = list(_capi.SIGNATURES)
    assert [sig.index(n) for n in names] == list(range(sig.index("gpf_lookahead_device_pointers") + 1, sig.index("gpf_lookahead_device_pointers") + 5))
    hdr = open(golden_path("../../include/gridpf.h")).read()
    assert [hdr.index(f"int {n}(") for n in names] == sorted(hdr.index(f"int {n}(") for n in names) and hdr.index("int gpf_lookahead_device_pointers(") < hdr.index("int gpf_set_lookahead_chain(")
    for text in ("#define GPF_N_LOOKAHEAD_CHAIN_POINTERS 5", "#define GPF_N_LOOKAHEAD_POINTERS 6", "#define GPF_ABI_VERSION 326", "#define GPF_N_DEVICE_POINTERS 34"):
        assert text in hdr, text
    assert _capi.N_LOOKAHEAD_CHAIN_POINTERS == 5 and _capi.N_LOOKAHEAD_POINTERS == 6 and _capi.ABI_VERSION == 326 and _capi.N_DEVICE_POINTERS == 34
    assert "set_lookahead_chain" in ROUTES[every] and "lookahead_chain" in ROUTES[every] and "lookahead_chain_values" in ROUTES[gather] and "lookahead_chain_views" in ROUTES[per_device]
    src = open(golden_path("../../grid2op_amd/csrc/gridpf_lookahead.hpp")).read()
    for rule in ("la_chain_row", "la_chain_step", "la_chain_failed", "la_chain_eligible", "la_chain_outranks", "la_chain_pick"):
        assert len([ln for ln in src.splitlines() if ln.startswith("GPF_LA_HD inline") and f" {rule}(" in ln]) == 1, rule    # stated once, for host and device


def test_sharded_engine_forwards_the_chain(load_model):
    from stub_engine import StubEngine
    from grid2op_amd.sharding import ShardedEngine

    class Stub(StubEngine):
        def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
            super().__init__(model, n_lanes, device, n_busbar)
            self.calls, self.n_lanes_ = [], n_lanes

        def set_lookahead_chain(self, max_steps):
            self.calls.append(("set", max_steps))

        def lookahead_chain(self, t_obs, n_steps, candidates=None, play=0, **kw):
            self.calls.append(("chain", t_obs, n_steps, candidates, play, kw))

        def lookahead_chain_values(self, lane0=0, n=None):                   # two environments per shard, inside the range asked for
            n = self.n_lanes_ - lane0 if n is None else n
            envs = [i for i in range(2) if lane0 <= i < lane0 + n]
            return dict(survived=np.array([[100 * self.device + i] * 3 for i in envs], np.int32).reshape(-1, 3), fallback=np.array(envs, np.int32))

        def lookahead_chain_views(self):
            return {"survived": self.device}

    m = load_model("l2rpn_case14_sandbox")
    se = ShardedEngine(m, 24, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: Stub(mm, n, dev, nbb))
    se.set_lookahead_chain(4)
    se.lookahead_chain(5, 3, play=2, cascade=True)
    assert all(e.calls == [("set", 4), ("chain", 5, 3, None, 2, {"cascade": True})] for e in se.engines)
    assert se.lookahead_chain_values()["survived"][:, 0].tolist() == [0, 1, 100, 101, 200, 201]
    assert se.lookahead_chain_values(9, 7)["fallback"].tolist() == [1]
    assert se.lookahead_chain_views() == [{"survived": e.device} for e in se.engines]


def test_sanitized_stand_alone_emulator_runs_clean():
    p = subprocess.run([LC.sanitized_program()], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK") and not p.stderr, (p.stdout, p.stderr[-2000:])
