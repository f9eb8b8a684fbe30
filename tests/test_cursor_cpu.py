"""The chronics cursor of the batched acting path (include/gridpf.h gpf_set_chronics_cursor), the parts that need no GPU: the numpy
restatement (tests/cursor_ref.py) and the library's rule compiled with g++ (tests/native/cursor_emul.cpp) against the resets recorded from
the unmodified reference (tests/golden/chronics_cursor_case14.npz) and against each other on seeded runs, the Philox path bit for bit, the
cdf against numpy's own ``choice``, every refusal a header-only handle can give, the exported symbols and the routing of `ShardedEngine`."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cursor_ref as CR
from conftest import golden_path

PLAIN, SET_ID, SAMPLED, INIT_TS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(golden_path("chronics_cursor_case14.npz")))


def phases(fx):
    """per phase: the rows at which an episode starts"""
    starts = np.flatnonzero(fx["is_reset"])
    return {int(ph): [int(i) for i in starts if fx["phase"][i] == ph] for ph in sorted(set(int(x) for x in fx["phase"]))}


def phase_config(fx, idx):
    """what a replay configures once per phase: policy, cdf, first_row, the first position, the uniforms"""
    sampled = int(fx["how"][idx[0]]) == SAMPLED
    return dict(policy=CR.SAMPLED if sampled else CR.SEQUENTIAL, cdf=CR.cdf_of(fx["probabilities"]) if sampled else None,
                first_row=int(fx["row"][idx[0]]), next_pos=-1 if sampled else int(fx["scenario"][idx[0]]),
                draws=fx["uniform"][idx] if sampled else None)


def test_fixture_covers_the_cases(recorded):
    fx = recorded
    starts = np.flatnonzero(fx["is_reset"])
    how, sc = fx["how"][starts], fx["scenario"][starts]
    plain = [int(s) for s, h, p in zip(sc, how, fx["phase"][starts]) if h == PLAIN and p == 0]
    assert plain[:6] == [1, 2, 0, 1, 2, 0]                                  # at least five consecutive plain resets: the order wraps
    assert (how == SET_ID).sum() == 1 and (how == SAMPLED).sum() >= 6 and (how == INIT_TS).sum() == 1
    assert len(set(int(s) for s in sc[how == SAMPLED])) >= 2 and len(set(fx["probabilities"])) == 3
    assert fx["terminated"].sum() == 1 and fx["truncated"].sum() == len(starts) - 1
    assert int(fx["row"][starts][how == INIT_TS][0]) == 2 and (fx["row"][starts][how != INIT_TS] == 0).all()
    assert set(int(x) for x in fx["max_step"]) <= {2, 3, 4}
    # the calendar restarts with every scenario (the three begin on the same day: the row shows in the hour and the minute)
    assert len(fx["start_minutes"]) == 3 and (fx["minute_of_hour"] + 60 * fx["hour_of_day"] == 5 * fx["row"]).all()
    for i in starts:
        if fx["how"][i] != INIT_TS:
            assert fx["hour_of_day"][i] == 0 and fx["minute_of_hour"][i] == 0


def test_restatement_recording_and_emulator_agree_on_every_episode(recorded):
    fx = recorded
    T = fx["chron_load_p"].shape[1]
    n_ep = 0
    for ph, idx in phases(fx).items():
        cfg = phase_config(fx, idx)
        draws = None if cfg["draws"] is None else cfg["draws"][None]
        kw = dict(policy=cfg["policy"], cdf=cfg["cdf"], first_row=cfg["first_row"], next_pos=cfg["next_pos"], draws=draws)
        ref, emu = CR.CursorRef(1, [0, 1, 2], T, **kw), CR.CursorEmul(1, [0, 1, 2], T, **kw)
        t = 5 * ph
        for i in idx:
            if fx["how"][i] == SET_ID:
                ref.next_pos[0] = emu.state[0, 3] = int(fx["set_id"][i])
            ref.start(0, t)
            emu.start(0, t)
            assert np.array_equal(ref.rows(), emu.rows()), (ph, i, ref.rows(), emu.rows())
            assert ref.table[0] == fx["scenario"][i] and (t + ref.offset[0]) % T == fx["row"][i], (ph, i)
            ep = np.flatnonzero((np.arange(len(fx["done"])) >= i) & fx["done"].astype(bool))[0]
            assert (fx["scenario"][i:ep + 1] == ref.table[0]).all() and np.array_equal(fx["row"][i:ep + 1], fx["row"][i] + np.arange(ep + 1 - i))
            t += ep + 1 - i
            n_ep += 1
        assert not ref.flags.any()
    assert n_ep == fx["is_reset"].sum()


def test_cdf_is_the_one_numpy_choice_searches(recorded):
    """RandomState.choice(order, p=float32 probabilities) on a copy of the generator gives the position the restatement finds with the
    uniform drawn from another copy"""
    rng = np.random.RandomState(3)
    for n in (1, 2, 3, 20):
        for _ in range(50):
            p = rng.uniform(0.0, 1.0, n) * (rng.uniform(0, 1, n) > 0.2)
            if p.sum() <= 1e-5:
                continue
            p32 = np.array(p, dtype=np.float32)
            p32 /= p32.sum()
            a, b = np.random.RandomState(), np.random.RandomState()
            a.set_state(rng.get_state()); b.set_state(rng.get_state())
            assert a.choice(np.arange(n), p=p32) == CR.search(CR.cdf_of(p), b.random_sample())
            rng.random_sample()
    from grid2op_amd.engine import cursor_cdf
    assert cursor_cdf(recorded["probabilities"]).tobytes() == CR.cdf_of(recorded["probabilities"]).tobytes()
    with pytest.raises(ValueError):
        cursor_cdf([0.0, 0.0])


@pytest.mark.parametrize("n_order", [1, 2, 3, 20])
@pytest.mark.parametrize("policy", [CR.SEQUENTIAL, CR.SAMPLED])
@pytest.mark.parametrize("source", [CR.TABLE, CR.PHILOX])
def test_emulator_equals_the_restatement_on_seeded_runs(n_order, policy, source):
    """7 lanes, 60 launches, episodes that end at random, next_pos written now and then (a bad one too), a draw table that runs out"""
    rng = np.random.default_rng(1000 * n_order + 10 * policy + source)
    n, T = 7, 13
    order = rng.permutation(n_order)
    kw = dict(policy=policy, cdf=CR.cdf_of(rng.uniform(0.05, 1.0, n_order)) if policy == CR.SAMPLED else None, first_row=rng.integers(0, T, n),
              next_pos=rng.integers(-1, n_order, n), draws=rng.uniform(0, 1, (n, 6)) if source == CR.TABLE else None,
              seed=0x123456789 if source == CR.PHILOX else None, lane_base=40)
    ref, emu = CR.CursorRef(n, order, T, **kw), CR.CursorEmul(n, order, T, **kw)
    steps = np.zeros(n, np.int64)
    skip = np.zeros(n, bool)
    skip[5] = True                                                          # a scratch lane: never moved
    seen = set()
    for t in range(60):
        if t % 9 == 4:
            k, v = int(rng.integers(0, n)), int(rng.integers(0, n_order + 2))
            ref.next_pos[k] = emu.state[k, 3] = v
        ref.prestep(t, steps, skip)
        emu.prestep(t, steps, skip)
        assert np.array_equal(ref.rows(), emu.rows()), t
        for k in range(n):
            if steps[k] == 0 and not skip[k]:
                assert ref.table[k] == order[ref.pos[k]] and (t + ref.offset[k]) % T == ref.first_row[k]
                seen.add(int(ref.pos[k]))
        steps = np.where(rng.uniform(0, 1, n) < 0.3, 0, steps + 1)
    assert ref.n_started[5] == 0 and ref.n_started.sum() > 40
    if policy == CR.SEQUENTIAL:
        assert not ref.draws_used.any() and seen == set(range(n_order))
    elif source == CR.TABLE:
        assert (ref.flags[ref.n_started > 8] & CR.FLAG_DRAWS_EXHAUSTED).all() and (ref.draws_used <= 6).all()
    else:
        assert not (ref.flags & CR.FLAG_DRAWS_EXHAUSTED).any() and ref.draws_used.sum() > 20


def test_philox_path_is_bit_equal_and_its_stream_is_not_the_opponents():
    from opponent_ref import philox4x32_10, philox_u
    rng = np.random.default_rng(5)
    for _ in range(200):
        ns, gl, seed = int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 2 ** 63))
        x = philox4x32_10((ns, 0, gl, CR.PHILOX_STREAM), (seed & 0xFFFFFFFF, seed >> 32))
        u = philox_u(x[0], x[1])
        assert 0.0 <= u < 1.0 and np.float64(u).tobytes() == np.float64(CR.emul_philox_u(ns, gl, seed)).tobytes()
        y = philox4x32_10((ns, 0, gl, 0), (seed & 0xFFFFFFFF, seed >> 32))       # the opponent's counter of the same draw, episode 0, lane
        assert philox_u(y[0], y[1]) != u
    # two shards with their lane_base equal one engine
    one = CR.CursorRef(6, [0, 1, 2], 9, CR.SAMPLED, CR.cdf_of([1, 2, 3]), seed=77)
    a, b = CR.CursorRef(4, [0, 1, 2], 9, CR.SAMPLED, CR.cdf_of([1, 2, 3]), seed=77), CR.CursorRef(2, [0, 1, 2], 9, CR.SAMPLED, CR.cdf_of([1, 2, 3]), seed=77, lane_base=4)
    for t in range(12):
        for r in (one, a, b):
            r.prestep(t, np.zeros(r.n))
        assert np.array_equal(one.rows(), np.concatenate([a.rows(), b.rows()]))


def test_every_refusal_on_a_header_only_handle(load_model):
    from grid2op_amd import _capi
    from grid2op_amd.engine import GridPFError, PowerFlowEngine
    m = load_model("l2rpn_case14_sandbox")
    eng = PowerFlowEngine(m, n_lanes=4, device=-1)
    for fn in (eng.chronics_cursor_state, eng.cursor_views, lambda: eng.upload_cursor_draws(np.zeros((4, 2)))):
        with pytest.raises(GridPFError, match="the chronics cursor is off"):
            fn()
    L = eng._lib
    rows = np.zeros((1, 7), np.int32)
    for rc in (L.gpf_get_cursor_state(eng._h, 0, 1, _capi.ptr(rows, C.c_int32)), L.gpf_set_cursor_state(eng._h, 0, 1, _capi.ptr(rows, C.c_int32)),
               L.gpf_upload_cursor_draws(eng._h, 0, None), L.gpf_cursor_device_pointers(eng._h, (C.c_void_p * _capi.N_CURSOR_POINTERS)(), _capi.N_CURSOR_POINTERS)):
        assert rc != 0 and b"the chronics cursor is off" in L.gpf_last_error()
    with pytest.raises(GridPFError, match="the order is empty"):
        eng.set_chronics_cursor(order=[])
    with pytest.raises(GridPFError, match=r"order\[1\] is negative"):
        eng.set_chronics_cursor(order=[0, -1])
    with pytest.raises(GridPFError, match="unknown policy 7"):
        eng.set_chronics_cursor(order=[0], policy=7)
    with pytest.raises(GridPFError, match=r"first_row -1 is outside \[0, T\)"):
        eng.set_chronics_cursor(order=[0, 1], first_row=-1)
    with pytest.raises(GridPFError, match=r"first_row -3 is outside \[0, T\)"):
        eng.set_chronics_cursor(order=[0, 1], first_row=[0, 1, -3, 2])
    with pytest.raises(GridPFError, match="next_pos 2 >= n_order = 2"):
        eng.set_chronics_cursor(order=[0, 1], next_pos=2)
    with pytest.raises(GridPFError, match="next_pos 5 >= n_order = 2"):
        eng.set_chronics_cursor(order=[0, 1], policy="sampled", next_pos=[0, -1, 5, 1])
    with pytest.raises(GridPFError, match="lane_base must not be negative"):
        eng.set_chronics_cursor(order=[0], lane_base=-1)
    order = np.arange(3, dtype=np.int32)
    for cdf, why in (([0.5, 0.4, 1.0], "entry 1"), ([0.2, 0.5, 0.9], "last entry is not 1"), ([0.2, np.nan, 1.0], "entry 1"), ([-0.1, 0.5, 1.0], "entry 0")):
        c = np.array(cdf, np.float64)
        d = _capi.GpfCursorDesc(n_order=3, order=_capi.ptr(order, C.c_int32), policy=CR.SAMPLED, cdf=_capi.ptr(c, C.c_double))
        assert L.gpf_set_chronics_cursor(eng._h, C.byref(d)) != 0
        msg = L.gpf_last_error().decode()
        assert "the cdf is not non-decreasing to 1" in msg and why in msg, msg
    d = _capi.GpfCursorDesc(n_order=3, order=_capi.ptr(order, C.c_int32), policy=CR.SAMPLED)
    assert L.gpf_set_chronics_cursor(eng._h, C.byref(d)) != 0 and b"needs a cdf" in L.gpf_last_error()
    eng.set_chronics_cursor(False)                                          # off is always possible
    opts = _capi.GpfStepOpts(max_iter=10, tol_mva=1e-4)
    assert L.gpf_step_n(eng._h, 0, 3, C.byref(opts)) != 0 and b"chronics cursor" not in L.gpf_last_error()     # off: another refusal (no chronics)
    with pytest.raises(GridPFError, match="no HIP device"):                 # a good call gets as far as the missing device
        eng.set_chronics_cursor(order=[0, 1, 2], policy="sampled", probabilities=[1, 2, 3], first_row=[0, 1, 2, 3], seed=9)
    with pytest.raises(GridPFError, match="the chronics cursor is off"):    # ... and leaves the getters refusing
        eng.chronics_cursor_state()
    assert L.gpf_step_n(eng._h, 0, 3, C.byref(opts)) != 0
    msg = L.gpf_last_error().decode()
    assert msg.startswith("gpf_step_n: with the chronics cursor on (gpf_set_chronics_cursor) a launch must be a one-step launch") and msg.endswith("use n_steps = 1")
    eng.set_chronics_cursor(False)
    assert L.gpf_step_n(eng._h, 0, 3, C.byref(opts)) != 0 and b"chronics cursor" not in L.gpf_last_error()
    eng.close()


def test_exported_symbols_and_constants():
    from grid2op_amd import _capi, engine
    names = ("gpf_set_chronics_cursor", "gpf_upload_cursor_draws", "gpf_get_cursor_state", "gpf_set_cursor_state", "gpf_cursor_device_pointers")
    assert all(n in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), n) for n in names)
    assert _capi.ABI_VERSION == 326 and _capi.N_DEVICE_POINTERS == 34 and _capi.N_CURSOR_POINTERS == 3
    assert engine.CURSOR_STATE_INTS == CR.STATE_INTS == len(engine.CursorState._COLS) == 7 and engine.CursorState._COLS == CR.COLS
    assert (engine.CURSOR_SEQUENTIAL, engine.CURSOR_SAMPLED) == (CR.SEQUENTIAL, CR.SAMPLED)
    assert (engine.CURSOR_FLAG_DRAWS_EXHAUSTED, engine.CURSOR_FLAG_NEXT_POS_WRAPPED) == (CR.FLAG_DRAWS_EXHAUSTED, CR.FLAG_NEXT_POS_WRAPPED)
    D = _capi.GpfCursorDesc
    assert C.sizeof(D) == 80 and (D.order.offset, D.cdf.offset, D.lane_first_row.offset, D.lane_next_pos.offset, D.draw_source.offset, D.lane_base.offset) == (8, 24, 40, 56, 64, 76)
    hdr = open(golden_path("../../include/gridpf.h")).read()
    assert "#define GPF_N_CURSOR_POINTERS 3" in hdr and "#define GPF_CURSOR_STATE_INTS 7" in hdr and "#define GPF_ABI_VERSION 326" in hdr
    st = engine.CursorState.from_rows(np.arange(14, dtype=np.int32).reshape(2, 7))
    assert np.array_equal(st.next_pos, [3, 10]) and np.array_equal(st.rows(), np.arange(14).reshape(2, 7))


def test_sharded_engine_forwards_the_cursor(load_model):
    from stub_engine import StubEngine
    from grid2op_amd.engine import CursorState
    from grid2op_amd.sharding import ShardedEngine

    class Stub(StubEngine):
        def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
            super().__init__(model, n_lanes, device, n_busbar)
            self.calls, self.draws, self.state = [], None, None

        def set_chronics_cursor(self, order=None, policy="sequential", probabilities=None, first_row=0, next_pos=None, seed=None, lane_base=0):
            self.calls.append(dict(order=order, policy=policy, probabilities=probabilities, first_row=first_row, next_pos=next_pos, seed=seed, lane_base=lane_base))

        def upload_cursor_draws(self, draws):
            self.draws = np.asarray(draws)

        def chronics_cursor_state(self, lane0=0, n=None):
            n = self.n_lanes - lane0 if n is None else n
            return CursorState.from_rows(np.tile((1000 * self.device + lane0 + np.arange(n))[:, None], (1, 7)).astype(np.int32))

        def set_chronics_cursor_state(self, state, lane0=0):
            self.state = (lane0, state.rows())

        def cursor_views(self):
            return {"next_pos": self.device}

    m = load_model("l2rpn_case14_sandbox")
    se = ShardedEngine(m, 10, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: Stub(mm, n, dev, nbb))
    first = np.arange(10) % 3
    se.set_chronics_cursor([2, 0, 1], "sampled", [1, 2, 3], first_row=first, next_pos=1, seed=5, lane_base=100)
    for e, (b0, bn) in zip(se.engines, se.blocks):                          # the shard's lane_base makes the shards one engine
        c = e.calls[-1]
        assert c["lane_base"] == 100 + b0 and np.array_equal(c["first_row"], first[b0:b0 + bn]) and c["next_pos"] == 1 and c["seed"] == 5
        assert c["order"] == [2, 0, 1] and c["policy"] == "sampled" and c["probabilities"] == [1, 2, 3]
    se.set_chronics_cursor(False)
    assert all(e.calls[-1]["order"] is False for e in se.engines)
    u = np.arange(20, dtype=np.float64).reshape(10, 2) / 20
    se.upload_cursor_draws(u)
    for e, (b0, bn) in zip(se.engines, se.blocks):
        assert np.array_equal(e.draws, u[b0:b0 + bn])
    want = np.concatenate([1000 * e.device + np.arange(bn) for e, (_, bn) in zip(se.engines, se.blocks)])
    assert np.array_equal(se.chronics_cursor_state(2, 7).pos, want[2:9])
    se.set_chronics_cursor_state(CursorState.from_rows(np.tile(np.arange(7)[:, None], (1, 7)).astype(np.int32)), lane0=2)
    got = np.concatenate([e.state[1][:, 0] for e in se.engines if e.state is not None])
    assert np.array_equal(got, np.arange(7)) and se.engines[0].state[0] == 2
    assert se.cursor_views() == [{"next_pos": e.device} for e in se.engines]


def test_sanitized_stand_alone_cursor_emulator_runs_clean():
    p = subprocess.run([CR.sanitized_program()], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK") and not p.stderr, (p.stdout, p.stderr[-2000:])
