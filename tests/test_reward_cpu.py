"""The environment's rewards of the batched acting path (include/gridpf.h gpf_set_rewards), the parts that need no GPU: the float64
restatement (tests/reward_ref.py) against the episodes recorded from the unmodified reference environment (tests/golden/reward_*.npz)
under the bounds of the reference's own float32 evaluation, the proof that those bounds discriminate, the library's rule core compiled
with g++ (tests/native/reward_emul.cpp) against the restatement at one float32 spacing, the three values outside the reference's domain,
every refusal through a header-only handle, `reward_config` against what the reference's ``initialize`` left, and the routing of
`ShardedEngine`."""
import subprocess

import numpy as np
import pytest

import reward_ref as R
from conftest import golden_path

TAGS = ("case14_topo", "case14_storage", "wcci2022")
SLOTS = [(R.REDISP, [5.0, 1.0e5, -10.0, 0.25, 300.0 / 3600.0]), (R.L2RPN, []), (R.LINES_CAPACITY, []),
         (R.ECONOMIC, [5.0e4, -0.5, 1.5, 300.0 / 3600.0]), (R.GAMEPLAY, [-1.0, 1.0])]


@pytest.fixture(scope="module", params=TAGS)
def recorded(request):
    return dict(np.load(golden_path(f"reward_{request.param}.npz")))


def _steps(fx):
    return [i for i in range(len(fx["done"])) if not fx["is_reset"][i]]


def test_fixtures_cover_the_branches():
    t, s, w = (dict(np.load(golden_path(f"reward_{k}.npz"))) for k in TAGS)
    step = t["is_reset"] == 0
    ill, amb, dn = t["is_illegal"].astype(bool), t["is_ambiguous"].astype(bool), t["done"].astype(bool)
    assert (ill & ~dn).sum() >= 10 and (amb & ~dn).sum() >= 5 and dn.sum() >= 3 and (step & ~ill & ~amb & ~dn).sum() >= 40
    assert (dn & (t["played"] >= int(t["n_table"]))).sum() >= 3                  # episodes ended by the agent's own disconnections
    assert s["failed_redisp"].sum() >= 3 and not s["is_illegal"].any()            # the cancelled redispatch is info's OTHER flag
    for fx in (s, w):
        both = (np.abs(fx["actual_dispatch"]).sum(1) > 0) & (np.abs(fx["storage_power"]).sum(1) > 0) & ~fx["failed_redisp"].astype(bool)
        assert both.sum() >= 1
    assert ((np.abs(s["storage_power"] - s["act_storage"]).max(1) > 0.5) & ~s["failed_redisp"].astype(bool)).sum() >= 1      # _compute_storage clamped a unit
    assert w["gen_p"].shape[1] == 62 and w["load_p"].shape[1] == 91 and w["a_or"].shape[1] == 186 and w["storage_power"].shape[1] == 7


def test_restatement_against_the_recorded_reference(recorded):
    """Every step, every slot.  The reference evaluates in float32 with at most K roundings, each at most 2^-24 of the largest intermediate
    magnitude (reward_ref.bound: K = n_gen + n_load + n_storage + 16 for RedispReward, n_line + 8 for L2RPNReward, derived the same way for
    the other two); the constant branches are exact."""
    fx = recorded
    slots = R.fixture_slots(fx)
    n_cmp = 0
    for i in _steps(fx):
        row, got = R.fixture_row(fx, i), R.fixture_rewards(fx, i)
        for s, (kind, p) in enumerate(slots):
            want = R.value(kind, p, **row)
            if R.constant_branch(kind, row["failed"], row["illegal"], row["ambiguous"]):
                assert want.tobytes() == got[s].tobytes(), (i, s, want, got[s])
            else:
                b = R.bound(kind, p, **row)
                assert abs(float(got[s]) - float(want)) <= b, (i, s, float(got[s]), float(want), b)
                n_cmp += 1
    assert n_cmp >= 30


@pytest.mark.parametrize("tag", TAGS[1:])
def test_the_bound_discriminates(tag):
    """On the steps with dispatch and storage power each wrong formula moves RedispReward by at least 100 bounds.  The requested storage
    power instead of the clamped one is another input only where _compute_storage clamped a unit: those steps are the small grid's.  On
    the 118-substation grid 100 bounds are about 0.25, which takes 69 MW of storage power at the dearest marginal cost (149): the storage
    term needs that much on the step and the requested power would have to exceed it by another 75 MW, but the seven units absorb 84 MW
    in all -- so that episode keeps every unit away from Emax / Emin and requested = clamped on all its steps (asserted below)."""
    fx = dict(np.load(golden_path(f"reward_{tag}.npz")))
    kind, p = R.fixture_slots(fx)[0]
    seen = dict(no_alpha=0, no_storage=0, min_cost=0, requested=0)
    for i in _steps(fx):
        row = R.fixture_row(fx, i)
        if row["illegal"] or not np.abs(row["dispatch"]).sum() > 0 or not np.abs(row["storage"]).sum() > 0:
            continue
        want, b = float(R.value(kind, p, **row)), R.bound(kind, p, **row)
        for v in ("no_alpha", "no_storage", "min_cost"):
            assert abs(float(R.value(kind, p, variant=v, **row)) - want) >= 100 * b, (i, v)
            seen[v] += 1
        if np.abs(fx["storage_power"][i] - fx["act_storage"][i]).max() > 0.5:
            req = dict(row, storage=fx["act_storage"][i])
            assert abs(float(R.value(kind, p, **req)) - want) >= 100 * b, (i, "requested")
            seen["requested"] += 1
    assert all(v >= 1 for k, v in seen.items() if k != "requested"), seen
    if tag == "case14_storage":
        assert seen["requested"] >= 1, seen
    else:
        assert seen["requested"] == 0 and np.abs(fx["storage_power"] - fx["act_storage"]).max() < 1e-5 and float(fx["gen_cost_per_MW"].max()) == 149.0


def _check_emulator(slots, row):
    got, want = R.emul_lane(slots, **row), R.lane_values(slots, **row)
    assert R.spacing_ok(got, want).all(), (got, want)
    for s, (kind, _) in enumerate(slots):
        if R.constant_branch(kind, row["failed"], row["illegal"], row["ambiguous"]):
            assert got[s].tobytes() == want[s].tobytes(), (s, got[s], want[s])


def test_emulator_equals_the_restatement_on_the_recorded_episodes(recorded):
    fx = recorded
    slots = R.fixture_slots(fx)
    for i in _steps(fx):
        _check_emulator(slots, R.fixture_row(fx, i))


def synthetic_row(rng, n, n_sto=None, dispatch=True):
    n_sto = n if n_sto is None else n_sto
    row = dict(gen_p=rng.uniform(-5, 80, n).astype(np.float32), load_p=rng.uniform(1, 60, n).astype(np.float32),
               a_or=rng.uniform(0, 900, n).astype(np.float32), rho=rng.uniform(0, 1.4, n).astype(np.float32), line_status=rng.random(n) > 0.2,
               thermal=rng.uniform(100, 800, n).astype(np.float32), dispatch=rng.uniform(-10, 10, n).astype(np.float32) if dispatch else None,
               storage=rng.uniform(-4, 4, n_sto).astype(np.float32), cost=rng.uniform(0, 90, n).astype(np.float32))
    row["gen_p"][rng.integers(n)] = 10.0             # (a generator that produces: inside the reference's domain)
    return row


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 257])
def test_emulator_equals_the_restatement_on_seeded_rows(n):
    rng = np.random.default_rng(500 + n)
    for rep in range(6):
        row = synthetic_row(rng, n, n_sto=n if rep % 2 else 0, dispatch=rep % 3 != 0)
        for f in range(8):
            _check_emulator(SLOTS, dict(row, failed=bool(f & 1), illegal=bool(f & 2), ambiguous=bool(f & 4)))


def test_values_outside_the_reference_domain():
    """stated in include/gridpf.h; the reference raises or is not defined there, so none is compared with it"""
    rng = np.random.default_rng(9)
    ok = dict(failed=False, illegal=False, ambiguous=False)
    # no generator at gen_p > 0: a quiet NaN
    row = dict(synthetic_row(rng, 7), **ok)
    row["gen_p"] = -np.abs(row["gen_p"])
    for got in (R.emul_lane(SLOTS[:1], **row), R.lane_values(SLOTS[:1], **row)):
        assert np.isnan(got[0])
    assert not np.isnan(R.emul_lane(SLOTS[1:], **row)).any()
    # a zero load sum: the IEEE quotient
    row = dict(synthetic_row(rng, 7), **ok)
    row["load_p"] = np.zeros(7, np.float32)
    sign = {}
    for name, fn in (("emulator", R.emul_lane), ("restatement", R.lane_values)):
        sign[name] = fn(SLOTS[:1], **row)[0]
        assert np.isinf(sign[name])
    assert sign["emulator"] == sign["restatement"]
    # no line connected: what numpy.interp gives LinesCapacityReward for xp = [0, 0]
    row = dict(synthetic_row(rng, 7), **ok)
    row["line_status"] = np.zeros(7, bool)
    numpy_says = np.interp(np.float32(0.0) - 0.0, [np.float32(0.0), 0.0], [np.float32(0.0), np.float32(1.0)])
    assert numpy_says == R.LINES_CAPACITY_NONE == 1.0
    for got in (R.emul_lane(SLOTS[2:3], **row), R.lane_values(SLOTS[2:3], **row)):
        assert got[0] == np.float32(numpy_says)


def test_every_refusal_on_a_header_only_handle(load_model):
    from grid2op_amd.engine import GridPFError, PowerFlowEngine, RW_ECONOMIC, RW_GAMEPLAY, RW_L2RPN, RW_LINES_CAPACITY, RW_REDISP
    m = load_model("l2rpn_case14_sandbox")
    eng = PowerFlowEngine(m, n_lanes=4, device=-1)
    cost = np.full(m.n_gen, 30.0, np.float32)
    good = [(RW_REDISP, [5.0, 1e5, -10.0, 0.0, 1 / 12]), RW_L2RPN, RW_LINES_CAPACITY, (RW_ECONOMIC, [5e4, 0.0, 1.0, 1 / 12]), (RW_GAMEPLAY, [-1.0, 1.0])]
    for fn in (eng.rewards, eng.rewards_eval, eng.reward_views):
        with pytest.raises(GridPFError, match="rewards are off"):
            fn()
    import ctypes as C
    out = np.zeros(8, np.float32)
    for rc in (eng._lib.gpf_get_rewards(eng._h, 0, 1, out.ctypes.data_as(C.POINTER(C.c_float))), eng._lib.gpf_rewards_eval(eng._h, 0, 1, None, None, 0),
               eng._lib.gpf_reward_device_pointers(eng._h, (C.c_void_p * 1)(), 1)):
        assert rc != 0 and b"rewards are off" in eng._lib.gpf_last_error()
    with pytest.raises(GridPFError, match=r"9 slots: outside \[0, GPF_REWARD_MAX_SLOTS = 8\]"):
        eng.set_rewards([RW_L2RPN] * 9)
    for bad in (0, 6, -1, 99):
        with pytest.raises(GridPFError, match=f"slot 1: unknown kind {bad}"):
            eng.set_rewards([RW_L2RPN, bad])
    for s, n_p in ((0, 5), (3, 4), (4, 2)):
        for j in range(n_p):
            for bad in (float("nan"), float("inf"), -float("inf")):
                slots = [x if isinstance(x, int) else (x[0], list(x[1])) for x in good]
                slots[s][1][j] = bad
                with pytest.raises(GridPFError, match=f"slot {s}: parameter {j} is not finite"):
                    eng.set_rewards(slots, cost)
    for s, j in ((0, 4), (3, 3)):
        for bad in (0.0, -1 / 12):
            slots = [x if isinstance(x, int) else (x[0], list(x[1])) for x in good]
            slots[s][1][j] = bad
            with pytest.raises(GridPFError, match=f"slot {s}: dts must be positive"):
                eng.set_rewards(slots, cost)
    for k in (0, 3):
        with pytest.raises(GridPFError, match="need gen_cost_per_mw"):
            eng.set_rewards([good[k]])
    for bad in (-1.0, float("nan"), float("inf")):
        c = cost.copy()
        c[2] = bad
        with pytest.raises(GridPFError, match=r"gen_cost_per_mw\[2\] is negative or not finite"):
            eng.set_rewards(good, c)
    with pytest.raises(GridPFError, match="no HIP device"):               # a good call gets as far as the missing device
        eng.set_rewards(good, cost)
    with pytest.raises(GridPFError, match="no HIP device"):               # the kinds without costs need no table
        eng.set_rewards([RW_L2RPN, RW_LINES_CAPACITY, (RW_GAMEPLAY, [-1.0, 1.0])])
    with pytest.raises(GridPFError, match="rewards are off"):             # ... and leaves rewards off
        eng.rewards()
    eng.set_rewards(None)                                                 # off is always possible
    eng.set_rewards([])
    eng.close()


def test_reward_config_derives_what_initialize_left(recorded):
    from grid2op_amd import engine
    fx = recorded
    kw = dict(gen_cost_per_MW=fx["gen_cost_per_MW"], gen_pmax=fx["gen_pmax"], delta_time_seconds=float(fx["delta_time_seconds"]))
    want = R.fixture_slots(fx)
    rd = engine.reward_config("RedispReward", **kw)
    assert rd["kind"] == engine.RW_REDISP == R.REDISP and rd["p"] == want[0][1]
    assert rd["max_regret"] == float(fx["redisp_max_regret"]) and rd["reward_max"] == float(fx["redisp_reward_max"])
    ec = engine.reward_config(engine.RW_ECONOMIC, **kw)
    assert ec["p"] == want[3][1] and ec["worst_cost"] == float(fx["economic_worst_cost"])
    gp = engine.reward_config("GameplayReward")
    assert gp["p"] == want[4][1] == [-1.0, 1.0]
    assert engine.reward_config("L2RPNReward") == dict(kind=R.L2RPN, p=[]) and engine.reward_config("LinesCapacityReward")["kind"] == R.LINES_CAPACITY
    assert engine.reward_config("RedispReward", alpha_redisph=2.0, reward_illegal_ambiguous=-1.0, **kw)["p"][:4:3] == [2.0, -1.0]
    with pytest.raises(ValueError, match="unknown meta-parameters"):
        engine.reward_config("GameplayReward", alpha=1.0)
    with pytest.raises(ValueError, match="needs gen_cost_per_MW"):
        engine.reward_config("RedispReward")
    with pytest.raises(ValueError, match="unknown reward kind"):
        engine.reward_config(17)


def test_exported_symbols_and_constants():
    from grid2op_amd import _capi, engine
    names = ("gpf_set_rewards", "gpf_get_rewards", "gpf_rewards_eval", "gpf_reward_device_pointers")
    assert all(n in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), n) for n in names)
    assert _capi.ABI_VERSION == 326 and _capi.N_DEVICE_POINTERS == 34 and _capi.N_REWARD_POINTERS == 1 and engine.REWARD_MAX_SLOTS == 8
    import ctypes as C
    assert C.sizeof(_capi.GpfRewardSlot) == C.sizeof(R.Slot) == 56
    assert (engine.RW_REDISP, engine.RW_L2RPN, engine.RW_LINES_CAPACITY, engine.RW_ECONOMIC, engine.RW_GAMEPLAY) == R.KINDS


def test_sharded_engine_forwards_the_rewards(load_model):
    from stub_engine import StubEngine
    from grid2op_amd.sharding import ShardedEngine

    class Stub(StubEngine):
        def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
            super().__init__(model, n_lanes, device, n_busbar)
            self.calls, self.n_lanes_ = [], n_lanes

        def set_rewards(self, slots, gen_cost_per_MW=None):
            self.calls.append(("set", slots, gen_cost_per_MW))

        def rewards(self, lane0=0, n=None):
            n = self.n_lanes_ - lane0 if n is None else n
            return np.tile((1000 * self.device + lane0 + np.arange(n))[:, None], (1, 2)).astype(np.float32)

        def rewards_eval(self, lane0=0, n=None, flags=None, out=None):
            self.calls.append(("eval", lane0, n, flags, out))
            return ("eval", self.device, lane0, n)

        def reward_views(self):
            return {"rewards": self.device}

    m = load_model("l2rpn_case14_sandbox")
    se = ShardedEngine(m, 10, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: Stub(mm, n, dev, nbb))
    se.set_rewards([2, 3], None)
    assert all(e.calls[-1] == ("set", [2, 3], None) for e in se.engines)
    want = np.concatenate([1000 * e.device + np.arange(bn) for e, (_, bn) in zip(se.engines, se.blocks)])
    assert np.array_equal(se.rewards(2, 7)[:, 0], want[2:9].astype(np.float32)) and se.rewards().shape == (10, 2)
    parts = se._parts(2, 7)
    got = se.rewards_eval(2, 7, flags=[f"f{i}" for i in range(len(parts))])
    assert got == [("eval", e.device, l0, k) for e, l0, k, _ in parts]
    for i, (e, l0, k, _) in enumerate(parts):
        assert e.calls[-1] == ("eval", l0, k, f"f{i}", None)
    with pytest.raises(ValueError, match="shards intersect the range"):
        se.rewards_eval(0, 10, out=[None])
    assert se.reward_views() == [{"rewards": e.device} for e in se.engines]


def test_sanitized_stand_alone_reward_emulator_runs_clean():
    p = subprocess.run([R.sanitized_program()], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK") and not p.stderr, (p.stdout, p.stderr[-2000:])
