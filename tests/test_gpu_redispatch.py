"""GPU parity of `gpf_redispatch` (gridpf_redispatch.hpp) with the closed-form reference (tests/redispatch_ref.py) on the seeded programs of
tests/redispatch_cases.py: 1 .. 256 generators, every branch of the kernel, both refusals, exact boundaries.  The conditions the inputs
meet are proven without a GPU in tests/test_redispatch_ref_cpu.py.

Tolerance: `after` against float32(reference) within ONE float32 spacing at that magnitude.  The kernel works in float64 and its bisections
leave 2^-64 of a bracket of a few hundred MW, so the only rounding that counts is the final cast, which may fall on the other side of a tie.
Refused lanes and generators outside G return float32(actual) bit for bit."""
import numpy as np
import pytest

from redispatch_cases import BASE_GRID, COUNTS, programs, recorded_calls, resized_model, solved, stacked
from redispatch_ref import dispatch_ref, feasibility_terms, spacing32

pytestmark = pytest.mark.gpu


def _set_limits(eng, lim):
    eng.set_gen_limits(lim["pmin"], lim["pmax"], lim["ramp_up"], lim["ramp_down"], lim["redispatchable"], eps_poly=lim["eps_poly"])


def spacings(got, ref):
    """|got - float32(ref)| in units of the float32 spacing at |float32(ref)|"""
    return np.abs(got.astype(np.float64) - np.float32(ref).astype(np.float64)) / spacing32(ref)


def _check(recs, ok, after, worst):
    """One call's results against the reference records of its lanes; `worst`: branch -> largest deviation in spacings."""
    for k, (p, lim, ok_ref, after_ref, q, info) in enumerate(recs):
        assert bool(ok[k]) == ok_ref, p.id
        if not ok_ref:
            assert np.array_equal(after[k], p.actual.astype(np.float32)), p.id                  # refused: actual, bit for bit
            continue
        part = q["part"]
        assert np.array_equal(after[k][~part], p.actual[~part].astype(np.float32)), p.id       # outside G: untouched
        dev = spacings(after[k], after_ref)
        worst[p.branch] = max(worst.get(p.branch, 0.0), float(dev.max()))
        assert (dev <= 1.0).all(), (p.id, float(dev.max()), int(dev.argmax()), after[k][dev.argmax()], after_ref[dev.argmax()])
        if p.bound is not None:                                                                 # boundary_exact, eps_poly = 0: ON the bound
            bound = np.zeros(p.n_gen)
            bound[part] = q[p.bound]
            assert np.array_equal(after[k], (p.actual + bound).astype(np.float32)), p.id


@pytest.mark.parametrize("n_gen", COUNTS)
def test_every_branch_matches_the_closed_form(n_gen, load_model):
    from grid2op_amd.engine import PowerFlowEngine
    progs, lims = programs(n_gen)
    recs = solved(n_gen)
    m = resized_model(load_model(BASE_GRID), n_gen)
    n_main = sum(p.lim == "main" for p in progs)
    eng = PowerFlowEngine(m, n_lanes=2 * n_main, device=0)
    worst = {}
    try:
        for key in lims:                                           # main first: the largest call, then smaller ones on the same buffers
            sel = [r for r in recs if r[0].lim == key]
            rows = stacked([r[0] for r in sel])
            _set_limits(eng, lims[key])
            ok, after = eng.redispatch(*rows)
            _check(sel, ok, after, worst)
            # the same lanes in another order: bit-identical rows (no state across lanes, rows indexed by k * n_gen only)
            perm = np.random.default_rng(n_gen).permutation(len(sel))
            ok_p, after_p = eng.redispatch(*[a[perm] for a in rows])
            assert np.array_equal(ok_p, ok[perm]) and np.array_equal(after_p.view(np.uint32), after[perm].view(np.uint32)), key
            if key == "main":
                # a larger call regrows the buffers (the ok bytes sit behind the mask at an offset that depends on n), then a smaller one
                twice = [np.concatenate([a, a[::-1]]) for a in rows]
                ok2, after2 = eng.redispatch(*twice)
                assert np.array_equal(ok2, np.concatenate([ok, ok[::-1]]))
                assert np.array_equal(after2.view(np.uint32), np.concatenate([after, after[::-1]]).view(np.uint32))
                ok3, after3 = eng.redispatch(*[a[5:8] for a in rows])
                assert np.array_equal(ok3, ok[5:8]) and np.array_equal(after3.view(np.uint32), after[5:8].view(np.uint32))
    finally:
        eng.close()
    print(f"n_gen = {n_gen}: worst |after - float32(ref)| in float32 spacings, per branch: "
          + ", ".join(f"{b} {v:.2f}" for b, v in sorted(worst.items())))


def test_sharded_engine_on_one_device_returns_the_same_bits(load_model):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.sharding import ShardedEngine
    n_gen = 65
    recs = [r for r in solved(n_gen) if r[0].lim == "main"]
    lim = programs(n_gen)[1]["main"]
    rows = stacked([r[0] for r in recs])
    n = len(recs)
    m = resized_model(load_model(BASE_GRID), n_gen)
    one = PowerFlowEngine(m, n_lanes=n + 6, device=0)
    se = ShardedEngine(m, n + 6, devices=[0, 0])
    try:
        _set_limits(one, lim)
        _set_limits(se, lim)
        b0, bn = se.blocks[1]
        assert 3 < b0 < 3 + n                                        # lanes 3 .. 3 + n - 1 lie across the shard border
        ok, after = one.redispatch(*rows, lane0=3)
        ok_s, after_s = se.redispatch(*rows, lane0=3)
        assert ok.any() and not ok.all()
        assert np.array_equal(ok_s, ok) and np.array_equal(after_s.view(np.uint32), after.view(np.uint32))
    finally:
        one.close()
        for e in se.engines:
            e.close()


def test_lane0_and_apply_install_the_dispatch_of_the_accepted_lanes_only(load_model, load_npz):
    """`redispatch(..., lane0=L, apply=True)` on a middle range of lanes, then one `step`: the non-slack generators produce the chronics row
    plus the returned dispatch on the accepted lanes, the chronics row alone outside the range, and the chronics row plus the dispatch an
    EARLIER apply installed on the refused lanes (left untouched, not zeroed)."""
    from test_gpu_multistep import _setup
    B, L, n, t = 12, 3, 6, 5
    m, ch, eng, tab, off, scale = _setup(load_model, load_npz, "l2rpn_case14_sandbox", B)
    _, lim = recorded_calls("l2rpn_case14_sandbox")
    assert lim["redispatchable"][[0, 1]].all() and not m.gen_slack[[0, 1]].any()
    T = tab.shape[0]
    lanes = L + np.arange(n)
    new_p = ch["prod_p"][(t + off[lanes]) % T].astype(np.float64)
    chron_prev = ch["prod_p"][(t - 1 + off[lanes]) % T].astype(np.float64)
    zero = np.zeros((n, m.n_gen))
    mod = np.zeros((n, m.n_gen), bool)
    mod[:, [0, 1]] = True

    def ref(actual, target, rhs):
        return zip(*[dispatch_ref(new_p[k], chron_prev[k] + actual[k], actual[k], target[k], mod[k], rhs[k], lim) for k in range(n)])

    try:
        _set_limits(eng, lim)
        # first apply: every lane of the range accepted, a distinct dispatch per lane (generator 0 up, generator 1 down, 1 .. 4.75 MW)
        amount = 1.0 + 0.75 * np.arange(n)
        target0 = zero.copy()
        target0[:, 0], target0[:, 1] = amount, -amount
        rhs0 = np.full(n, 0.5)
        ok0, after0 = eng.redispatch(new_p, chron_prev, zero, target0, mod, rhs0, lane0=L, apply=True)
        ok0_ref, after0_ref = ref(zero, target0, rhs0)
        assert ok0.all() and all(ok0_ref)
        assert (spacings(after0, np.array(after0_ref)) <= 1.0).all()
        # second apply: even lanes ask for 1.5 MW more and are accepted, odd lanes are refused (3 MW more than the generators can move)
        actual1 = after0.astype(np.float64)
        target1 = actual1.copy()
        target1[:, 0] += 1.5
        target1[:, 1] -= 1.5
        rhs1 = np.full(n, -0.25)
        for k in range(1, n, 2):
            f = feasibility_terms(new_p[k], chron_prev[k] + actual1[k], actual1[k], target1[k], 0.0, lim)
            rhs1[k] = float(f["s_up"] - f["sum_move"]) + 3.0
        ok1, after1 = eng.redispatch(new_p, chron_prev + actual1, actual1, target1, mod, rhs1, lane0=L, apply=True)
        ok1_ref, after1_ref = ref(actual1, target1, rhs1)
        assert np.array_equal(ok1, np.array(ok1_ref)) and np.array_equal(ok1, np.arange(n) % 2 == 0)
        assert (spacings(after1, np.array(after1_ref)) <= 1.0).all()
        assert np.array_equal(after1[~ok1], after0[~ok1])
        assert np.abs(after1 - after0)[ok1][:, [0, 1]].min() > 0.5 and np.abs(after0)[:, [0, 1]].min() > 0.5
        eng.step(t)
        r = eng.results()
        assert r.converged.all()
        delta = np.zeros((B, m.n_gen), np.float32)
        delta[lanes] = np.where(ok1[:, None], after1, after0)
        ns = ~m.gen_slack
        expect = (ch["prod_p"][(t + off) % T].astype(np.float32) + delta).astype(np.float64)
        err = np.abs(r.gen_p.astype(np.float64) - expect)[:, ns]
        assert (err <= (2e-4 + 5e-6 * np.abs(expect))[:, ns]).all(), float(err.max())          # tolerance of test_gpu_parity._compare
    finally:
        eng.close()
