"""CPU conditions of the parity tests of `gpf_redispatch` (tests/test_gpu_redispatch.py): (1) every seeded program of
tests/redispatch_cases.py reaches the branch it names, classified from the reference alone, and no branch x generator-count cell is empty;
(2) the closed-form reference (tests/redispatch_ref.py) satisfies the KKT conditions, agrees with the oracle's bisection and is never worse
than the recorded SLSQP results; (3) the inputs DISCRIMINATE: dropping a feature of the kernel moves the answer by more than 100 times the GPU
tolerance; (4) the capacity refusal and `ShardedEngine.redispatch`'s routing, without a device."""
import numpy as np
import pytest

from oracle.redispatch_oracle import objective_mw, solve_exact

from redispatch_cases import BASE_GRID, BRANCHES, COUNTS, MARGIN, branch_exists, programs, recorded_calls, resized_model, solved
from redispatch_ref import L, dispatch_ref, feasibility_terms, spacing32
from stub_engine import StubEngine

KKT_TOL = 1e-9                   # MW
def classify(p, lim, ok, after, q, info):
    """The branches a program reaches, from the reference's terms alone."""
    f = feasibility_terms(p.new_p, p.prev_p, p.actual, p.target, p.rhs, lim)
    part, red = f["part"], lim["redispatchable"].astype(bool)
    tags = set()
    if not part.any():
        tags.add("empty_G_rhs0" if (p.rhs == 0.0 and ok and np.array_equal(after, p.actual)) else "empty_G_rhs_nonzero" if (p.rhs != 0.0 and not ok) else "?")
    elif not ok:
        tags.add("refused_move_up" if f["sum_move"] > f["s_up"] else "refused_move_down" if f["sum_move"] < f["s_down"] else "?")
    else:
        tags.add(info["branch"])
        if not p.modified[part].any():
            tags.add("nomod")
    if ((p.new_p > 0) & ~red).any() and np.array_equal(after[~red], p.actual[~red]):
        tags.add("not_redispatchable")
    out = red & (p.new_p == 0.0) & (np.abs(p.actual) < 1e-7) & (p.target == p.actual)
    if out.any() and not part[out].any() and np.array_equal(after[out], p.actual[out]):
        tags.add("zero_new_p")
    if p.exact and part.any():
        quarter = L(0.25)
        on_edge = f["sum_move"] in (f["s_up"], f["s_down"]) and ok
        beyond = (f["sum_move"] - f["s_up"] == quarter or f["s_down"] - f["sum_move"] == quarter) and not ok
        wide = (L(p.rhs) in (f["s_hi"], f["s_lo"])) and lim["eps_poly"] > 0 and not ok
        if on_edge or beyond or wide:
            tags.add("boundary_exact")
    return tags


def test_every_program_reaches_its_branch_and_no_cell_is_empty():
    for n in COUNTS:
        seen = {b: 0 for b in BRANCHES}
        for rec in solved(n):
            tags = classify(*rec)
            assert rec[0].branch in tags, (rec[0].id, tags)
            for t in tags & set(BRANCHES):
                seen[t] += 1
        for b in BRANCHES:
            assert (seen[b] >= 1) == branch_exists(b, n), (n, b, seen[b])
        assert len(solved(n)) <= 300                                       # a few hundred lanes per count at most


@pytest.mark.parametrize("n", COUNTS)
def test_boundary_exact_programs(n):
    """Equality is accepted (the comparisons are strict), a quarter MW beyond is refused, rhs == s_hi with eps_poly > 0 is refused by the FIRST
    check; with eps_poly = 0 the accepted lanes end exactly on the bound, with eps_poly = 2**-13 within |G| eps_poly / 2 of it."""
    kinds = set()
    for p, lim, ok, after, q, info in solved(n):
        if p.branch != "boundary_exact":
            continue
        for a in (p.new_p, p.prev_p, p.actual, p.target, lim["pmin"], lim["pmax"], lim["ramp_up"], lim["ramp_down"]):
            assert np.array_equal(a * 4, np.round(a * 4))
        f = feasibility_terms(p.new_p, p.prev_p, p.actual, p.target, p.rhs, lim)
        tag = "wide_eq" if p.id.endswith("_wide_eq") else p.id.split("_")[-1]
        side = "hi" if "_hi_" in p.id else "lo"
        kinds.add((p.lim, side, tag))
        if tag == "wide_eq":
            assert not ok and L(p.rhs) == (f["s_hi"] if side == "hi" else f["s_lo"]) and f["sum_move"] != (f["s_up"] if side == "hi" else f["s_down"])
        elif tag == "eq":
            assert ok and f["sum_move"] == (f["s_up"] if side == "hi" else f["s_down"])
            bound = p.actual + q[side]
            if lim["eps_poly"] == 0.0:
                assert p.bound == side and np.array_equal(after, bound) and L(p.rhs) == (f["s_hi"] if side == "hi" else f["s_lo"])
            else:
                slack = n * 0.5 * lim["eps_poly"]
                assert p.bound is None and (np.abs(after - bound) <= slack + 1e-12).all()
        else:
            assert tag == "beyond" and not ok and np.array_equal(after, p.actual)
    assert len(kinds) == 10, kinds               # {dyadic: eq, beyond, wide_eq; dyadic0: eq, beyond} x {hi, lo}


def test_margins_of_the_feasibility_checks():
    """Wave reduction and numpy sum in different orders: `ok` is only defined when the compared sums are not within rounding of each other."""
    n_checked = 0
    for n in COUNTS:
        for p, lim, ok, after, q, info in solved(n):
            if p.exact:
                continue
            f = feasibility_terms(p.new_p, p.prev_p, p.actual, p.target, p.rhs, lim)
            for a, b in (("sum_move", "s_up"), ("sum_move", "s_down")):
                assert abs(f[a] - f[b]) >= MARGIN, (p.id, a, b)
            assert abs(L(p.rhs) - f["s_lo"]) >= MARGIN and abs(L(p.rhs) - f["s_hi"]) >= MARGIN, p.id
            if ok and info["branch"] in ("up", "down", "share") and p.id.split("_")[-1] != "left":
                # ... and the branch itself is chosen with the same margin (the answer is continuous across it, but the claim is not)
                d = L(p.rhs) - info["s0"]
                assert abs(d - info["f_hi"]) >= MARGIN and abs(d - info["f_lo"]) >= MARGIN, p.id
            n_checked += 1
    assert n_checked >= 300


def test_inputs_have_the_shapes_the_kernel_can_get_wrong():
    for n in COUNTS:
        recs = solved(n)
        lim = programs(n)[1]["main"]
        mod_at, free_at, last_mod, frac_actual, pmax_lim = set(), set(), False, [], 0
        for p, lm, ok, after, q, info in recs:
            assert (np.abs(p.prev_p - p.new_p) < np.minimum(lm["ramp_up"], lm["ramp_down"])).all(), p.id
            if not ok or q is None or not q["part"].any():
                continue
            part = q["part"]
            idx = np.nonzero(part)[0]
            mod_at.update(idx[q["modified_part"]].tolist())
            if q["modified_part"].any():
                free_at.update(idx[~q["modified_part"]].tolist())
            last_mod |= bool(part[n - 1] and p.modified[n - 1])
            if p.lim == "main" and len(idx) >= 20:
                frac_actual.append((p.actual[part] != 0).mean())
            incr = p.new_p - (p.prev_p - p.actual)
            pmax_lim += int(((lm["pmax"] - p.new_p - p.actual < lm["ramp_up"] - incr) & part).sum())
        assert last_mod, n
        assert pmax_lim >= 1, n
        if n > 64:
            assert max(mod_at) >= 64 and max(free_at) >= 64, n
            assert len([i for i in mod_at if i >= 64]) >= 1 and len([i for i in free_at if i >= 64]) >= 1
        if n > 192:
            assert len([i for i in mod_at if i >= 192]) >= 1 and len([i for i in free_at if i >= 192]) >= 1
        if n >= 63:
            assert (lim["ramp_up"] != lim["ramp_down"]).sum() >= 3 and 0.35 < np.mean(frac_actual) < 0.65, n


def _kkt(pid, lim, q, info):
    x = info["x"].astype(L)
    lo, hi = info["lo"].astype(L), info["hi"].astype(L)
    w, tv, mod = q["w"].astype(L), q["tv"].astype(L), q["mod"]
    assert abs(x.sum() - L(q["rhs"])) <= KKT_TOL, pid
    assert (x >= lo - KKT_TOL).all() and (x <= hi + KKT_TOL).all(), pid
    at_lo, at_hi = x <= lo + KKT_TOL, x >= hi - KKT_TOL
    inside = ~at_lo & ~at_hi
    # the multiplier of the sum constraint, in units of x of generator i: u_i(lam) = t_i - lam / (2 w_i)
    lam_i = -2 * w * (x - tv)
    lam_max = np.min(np.where(mod & at_hi, 2 * w * (tv - hi + KKT_TOL), np.inf))        # at hi: t_i - lam / (2 w_i) >= hi_i
    lam_min = np.max(np.where(mod & at_lo, 2 * w * (tv - lo - KKT_TOL), -np.inf))       # at lo: t_i - lam / (2 w_i) <= lo_i
    if (mod & inside).any():
        lam = lam_i[mod & inside][0]
        assert (np.abs((lam_i - lam) / (2 * w))[mod & inside] <= KKT_TOL).all(), pid  # one value of 2 w_i (x_i - t_i), measured in MW
        lam_lo_ok = lam_hi_ok = lam
    else:
        lam_lo_ok, lam_hi_ok = lam_min, lam_max
        assert lam_min <= lam_max, pid
    slack = 2 * w.max() * KKT_TOL
    assert lam_hi_ok <= lam_max + slack and lam_lo_ok >= lam_min - slack, pid
    free = ~mod
    if free.any():
        if at_hi[free].all() and lam_lo_ok <= slack and info["branch"] == "up":
            return
        if at_lo[free].all() and lam_hi_ok >= -slack and info["branch"] == "down":
            return
        # lambda = 0: the modified generators at their clipped targets, the free ones on the ray x_i = alpha / w_i or at the bound it crosses
        assert lam_lo_ok <= slack and lam_hi_ok >= -slack, pid
        assert (np.abs(x - np.clip(tv, lo, hi))[mod] <= KKT_TOL).all(), pid
        a_i = x * w
        fi = free & inside
        a_max = np.min(np.where(free & at_lo, (lo + KKT_TOL) * w, np.inf))              # at lo: alpha / w_i <= lo_i
        a_min = np.max(np.where(free & at_hi, (hi - KKT_TOL) * w, -np.inf))
        if fi.any():
            alpha = a_i[fi][0]
            assert (np.abs((a_i - alpha) / w)[fi] <= KKT_TOL).all(), pid
            assert a_min - KKT_TOL * w.max() <= alpha <= a_max + KKT_TOL * w.max(), pid
        else:
            assert a_min <= a_max, pid


def test_closed_form_satisfies_kkt_and_agrees_with_the_bisection():
    n_checked, branches = 0, set()
    for n in COUNTS:
        for p, lim, ok, after, q, info in solved(n):
            if not ok or not q["part"].any():
                continue
            _kkt(p.id, lim, q, info)
            assert np.abs(info["x"] - solve_exact(q, lim["eps_poly"])).max() <= KKT_TOL, p.id
            branches.add(info["branch"])
            n_checked += 1
    assert branches == {"up", "down", "share", "nofree"} and n_checked >= 250


ENVS = ["l2rpn_case14_sandbox", "l2rpn_wcci_2022_dev", "educ_case14_storage"]


@pytest.mark.parametrize("env", ENVS)
def test_closed_form_on_the_recorded_calls_is_never_worse_than_slsqp(env):
    """The recorded x is stored in float32 and satisfies the constraints to ~1e-6 MW only; a point that violates them by v can undercut the
    constrained optimum by at most |gradient|_max v (first order, the objective is convex) -- that, and nothing else, is allowed."""
    c, lim = recorded_calls(env)
    for k in range(len(c["ok"])):
        ok, after, q, info = dispatch_ref(c["new_p"][k], c["prev"][k], c["actual"][k], c["target"][k], c["modified"][k], c["rhs"][k], lim, with_info=True)
        assert ok and c["ok"][k]
        _kkt(f"{env}[{k}]", lim, q, info)
        assert np.abs(info["x"] - solve_exact(q, lim["eps_poly"])).max() <= KKT_TOL
        x_s = (c["actual_after"][k] - c["actual"][k])[q["part"]]
        viol = abs(x_s.sum() - q["rhs"]) + np.maximum(info["lo"] - x_s, 0).sum() + np.maximum(x_s - info["hi"], 0).sum()
        grad = np.abs(2 * q["w"] * (x_s - q["tv"]))[q["mod"]].max()
        assert objective_mw(q, info["x"]) <= objective_mw(q, x_s) + grad * viol + 1e-12, (k, objective_mw(q, info["x"]), objective_mw(q, x_s), viol)


def test_dropping_a_feature_moves_the_answer_by_100_tolerances():
    moved = {"nomod_as_nothing": 0, "free_at_the_wrong_bound": 0, "generators_from_64_ignored": 0}
    wanted = {"nomod_as_nothing": 0, "free_at_the_wrong_bound": 0, "generators_from_64_ignored": 0}
    for n in COUNTS:
        progs, lims = programs(n)
        for p, lim, ok, after, q, info in solved(n):
            if not ok or not q["part"].any():
                continue
            bar = 100.0 * spacing32(after)
            part = q["part"]
            if p.branch == "nomod":                              # "no modified generator: nothing to do"
                wanted["nomod_as_nothing"] += 1
                moved["nomod_as_nothing"] += int((np.abs(p.actual - after) > bar).any())
            free = np.nonzero(part)[0][~q["mod"]]
            if info["branch"] in ("up", "down") and len(free):   # free generators at lo where hi is right (and the other way round)
                wanted["free_at_the_wrong_bound"] += 1
                other = after.copy()
                other[free] = p.actual[free] + (info["lo"] if info["branch"] == "up" else info["hi"])[~q["mod"]]
                moved["free_at_the_wrong_bound"] += int((np.abs(other - after)[free] > bar[free]).all())
            if n > 64 and p.lim == "main":                       # only the generators of lane slot q = 0 are seen
                wanted["generators_from_64_ignored"] += 1
                lim64 = {k: (v[:64] if isinstance(v, np.ndarray) else v) for k, v in lim.items()}
                ok64, after64 = dispatch_ref(p.new_p[:64], p.prev_p[:64], p.actual[:64], p.target[:64], p.modified[:64], p.rhs, lim64)
                moved["generators_from_64_ignored"] += int((not ok64) or (np.abs(after64 - after[:64]) > bar[:64]).any())
    for k in moved:
        assert wanted[k] >= 20 and moved[k] == wanted[k], (k, moved[k], wanted[k])


def test_the_tolerance_is_meaningful_on_every_compared_entry():
    """One float32 spacing at |ref| only bounds the final cast when it is far above the kernel's float64 rounding (a few ulps of a sum of a few
    hundred MW, spread over the generators inside their bounds: ~1e-14 MW): every entry the solver moves is either exact by construction
    (dyadic data) or at least 1e-5 MW in magnitude, where the spacing is 9e-13 MW."""
    for n in COUNTS:
        for p, lim, ok, after, q, info in solved(n):
            if not ok or not q["part"].any() or p.exact:
                continue
            x = np.zeros(n)
            x[q["part"]] = info["x"]
            exact_entry = (x == 0.0) | (info["branch"] == "nofree") | ((info["branch"] == "share") & (p.id.endswith("zero_left")))
            assert (np.abs(after) >= 1e-5)[~exact_entry].all(), (p.id, np.abs(after)[~exact_entry].min())


def test_more_than_256_generators_are_refused_before_any_device_call(load_model):
    from grid2op_amd._capi import GridPFError
    from grid2op_amd.engine import PowerFlowEngine
    base = load_model(BASE_GRID)
    for n in (1, 65, 256, 257):
        m = resized_model(base, n)
        assert m.n_gen == n and m.gen_slack.sum() == 1 and m.dim_topo == base.dim_topo + n - base.n_gen
        assert len(set(m.gen_pos_topo_vect.tolist())) == n
        eng = PowerFlowEngine(m, n_lanes=4, device=-1)                       # header-only handle
        try:
            if n == 257:
                lim = programs(256)[1]["main"]
                ext = lambda a: np.concatenate([a, a[:1]])  # noqa: E731
                with pytest.raises(GridPFError, match="more than 256 generators"):
                    eng.set_gen_limits(ext(lim["pmin"]), ext(lim["pmax"]), ext(lim["ramp_up"]), ext(lim["ramp_down"]), ext(lim["redispatchable"]))
        finally:
            eng.close()


class _RedispStub(StubEngine):
    """StubEngine + `redispatch`: records what arrives and answers with rows that name the device and the local lane."""
    def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
        super().__init__(model, n_lanes, device, n_busbar)
        self.calls = []

    def set_gen_limits(self, *a, **kw):
        self.calls.append(("limits", a, kw))

    def redispatch(self, new_p, prev_p, actual, target, modified, rhs, lane0=0, apply=False):
        n = len(new_p)
        assert 0 <= lane0 and lane0 + n <= self.n_lanes and np.shape(rhs) == (n,)
        self.calls.append(("redispatch", [np.array(a) for a in (new_p, prev_p, actual, target, modified)], np.array(rhs), lane0, apply))
        after = np.zeros((n, self.model.n_gen), np.float32)
        after[:, 0] = 1000 * self.device + lane0 + np.arange(n)
        return (lane0 + np.arange(n)) % 2 == 0, after


def test_sharded_redispatch_routes_rows_to_their_engines(load_model):
    from grid2op_amd.sharding import ShardedEngine
    m = load_model("l2rpn_case14_sandbox")
    se = ShardedEngine(m, 37, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: _RedispStub(mm, n, dev, nbb))
    assert se.blocks == [(0, 13), (13, 12), (25, 12)]
    se.set_gen_limits(1, 2, 3, 4, 5, eps_poly=1e-3)
    assert all(e.calls == [("limits", (1, 2, 3, 4, 5), dict(eps_poly=1e-3))] for e in se.engines)
    lane0, n = 9, 20                                            # lanes 9 .. 28: across both shard borders
    rng = np.random.default_rng(5)
    rows = [rng.standard_normal((n, m.n_gen)) for _ in range(4)] + [rng.random((n, m.n_gen)) < 0.5]
    rhs = rng.standard_normal(n)
    ok, after = se.redispatch(*rows, rhs, lane0=lane0, apply=True)
    expect = [(0, 9, 4, 0), (1, 0, 12, 4), (2, 0, 4, 16)]       # device, local lane0, count, offset into the caller's rows
    for (dev, l0, k, off), e in zip(expect, se.engines):
        (kind, got, got_rhs, got_l0, got_apply), = [c for c in e.calls if c[0] == "redispatch"]
        assert e.device == dev and got_l0 == l0 and got_apply is True
        for a, b in zip(got, rows):
            assert np.array_equal(a, b[off:off + k])
        assert np.array_equal(got_rhs, rhs[off:off + k])
    glob = lane0 + np.arange(n)
    dev_of = np.array([0 if g < 13 else 1 if g < 25 else 2 for g in glob])
    local = glob - np.array([0, 13, 25])[dev_of]
    assert after.shape == (n, m.n_gen) and np.array_equal(after[:, 0], (1000 * dev_of + local).astype(np.float32))      # global order
    assert np.array_equal(ok, local % 2 == 0)
    # a scalar rhs is broadcast; a range inside one shard reaches that shard only; apply defaults to False
    for e in se.engines:
        e.calls.clear()
    ok, after = se.redispatch(*[r[:5] for r in rows], 0.75, lane0=14)
    assert [len(e.calls) for e in se.engines] == [0, 1, 0]
    _, _, got_rhs, got_l0, got_apply = se.engines[1].calls[0]
    assert np.array_equal(got_rhs, np.full(5, 0.75)) and got_l0 == 1 and got_apply is False and ok.shape == (5,)
    with pytest.raises(ValueError):
        se.redispatch(*rows, rhs, lane0=20)
