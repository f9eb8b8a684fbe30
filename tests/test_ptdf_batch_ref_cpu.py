"""CPU conditions of the parity tests of `gpf_ptdf_build_batch` (tests/test_gpu_ptdf_batch_parity.py), on the oracle alone: (1) every case
delivers what it claims -- the reduced dimensions, the statuses, ragged classes, the special LODF columns; (2) the LODF reference
(tests/ptdf_batch_ref.py) agrees with brute force: the oracle's DC power flow with the line forced off; (3) the kernels' `1e-8` switch on
|1 - H_kk| decides nothing on these inputs (no in-service line within [1e-10, 1e-4]); (4) B' of every class is well conditioned and a
pivot-free float64 Gauss-Jordan -- the kernels' algorithm without tiles -- reproduces `ptdf()` to 1 % of the PTDF bar, so the bar tests
the kernel, not the conditioning; (5) the inputs discriminate: one split fewer moves PTDF entries by >= 100 bars."""
import numpy as np
import pytest

from oracle.pf_oracle import element_buses, ptdf, solve

from ptdf_batch_cases import CASE_IDS, NR_CLAIMS, batch_cases, class_reference, n_blocks
from ptdf_batch_ref import PTDF_BAR, lodf_tolerance, ptdf_by_gauss_jordan, reduced_dim, reduced_matrix, state_of, verdict, without_line


def _case(cid, load_model):
    c = batch_cases(load_model)[cid]
    return c, c.model(load_model)


def _lane_of(c, build, i):
    return int(np.nonzero(c.builds[build] == i)[0][0])


def test_the_case_list_is_complete(load_model):
    assert sorted(batch_cases(load_model)) == sorted(CASE_IDS)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_every_case_delivers_the_dimensions_statuses_and_columns_it_claims(cid, load_model):
    c, m = _case(cid, load_model)
    assert c.nr == [reduced_dim(m, state_of(m, t)) for t in c.topos]
    if cid in NR_CLAIMS:
        assert [n for n, s in zip(c.nr, c.status) if s == 0] == NR_CLAIMS[cid], c.nr
    oracle = c.extra.get("oracle_status", c.status)
    assert [verdict(m, state_of(m, t)) for t in c.topos] == oracle
    for lt in c.builds:                                      # more lanes than topologies, ragged classes, 8 .. 24 lanes
        sizes = np.bincount(lt, minlength=len(c.topos))
        used = sizes[sizes > 0]
        assert 8 <= len(lt) <= 24 and len(lt) > len(used) and len(set(used.tolist())) > 1, (cid, sizes)
    assert (np.bincount(np.concatenate(c.builds), minlength=len(c.topos)) > 0).all()
    kinds = {k: 0 for k in ("off", "nan", "stub", "live")}
    for i, s in enumerate(c.status):
        if s == 0:
            kd = class_reference(c, m, i)["kind"]
            for k in kinds:
                kinds[k] += int((kd == k).sum())
    print(f"[ptdf_batch_cases] {cid}: nr {c.nr}, status {c.status}, kernels "
          f"{[[c.kernel(b, md) for md in c.modes] for b in range(len(c.builds))]}, LODF columns {kinds}")
    assert kinds["live"] > 0 and all(kinds[k] > 0 for k in c.claims), (cid, kinds)
    if cid == "idf_over_128":
        ks = {(c.kernel(0, "default"), n_blocks(n)) for n, s in zip(c.nr, c.status) if s == 0}
        assert {("global", 8), ("global", 9), ("global", 10)} <= ks
        assert sorted(c.status).count(2) == 2 and c.status.count(3) == 1 and c.nr[c.extra["single"]] == 145
    if cid == "idf_switch":
        assert [c.kernel(b, "default") for b in range(3)] == ["resident", "global", "resident"] and np.array_equal(c.builds[0], c.builds[2])
        assert (c.builds[1] != c.builds[0]).sum() == 1
    if cid == "case5_floor":
        # nr = 3 is the floor: every substation but one carries a generator or a load, which no line outage takes out of service
        assert len(set(m.gen_sub.tolist()) | set(m.load_sub.tolist())) == min(c.nr) + 1 == 4 and max(n_blocks(n) for n in c.nr) == 1
    if cid.startswith("stub_and_bridge"):
        base = class_reference(c, m, 3)["kind"]                           # (the row with one line out: the other lines as in the base topology)
        for i, l in c.extra["stub_lines"].items():
            assert class_reference(c, m, i)["kind"][l] == "stub", (i, l)
        assert class_reference(c, m, 2)["kind"][c.extra["bridge_line"]] == "nan" and base[c.extra["bridge_line"]] == "live"
        assert class_reference(c, m, 3)["kind"][c.extra["out_line"]] == "off"
    if cid == "singular_pivot":
        l, s = c.extra["leaf_line"], c.extra["leaf_sub"]
        assert m.br_bdc[l] == 1e-14 and load_model(c.grid).br_bdc[l] > 1.0          # the committed model is untouched
        on = [bool(element_buses(m, state_of(m, t))[2][l]) for t in c.topos]
        assert [st == 1 for st in c.status] == on and c.status.count(0) == 1 and c.status.count(2) == 1
        # compact index of the leaf bus among the active non-reference buses: even (first pivot of a 2 x 2 block) and odd (second)
        par = set()
        for t, st in zip(c.topos, c.status):
            if st == 1:
                free = reduced_matrix(m, state_of(m, t))[1]
                leaf_bus = element_buses(m, state_of(m, t))[3][np.nonzero(m.gen_sub == s)[0][0]]
                par.add(int(np.nonzero(free == leaf_bus)[0][0]) % 2)
        assert par == {0, 1}


@pytest.mark.parametrize("cid", CASE_IDS)
def test_lodf_reference_equals_brute_force_outages(cid, load_model):
    """For outage k on a lane's injections: f(k out) - f = L[:, k] f_k within 1e-7 (1 + |f|), from `solve(is_dc=True)`; NaN columns
    exactly where the solve of the contingency fails; zero columns exactly where it converges with the flows unchanged.  Every outage
    of every class on the grids of <= 59 lines, 3 sampled outages per class (one of them on a cycle) on the 186-line grid."""
    c, m = _case(cid, load_model)
    rng = np.random.default_rng(11)
    states = {}
    n_live = 0
    for i, s in enumerate(c.status):
        if s != 0:
            continue
        b = next(b for b in range(len(c.builds)) if (c.builds[b] == i).any())        # (every topology is in a build: the claims test)
        if b not in states:
            states[b] = c.states(m, b)
        p = class_reference(c, m, i)
        L, kind = p["L"], p["kind"]
        st = states[b][_lane_of(c, b, i)]
        f = solve(m, st, is_dc=True).p_or
        tol = 1e-7 * (1.0 + np.abs(f))
        ks = np.arange(m.n_line)
        if m.n_line > 59:
            ks = np.concatenate([rng.choice(np.nonzero(kind == "live")[0], 1), rng.choice(m.n_line, 2, replace=False)])
        for k in ks:
            r = solve(m, without_line(st, m, k), is_dc=True)
            if not r.converged:
                assert np.isnan(L[:, k]).all(), (cid, i, k)
                continue
            assert not np.isnan(L[:, k]).any(), (cid, i, k)
            moved = np.abs(r.p_or - f) > tol
            moved[k] = False                                              # (the line itself goes to 0)
            if kind[k] == "live":
                assert abs(f[k]) > 1e-6 and L[k, k] == -1.0, (cid, i, k, f[k])
                assert np.all(np.abs(r.p_or - f - L[:, k] * f[k]) <= tol), (cid, i, k, np.abs(r.p_or - f - L[:, k] * f[k]).max())
                n_live += 1
            else:
                assert not moved.any() and abs(f[k]) <= tol[k] and (L[:, k] == 0.0).all(), (cid, i, k, kind[k])
    assert n_live > 0


@pytest.mark.parametrize("cid", CASE_IDS)
def test_decision_gap_conditioning_and_pivot_free_elimination(cid, load_model):
    c, m = _case(cid, load_model)
    for i, s in enumerate(c.status):
        if s != 0:
            continue
        p = class_reference(c, m, i)
        st = state_of(m, c.topos[i])
        on = p["kind"] != "off"
        den = np.abs(1.0 - np.diag(p["H"]))[on]
        assert not ((den >= 1e-10) & (den <= 1e-4)).any(), (cid, i, np.sort(den)[:4])
        cond = float(np.linalg.cond(reduced_matrix(m, st)[0]))
        gj = float(np.abs(ptdf_by_gauss_jordan(m, st) - p["T"]).max())
        live = p["kind"] == "live"
        print(f"[ptdf_batch_cases] {cid} topology {i}: nr {c.nr[i]}, cond(B') {cond:.3g}, pivot-free Gauss-Jordan vs ptdf() {gj:.2e}, "
              f"smallest |1 - H_kk| of a cycle line {den[live[on]].min():.3g}, largest of the others {np.r_[0.0, den[~live[on]]].max():.2e}")
        assert cond < 1e6, (cid, i, cond)
        assert gj < 0.01 * PTDF_BAR, (cid, i, gj)


def test_one_split_fewer_moves_ptdf_entries_by_100_bars(load_model):
    """The nr = 129 topology of the idf cases against the same with ONE of its 12 split substations merged again (nr = 128: what a
    builder that stopped at 128 buses, or took the tables of the neighbouring class, would return), for each of the 12."""
    c, m = _case("idf_switch", load_model)
    i = c.nr.index(129)
    t = c.topos[i]
    T = class_reference(c, m, i)["T"]
    from ptdf_batch_cases import _pos_sub
    ps = _pos_sub(m)
    subs = sorted(set(ps[t == 2].tolist()))
    assert len(subs) == 12
    for s in subs:
        t2 = t.copy()
        t2[(ps == s) & (t2 == 2)] = 1
        assert reduced_dim(m, state_of(m, t2)) == 128
        d = float(np.abs(ptdf(m, state_of(m, t2))[:, :m.n_sub] - T[:, :m.n_sub]).max())
        assert d >= 100 * PTDF_BAR, (s, d)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_float32_storage_alone_takes_up_to_half_the_lodf_bar(cid, load_model):
    """The LODF table is stored in float32.  A builder that computed every entry EXACTLY and rounded it to nearest would sit at up to half
    of the first term of `lodf_tolerance` (2^-23 |ref| is a whole spacing): the figure printed here is what the GPU test's
    `max_err_over_tol` of the case is to be read against."""
    c, m = _case(cid, load_model)
    worst = 0.0
    for i, s in enumerate(c.status):
        if s != 0:
            continue
        p = class_reference(c, m, i)
        L, tol = p["L"], lodf_tolerance(p["L"], p["inv_den"])
        q = np.isfinite(L) & np.isfinite(tol)
        assert (tol[q] > 0).all()
        worst = max(worst, float((np.abs(L.astype(np.float32).astype(np.float64) - L)[q] / tol[q]).max()))
    print(f"[ptdf_batch_cases] {cid}: float32(reference) against the LODF bar: {worst:.3g}")
    assert 0.0 < worst <= 0.5
