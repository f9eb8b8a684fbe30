"""CPU conditions of the parity tests of `gpf_ptdf_flows_rows` (tests/test_gpu_ptdf_rows.py): (1) the plain-numpy reference
(tests/ptdf_rows_ref.py) agrees with the C oracle's DC power flow of the same injections, and `COracle.step_batch` reproduces the
injections themselves where it can express them (one table at a time, no redispatch delta); (2) the inputs DISCRIMINATE: for every
feature a case claims to cover, the reference recomputed without that feature differs from the true one by at least 100 times the
tolerance of the entry, on at least one line of every pair that exercises the feature.  A case that could not fail is not a case."""
import numpy as np
import pytest

from oracle.pf_oracle import element_buses, ptdf
from oracle.spot_check import ABS_TOL, REL_TOL

from ptdf_rows_cases import BATCH_IDS, SINGLE_IDS, base_inj, per_lane_topology_cases, single_topology_cases
from ptdf_rows_ref import inj_offsets, lane_state, rows_injections, rows_reference

ALL_IDS = SINGLE_IDS + BATCH_IDS

_REF = {}


def _case(cid, load_model, load_npz):
    cases = single_topology_cases(load_model, load_npz) if cid in SINGLE_IDS else per_lane_topology_cases(load_model, load_npz)
    return cases[cid]


def _reference(c, m):
    if c.id not in _REF:
        _REF[c.id] = rows_reference(m, **c.ref_args())
    return _REF[c.id]


def _row_sums(c):
    """Unwrapped row index t0 + j + lane_offset[k] of every pair, [n_rows, n_lanes]."""
    off = np.zeros(c.n_lanes, np.int64) if c.lane_offset is None else c.lane_offset.astype(np.int64)
    return c.t0 + np.arange(c.n_rows)[:, None] + off[None, :]


def _reference_at_rows(c, m, idx):
    """The reference with the table row of every pair given explicitly (`idx` [n_rows, n_lanes], inside the table)."""
    return np.stack([rows_reference(m, **c.ref_args(t0=0, n_rows=1, lane_offset=idx[j]))[0] for j in range(c.n_rows)])


def test_the_case_lists_are_complete(load_model, load_npz):
    assert sorted(single_topology_cases(load_model, load_npz)) == sorted(SINGLE_IDS)
    assert sorted(per_lane_topology_cases(load_model, load_npz)) == sorted(BATCH_IDS)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_reference_equals_the_c_oracle_dc_power_flow(cid, load_model, load_npz):
    """At least 32 (row, lane) pairs per grid row of the case table (every pair of the cases that have fewer than 48): the reference's
    flows against `COracle.solve_rows(is_dc=True)` on the same injection rows and topologies, within ABS_TOL + REL_TOL |x|; lanes the C
    oracle rejects are exactly the all-NaN lanes of the reference."""
    from oracle.pf_oracle_c import COracle
    c = _case(cid, load_model, load_npz)
    m = load_model(c.grid)
    ref = _reference(c, m)
    x = rows_injections(m, **{k: v for k, v in c.ref_args().items() if k not in ("topo", "shunt_bus")})
    pairs = [(j, k) for j in range(c.n_rows) for k in range(c.n_lanes)]
    if len(pairs) > 48:
        rng = np.random.default_rng(7)
        pairs = [pairs[i] for i in rng.choice(len(pairs), 48, replace=False)]
    assert len(pairs) >= 32 or len(pairs) == c.n_rows * c.n_lanes
    topo = np.broadcast_to(c.topo, (c.n_lanes, m.dim_topo))
    sb = np.broadcast_to(c.shunt_bus, (c.n_lanes, m.n_shunt))
    js, ks = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    out = COracle(m).solve_rows(x[js, ks], topo[ks], sb[ks] if m.n_shunt else None, is_dc=True)
    p_ref = out["out"][:, :m.n_line]
    bad = out["status"][:, 0] != 0
    got = ref[js, ks]
    assert np.array_equal(np.isnan(got).all(axis=1), bad) and np.array_equal(np.isnan(got).any(axis=1), bad)
    err = np.abs(got[~bad] - p_ref[~bad])
    assert np.all(err <= ABS_TOL + REL_TOL * np.abs(p_ref[~bad])), float(err.max())
    if cid in BATCH_IDS:
        assert bad.any() and (~bad).sum() >= 24                     # islanded lanes were sampled, and enough others


@pytest.mark.parametrize("cid", ALL_IDS)
def test_step_batch_reproduces_the_injections(cid, load_model, load_npz):
    """`COracle.step_batch` gathers a chronics row into injections by itself (one table, jitter, rebalancing; no delta) and solves the AC
    power flow on the base topology: the load_p and non-slack gen_p of its result rows ARE the set-points.  They must equal the
    reference's bit for bit -- per table, with the redispatch delta taken out where the case has one."""
    from oracle.pf_oracle_c import COracle
    c = _case(cid, load_model, load_npz)
    m = load_model(c.grid)
    o = inj_offsets(m)
    orc = COracle(m)
    ns = ~m.gen_slack
    rng = np.random.default_rng(9)
    n_checked = 0
    for tb in range(c.tables.shape[0]):
        lanes = np.arange(c.n_lanes) if c.lane_table is None else np.nonzero(c.lane_table == tb)[0]
        args = {k: v for k, v in c.ref_args(tables=c.tables[tb], lane_table=None, gen_delta=None).items() if k not in ("topo", "shunt_bus")}
        x = rows_injections(m, **args)
        pairs = [(j, int(k)) for j in range(c.n_rows) for k in lanes]
        if len(pairs) > 32:
            pairs = [pairs[i] for i in rng.choice(len(pairs), 32, replace=False)]
        off = np.zeros(c.n_lanes, np.int32) if c.lane_offset is None else c.lane_offset
        for j, k in pairs:
            _, out, st = orc.step_batch(c.tables[tb], off, c.lane_scale, c.rebalance_value, c.t0 + j, k, 1, want_out=True)
            assert st[0, 0] == 0, (tb, j, k)
            gen_p = out[0, 10 * m.n_line:10 * m.n_line + m.n_gen]
            load_p = out[0, 10 * m.n_line + 4 * m.n_gen:10 * m.n_line + 4 * m.n_gen + m.n_load]
            assert np.array_equal(load_p, x[j, k, o["load_p"]:o["load_p"] + m.n_load]), (tb, j, k)
            assert np.array_equal(gen_p[ns], x[j, k, o["gen_p"]:o["gen_p"] + m.n_gen][ns]), (tb, j, k)
            n_checked += 1
    assert n_checked >= min(32, c.n_rows * c.n_lanes)


def _ablations(c, m):
    """feature -> (reference without the feature, [n_rows, n_lanes] mask of the pairs that exercise it)"""
    T = c.tables.shape[1]
    nl = m.n_load
    every = np.ones((c.n_rows, c.n_lanes), bool)
    u = _row_sums(c)
    out = {}
    for f in c.features:
        if f == "jitter":
            assert (np.abs(c.lane_scale[:, :nl] - 1) > 1e-3).any(axis=1).all()
            out[f] = (rows_reference(m, **c.ref_args(lane_scale=None)), every)
        elif f == "delta":
            assert (c.gen_delta[:, ~m.gen_slack] != 0).any(axis=1).all()                      # a delta on every lane
            out[f] = (rows_reference(m, **c.ref_args(gen_delta=None)), every)
        elif f == "offset":
            mask = np.broadcast_to((c.lane_offset % T != 0)[None, :], every.shape)
            assert mask.any()
            out[f] = (rows_reference(m, **c.ref_args(lane_offset=None)), mask)
        elif f == "second_table":
            assert c.tables.shape[0] == 2 and 0 < (c.lane_table == 1).sum() < c.n_lanes
            out[f] = (rows_reference(m, **c.ref_args(lane_table=None)), np.broadcast_to((c.lane_table == 1)[None, :], every.shape))
        elif f == "rebalance":
            lt = np.zeros(c.n_lanes, np.int64) if c.lane_table is None else c.lane_table
            prod = c.tables[lt[None, :], u % T][:, :, 2 * nl:2 * nl + m.n_gen][:, :, ~m.gen_slack].astype(np.float64).sum(axis=2)
            assert c.rebalance_value > 0
            out[f] = (rows_reference(m, **c.ref_args(rebalance=0.0)), prod > 0)
        elif f == "sto_shunt":
            o = inj_offsets(m)
            plain = c.inj_row.copy()
            for name, n in (("storage_p", m.n_storage), ("shunt_p", m.n_shunt)):
                assert n > 0 and (c.inj_row[:, o[name]:o[name] + n] != 0).all()
                plain[:, o[name]:o[name] + n] = base_inj(m)[o[name]:o[name] + n]
            out[f] = (rows_reference(m, **c.ref_args(inj_row=plain)), every)
        elif f == "wrap":                                   # a gather that does not wrap stops at the last row
            mask = u >= T
            assert mask.sum() >= 6 and (u >= 2 * T).any()
            out[f] = (_reference_at_rows(c, m, np.where(mask, T - 1, u % T)), mask)
        elif f == "negative_t0":                            # a gather that does not lift a negative remainder stops at row 0
            mask = u < 0
            assert c.t0 < 0 and mask.sum() >= 4
            out[f] = (_reference_at_rows(c, m, np.where(mask, 0, u % T)), mask)
        elif f == "gen_tail_delta":
            # generators of index >= 32 are re-read in the tail loop when 4 threads gather a pair: the delta must sit on such a generator whose
            # bus has a non-zero PTDF column, and ONLY the delta of those generators is taken away
            tail = c.extra["tail_gens"]
            assert (tail >= 32).all() and not m.gen_slack[tail].any() and (c.gen_delta[:, tail] != 0).all()
            st = lane_state(m, c.inj_row[0], c.topo, c.shunt_bus)
            gbus = element_buses(m, st)[3]
            col = np.abs(ptdf(m, st)[:, gbus[tail]]).max(axis=0)
            assert (gbus[tail] >= 0).all() and (col > 1e-3).any()
            d = c.gen_delta.copy()
            d[:, tail] = 0.0
            out[f] = (rows_reference(m, **c.ref_args(gen_delta=d)), every)
        elif f in ("load_tail_64", "load_tail_32"):
            # loads of index >= 64 (8 gather threads per pair) / 32 .. 63 (4 threads per pair: index >= 32) are re-read in the tail loop
            lo, hi = (64, nl) if f == "load_tail_64" else (32, 64)
            assert nl > 64 and (np.abs(c.lane_scale[:, lo:hi] - 1) > 1e-3).any(axis=1).all()
            s = c.lane_scale.copy()
            s[:, lo:hi] = 1.0
            out[f] = (rows_reference(m, **c.ref_args(lane_scale=s)), every)
        else:
            raise AssertionError(f"unknown feature {f}")
    return out


@pytest.mark.parametrize("cid", ALL_IDS)
def test_inputs_discriminate_every_feature_the_case_claims(cid, load_model, load_npz):
    c = _case(cid, load_model, load_npz)
    m = load_model(c.grid)
    ref = _reference(c, m)
    live = ~np.isnan(ref).any(axis=2)
    assert live.any(axis=0).sum() >= c.n_lanes // 2
    bar = 100.0 * (ABS_TOL + REL_TOL * np.abs(ref))
    abl = _ablations(c, m)
    assert set(abl) == set(c.features) and c.features
    for f, (other, mask) in abl.items():
        assert np.array_equal(np.isnan(other), np.isnan(ref)), f
        pairs = mask & live
        assert pairs.any(), f
        with np.errstate(invalid="ignore"):
            moved = (np.abs(other - ref) >= bar).any(axis=2)
        assert moved[pairs].all(), (cid, f, int((~moved[pairs]).sum()), int(pairs.sum()))
    if c.zero_prod_row is not None:
        # the row without non-slack production is met by a pair, with load on it: a gather that divided by sum_prod would give inf / NaN
        T, nl = c.tables.shape[1], m.n_load
        hit = (_row_sums(c) % T) == c.zero_prod_row
        row = c.tables[0, c.zero_prod_row]
        assert hit.any() and row[2 * nl:2 * nl + m.n_gen][~m.gen_slack].sum() == 0 and row[:nl].sum() > 0 and c.rebalance_value > 0
    if c.rebalance is None:
        assert c.rebalance_value == 0.0


@pytest.mark.parametrize("cid", BATCH_IDS)
def test_per_lane_topology_cases_have_ragged_and_islanded_classes(cid, load_model, load_npz):
    c = _case(cid, load_model, load_npz)
    m = load_model(c.grid)
    ref = _reference(c, m)
    lane_topo = c.extra["lane_topo"]
    dead = np.isnan(ref).all(axis=(0, 2))
    assert np.array_equal(dead, lane_topo >= c.extra["n_topo"] - c.extra["n_islanded_topo"]) and dead.any()
    assert np.array_equal(np.isnan(ref).any(axis=(0, 2)), dead)
    sizes = np.bincount(lane_topo, minlength=c.extra["n_topo"])
    assert (sizes > 0).all() and (sizes % 16 != 0).all() and len(set(sizes.tolist())) > 1      # every class is padded with -1 slots
    assert c.n_rows % 2 == 1
    # the rebuild moves lanes (some of them islanded before) to a live topology; its reference has fewer NaN lanes
    ref2 = rows_reference(m, **c.ref_args(topo=c.extra["topo_rebuild"]))
    moved = c.extra["moved"]
    assert moved.any() and not np.isnan(ref2[:, moved]).any() and (dead & moved).any()
    assert np.array_equal(ref2[:, ~moved], ref[:, ~moved], equal_nan=True)
