"""Inputs of the parity tests of `gpf_ptdf_flows_rows` (tests/test_gpu_ptdf_rows.py) and of the conditions those inputs must meet
(tests/test_ptdf_rows_ref_cpu.py): small shapes on the committed grids, every one seeded.  Each case names the features it claims to
cover; the CPU test proves on the reference alone that taking a feature away moves the expected flows by far more than the tolerance."""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from oracle.pf_oracle import LaneState, element_buses, solve

from ptdf_rows_ref import inj_offsets
from test_gpu_ptdf_batch import random_topologies


@dataclass
class RowsCase:
    id: str
    grid: str
    n_lanes: int
    n_rows: int
    t0: int
    rebalance: Optional[float]             # None: the Python wrapper's default (0.0) is used, the argument is not passed
    tables: np.ndarray                     # float32 [n_tab, T, n_chron]
    lane_table: Optional[np.ndarray]
    lane_offset: Optional[np.ndarray]
    lane_scale: Optional[np.ndarray]       # None: never set on the engine
    gen_delta: Optional[np.ndarray]
    inj_row: np.ndarray                    # float64 [n_lanes, n_inj]
    topo: np.ndarray                       # [dim_topo] (gpf_ptdf_build) or [n_lanes, dim_topo] (gpf_ptdf_build_batch)
    shunt_bus: np.ndarray
    features: Tuple[str, ...] = ()
    zero_prod_row: Optional[int] = None    # table row whose non-slack prod_p is all zero
    extra: dict = field(default_factory=dict)

    @property
    def rebalance_value(self):
        return 0.0 if self.rebalance is None else self.rebalance

    def ref_args(self, **over):
        a = dict(topo=self.topo, shunt_bus=self.shunt_bus, inj_row=self.inj_row, tables=self.tables, lane_table=self.lane_table,
                 lane_offset=self.lane_offset, lane_scale=self.lane_scale, gen_delta=self.gen_delta, t0=self.t0, n_rows=self.n_rows,
                 rebalance=self.rebalance_value)
        a.update(over)
        return a


def base_inj(m):
    return np.concatenate([m.gen_p0, m.gen_vm0, m.load_p0, m.load_q0, m.storage_p0, m.storage_q0, m.shunt_p0, m.shunt_q0]).astype(np.float64)


def pos_sub(m):
    ps = np.empty(m.dim_topo, dtype=np.int64)
    ps[m.line_or_pos_topo_vect] = m.line_or_sub
    ps[m.line_ex_pos_topo_vect] = m.line_ex_sub
    ps[m.gen_pos_topo_vect] = m.gen_sub
    ps[m.load_pos_topo_vect] = m.load_sub
    if m.n_storage:
        ps[m.storage_pos_topo_vect] = m.storage_sub
    return ps


def one_out_one_split(m, rng):
    """A topology with one line out AND one substation split over two busbars that the DC power flow accepts (found as
    test_gpu_parity.py::test_ptdf_path_matches_dc_power_flow finds its topology, but the split is required)."""
    ps = pos_sub(m)
    for _ in range(200):
        st = LaneState.from_model(m)
        l_out = int(rng.integers(m.n_line))
        st.topo[m.line_or_pos_topo_vect[l_out]] = -1
        st.topo[m.line_ex_pos_topo_vect[l_out]] = -1
        pos = np.nonzero(ps == int(rng.integers(m.n_sub)))[0]
        if len(pos) < 4:
            continue
        st.topo[pos[::2]] = np.where(st.topo[pos[::2]] >= 1, 2, st.topo[pos[::2]])
        if (st.topo[pos] == 2).any() and (st.topo[pos] == 1).any() and solve(m, st, is_dc=True).converged:
            return st.topo.astype(np.int32)
    raise AssertionError("no connected topology with a line out and a split substation")


def n_active_buses(m, topo):
    st = LaneState.from_model(m)
    st.topo = np.asarray(topo).copy()
    parts = element_buses(m, st)
    buses = np.concatenate([np.asarray(parts[i]) for i in (0, 1, 3, 4, 5, 6)])
    return len(np.unique(buses[buses >= 0]))


def committed_table(m, ch, rows):
    """The committed chronics rows `rows` as one `[T, n_chron]` float32 table."""
    prod_v = ch["prod_v"] if "prod_v" in ch else np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
    tab = np.concatenate([ch["load_p"], ch["load_q"], ch["prod_p"], prod_v], axis=-1).astype(np.float32)
    return np.ascontiguousarray(tab[rows])


def synthetic_table(m, T, rng):
    """`[T, n_chron]` float32 around the model's base load_p / gen_p, rows independent of each other."""
    lp = m.load_p0 * (1 + 0.25 * rng.standard_normal((T, m.n_load)))
    lq = m.load_q0 * (1 + 0.25 * rng.standard_normal((T, m.n_load)))
    pp = np.abs(m.gen_p0 * (1 + 0.25 * rng.standard_normal((T, m.n_gen)))) + rng.uniform(0.5, 2.0, (T, m.n_gen))
    pv = np.tile(m.gen_vm0 * m.sub_vn_kv[m.gen_sub], (T, 1))
    return np.concatenate([lp, lq, pp, pv], axis=-1).astype(np.float32)


def _scale(m, n, rng, sd=0.1):
    return (1.0 + sd * rng.standard_normal((n, 2 * m.n_load))).astype(np.float32)


def _delta(m, n, rng, gens=None, amp=6.0):
    d = np.zeros((n, m.n_gen), dtype=np.float32)
    gens = np.nonzero(~m.gen_slack)[0] if gens is None else np.asarray(gens)
    d[:, gens] = (rng.uniform(0.5, 1.0, (n, len(gens))) * rng.choice([-1.0, 1.0], (n, len(gens))) * amp).astype(np.float32)
    return d


SINGLE_IDS = ["case5_1x1", "case5_13x5", "case5_four_buses", "case14_default_rebalance", "case14_zero_prod_row", "educ_17x4", "neurips_37x3",
              "wcci_21x6"]
BATCH_IDS = ["batch_l2rpn_neurips_2020_track1", "batch_l2rpn_case14_sandbox"]

_CACHE = {}


def single_topology_cases(load_model, load_npz):
    """The cases of one topology for all lanes (gpf_ptdf_build), by id."""
    if "single" in _CACHE:
        return _CACHE["single"]
    cases = {}

    # ---- rte_case5_example: 3 loads / 2 generators (fewer than the gather threads of a pair), 6 active buses -> nb_pad = 8, kpad = 32: ONE trip of the GEMM loop
    name = "rte_case5_example"
    m = load_model(name)
    ch = load_npz(f"{name}.chronics.npz")
    rng = np.random.default_rng(501)
    topo = one_out_one_split(m, rng)
    tab = committed_table(m, ch, np.arange(0, 350, 7))[None]                  # 50 rows, 35 minutes apart
    for n, r, t0 in ((1, 1, 4), (13, 5, 9)):
        cases[f"case5_{n}x{r}"] = RowsCase(
            id=f"case5_{n}x{r}", grid=name, n_lanes=n, n_rows=r, t0=t0, rebalance=1.02, tables=tab, lane_table=None,
            lane_offset=(3 + 13 * np.arange(n)).astype(np.int32), lane_scale=_scale(m, n, rng), gen_delta=None,
            inj_row=np.tile(base_inj(m), (n, 1)), topo=topo, shunt_bus=m.initial_shunt_bus().astype(np.int32),
            features=("jitter", "offset", "rebalance"))

    # (an extra: substation 2 carries lines only; with its four lines out it is not an active bus: 4 active buses, the floor nb_pad = 4)
    topo4 = m.initial_topo_vect().astype(np.int32)
    at_sub2 = np.nonzero((m.line_or_sub == 2) | (m.line_ex_sub == 2))[0]
    assert not (m.gen_sub == 2).any() and not (m.load_sub == 2).any() and len(at_sub2) == 4
    topo4[m.line_or_pos_topo_vect[at_sub2]] = -1
    topo4[m.line_ex_pos_topo_vect[at_sub2]] = -1
    assert n_active_buses(m, topo4) == 4
    cases["case5_four_buses"] = RowsCase(
        id="case5_four_buses", grid=name, n_lanes=5, n_rows=3, t0=2, rebalance=1.02, tables=tab, lane_table=None,
        lane_offset=(3 + 13 * np.arange(5)).astype(np.int32), lane_scale=_scale(m, 5, rng), gen_delta=None,
        inj_row=np.tile(base_inj(m), (5, 1)), topo=topo4, shunt_bus=m.initial_shunt_bus().astype(np.int32),
        features=("jitter", "offset", "rebalance"))

    # ---- l2rpn_case14_sandbox: rebalance = 0.0 through the wrapper's default; a row without non-slack production under rebalance = 1.02
    name = "l2rpn_case14_sandbox"
    m = load_model(name)
    ch = load_npz(f"{name}.chronics.npz")
    rng = np.random.default_rng(1401)
    topo = one_out_one_split(m, rng)
    tab = committed_table(m, ch, np.arange(0, 576, 12))                       # 48 rows
    zero_row = 21
    tab[zero_row, 2 * m.n_load:2 * m.n_load + m.n_gen][~m.gen_slack] = 0.0
    off = (5 * np.arange(7) + 3).astype(np.int32)                               # 3, 8, .., 33: lane 3 (offset 18) meets row 21 at t0 + 1
    common = dict(grid=name, n_lanes=7, n_rows=3, t0=2, tables=tab[None], lane_table=None, lane_offset=off, lane_scale=_scale(m, 7, rng),
                  gen_delta=_delta(m, 7, rng, amp=3.0), inj_row=np.tile(base_inj(m), (7, 1)), topo=topo,
                  shunt_bus=m.initial_shunt_bus().astype(np.int32))
    cases["case14_default_rebalance"] = RowsCase(id="case14_default_rebalance", rebalance=None, features=("jitter", "offset", "delta"), **common)
    cases["case14_zero_prod_row"] = RowsCase(id="case14_zero_prod_row", rebalance=1.02, features=("jitter", "offset", "delta", "rebalance"),
                                             zero_prod_row=zero_row, **common)

    # ---- educ_case14_storage: no chronics committed -> a synthetic table; storage and shunt set-points of the injection rows; no lane_scale
    name = "educ_case14_storage"
    m = load_model(name)
    rng = np.random.default_rng(1402)
    topo = one_out_one_split(m, rng)
    o = inj_offsets(m)
    inj = np.tile(base_inj(m), (17, 1))
    inj[:, o["storage_p"]:o["storage_p"] + m.n_storage] = rng.uniform(1.0, 4.0, (17, m.n_storage)) * rng.choice([-1.0, 1.0], (17, m.n_storage))
    inj[:, o["shunt_p"]:o["shunt_p"] + m.n_shunt] = rng.uniform(1.0, 3.0, (17, m.n_shunt))
    cases["educ_17x4"] = RowsCase(
        id="educ_17x4", grid=name, n_lanes=17, n_rows=4, t0=6, rebalance=1.02, tables=synthetic_table(m, 40, rng)[None], lane_table=None,
        lane_offset=(9 + 3 * np.arange(17)).astype(np.int32), lane_scale=None, gen_delta=None, inj_row=inj, topo=topo,
        shunt_bus=m.initial_shunt_bus().astype(np.int32), features=("offset", "rebalance", "sto_shunt"))

    # ---- l2rpn_neurips_2020_track1: two tables, wraps past T, a negative t0, a delta on every lane
    name = "l2rpn_neurips_2020_track1"
    m = load_model(name)
    ch = load_npz(f"{name}.chronics.npz")
    rng = np.random.default_rng(3601)
    topo = one_out_one_split(m, rng)
    T = 30
    tabs = np.stack([committed_table(m, ch, np.arange(0, 600, 20)), synthetic_table(m, T, rng)])
    n = 37
    off = (4 * np.arange(n) + 5).astype(np.int32) % T
    off[:4] = (0, 1, 2, 0)                                                       # t0 = -3: negative row sums on these lanes
    off[4:12] = (T + 1, T + 2, T + 3, 2 * T + 4, T + 5, 3 * T + 6, T + 9, 2 * T + 3)        # row sums of T and beyond, also by more than one period
    lt = (rng.random(n) < 0.5).astype(np.int32)
    lt[:12] = (0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1)
    cases["neurips_37x3"] = RowsCase(
        id="neurips_37x3", grid=name, n_lanes=n, n_rows=3, t0=-3, rebalance=1.02, tables=tabs, lane_table=lt, lane_offset=off,
        lane_scale=_scale(m, n, rng), gen_delta=_delta(m, n, rng), inj_row=np.tile(base_inj(m), (n, 1)), topo=topo,
        shunt_bus=m.initial_shunt_bus().astype(np.int32),
        features=("jitter", "offset", "rebalance", "delta", "second_table", "wrap", "negative_t0"))

    # ---- l2rpn_wcci_2022_dev: 91 loads, 62 generators, 7 storages, 14 shunts: loads >= 64 (8 threads per pair) / loads and generators >= 32
    #      (4 threads per pair) are the re-read tails of the gather
    name = "l2rpn_wcci_2022_dev"
    m = load_model(name)
    ch = load_npz(f"{name}.chronics.npz")
    rng = np.random.default_rng(11801)
    topo = one_out_one_split(m, rng)
    n = 21
    o = inj_offsets(m)
    inj = np.tile(base_inj(m), (n, 1))
    inj[:, o["storage_p"]:o["storage_p"] + m.n_storage] = rng.uniform(2.0, 8.0, (n, m.n_storage)) * rng.choice([-1.0, 1.0], (n, m.n_storage))
    inj[:, o["shunt_p"]:o["shunt_p"] + m.n_shunt] = rng.uniform(1.0, 4.0, (n, m.n_shunt))
    tail_gens = [g for g in range(32, m.n_gen) if not m.gen_slack[g]]
    cases["wcci_21x6"] = RowsCase(
        id="wcci_21x6", grid=name, n_lanes=n, n_rows=6, t0=3, rebalance=1.02, tables=committed_table(m, ch, np.arange(0, 288, 6))[None],
        lane_table=None, lane_offset=(13 + 5 * np.arange(n)).astype(np.int32), lane_scale=_scale(m, n, rng),
        gen_delta=_delta(m, n, rng, gens=tail_gens, amp=10.0), inj_row=inj, topo=topo, shunt_bus=m.initial_shunt_bus().astype(np.int32),
        features=("jitter", "offset", "rebalance", "sto_shunt", "gen_tail_delta", "load_tail_64", "load_tail_32"),
        extra=dict(tail_gens=np.asarray(tail_gens)))
    _CACHE["single"] = cases
    return cases


def per_lane_topology_cases(load_model, load_npz):
    """Per-lane topologies (gpf_ptdf_build_batch): about 40 lanes over 12 topologies of `random_topologies`, every one with a split
    substation, at least one islanded; 5 rows (no multiple of 2 or 4).  `extra["topo_rebuild"]`: the topology rows after the lanes of
    three topologies moved to one WITHOUT a split (fewer active buses): fewer classes than before, so the class slot of the new
    topology held the PTDF^T block of a larger one."""
    if "batch" in _CACHE:
        return _CACHE["batch"]
    cases = {}
    for name, seed, n_lanes in (("l2rpn_neurips_2020_track1", 3602, 41), ("l2rpn_case14_sandbox", 1403, 39)):
        m = load_model(name)
        ch = load_npz(f"{name}.chronics.npz")
        rng = np.random.default_rng(seed)
        pool = [t for t in random_topologies(m, 120, rng) if (t == 2).any()]

        def ok(t):
            st = LaneState.from_model(m)
            st.topo = t.copy()
            return solve(m, st, is_dc=True).converged
        bad = [t for t in pool if not ok(t)]
        good = [t for t in pool if ok(t)]
        n_bad = min(2, len(bad))
        assert n_bad >= 1 and len(good) >= 12 - n_bad, (name, len(bad), len(good))
        topos = good[:12 - n_bad] + bad[:n_bad]                  # (the islanded ones last)
        n_topo = len(topos)
        lane_topo = np.concatenate([np.arange(n_topo), rng.integers(0, n_topo, n_lanes - n_topo)])
        rng.shuffle(lane_topo)
        topo = np.stack([topos[i] for i in lane_topo]).astype(np.int32)
        # the rebuild: every lane of topologies 0, 1 and the last (islanded) moves to a topology with one line out and no split
        small = m.initial_topo_vect().astype(np.int32)
        for l_out in range(m.n_line):
            t = small.copy()
            t[m.line_or_pos_topo_vect[l_out]] = -1
            t[m.line_ex_pos_topo_vect[l_out]] = -1
            if ok(t):
                small = t
                break
        moved = np.isin(lane_topo, (0, 1, n_topo - 1))
        topo2 = topo.copy()
        topo2[moved] = small
        assert all(n_active_buses(m, small) < n_active_buses(m, t) for t in topos), name
        T = 48
        cid = f"batch_{name}"
        cases[cid] = RowsCase(
            id=cid, grid=name, n_lanes=n_lanes, n_rows=5, t0=7, rebalance=1.02, tables=committed_table(m, ch, np.arange(0, 576, 12))[None],
            lane_table=None, lane_offset=((11 * np.arange(n_lanes) + 2) % T).astype(np.int32), lane_scale=_scale(m, n_lanes, rng),
            gen_delta=_delta(m, n_lanes, rng, amp=4.0), inj_row=np.tile(base_inj(m), (n_lanes, 1)), topo=topo,
            shunt_bus=np.tile(m.initial_shunt_bus().astype(np.int32), (n_lanes, 1)), features=("jitter", "offset", "rebalance", "delta"),
            extra=dict(lane_topo=lane_topo, n_topo=n_topo, topo_rebuild=topo2, moved=moved, n_islanded_topo=n_bad))
    _CACHE["batch"] = cases
    return cases
