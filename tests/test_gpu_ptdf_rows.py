"""GPU parity tests of `gpf_ptdf_flows_rows` (`ptdf_rows_kernel<MT>`, grid2op_amd/csrc/gridpf_ptdf.hpp) at small shapes, and of
`gpf_lodf_screen` on a modified single topology.

Every (row, lane, line) entry of every case is compared with the plain-numpy reference of tests/ptdf_rows_ref.py (the chronics rule of
the step kernel restated, then `ptdf(m, state) @ dc_bus_injection(m, state)` of oracle/pf_oracle.py on the lane's own topology), within
the project's float32 bar `ABS_TOL + REL_TOL |x|` of oracle/spot_check.py; NaN patterns must match exactly.  The cases and what each
pins are in tests/ptdf_rows_cases.py; tests/test_ptdf_rows_ref_cpu.py proves, without a GPU, that the reference agrees with the C oracle
and that every case's inputs discriminate the features it claims (removing one moves the expected flows by >= 100 x the tolerance).

The tile height of the kernel (`GRIDPF_PTDF_MT` = 1 | 2 | 4) is read once per process: the last test of this file runs
the file again in fresh child processes with MT = 1 and MT = 4."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.pf_oracle import LaneState, dc_n1_worst_loading
from oracle.spot_check import ABS_TOL, REL_TOL

from conftest import ROOT
from helpers import pack_states
from ptdf_rows_cases import BATCH_IDS, SINGLE_IDS, one_out_one_split, per_lane_topology_cases, single_topology_cases
from ptdf_rows_ref import rows_reference

pytestmark = pytest.mark.gpu

GPF_E_INVALID = -1                                  # include/gridpf.h
MT_LABEL = os.environ.get("GRIDPF_PTDF_MT", "default")
# ten times the measured wall time of `python -m pytest -q -m gpu tests/test_gpu_ptdf_rows.py` as a process of its own at the default
# tile height on an MI355X host, the child runs left out: 5.4 s (of which 3.4 s in the tests)
CHILD_TIMEOUT_S = 54


def _engine(c, m):
    from grid2op_amd.engine import PowerFlowEngine
    eng = PowerFlowEngine(m, n_lanes=c.n_lanes, device=0)
    eng.upload_chronics(c.tables)
    eng.set_lane_chronics(lane_table=c.lane_table, lane_offset=c.lane_offset, lane_scale=c.lane_scale)      # lane_scale None: never set
    if c.gen_delta is not None:
        eng.set_lane_redispatch(c.gen_delta)
    eng.set_injections(c.inj_row)
    return eng


def _launch(eng, c, t0, n_rows, **kw):
    if c.rebalance is None:                          # the wrapper's own default
        return eng.ptdf_flows_rows(t0, n_rows, **kw)
    return eng.ptdf_flows_rows(t0, n_rows, rebalance=c.rebalance, **kw)


def _compare(tag, got, ref):
    """every entry; prints the figures before it asserts"""
    assert got.shape == ref.shape and got.dtype == np.float32, (got.shape, ref.shape)
    nan_same = np.array_equal(np.isnan(got), np.isnan(ref))
    live = ~np.isnan(ref)
    err = np.abs(got.astype(np.float64)[live] - ref[live])
    tol = ABS_TOL + REL_TOL * np.abs(ref[live])
    fig = dict(case=tag, mt=MT_LABEL, entries=int(ref.size), nan_entries=int((~live).sum()), max_abs_err=float(np.nanmax(err)),
               max_excess=float(np.nanmax(err - tol)), max_err_over_tol=float(np.nanmax(err / tol)), nan_pattern_equal=bool(nan_same))
    print("[ptdf_rows] " + json.dumps(fig))
    assert nan_same, fig
    assert not np.isnan(err).any() and fig["max_excess"] <= 0.0, fig


def _get_rows(eng, row0, n_rows, lane0, n):
    from grid2op_amd._capi import ptr
    out = np.full((max(n_rows, 0), n, eng.model.n_line), -7.0, dtype=np.float32)
    rc = eng._lib.gpf_get_ptdf_flows_rows(eng._h, int(row0), int(n_rows), int(lane0), int(n), ptr(out, C.c_float))
    return rc, out


@pytest.mark.parametrize("cid", SINGLE_IDS)
def test_single_topology_every_entry_vs_reference(cid, load_model, load_npz):
    """One topology for all lanes (`ptdf_build(0)`), with one line out and one split substation (case5_four_buses: the four lines of the
    substation that carries nothing else are out instead, 4 active buses: the floor nb_pad = 4).  What each case pins:
    case5 (1 x 1, 13 x 5): 3 loads / 2 generators, fewer than the gather threads of a pair; 6 active buses (nb_pad = 8, kpad = 32): the
    GEMM loop runs ONE trip, whose re-fetch of its own operands reads the zero rows behind nb_pad; blocks that span several chronics rows;
    65 pairs (ragged for 16 / 32 / 64 pairs per block).  case14 (nb_pad = 16, kpad = 32): `rebalance = 0.0` through the wrapper's default; a table row without
    non-slack production under `rebalance = 1.02`.  educ: storage and shunt set-points of the injection rows, `lane_scale` never set.
    neurips: two tables, row sums past T (also by more than one period), `t0 = -3`, a redispatch delta on every lane.  wcci: 91 loads,
    62 generators, 7 storages, 14 shunts -- the load tail at MT = 2, both tails at MT = 4 (jitter on loads >= 64 and 32 .. 63, delta on
    generators >= 32 only), dynamic LDS beyond 64 KB at MT = 4.
    Also: launches of ONE row at t0 + j equal row j of the multi-row launch bit for bit; a lane sub-range equals the slice;
    `gpf_get_ptdf_flows_rows` with row0 > 0 returns the later rows and refuses rows beyond the last launch."""
    c = single_topology_cases(load_model, load_npz)[cid]
    m = load_model(c.grid)
    ref = rows_reference(m, **c.ref_args())
    assert not np.isnan(ref).any()
    eng = _engine(c, m)
    eng.set_topology(np.tile(c.topo, (c.n_lanes, 1)), np.tile(c.shunt_bus, (c.n_lanes, 1)) if m.n_shunt else None)
    eng.ptdf_build(0)
    rows = _launch(eng, c, c.t0, c.n_rows)
    _compare(cid, rows, ref)
    # rows row0 .. of that launch, straight from the C ABI; one row too many is refused and writes nothing
    r0 = min(2, c.n_rows - 1)
    rc, later = _get_rows(eng, r0, c.n_rows - r0, 0, c.n_lanes)
    assert rc == 0 and np.array_equal(later, rows[r0:])
    rc, untouched = _get_rows(eng, r0, c.n_rows - r0 + 1, 0, c.n_lanes)
    assert rc == GPF_E_INVALID and (untouched == -7.0).all()
    # a lane sub-range (relaunches, fetches lanes lane0 .. lane0 + n)
    lane0 = 3 if c.n_lanes > 3 else 0
    n = min(5, c.n_lanes - lane0)
    part = _launch(eng, c, c.t0, c.n_rows, lane0=lane0, n=n)
    assert np.array_equal(part, rows[:, lane0:lane0 + n])
    # one row per launch
    for j in range(c.n_rows):
        one = _launch(eng, c, c.t0 + j, 1)
        assert one.shape == (1, c.n_lanes, m.n_line) and np.array_equal(one[0], rows[j]), j
    rc, _ = _get_rows(eng, 1, 1, 0, c.n_lanes)                      # the last launch had ONE row
    assert rc == GPF_E_INVALID
    eng.close()


@pytest.mark.parametrize("cid", BATCH_IDS)
def test_per_lane_topologies_every_row_vs_reference(cid, load_model, load_npz):
    """`ptdf_build_batch()`: about 40 lanes over 12 topologies of `random_topologies` (ragged classes, -1 padded slots, islanded ones),
    5 rows (no multiple of the tile height: a block holds a valid tile and one past the end), jitter + delta + offsets.  Every row of
    every lane against the reference on that lane's own topology; lanes of classes with a non-zero status are NaN in all 5 rows.  Then
    a rebuild after the lanes of three topologies moved to one with fewer active buses -- its class slot held a larger PTDF^T block."""
    c = per_lane_topology_cases(load_model, load_npz)[cid]
    m = load_model(c.grid)
    ref = rows_reference(m, **c.ref_args())
    eng = _engine(c, m)
    eng.set_topology(c.topo, c.shunt_bus if m.n_shunt else None)
    info = eng.ptdf_build_batch(with_lodf=False)
    assert info["n_classes"] == c.extra["n_topo"]
    rows = _launch(eng, c, c.t0, c.n_rows)
    _compare(cid, rows, ref)
    dead = info["class_status"][info["lane_class"]] != 0
    assert dead.any() and np.isnan(rows[:, dead]).all() and not np.isnan(rows[:, ~dead]).any()
    for j in range(c.n_rows):
        one = _launch(eng, c, c.t0 + j, 1)
        assert np.array_equal(one[0], rows[j], equal_nan=True), j
    # rebuild
    moved = c.extra["moved"]
    ref2 = rows_reference(m, **c.ref_args(topo=c.extra["topo_rebuild"]))
    eng.set_topology(c.extra["topo_rebuild"], c.shunt_bus if m.n_shunt else None)
    info2 = eng.ptdf_build_batch(with_lodf=False)
    assert info2["n_classes"] == c.extra["n_topo"] - 2
    slot = int(info2["lane_class"][np.nonzero(moved)[0][0]])
    assert (info2["lane_class"][moved] == slot).all() and info2["class_status"][slot] == 0
    assert info2["class_n"][slot] < info["class_n"][slot]              # the slot's block shrank: rows of the old one lie behind it
    rows2 = _launch(eng, c, c.t0, c.n_rows)
    _compare(cid + " rebuilt", rows2, ref2)
    eng.close()


@pytest.mark.parametrize("name", ["rte_case5_example", "l2rpn_case14_sandbox"])
def test_lodf_screening_of_a_modified_topology_and_lane_sub_ranges(name, load_model, load_npz):
    """`gpf_lodf_screen` on the single-topology LODF table the HOST builds, for a topology with one line out and one split substation
    (the base topology is all test_gpu_parity.py screens), over all 10 lanes and over lanes 3 .. 8 (`worst` is indexed by lane, the
    block's lanes by lane0 + r0): every lane and every outage against the brute-force DC N-1 of the oracle, same inf pattern, the
    tolerances of test_lodf_screening_matches_brute_force_dc_n1; the sub-range equals the slice bit for bit."""
    from grid2op_amd.engine import PowerFlowEngine
    m = load_model(name)
    rng = np.random.default_rng(17)
    topo = one_out_one_split(m, rng)
    base = LaneState.from_model(m)
    states = []
    for _ in range(10):
        st = LaneState.from_model(m)
        st.topo = topo.copy()
        st.load_p = base.load_p * (1 + 0.2 * rng.standard_normal(m.n_load))
        st.gen_p = base.gen_p * (1 + 0.2 * rng.standard_normal(m.n_gen))
        states.append(st)
    ch = load_npz(f"{name}.chronics.npz")
    lim = np.asarray(ch["thermal_limits"], dtype=np.float64) if "thermal_limits" in ch else np.full(m.n_line, 400.0)
    cap = np.sqrt(3.0) * m.sub_vn_kv[m.line_or_sub] * lim / 1000.0        # MW at 1 pu
    eng = PowerFlowEngine(m, n_lanes=10, device=0)
    inj, tp, sb = pack_states(m, states)
    eng.set_injections(inj)
    eng.set_topology(tp, sb)
    eng.ptdf_build(0)
    eng.ptdf_flows(fetch=False)
    def check(got, lanes, caps):
        assert not np.isnan(got).any()
        for row, k in zip(got, lanes):
            ref = refs[caps is not None][k]
            assert np.array_equal(np.isinf(row), np.isinf(ref)), (k, np.isinf(row), np.isinf(ref))
            ok = np.isfinite(ref)
            assert np.allclose(row[ok], ref[ok], rtol=2e-5, atol=2e-4 if caps is None else 2e-6), (k, np.abs(row[ok] - ref[ok]).max())

    refs = [[dc_n1_worst_loading(m, st, caps) for st in states] for caps in (None, cap)]
    for k in range(3, 9):                                          # (the two runs leave different values in the engine's result buffer)
        fin = np.isfinite(refs[0][k])
        assert fin.any() and (np.abs(refs[0][k][fin] - refs[1][k][fin]) > 0.5 * np.abs(refs[0][k][fin])).all()
    for caps in (None, cap):
        # the sub-range FIRST: the engine's result buffer is indexed by lane and persists between calls -- what lanes 3 .. 8 hold now is fresh
        # memory or the other capacities' values, so a launch that wrote other lanes, or nothing, cannot hand back correct results
        part = eng.lodf_screen(lane0=3, n=6, cap_mw=caps)
        check(part, range(3, 9), caps)
        w = eng.lodf_screen(cap_mw=caps)
        check(w, range(10), caps)
        assert np.array_equal(part, w[3:9])
    eng.close()


def test_other_tile_heights_in_fresh_processes():
    """MT = 1 and MT = 4: this file again, in a fresh child process each (`GRIDPF_PTDF_MT` is read once per process).  The tile height
    cannot be observed through the API: that the children run the other instantiations rests on the single host line of
    gpf_ptdf_flows_rows that reads the variable, in a process that has not called gpf_ptdf_flows_rows before.  One test, asserting
    after each child: a child that fails, aborts or times out keeps the next one from starting.  The children report the output of their
    passed tests (-rP): their `[ptdf_rows]` figure lines are printed here again."""
    if os.environ.get("GRIDPF_PTDF_MT") is not None:
        pytest.skip("this IS a run at a chosen tile height")
    for mt in ("1", "4"):
        p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-rP", "tests/test_gpu_ptdf_rows.py"],
                           capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, GRIDPF_PTDF_MT=mt), timeout=CHILD_TIMEOUT_S)
        figures = [ln for ln in p.stdout.splitlines() if ln.startswith("[ptdf_rows] ")]
        print("\n".join(figures))
        tail = p.stdout[-3000:] + p.stderr[-2000:]
        assert p.returncode == 0, (mt, tail)
        last = p.stdout.strip().splitlines()[-1]
        assert " passed" in last and "failed" not in last and "error" not in last, (mt, tail)
        assert len(figures) == len(SINGLE_IDS) + 2 * len(BATCH_IDS) and all(f'"mt": "{mt}"' in ln for ln in figures), (mt, figures)
