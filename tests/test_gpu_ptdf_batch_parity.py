"""GPU parity tests of `gpf_ptdf_build_batch` (`ptdf_build_lds_kernel` / `ptdf_build_kernel`, grid2op_amd/csrc/gridpf_ptdf_batch.hpp; host
half in gridpf_capi_ptdf.hip) and of what runs on its tables (`ptdf_flows_kernel`, `lodf_screen_kernel`, `gpf_ptdf_batch_get`), at the
sizes the suite had never launched: more than 128 non-reference buses (N = 9, 10 block rows in the global-memory kernel, classes of
different n_pad in one build, the host's switch at 128 | 129), the tile boundaries 16 | 17 and 48 | 49, N = 1 with 3 .. 6 buses, and the
status codes 1 (singular pivot, both tile inverters, both pivots of a 2 x 2 block), 2 and 3.

Every PTDF and every LODF entry of every class is compared with the float64 reference of tests/ptdf_batch_ref.py (oracle/pf_oracle.py
`ptdf` and its DC power flow with one line forced off): PTDF within the suite's 1e-9, columns of inactive / reference buses exactly 0;
LODF with the NaN columns (islanding outages), the zero columns (lines out of service; stubs: a line end alone on a bus) and the -1
diagonal EXACT and everything else within `lodf_tolerance` (float32 rounding of the stored value + twice the PTDF bar pushed through the
quotient).  Flows and N-1 screening per lane at the tolerances of tests/test_gpu_ptdf_batch.py.  The cases are in
tests/ptdf_batch_cases.py; tests/test_ptdf_batch_ref_cpu.py proves without a GPU what each delivers.  Every comparison prints one
`[ptdf_batch]` JSON line before it asserts.

Which kernel built a class cannot be observed through the API: the `kernel` field restates the host's rule (largest n_pad of the build
<= 128 and `GRIDPF_PTDFB_GLOBAL` unset: resident), read at every call.

Measured on an MI355X, first green run of this file (max error / tolerance over all classes, builds and modes of the case):

  case                            ptdf      lodf    flows    screen
  idf_over_128                    4.3e-05   0.41    0.0096   0.0043   (gpf_ptdf_build on the nr = 145 lane: ptdf 1.9e-05, screen 0.0043)
  idf_switch                      1.4e-05   0.41    0.0091   0.0053
  idf_forced_global_vs_resident   1.4e-05   0.42    0.0091   0.0041
  neurips_48_49                   4.0e-05   0.36    0.0080   0.0022
  case14_16_17                    4.6e-06   0.28    0.0083   0.0047
  case5_floor                     6.7e-07   0.33    0.0025   0.0021
  stub_and_bridge_case14          4.1e-06   0.37    0.0063   0.0039
  stub_and_bridge_neurips         1.8e-05   0.43    0.0068   0.0037
  singular_pivot                  1.3e-06   0.35    0.0038   0.0030

The LODF figures are above 0.1 of the bar and were looked into: they are the float32 storage of the table and nothing else.  The bar's
first term is a whole float32 spacing relative to |ref| (2^-23 |ref|); rounding the EXACT value to nearest errs by up to half a spacing,
i.e. up to 0.5 of that term, and `float32(reference)` itself gives 0.415, 0.415, 0.42, 0.359, 0.282, 0.335, 0.374, 0.432, 0.345 on these
nine cases (tests/test_ptdf_batch_ref_cpu.py::test_float32_storage_alone_takes_up_to_half_the_lodf_bar) -- the kernels' figures, digit for
digit.  What the kernels add on top is reported per class as `err_beyond_f32_storage_over_tol`.  Wall time of the file: 14.1 s in the tests
(5.4 s idf_over_128, 4.5 s idf_switch, 1.9 s neurips_48_49, 1.7 s idf_forced_global_vs_resident; the references' DC power flows)."""
import json
import time

import numpy as np
import pytest

from oracle.pf_oracle import dc_bus_injection, dc_n1_worst_loading

from helpers import pack_states
from ptdf_batch_cases import CASE_IDS, batch_cases, class_reference, n_blocks
from ptdf_batch_ref import PTDF_BAR, active_buses, lodf_tolerance, reference_buses, state_of

pytestmark = pytest.mark.gpu


def _report(what, got, ref, tol, strict=False, **tag):
    """every entry; prints the figures before it asserts"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    special_same = np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    live = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        err = np.abs(got[live] - ref[live])
    tol = np.broadcast_to(tol, ref.shape)[live]
    ratio = err / tol
    fig = dict(what=what, **tag, entries=int(ref.size), nan_entries=int((~live).sum()), max_abs_err=float(err.max()) if err.size else 0.0,
               max_err_over_tol=float(ratio.max()) if err.size else 0.0, nan_pattern_equal=bool(special_same))
    print("[ptdf_batch] " + json.dumps(fig))
    assert special_same, fig
    assert not np.isnan(ratio).any() and (fig["max_err_over_tol"] < 1.0 if strict else fig["max_err_over_tol"] <= 1.0), fig
    return fig


def _check_lodf(L, p, **tag):
    """NaN columns, zero columns and the diagonal exact; the quotient columns within `lodf_tolerance`."""
    kind, ref = p["kind"], p["L"]
    zero = (kind == "off") | (kind == "stub")
    live = kind == "live"
    tol = lodf_tolerance(ref, p["inv_den"])
    tol = np.where(np.isnan(tol), 1.0, tol)                       # (columns that are no quotient: compared exactly below)
    # (what float32 storage of the EXACT value costs against this bar, and what the kernel adds to it: figures only)
    with np.errstate(invalid="ignore"):
        e32 = np.abs(ref.astype(np.float32).astype(np.float64) - ref)
        q = np.isfinite(ref)
        f32_only = float((e32[q] / tol[q]).max())
        beyond = float(((np.abs(L - ref)[q] - e32[q]) / tol[q]).max())
    fig = _report("lodf", L, ref, tol, **tag, nan_cols=int((kind == "nan").sum()), off_cols=int((kind == "off").sum()),
                  stub_cols=int((kind == "stub").sum()), f32_storage_alone_over_tol=f32_only, err_beyond_f32_storage_over_tol=beyond)
    assert (L[:, zero] == 0.0).all(), (tag, np.nonzero(zero)[0][(L[:, zero] != 0.0).any(axis=0)], kind[zero][(L[:, zero] != 0.0).any(axis=0)])
    assert np.isnan(L[:, kind == "nan"]).all(), tag
    assert (np.diag(L)[live] == -1.0).all(), tag
    return fig


def _screen_lanes(c, lane_topo, rows_ok, must=None):
    """Lanes whose screening is compared: all, or `c.screen_lanes` of them -- the first lane of every live class, then the others."""
    ok = [k for k in range(len(lane_topo)) if rows_ok[lane_topo[k]]]
    if c.screen_lanes is None or len(ok) <= c.screen_lanes:
        return ok
    first = [int(np.nonzero(lane_topo == i)[0][0]) for i in sorted(set(lane_topo[ok].tolist()))]
    pick = ([must] if must is not None else []) + [k for k in first if k != must] + [k for k in ok if k not in first and k != must]
    return sorted(pick[:c.screen_lanes])


def _build_and_check(c, m, eng, build, mode, refs_n1, must=None):
    lane_topo = c.builds[build]
    kern = c.kernel(build, mode)
    states = c.states(m, build)
    inj, topo, sb = pack_states(m, states)
    eng.set_injections(inj)
    eng.set_topology(topo, sb)
    info = eng.ptdf_build_batch(with_lodf=True)
    lc = info["lane_class"]
    used = sorted(set(lane_topo.tolist()))
    tag0 = dict(case=c.id, build=build, kernel=kern)
    # ---- partition: the classes are the topology rows
    assert info["n_classes"] == len(used) and sorted(set(lc.tolist())) == list(range(len(used))), (tag0, lc)
    for a in range(len(lane_topo)):
        assert np.array_equal(lc == lc[a], lane_topo == lane_topo[a]), (tag0, a)
    cls_of = {i: int(lc[np.nonzero(lane_topo == i)[0][0]]) for i in used}
    # ---- status and dimension
    got_status = {i: int(info["class_status"][cls_of[i]]) for i in used}
    got_n = {i: int(info["class_n"][cls_of[i]]) for i in used}
    print("[ptdf_batch] " + json.dumps(dict(what="status", **tag0, nr={i: c.nr[i] for i in used}, status=got_status, class_n=got_n)))
    assert got_status == {i: c.status[i] for i in used}, tag0
    assert got_n == {i: c.nr[i] for i in used}, tag0
    flows = eng.ptdf_flows()
    worst = eng.lodf_screen()
    tables = {}
    rows_ok = {i: c.status[i] == 0 for i in range(len(c.topos))}
    picked = _screen_lanes(c, lane_topo, rows_ok, must=must)
    for i in used:
        lanes = np.nonzero(lane_topo == i)[0]
        tag = dict(**tag0, topology=i, nr=c.nr[i], N=n_blocks(c.nr[i]))
        if c.status[i] != 0:                                      # no tables: NaN flows and NaN screening for every lane of the class
            assert np.isnan(flows[lanes]).all() and np.isnan(worst[lanes]).all(), tag
            continue
        p = class_reference(c, m, i)
        st = state_of(m, c.topos[i])
        T, L = eng.ptdf_class(cls_of[i], lodf=True)
        tables[i] = (T, L)
        _report("ptdf", T, p["T"], PTDF_BAR, strict=True, **tag)
        dead = ~(active_buses(m, st) & ~reference_buses(m, st))
        assert (T[:, dead] == 0.0).all(), tag
        _check_lodf(L, p, **tag)
        ref_f = np.stack([p["T"] @ dc_bus_injection(m, states[k]) for k in lanes])
        _report("flows", flows[lanes], ref_f, 2e-4 + 5e-6 * np.abs(ref_f), **tag)
        ks = [k for k in lanes if k in picked]
        if ks:
            for k in ks:
                if (build, k) not in refs_n1:
                    refs_n1[(build, k)] = dc_n1_worst_loading(m, states[k], None)
            ref_w = np.stack([refs_n1[(build, k)] for k in ks])
            with np.errstate(invalid="ignore"):
                _report("screen", worst[ks], ref_w, 2e-4 + 2e-5 * np.abs(ref_w), **tag, lanes=len(ks))
            assert not np.isnan(worst[lanes]).any(), tag
    return dict(info=info, tables=tables, flows=flows, worst=worst, states=states, cls_of=cls_of)


def _same_tables(a, b):
    assert sorted(a["tables"]) == sorted(b["tables"])
    for i in a["tables"]:
        assert np.array_equal(a["tables"][i][0], b["tables"][i][0]) and np.array_equal(a["tables"][i][1], b["tables"][i][1], equal_nan=True), i
    assert np.array_equal(a["info"]["class_status"], b["info"]["class_status"]) and np.array_equal(a["info"]["class_n"], b["info"]["class_n"])
    assert np.array_equal(a["info"]["lane_class"], b["info"]["lane_class"])


@pytest.mark.parametrize("cid", CASE_IDS)
def test_every_table_entry_flow_and_screening_vs_reference(cid, load_model, monkeypatch):
    """What each case pins is in its docstring in tests/ptdf_batch_cases.py.  Per build and mode: the partition of the lanes, status and
    dimension of every class, every PTDF / LODF entry, the flows of every lane, the screening of every lane (6 lanes on the 186-line
    grid).  idf_switch: the first and the third build (resident, around a global one on the same engine) give the same tables bit for
    bit.  idf_over_128 and the stub_and_bridge cases: `gpf_ptdf_build` on a lane of the nr = 145 class / of the two stub rows and the
    bridge row gives that reference too (PTDF; the screening of that lane on the host-built LODF table, which has no getter), and the
    batch build that follows gives the tables of the one before bit for bit."""
    from grid2op_amd.engine import PowerFlowEngine
    t_start = time.perf_counter()
    c = batch_cases(load_model)[cid]
    m = c.model(load_model)
    n_lanes = len(c.builds[0])
    singles = [(int(i), int(np.nonzero(c.builds[0] == i)[0][0])) for i in np.atleast_1d(c.extra.get("single", []))]
    single_lane = singles[0][1] if c.screen_lanes is not None and singles else None       # (must be among the screened lanes)
    eng = PowerFlowEngine(m, n_lanes=n_lanes, device=0)
    refs_n1 = {}
    runs = {}
    for mode in c.modes:
        if mode == "global":
            monkeypatch.setenv("GRIDPF_PTDFB_GLOBAL", "1")
        else:
            monkeypatch.delenv("GRIDPF_PTDFB_GLOBAL", raising=False)
        for build in range(len(c.builds)):
            runs[(mode, build)] = _build_and_check(c, m, eng, build, mode, refs_n1, must=single_lane if build == 0 else None)
    monkeypatch.delenv("GRIDPF_PTDFB_GLOBAL", raising=False)
    if cid == "idf_switch":
        _same_tables(runs[("default", 0)], runs[("default", 2)])
    before = runs[("default", 0)]
    for i, k in singles:
        p = class_reference(c, m, i)
        tag = dict(case=cid, build=0, kernel="host", topology=i, nr=c.nr[i], N=n_blocks(c.nr[i]), stub_cols=int((p["kind"] == "stub").sum()))
        eng.ptdf_build(lane=k)
        _report("ptdf gpf_ptdf_build", eng.ptdf(), p["T"], PTDF_BAR, strict=True, **tag)
        eng.ptdf_flows(fetch=False)                              # every lane on lane k's tables: lane k's own flows are its DC power flow
        w1 = eng.lodf_screen(lane0=k, n=1)
        ref_w = refs_n1[(0, k)][None]
        with np.errstate(invalid="ignore"):
            _report("screen gpf_ptdf_build", w1, ref_w, 2e-4 + 2e-5 * np.abs(ref_w), **tag, lanes=1)
    if singles:
        info = eng.ptdf_build_batch(with_lodf=True)
        after = dict(info=info, tables={j: eng.ptdf_class(before["cls_of"][j], lodf=True) for j in before["tables"]})
        _same_tables(before, after)
        assert np.array_equal(eng.ptdf_flows(), before["flows"], equal_nan=True) and np.array_equal(eng.lodf_screen(), before["worst"], equal_nan=True)
    eng.close()
    print("[ptdf_batch] " + json.dumps(dict(what="wall", case=cid, seconds=round(time.perf_counter() - t_start, 2))))
