"""The bus-graph observation (include/gridpf.h gpf_set_graph_obs) without a GPU: the restatement of tests/graph_ref.py against the answers
recorded from the unmodified reference (tests/golden/graph_*.npz, made by tests/golden/make_graph_fixtures.py), the library's rule core
(tests/native/graph_emul.cpp, the same header the kernel compiles) against the restatement bit for bit, and the ABI, the binding and the
refusals through a header-only handle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import graph_ref as G
from conftest import ROOT

PF_TOL_MVA = 1e-8
FIXTURES = {"graph_case14.npz": "l2rpn_case14_sandbox", "graph_wcci118.npz": "l2rpn_wcci_2022_dev"}


def emul_of_state(m, n_busbar, st, over=False, cooldown=True):
    row, off = G.pack_row(st)
    return G.emul_lane(m, n_busbar, topo_vect=st["topo_vect"], shunt_bus=st["shunt_bus"], row=row, offsets=off,
                       sub_cooldown=st["sub_cooldown"] if cooldown else None, over=over)


def assert_same(got, want, what):
    for k in ("index", "features", "dense"):
        assert G.same_bits(got[k], want[k]), (what, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:5])


# ---- the restatement against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", list(FIXTURES))
def test_restatement_agrees_with_the_recorded_reference(fname, load_model, load_npz):
    """integers exactly (disconnected entries: -1 here, at most 10 % of the element entries), floats within (terms + 1) 2^-24 sum |terms|"""
    fx, m = load_npz(fname), load_model(FIXTURES[fname])
    excluded = compared = 0
    for i in range(len(fx["done"])):
        e, c, _ = G.compare_reference(m, fx, i)
        excluded, compared = excluded + e, compared + c
    assert 0 < excluded <= 0.10 * compared


def test_fixtures_cover_what_the_recorder_promises(load_npz):
    c14, wcci = load_npz("graph_case14.npz"), load_npz("graph_wcci118.npz")
    assert list(c14["tags"]) == ["reset", "one_split", "two_splits", "line_open", "line_still_open", "line_reconnected", "game_over"]
    assert list(c14["ref_n_bus"]) == [14, 15, 16, 16, 16, 16, 1] and c14["done"][-1] == 1 and (c14["shunt_bus"][:-1] == 1).all()
    assert wcci["ref_n_bus"].max() > 128 and (np.abs(wcci["storage_p"]) > 0.1).any() and not wcci["line_status"][2][30]


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_kirchhoff_rows_of_the_flow_planes(fname, load_model, load_npz):
    """A row of a flow plane sums to zero up to two things, and their sum is the bound: the float32 roundings of its terms, (terms + 1)
    2^-24 sum |terms| over the node's terms and the flows that leave the bus, and the power flow's own stopping criterion, a mismatch of at
    most tol_mva = 1e-8 MVA at every bus (the default of the oracle behind the recorded environment and of gpf_step_opts) -- which is what
    is left on a bus whose terms are all (nearly) zero."""
    fx, m = load_npz(fname), load_model(FIXTURES[fname])
    for i in range(len(fx["done"])):
        r = G.restate(m, 2, G.state_of(fx, i), over=bool(fx["done"][i]))
        for pl in (0, 1):
            rows, bound = r["dense"][1 + pl].astype(np.float64).sum(1), r["bound_rows"][pl] + PF_TOL_MVA
            print(fname, i, pl, "worst |row sum| / bound", float(np.max(np.abs(rows) / bound)))
            assert (np.abs(rows) <= bound).all(), (i, pl, float(np.abs(rows).max()))


# ---- the library's rule core against the restatement, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("fname", list(FIXTURES))
def test_emulator_equals_restatement_on_the_fixtures(fname, load_model, load_npz):
    fx, m = load_npz(fname), load_model(FIXTURES[fname])
    for i in range(len(fx["done"])):
        st = G.state_of(fx, i)
        for over in sorted({False, bool(fx["done"][i])}):
            assert_same(emul_of_state(m, 2, st, over=over), G.restate(m, 2, st, over=over), (fname, i, over))


@pytest.mark.parametrize("grid,n_busbar", [("rte_case5_example", 2), ("rte_case5_example", 3), ("educ_case14_storage", 2), ("educ_case14_storage", 3),
                                           ("l2rpn_wcci_2022_dev", 2)])
def test_emulator_equals_restatement_on_synthetic_states(grid, n_busbar, load_model):
    """random busbars for every element (shunts on busbar 2 and 3 among them), open lines, disconnected elements; with and without cooldowns"""
    m = load_model(grid)
    rng = np.random.default_rng(n_busbar * 1000 + m.n_sub)
    seen_dead = seen_shunt2 = 0
    for rep in range(3 if m.n_sub > 100 else 40):
        st = G.random_state(m, n_busbar, rng, p_open=(0.0, 0.15, 0.6)[rep % 3])
        want = G.restate(m, n_busbar, st if rep % 2 else dict(st, sub_cooldown=None))
        assert_same(emul_of_state(m, n_busbar, st, cooldown=bool(rep % 2)), want, (grid, n_busbar, rep))
        lay = G.layout(m, n_busbar)
        seen_dead += int(((want["index"][lay["load_bus"]] < 0) & (st["topo_vect"][m.load_pos_topo_vect] > 0)).sum())
        seen_shunt2 += int(((want["index"][lay["shunt_bus"]] >= 0) & (st["shunt_bus"] >= 2)).sum())
    assert seen_dead > 0 and (seen_shunt2 > 0 or m.n_shunt == 0)


def test_an_element_alone_on_a_dead_busbar(load_model):
    """a load alone on busbar 2: the busbar holds no line end, so it is no bus -- the load gets -1 and its power appears nowhere"""
    m = load_model("educ_case14_storage")
    rng = np.random.default_rng(5)
    st = G.random_state(m, 2, rng, p_open=0.0, p_off=0.0)
    st["topo_vect"][:] = 1
    st["shunt_bus"][:] = 1
    st["topo_vect"][m.load_pos_topo_vect[3]] = 2
    r, lay = G.restate(m, 2, st), G.layout(m, 2)
    assert r["index"][0] == m.n_sub and r["index"][lay["load_bus"]][3] == -1 and (np.delete(r["index"][lay["load_bus"]], 3) >= 0).all()
    absent = dict(st, topo_vect=np.ones_like(st["topo_vect"]), load_p=st["load_p"].copy(), load_q=st["load_q"].copy())
    absent["load_p"][3] = absent["load_q"][3] = 0.0         # (x - 0.0 is x: the same sums as without the load)
    assert G.same_bits(r["features"], G.restate(m, 2, absent)["features"]) and st["load_p"][3] != 0
    assert_same(emul_of_state(m, 2, st), r, "dead busbar")


def test_parallel_lines_add_up_and_split_pairs_do_not(load_model):
    """lines 17 / 18 of the 118-substation grid join the same two substations: on the same buses their flows add up in index order; with
    one end of line 18 on busbar 2 each line has its own pair of entries"""
    m = load_model("l2rpn_wcci_2022_dev")
    assert {m.line_or_sub[17], m.line_ex_sub[17]} == {m.line_or_sub[18], m.line_ex_sub[18]}
    st = G.random_state(m, 2, np.random.default_rng(1), p_open=0.0, p_off=0.0)
    st["topo_vect"][:] = 1
    r, lay = G.restate(m, 2, st), G.layout(m, 2)
    a, b = r["index"][lay["line_or_bus"]][17], r["index"][lay["line_ex_bus"]][17]
    same_dir = m.line_or_sub[17] == m.line_or_sub[18]
    t18 = st["p_or"][18] if same_dir else st["p_ex"][18]
    assert r["dense"][1, a, b] == np.float32(-(np.float64(st["p_or"][17]) + np.float64(t18)))
    assert_same(emul_of_state(m, 2, st), r, "parallel")
    st["topo_vect"][m.line_or_pos_topo_vect[18]] = 2
    st["topo_vect"][m.line_or_pos_topo_vect[19]] = 2          # (a second line end keeps the new bus from depending on line 18 alone)
    r = G.restate(m, 2, st)
    a, b = r["index"][lay["line_or_bus"]][17], r["index"][lay["line_ex_bus"]][17]
    assert r["dense"][1, a, b] == np.float32(-np.float64(st["p_or"][17]))
    assert_same(emul_of_state(m, 2, st), r, "pair apart")


def test_rule_core_under_sanitizers():
    """the stand-alone program of tests/native/graph_emul.cpp under AddressSanitizer + UBSan (host code; exactly sized arrays)"""
    out = subprocess.run([G.sanitized_program()], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


# ---- ABI, binding, refusals -------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gpf_set_graph_obs", "gpf_graph_layout", "gpf_graph_obs", "gpf_graph_obs_host")


def header():
    return open(os.path.join(ROOT, "include", "gridpf.h")).read()


def test_symbols_constants_and_abi():
    import __graft_entry__ as entry
    entry.build()
    from grid2op_amd import _capi, engine, sharding
    hdr = header()
    L = _capi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name in _capi.SIGNATURES and hasattr(L, name), name
    assert "#define GPF_ABI_VERSION 326" in hdr and "#define GPF_N_DEVICE_POINTERS 34" in hdr and L.gpf_version() == 326
    defs = dict(re.findall(r"#define GPF_GRAPH_(\w+) (\d+)", hdr))
    assert [int(defs[k.upper()]) for k in engine.GRAPH_SECTIONS] == list(range(8)) and int(defs["N_SECTIONS"]) == 8
    for k in engine.GRAPH_SECTIONS:
        assert getattr(engine, "GRAPH_" + k.upper()) == int(defs[k.upper()])
    assert _capi.GRAPH_N_SECTIONS == 8 and _capi.GRAPH_N_FEATURES == int(defs["N_FEATURES"]) == 4 and _capi.GRAPH_MAX_BUS == int(defs["MAX_BUS"])
    assert engine.GRAPH_SECTIONS == G.SECTIONS
    routes = {name: rule.__name__ for rule, names in sharding.ROUTES.items() for name in names}
    assert [routes[k] for k in ("set_graph_obs", "graph_layout", "graph_observation", "graph_observation_host")] == \
        ["every", "first", "per_shard_tensor", "gather"] and len(sharding.NOT_SHARDED) == 14


@pytest.mark.parametrize("grid,n_busbar", [("rte_case5_example", 3), ("l2rpn_wcci_2022_dev", 2)])
def test_layout_matches_the_header_order(grid, n_busbar, load_model):
    from grid2op_amd.engine import PowerFlowEngine
    m = load_model(grid)
    eng = PowerFlowEngine(m, n_lanes=4, device=-1, n_busbar=n_busbar)
    lay, want = eng.graph_layout(), G.layout(m, n_busbar)
    assert list(lay)[:8] == list(G.SECTIONS) and all(lay[k] == want[k] for k in G.SECTIONS)
    assert lay["width"] == want["width"] and lay["NB"] == m.n_sub * n_busbar and lay["n_features"] == 4
    eng.close()


def test_refusals_through_a_header_only_handle(load_model):
    """validated before the device is touched: feature off, lane range, null outputs, NB above the cap"""
    from grid2op_amd.engine import PowerFlowEngine, GridPFError
    m = load_model("l2rpn_case14_sandbox")
    eng = PowerFlowEngine(m, n_lanes=4, device=-1)
    idx, feat = np.zeros(4 * 200, np.int32), np.zeros(4 * 28 * 4, np.float32)
    ip, fp = idx.ctypes.data_as(C.POINTER(C.c_int32)), feat.ctypes.data_as(C.POINTER(C.c_float))
    for name in ("gpf_graph_obs", "gpf_graph_obs_host"):
        with pytest.raises(GridPFError, match="graph observation is off"):
            eng._call(name, 0, 4, ip, fp, None)
    with pytest.raises(GridPFError, match="graph observation is off"):
        eng.graph_observation_host()
    with pytest.raises(GridPFError, match="graph observation is off"):
        eng.graph_observation()
    eng.set_graph_obs(True)
    for name in ("gpf_graph_obs", "gpf_graph_obs_host"):
        for lane0, n in ((-1, 2), (3, 2), (0, 5), (0, -1)):
            with pytest.raises(GridPFError, match="bad lane range"):
                eng._call(name, lane0, n, ip, fp, None)
        with pytest.raises(GridPFError, match="must not be NULL"):
            eng._call(name, 0, 4, None, fp, None)
        with pytest.raises(GridPFError, match="must not be NULL"):
            eng._call(name, 0, 4, ip, None, None)
        with pytest.raises(GridPFError, match="header-only handle"):
            eng._call(name, 0, 4, ip, fp, None)
    eng.set_graph_obs(False)
    with pytest.raises(GridPFError, match="graph observation is off"):
        eng._call("gpf_graph_obs", 0, 4, ip, fp, None)
    eng.close()
    big = PowerFlowEngine(load_model("l2rpn_wcci_2022_dev"), n_lanes=4, device=-1, n_busbar=9)      # 1062 buses
    with pytest.raises(GridPFError, match="more than GPF_GRAPH_MAX_BUS = 1024"):
        big.set_graph_obs(True)
    big.close()
