"""The bus-graph observation on the device (include/gridpf.h: gpf_set_graph_obs / gpf_graph_obs; grid2op_amd/csrc/gridpf_graph.hpp) on the
engine's own result rows: index row, node features and dense planes equal the host emulator of the same rule core bit for bit, and the
numpy restatement of tests/graph_ref.py with it -- at every place in the batch, between calls, between the device and the host getter,
into caller-supplied tensors and through a ShardedEngine."""
import numpy as np
import pytest

import graph_ref as G
from conftest import golden_path
from topo_rules_ref import topo_pos_sub

pytestmark = pytest.mark.gpu


def model_of(name):
    from grid2op_amd.grid_model import GridModel
    return GridModel.load_npz(golden_path(f"{name}.grid.npz"))


def solved_engine(m, n_busbar, topo, shunt, scale, factory=None):
    """an engine whose lanes hold the given topologies and scaled loads, after one power flow"""
    from grid2op_amd.engine import PowerFlowEngine
    n = len(topo)
    eng = factory(n) if factory else PowerFlowEngine(m, n_lanes=n, device=0, n_busbar=n_busbar)
    inj = eng.pack_injections(n)
    inj[:, eng.inj_slices["load_p"]] *= np.asarray(scale)[:, None]
    if m.n_storage:
        inj[:, eng.inj_slices["storage_p"]] = np.where(np.arange(m.n_storage) % 2, -2.0, 3.0)
    eng.set_injections(inj)
    eng.set_topology(topo, shunt if m.n_shunt else None)
    eng.runpf()
    return eng


def expected(m, eng, n_busbar, lane0, n, sub_cd=None, over=None):
    """the emulator on the engine's own rows, lane by lane, held to the restatement on the way"""
    res = eng.results(lane0, n, with_bus=False)
    offs = [eng.out_slices[k].start for k in G.FLOATS]
    rows = []
    for k in range(n):
        o = bool(over[k]) if over is not None else False
        cd = None if sub_cd is None else sub_cd[k]
        e = G.emul_lane(m, n_busbar, topo_vect=res.topo_vect[k], shunt_bus=res.shunt_bus[k], row=res.out[k], offsets=offs, sub_cooldown=cd, over=o)
        st = {f: res.out[k, eng.out_slices[f]] for f in G.FLOATS}
        st.update(topo_vect=res.topo_vect[k], shunt_bus=res.shunt_bus[k], sub_cooldown=cd)
        r = G.restate(m, n_busbar, st, over=o)
        assert all(G.same_bits(e[key], r[key]) for key in ("index", "features", "dense")), k
        rows.append(e)
    return {key: np.stack([r[key] for r in rows]) for key in ("index", "features", "dense")}, res


def assert_same(got, want, what=""):
    for key in ("index", "features", "dense"):
        assert G.same_bits(got[key], want[key]), (what, key, np.argwhere(np.asarray(got[key]) != np.asarray(want[key]))[:5])


def on_host(tensors):
    return {key: None if t is None else t.cpu().numpy() for key, t in zip(("index", "features", "dense"), tensors)}


@pytest.mark.parametrize("n_busbar", [2, 3])
def test_case5_lanes_equal_the_emulator_at_every_place_in_the_batch(n_busbar):
    """5 lanes from lane 1 (not a multiple of the 4 lanes of a block), their mirror image behind them; NB = 10 and 15"""
    import torch
    from grid2op_amd.engine import GridPFError
    m = model_of("rte_case5_example")
    topo, shunt, scale = G.case5_lanes(m, n_busbar)
    order = [0] + list(range(5)) + list(range(5))[::-1]
    eng = solved_engine(m, n_busbar, topo[order], shunt[order], scale[order])
    with pytest.raises(GridPFError, match="graph observation is off"):
        eng.graph_observation(1, 5)
    eng.set_graph_obs(True)
    want, res = expected(m, eng, n_busbar, 1, 5)
    assert res.converged.all()
    lay = eng.graph_layout()
    assert want["index"][:, 0].tolist() == [5, 4 + n_busbar, 4 + n_busbar, 6, 5] and (want["index"][2, lay["line_or_bus"]] == -1).sum() == 1
    got = eng.graph_observation_host(1, 5, dense=True)
    assert_same(got, want, "host getter")
    assert_same(eng.graph_observation_host(1, 5, dense=True), got, "second call")
    mirror = eng.graph_observation_host(6, 5, dense=True)
    assert_same({k: v[::-1] for k, v in mirror.items()}, got, "mirror image")
    for k in range(5):                                      # alone, and in a pair: another wavefront of another block
        assert_same(eng.graph_observation_host(1 + k, 1, dense=True), {key: v[k:k + 1] for key, v in got.items()}, ("alone", k))
    for k in range(4):
        assert_same(eng.graph_observation_host(1 + k, 2, dense=True), {key: v[k:k + 2] for key, v in got.items()}, ("pair", k))
    no_dense = eng.graph_observation_host(1, 5)
    assert no_dense["dense"] is None and G.same_bits(no_dense["index"], got["index"]) and G.same_bits(no_dense["features"], got["features"])
    # device tensors; caller-supplied outputs
    views = eng.device_views()
    dev = eng.graph_observation(1, 5, dense=True)
    views["stream"].synchronize()
    assert dev[0].dtype == torch.int32 and tuple(dev[2].shape) == (5, 3, lay["NB"], lay["NB"]) and dev[1].device.index == 0
    assert_same(on_host(dev), got, "device tensors")
    assert eng.graph_observation(1, 5)[2] is None
    mine = (torch.full((5, lay["width"]), -9, dtype=torch.int32, device="cuda:0"), torch.full((5, lay["NB"], 4), 7.5, device="cuda:0"),
            torch.full((5, 3, lay["NB"], lay["NB"]), 7.5, device="cuda:0"))
    torch.cuda.synchronize()
    back = eng.graph_observation(1, 5, out_index=mine[0], out_features=mine[1], out_dense=mine[2])
    views["stream"].synchronize()
    assert all(a is b for a, b in zip(back, mine))
    assert_same(on_host(mine), got, "caller-supplied tensors")
    mine[2].fill_(3.0)
    torch.cuda.synchronize()
    back = eng.graph_observation(1, 5, out=mine)
    views["stream"].synchronize()
    assert_same(on_host(back), got, "the three as one tuple")
    with pytest.raises(ValueError):
        eng.graph_observation(1, 4, out_index=mine[0])
    with pytest.raises(ValueError):
        eng.graph_observation(1, 5, out_features=mine[1].double())
    with pytest.raises(TypeError):
        eng.graph_observation(1, 5, out_index=mine[0], out=mine)
    with pytest.raises(GridPFError, match="bad lane range"):
        eng.graph_observation_host(8, 4)
    eng.set_graph_obs(False)
    before = torch.cuda.memory_allocated(0)
    with pytest.raises(GridPFError, match="graph observation is off"):
        eng.graph_observation(1, 5, dense=True)
    with pytest.raises(GridPFError, match="graph observation is off"):
        eng.graph_observation_host(1, 5)
    assert torch.cuda.memory_allocated(0) == before
    eng.close()


def test_case14_replay_game_over_and_cooldowns():
    """7 lanes replay the recorded topologies (the last one with the recorded game-over line open) through one env step that carries a
    topology action: the substation cooldown shows in column 3, the failed lane gets the game-over rows, or -- fill off -- its own"""
    from grid2op_amd.engine import PowerFlowEngine
    m = model_of("l2rpn_case14_sandbox")
    fx = np.load(golden_path("graph_case14.npz"))
    ch = np.load(golden_path("l2rpn_case14_sandbox.chronics.npz"))
    topo = np.array(list(fx["topo_vect"][:6]) + [G.open_line(m, fx["topo_vect"][5], int(fx["game_over_line"]))], np.int32)
    shunt = np.array(list(fx["shunt_bus"][:6]) + [fx["shunt_bus"][5]], np.int32)
    eng = PowerFlowEngine(m, n_lanes=7, device=0)
    eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    eng.set_thermal_limits(ch["thermal_limits"])
    eng.set_lane_chronics(lane_offset=(5 * np.arange(7)).astype(np.int32))
    eng.set_topology(topo, shunt)
    moved = np.flatnonzero(fx["topo_vect"][1] != fx["topo_vect"][0])
    sub = int(topo_pos_sub(m)[moved[0]])
    eng.upload_topo_actions([{"set_bus": {int(p): 1 for p in moved}}])             # the first split, merged again
    eng.set_topo_rules(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=0)
    eng.set_lane_topo_actions(np.array([-1, 0, -1, -1, -1, -1, -1], np.int32))
    eng.step(1)
    done = eng.episode()[0].astype(bool)
    cd = eng.sub_cooldown()
    assert done.tolist() == [False] * 6 + [True] and cd[1, sub] > 0 and not cd[0].any()
    eng.set_graph_obs(True)
    want, res = expected(m, eng, 2, 0, 7, sub_cd=cd, over=done)
    assert res.converged[:6].all() and want["index"][:, 0].tolist() == [14, 14, 16, 16, 16, 16, 1]
    got = eng.graph_observation_host(dense=True)
    assert_same(got, want, "fill on")
    lay = eng.graph_layout()
    k = int(np.flatnonzero(got["index"][1, lay["bus_global"]] == sub)[0])
    assert got["features"][1, k, 3] == cd[1, sub] and not got["features"][0, :, 3].any()
    assert got["index"][6, lay["gen_bus"]].tolist() == [0] * m.n_gen and not got["features"][6].any() and not got["dense"][6].any()
    eng.set_graph_obs(True, game_over_fill=False)
    want_off, _ = expected(m, eng, 2, 0, 7, sub_cd=cd)
    got_off = eng.graph_observation_host(dense=True)
    assert_same(got_off, want_off, "fill off")
    assert got_off["index"][6, 0] == 0 and (got_off["index"][6, 1:] == -1).all() and G.same_bits(got_off["index"][:6], got["index"][:6])
    eng.close()


def test_wcci_lanes_cross_two_chunks_of_64_buses_and_merge_parallel_lines():
    """NB = 236, 186 lines: a lane with more than 128 live buses, parallel pairs joined, opened and on different busbars, shunts on busbars
    1 and 2, storage units that run"""
    m = model_of("l2rpn_wcci_2022_dev")
    fx = np.load(golden_path("graph_wcci118.npz"))
    topo, shunt, scale = G.wcci_lanes(m, fx)
    eng = solved_engine(m, 2, topo, shunt, scale)
    eng.set_graph_obs(True)
    want, res = expected(m, eng, 2, 0, 6)
    assert res.converged.all() and want["index"][1, 0] > 128 and want["index"][0, 0] == 118
    lay = eng.graph_layout()
    assert lay["NB"] == 236 and (want["index"][4, lay["shunt_bus"]] >= 118).any() and (want["index"][5, lay["shunt_bus"]] >= 0).all()
    got = eng.graph_observation_host(dense=True)
    assert_same(got, want, "host getter")
    lor, lex = got["index"][:, lay["line_or_bus"]], got["index"][:, lay["line_ex_bus"]]
    p_or = res.out[:, eng.out_slices["p_or"]]
    same_dir = m.line_or_sub[17] == m.line_or_sub[18]
    t18 = (p_or if same_dir else res.out[:, eng.out_slices["p_ex"]])[0, 18]
    assert got["dense"][0, 1, lor[0, 17], lex[0, 17]] == np.float32(-(np.float64(p_or[0, 17]) + np.float64(t18)))       # the pair adds up
    assert {lor[1, 17], lex[1, 17]} != {lor[1, 18], lex[1, 18]}                                                            # ... apart: each its own entry
    assert got["dense"][1, 1, lor[1, 17], lex[1, 17]] == np.float32(-np.float64(p_or[1, 17]))
    assert lor[2, 30] == -1 and got["dense"][2, 1, lor[2, 31], lex[2, 31]] == np.float32(-np.float64(p_or[2, 31]))          # ... one open
    assert np.abs(res.out[:, eng.out_slices["storage_p"]]).min() > 1.0
    dev = eng.graph_observation(dense=True)
    eng.sync()
    assert_same(on_host(dev), got, "device tensors")
    assert_same(eng.graph_observation_host(3, 3, dense=True), {k: v[3:] for k, v in got.items()}, "a sub-range")
    eng.close()


@pytest.mark.parametrize("grid,n_busbar", [("rte_case5_example", 3), ("l2rpn_wcci_2022_dev", 2)])
def test_gathers_from_global_memory_give_the_same_bits(grid, n_busbar, monkeypatch):
    """GRIDPF_GRAPH_STAGE=0 turns the LDS copies of the lanes' rows off: the path of grids too large for them"""
    m = model_of(grid)
    topo, shunt, scale = G.case5_lanes(m, n_busbar) if m.n_sub == 5 else G.wcci_lanes(m, np.load(golden_path("graph_wcci118.npz")))
    got = []
    for stage in ("1", "0"):
        monkeypatch.setenv("GRIDPF_GRAPH_STAGE", stage)
        eng = solved_engine(m, n_busbar, topo, shunt, scale)
        eng.set_graph_obs(True)
        want, _ = expected(m, eng, n_busbar, 0, len(topo))
        got.append(eng.graph_observation_host(dense=True))
        assert_same(got[-1], want, stage)
        eng.close()
    assert_same(got[0], got[1], "staged against not staged")


def test_two_shards_on_one_device_equal_one_engine():
    import torch
    from grid2op_amd.sharding import ShardedEngine
    m = model_of("l2rpn_case14_sandbox")
    fx = np.load(golden_path("graph_case14.npz"))
    topo = np.array(list(fx["topo_vect"][:6]) + [fx["topo_vect"][2], fx["topo_vect"][0], fx["topo_vect"][3]], np.int32)
    shunt = np.ones((9, m.n_shunt), np.int32)
    scale = 1.0 + 0.01 * np.arange(9)
    one = solved_engine(m, 2, topo, shunt, scale)
    sh = solved_engine(m, 2, topo, shunt, scale, factory=lambda n: ShardedEngine(m, n, devices=[0, 0]))
    assert sh.blocks == [(0, 5), (5, 4)]
    for e in (one, sh):
        e.set_graph_obs(True)
    want, _ = expected(m, one, 2, 0, 9)
    assert_same(one.graph_observation_host(dense=True), want, "one engine")
    assert sh.graph_layout() == one.graph_layout()
    assert_same(sh.graph_observation_host(dense=True), want, "gathered")
    assert_same(sh.graph_observation_host(3, 4, dense=True), {k: v[3:7] for k, v in want.items()}, "a range across the boundary")
    parts = sh.graph_observation(1, 7, dense=True)
    sh.sync()
    assert len(parts) == 2 and [p[0].shape[0] for p in parts] == [4, 3]
    assert_same({k: np.concatenate([on_host(p)[k] for p in parts]) for k in want}, {k: v[1:8] for k, v in want.items()}, "per shard tensors")
    lay = sh.graph_layout()
    mine = [(torch.zeros((k, lay["width"]), dtype=torch.int32, device="cuda:0"), torch.ones((k, lay["NB"], 4), device="cuda:0"), None) for k in (4, 3)]
    torch.cuda.synchronize()
    back = sh.graph_observation(1, 7, out=mine)
    sh.sync()
    assert all(b[0] is g[0] and b[1] is g[1] and b[2] is None for b, g in zip(back, mine))
    assert G.same_bits(np.concatenate([g[0].cpu().numpy() for g in mine]), want["index"][1:8])
    one.close(); sh.close()
