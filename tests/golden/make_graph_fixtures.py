#!/usr/bin/env python
"""Record the BUS-GRAPH observations of the unmodified reference environment (build container only, never on a GPU box).

    python tests/golden/make_graph_fixtures.py /path/to/reference [case14 wcci]    # -> tests/golden/graph_*.npz

The environment -- façade over the CPU oracle (tests/conformance_backend.py) -- is driven by a scripted topology agent:

  graph_case14.npz    l2rpn_case14_sandbox: one substation split, a second one, a line opened, left open, reconnected, then the line whose
                      loss is a game over (game_over_line)
  graph_wcci118.npz   l2rpn_wcci_2022_dev (118 substations, 186 lines, 7 storage units, parallel pairs 17/18, 30/31, 33/34, 131/132,
                      141/142): storage set-points every step, a dozen substations split in one action (more than 128 live buses; the two
                      lines of a pair on different busbars), one line of another pair opened

Per observation: the inputs (topo_vect, _shunt_bus, line_status, time_before_cooldown_sub, the P / Q / V vectors of every element class)
and the reference's answers: bus_connectivity_matrix(return_lines_index=True), both flow_bus_matrix calls with their five index vectors,
and the node attributes v and cooldown of get_energy_graph.  The recorder asserts its coverage, that the compared integer entries are
equal and that every recorded float lies within HALF the bound that tests/graph_ref.py derives for the reference's float32 evaluation;
entries of disconnected elements are compared with -1 instead of the reference's answer (at most 10 % of the element entries).  Data only."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
MAX_BYTES = 195216                     # what make_reward_fixtures.py holds itself to
PAIRS = ((17, 18), (30, 31), (33, 34), (131, 132), (141, 142))
INPUTS = ("p_or", "q_or", "v_or", "p_ex", "q_ex", "v_ex", "gen_p", "gen_q", "load_p", "load_q", "storage_p", "shunt_p", "shunt_q")


def make_env(env_name):
    import grid2op
    from grid2op.Parameters import Parameters
    from conformance_backend import OracleHipBackend
    p = Parameters()
    p.NO_OVERFLOW_DISCONNECTION = True
    p.MAX_SUB_CHANGED = 99
    p.MAX_LINE_STATUS_CHANGED = 99
    p.NB_TIMESTEP_COOLDOWN_SUB = 3
    p.NB_TIMESTEP_COOLDOWN_LINE = 0
    return grid2op.make(env_name, test=True, backend=OracleHipBackend(), param=p)


def observe(obs, n_sub, tag):
    """the inputs and the reference's answers of one observation, matrices padded to [2 n_sub][2 n_sub]"""
    cls = type(obs)
    NB = 2 * n_sub
    row = dict(tag=tag, done=int(obs._is_done), topo_vect=np.array(obs.topo_vect, np.int32), shunt_bus=np.array(obs._shunt_bus, np.int32),
               line_status=np.array(obs.line_status, bool), time_before_cooldown_sub=np.array(obs.time_before_cooldown_sub, np.int32),
               p_or=obs.p_or, q_or=obs.q_or, v_or=obs.v_or, p_ex=obs.p_ex, q_ex=obs.q_ex, v_ex=obs.v_ex, gen_p=obs.gen_p, gen_q=obs.gen_q,
               load_p=obs.load_p, load_q=obs.load_q, storage_p=obs.storage_power, shunt_p=obs._shunt_p, shunt_q=obs._shunt_q)
    for k in INPUTS:
        assert np.asarray(row[k]).dtype == np.float32, k
        row[k] = np.array(row[k], np.float32)
    res = obs.bus_connectivity_matrix(return_lines_index=True)
    conn, (c_lor, c_lex) = (res[0], res[1:]) if len(res) == 3 else res         # (a game over returns the three flat)
    fp, (load_bus, gen_bus, sto_bus, lor_bus, lex_bus) = obs.flow_bus_matrix(active_flow=True)
    fq, _ = obs.flow_bus_matrix(active_flow=False)
    nb = conn.shape[0]
    assert fp.shape == fq.shape == (nb, nb) and fp.dtype == np.float32

    def pad(a):
        out = np.zeros((NB, NB), np.float32)
        out[:nb, :nb] = a
        return out
    bus_v, bus_cd = np.zeros(NB, np.float32), np.zeros(NB, np.float32)
    if not obs._is_done:
        graph = obs.get_energy_graph()
        assert len(graph.nodes) == nb
        for k in range(nb):
            bus_v[k], bus_cd[k] = graph.nodes[k]["v"], graph.nodes[k]["cooldown"]
    row.update(ref_n_bus=nb, ref_conn=pad(conn), ref_flow_p=pad(fp), ref_flow_q=pad(fq), ref_load_bus=np.array(load_bus, np.int32),
               ref_gen_bus=np.array(gen_bus, np.int32), ref_storage_bus=np.array(sto_bus, np.int32), ref_line_or_bus=np.array(lor_bus, np.int32),
               ref_line_ex_bus=np.array(lex_bus, np.int32), ref_conn_line_or_bus=np.array(c_lor, np.int32),
               ref_conn_line_ex_bus=np.array(c_lex, np.int32), ref_bus_v=bus_v, ref_bus_cooldown=bus_cd)
    return row


def split(cls, sub, apart=None):
    """set_bus of substation `sub`: its line ends alternate between busbars 1 and 2 (first one on 1), its other elements too; `apart`: two
    lines whose ends here go to busbars 1 and 2"""
    pos = np.nonzero(cls.grid_objects_types[:, cls.SUB_COL] == sub)[0]
    is_line = np.isin(pos, np.concatenate([cls.line_or_pos_topo_vect, cls.line_ex_pos_topo_vect]))
    bus = np.zeros(len(pos), int)
    bus[is_line] = 1 + np.arange(is_line.sum()) % 2
    bus[~is_line] = 1 + np.arange((~is_line).sum()) % 2
    if apart is not None:
        for l, b in zip(apart, (1, 2)):
            for p_ in (cls.line_or_pos_topo_vect[l], cls.line_ex_pos_topo_vect[l]):
                if p_ in pos:
                    bus[list(pos).index(p_)] = b
    assert (bus[is_line] == 1).any() and (bus[is_line] == 2).any(), sub
    return (int(sub), [int(b) for b in bus])


def n_line_ends(cls, sub):
    return int((cls.line_or_to_subid == sub).sum() + (cls.line_ex_to_subid == sub).sum())


def finish(tag, env_name, rows, **extra):
    import graph_ref as G
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(os.path.join(HERE, env_name + ".grid.npz"))
    out = dict(extra, grid=np.array(env_name), tags=np.array([r["tag"] for r in rows]))
    for k in rows[0]:
        if k != "tag":
            out[k] = np.asarray([r[k] for r in rows])
    excluded = compared = 0
    worst = 0.0
    for i in range(len(rows)):
        ns = m.n_sub
        live1 = np.zeros(ns, bool)                                   # the domain in which the reference's shunt shortcut is right
        t = out["topo_vect"][i]
        if not out["done"][i]:
            on = (t[m.line_or_pos_topo_vect] > 0) & (t[m.line_ex_pos_topo_vect] > 0)
            live1[np.asarray(m.line_or_sub)[on & (t[m.line_or_pos_topo_vect] == 1)]] = True
            live1[np.asarray(m.line_ex_sub)[on & (t[m.line_ex_pos_topo_vect] == 1)]] = True
            assert live1.all(), (tag, i, "a substation without a live busbar 1")
            assert (out["shunt_bus"][i] <= 1).all(), (tag, i, "a connected shunt off busbar 1")
        e, c, w = G.compare_reference(m, out, i, half=True)
        excluded, compared, worst = excluded + e, compared + c, max(worst, w)
    assert excluded <= 0.10 * compared, (tag, excluded, compared)
    path = os.path.join(HERE, f"graph_{tag}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{tag}: {len(rows)} observations, {excluded} of {compared} element entries excluded, worst reference error / bound {worst:.4f}, {size} bytes", flush=True)
    assert size <= MAX_BYTES, "cut observations"
    return out


def record_case14():
    env_name = "l2rpn_case14_sandbox"
    env = make_env(env_name)
    cls = type(env)
    env.seed(0)
    env.set_id(0)
    obs = env.reset()
    rows = [observe(obs, cls.n_sub, "reset")]

    def play(act, tag, want_done=False):
        nonlocal obs
        obs, _, done, info = env.step(env.action_space(act))
        assert done == want_done, (tag, info["exception"])
        assert not info["is_illegal"] and not info["is_ambiguous"], tag
        rows.append(observe(obs, cls.n_sub, tag))
    by_size = [int(s) for s in np.argsort(-cls.sub_info, kind="stable") if n_line_ends(cls, s) >= 4]
    play({"set_bus": {"substations_id": [split(cls, by_size[0])]}}, "one_split")
    play({"set_bus": {"substations_id": [split(cls, by_size[1])]}}, "two_splits")
    # a line whose loss the grid survives, away from the split substations
    line = next(l for l in range(cls.n_line) if cls.line_or_to_subid[l] not in by_size[:2] and cls.line_ex_to_subid[l] not in by_size[:2]
                and not env.copy().step(env.action_space({"set_line_status": [(l, -1)]}))[2])
    play({"set_line_status": [(line, -1)]}, "line_open")
    play({}, "line_still_open")
    play({"set_line_status": [(line, +1)]}, "line_reconnected")
    kill = next(l for l in range(cls.n_line) if env.copy().step(env.action_space({"set_line_status": [(l, -1)]}))[2])
    play({"set_line_status": [(kill, -1)]}, "game_over", want_done=True)
    env.close()
    fx = finish("case14", env_name, rows, game_over_line=np.int32(kill))
    tags = list(fx["tags"])
    n_split = [int(((fx["topo_vect"][i] == 2).reshape(-1)).any()) for i in range(len(tags))]
    assert fx["ref_n_bus"][tags.index("one_split")] == cls.n_sub + 1 and fx["ref_n_bus"][tags.index("two_splits")] == cls.n_sub + 2, n_split
    assert not fx["line_status"][tags.index("line_open")].all() and fx["line_status"][tags.index("line_reconnected")].all()
    assert (fx["shunt_bus"][:-1] == 1).any(), "no connected shunt"
    assert fx["done"][-1] == 1 and fx["ref_n_bus"][-1] == 1
    assert (fx["time_before_cooldown_sub"] > 0).any()


def record_wcci():
    env_name = "l2rpn_wcci_2022_dev"
    env = make_env(env_name)
    cls = type(env)
    env.seed(0)
    env.set_id(0)
    obs = env.reset()
    rows = []
    for a, b in PAIRS:
        assert {cls.line_or_to_subid[a], cls.line_ex_to_subid[a]} == {cls.line_or_to_subid[b], cls.line_ex_to_subid[b]}, (a, b)

    def play(act, tag):
        nonlocal obs
        act = dict(act, set_storage=[(i, float(s * 0.5 * cls.storage_max_p_absorb[i])) for i, s in zip(range(cls.n_storage), (1, -1, 1, -1, 1, -1, 1))])
        obs, _, done, info = env.step(env.action_space(act))
        assert not done and not info["is_illegal"] and not info["is_ambiguous"], (tag, info["exception"])
        rows.append(observe(obs, cls.n_sub, tag))
    play({}, "storage")
    pair_sub = int(cls.line_or_to_subid[PAIRS[0][0]])
    subs = [s for s in np.argsort(-cls.sub_info, kind="stable") if n_line_ends(cls, s) >= 4 and s != pair_sub][:13]
    play({"set_bus": {"substations_id": [split(cls, pair_sub, apart=PAIRS[0])] + [split(cls, s) for s in subs]}}, "splits")
    play({"set_line_status": [(PAIRS[1][0], -1)]}, "pair_line_open")
    play({}, "after")
    env.close()
    fx = finish("wcci118", env_name, rows)
    tags = list(fx["tags"])
    assert fx["ref_n_bus"].max() > 128, fx["ref_n_bus"]
    i = tags.index("storage")
    assert all(fx["line_status"][i][list(p)].all() for p in PAIRS)
    i = tags.index("pair_line_open")
    assert not fx["line_status"][i][PAIRS[1][0]] and fx["line_status"][i][PAIRS[1][1]]
    i = tags.index("splits")
    a, b = PAIRS[0]
    t = fx["topo_vect"][i]
    ends = [(t[cls.line_or_pos_topo_vect[l]], t[cls.line_ex_pos_topo_vect[l]]) for l in (a, b)]
    assert fx["line_status"][i][[a, b]].all() and ends[0] != ends[1], ends
    assert (np.abs(fx["storage_p"]) > 0.1).any()
    if not (fx["shunt_bus"] == 1).any():
        print("wcci118: no shunt is connected in this fixture; graph_case14.npz carries the connected shunt", flush=True)


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    reference = os.path.abspath(sys.argv[1])
    for q in (ROOT, os.path.join(ROOT, "tests"), HERE, reference, os.path.join(ROOT, "tests", "_refshim")):
        if q not in sys.path:
            sys.path.insert(0, q)
    os.environ.setdefault("_GRID2OP_FORCE_TEST", "1")
    warnings.filterwarnings("ignore")
    only = sys.argv[2:]
    if not only or "case14" in only:
        record_case14()
    if not only or "wcci" in only:
        record_wcci()


if __name__ == "__main__":
    main()
