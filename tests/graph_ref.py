"""The bus-graph observation (include/gridpf.h gpf_set_graph_obs) restated in numpy on the float32 inputs the engine reads -- what
tests/test_graph_cpu.py holds against the observations recorded from the unmodified reference and what the device and the host emulator
are held to bit for bit --, the bound of the reference's own float32 evaluation, and the loader of the g++ host emulator of the library's
rule core (tests/native/graph_emul.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SECTIONS = ("n_bus", "load_bus", "gen_bus", "storage_bus", "line_or_bus", "line_ex_bus", "shunt_bus", "bus_global")
FLOATS = ("p_or", "q_or", "v_or", "p_ex", "q_ex", "v_ex", "gen_p", "gen_q", "load_p", "load_q", "storage_p", "shunt_p", "shunt_q")
U = 2.0 ** -24                       # one float32 rounding, relative to the magnitude it rounds
f64 = np.float64


def layout(m, n_busbar):
    """{section: slice} of the index row, "width" and "NB" (the order of GPF_GRAPH_*)"""
    widths = (1, m.n_load, m.n_gen, m.n_storage, m.n_line, m.n_line, m.n_shunt, m.n_sub * n_busbar)
    lay, at = {}, 0
    for name, w in zip(SECTIONS, widths):
        lay[name] = slice(at, at + w)
        at += w
    lay.update(width=at, NB=m.n_sub * n_busbar)
    return lay


def restate(m, n_busbar, st, over=False):
    """One lane.  ``st``: topo_vect, shunt_bus, the float32 vectors of `FLOATS`, sub_cooldown (None: not tracked).  Returns index (int32
    row), features float32 [NB, 4], dense float32 [3, NB, NB], and per float entry the bound of a float32 evaluation of the same sum:
    (terms + 1) * 2^-24 * sum |terms| (bound_features [NB, 2], bound_dense [2, NB, NB])."""
    ns, lay = m.n_sub, layout(m, n_busbar)
    NB = lay["NB"]
    idx = np.full(lay["width"], -1, np.int32)
    feat, dense = np.zeros((NB, 4), np.float32), np.zeros((3, NB, NB), np.float32)
    bf, bd = np.zeros((NB, 2)), np.zeros((2, NB, NB))
    if over:
        idx[:lay["bus_global"].start] = 0
        idx[0], idx[lay["bus_global"].start] = 1, 0
        return dict(index=idx, features=feat, dense=dense, bound_features=bf, bound_dense=bd, bound_rows=np.zeros((2, NB)))
    topo, shb = np.asarray(st["topo_vect"], np.int64), np.asarray(st["shunt_bus"], np.int64)
    v = {k: np.asarray(st[k], np.float32).astype(f64) for k in FLOATS}
    lor_b, lex_b = topo[m.line_or_pos_topo_vect], topo[m.line_ex_pos_topo_vect]
    on = (lor_b > 0) & (lex_b > 0)
    live = np.zeros(NB, bool)
    live[np.asarray(m.line_or_sub)[on] + (lor_b[on] - 1) * ns] = True
    live[np.asarray(m.line_ex_sub)[on] + (lex_b[on] - 1) * ns] = True
    n_bus = int(live.sum())
    comp = np.full(NB, -1, np.int64)
    comp[live] = np.arange(n_bus)

    def elem(sub, b):
        res = np.full(len(b), -1, np.int64)
        ok = (b > 0) & (b <= n_busbar)
        res[ok] = comp[np.asarray(sub)[ok] + (b[ok] - 1) * ns]
        return res
    bus = dict(load_bus=elem(m.load_sub, topo[m.load_pos_topo_vect]), gen_bus=elem(m.gen_sub, topo[m.gen_pos_topo_vect]),
               storage_bus=elem(m.storage_sub, topo[m.storage_pos_topo_vect]), line_or_bus=np.where(on, elem(m.line_or_sub, lor_b), -1),
               line_ex_bus=np.where(on, elem(m.line_ex_sub, lex_b), -1), shunt_bus=elem(m.shunt_sub, shb))
    idx[0] = n_bus
    for k, a in bus.items():
        idx[lay[k]] = a
    idx[lay["bus_global"]][:n_bus] = np.nonzero(live)[0]
    # node sums: float64, sequential, class by class in index order (sums of different buses do not meet)
    acc, n_term, s_abs = np.zeros((NB, 2)), np.zeros((NB, 2), np.int64), np.zeros((NB, 2))

    def add(where, col, vals, sign):
        for i, b in enumerate(where):
            if b >= 0:
                acc[b, col] = acc[b, col] + vals[i] if sign > 0 else acc[b, col] - vals[i]
                n_term[b, col] += 1
                s_abs[b, col] += abs(vals[i])
    add(bus["gen_bus"], 0, v["gen_p"], +1); add(bus["load_bus"], 0, v["load_p"], -1); add(bus["storage_bus"], 0, v["storage_p"], -1)
    add(bus["shunt_bus"], 0, v["shunt_p"], -1)
    add(bus["gen_bus"], 1, v["gen_q"], +1); add(bus["load_bus"], 1, v["load_q"], -1); add(bus["shunt_bus"], 1, v["shunt_q"], -1)
    feat[:n_bus, :2] = acc[:n_bus].astype(np.float32)
    bf[:n_bus] = ((n_term + 1) * U * s_abs)[:n_bus]
    for l in np.nonzero(on)[0]:                      # the overwrite order of baseObservation.py:2694-2695: every origin, then every extremity
        feat[bus["line_or_bus"][l], 2] = st["v_or"][l]
    for l in np.nonzero(on)[0]:
        feat[bus["line_ex_bus"][l], 2] = st["v_ex"][l]
    cd = st.get("sub_cooldown")
    if cd is not None:
        feat[:n_bus, 3] = np.asarray(cd)[np.nonzero(live)[0] % ns]
    # dense planes
    k = np.arange(n_bus)
    dense[0, k, k] = 1.0
    dense[1, k, k], dense[2, k, k] = feat[:n_bus, 0], feat[:n_bus, 1]
    bd[0, k, k], bd[1, k, k] = bf[:n_bus, 0], bf[:n_bus, 1]
    off, cnt, sab = np.zeros((2, NB, NB)), np.zeros((2, NB, NB), np.int64), np.zeros((2, NB, NB))
    for l in np.nonzero(on)[0]:
        a, b = bus["line_or_bus"][l], bus["line_ex_bus"][l]
        if a == b:
            continue
        dense[0, a, b] = dense[0, b, a] = 1.0
        for pl, (o_, e_) in enumerate((("p_or", "p_ex"), ("q_or", "q_ex"))):
            for (i, j, val) in ((a, b, v[o_][l]), (b, a, v[e_][l])):       # a line's or-term, then its ex-term
                off[pl, i, j] = off[pl, i, j] + val
                cnt[pl, i, j] += 1
                sab[pl, i, j] += abs(val)
    touched = cnt > 0
    dense[1:][touched] = (-off[touched]).astype(np.float32)
    bd[touched] = ((cnt + 1) * U * sab)[touched]
    # a row of a flow plane as one sum (Kirchhoff): its terms are the node's and those of the lines that leave the bus
    row_terms, row_abs = n_term.T + cnt.sum(2), s_abs.T + sab.sum(2)
    return dict(index=idx, features=feat, dense=dense, bound_features=bf, bound_dense=bd, bound_rows=(row_terms + 1) * U * row_abs)


def random_state(m, n_busbar, rng, p_open=0.15, p_off=0.05):
    """a synthetic lane: every element on a random busbar, lines opened with ``p_open`` (both ends -1), other elements and shunts
    disconnected with ``p_off``, random float32 vectors, random substation cooldowns"""
    topo = rng.integers(1, n_busbar + 1, m.dim_topo).astype(np.int32)
    topo[rng.random(m.dim_topo) < p_off] = -1
    for l in np.nonzero((rng.random(m.n_line) < p_open) | (topo[m.line_or_pos_topo_vect] < 0) | (topo[m.line_ex_pos_topo_vect] < 0))[0]:
        topo[m.line_or_pos_topo_vect[l]] = topo[m.line_ex_pos_topo_vect[l]] = -1
    shb = rng.integers(1, n_busbar + 1, m.n_shunt).astype(np.int32)
    shb[rng.random(m.n_shunt) < p_off] = -1
    sizes = dict(p_or=m.n_line, q_or=m.n_line, v_or=m.n_line, p_ex=m.n_line, q_ex=m.n_line, v_ex=m.n_line, gen_p=m.n_gen, gen_q=m.n_gen,
                 load_p=m.n_load, load_q=m.n_load, storage_p=m.n_storage, shunt_p=m.n_shunt, shunt_q=m.n_shunt)
    st = {k: rng.uniform(-120.0, 120.0, sizes[k]).astype(np.float32) for k in FLOATS}
    st.update(topo_vect=topo, shunt_bus=shb, sub_cooldown=rng.integers(0, 4, m.n_sub).astype(np.int32))
    return st


def state_of(fx, i):
    """observation i of a recorded fixture (tests/golden/graph_*.npz) as the restatement's input"""
    st = {k: fx[k][i] for k in FLOATS}
    st.update(topo_vect=fx["topo_vect"][i], shunt_bus=fx["shunt_bus"][i], sub_cooldown=fx["time_before_cooldown_sub"][i])
    return st


def compare_reference(m, fx, i, half=False):
    """Holds the restatement of recorded observation i to the reference's recorded answers: integers exactly (entries of disconnected
    elements against -1 instead), floats within the bound (``half``: half of it).  Returns (excluded, compared) element entries and the
    worst error / bound."""
    lay = layout(m, 2)
    over = bool(fx["done"][i])
    r = restate(m, 2, state_of(fx, i), over=over)
    idx, nb = r["index"], int(fx["ref_n_bus"][i])
    assert idx[0] == nb, (i, idx[0], nb)
    excluded = compared = 0
    for key in ("load_bus", "gen_bus", "storage_bus", "line_or_bus", "line_ex_bus"):
        got, ref = idx[lay[key]], fx["ref_" + key][i]
        out = got < 0 if not over else np.zeros(len(got), bool)
        assert np.array_equal(got[~out], ref[~out]), (i, key)
        excluded += int(out.sum()); compared += len(got)
    for key in ("line_or_bus", "line_ex_bus"):                   # the second pair of line vectors: bus_connectivity_matrix's
        got, ref = idx[lay[key]], fx["ref_conn_" + key][i]
        out = got < 0 if not over else np.zeros(len(got), bool)
        assert np.array_equal(got[~out], ref[~out]), (i, "conn", key)
    disc_lines = idx[lay["line_or_bus"]] < 0
    if not over:
        assert np.array_equal(disc_lines, ~(np.asarray(fx["line_status"][i]).astype(bool))), (i, "line_status")
    worst = 0.0
    scale = 0.5 if half else 1.0
    assert np.array_equal(r["dense"][0, :nb, :nb], fx["ref_conn"][i][:nb, :nb]), (i, "bus_connectivity_matrix")
    for pl, key in ((1, "ref_flow_p"), (2, "ref_flow_q")):
        err = np.abs(r["dense"][pl, :nb, :nb].astype(f64) - fx[key][i][:nb, :nb].astype(f64))
        b = r["bound_dense"][pl - 1, :nb, :nb]
        assert (err <= scale * b).all(), (i, key, float(err.max()))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(b > 0, err / b, 0.0))))
    assert not r["dense"][:, nb:].any() and not r["dense"][:, :, nb:].any() and not r["features"][nb:].any()
    if not over:
        assert np.array_equal(r["features"][:nb, 2], fx["ref_bus_v"][i][:nb]), (i, "bus_v")
        assert np.array_equal(r["features"][:nb, 3], fx["ref_bus_cooldown"][i][:nb]), (i, "cooldown")
    return excluded, compared, worst


# ---- the library's rule core on the host (tests/native/graph_emul.cpp) ----
_BUILD = os.path.join(tempfile.gettempdir(), f"gridpf_graph_emul_{os.getuid()}")
SRC = os.path.join(HERE, "native", "graph_emul.cpp")
_emul = None


def _compile(out, flags):
    os.makedirs(_BUILD, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_graph.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", *flags, SRC, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


def emul_lib():
    global _emul
    if _emul is None:
        _emul = C.CDLL(_compile(os.path.join(_BUILD, "libgraphemul.so"), ["-O2", "-fPIC", "-shared"]))
        _emul.graph_emul_lane.restype = None
    return _emul


def sanitized_program():
    return _compile(os.path.join(_BUILD, "graph_emul_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGRAPH_EMUL_MAIN"])


def pack_row(st):
    """the float32 vectors of `FLOATS` as one results row and its 13 offsets"""
    parts = [np.asarray(st[k], np.float32) for k in FLOATS]
    off = np.cumsum([0] + [len(p) for p in parts[:-1]]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(parts), np.float32), off


def emul_lane(m, n_busbar, *, topo_vect, shunt_bus, row, offsets, sub_cooldown=None, over=False):
    """the library's rule core on one lane, on a results row with the given 13 column offsets (the order of `FLOATS`)"""
    lay = layout(m, n_busbar)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    dims = i32([m.n_sub, n_busbar, m.n_load, m.n_gen, m.n_storage, m.n_line, m.n_shunt, m.dim_topo])
    tabs = [i32(a) for a in (m.load_sub, m.load_pos_topo_vect, m.gen_sub, m.gen_pos_topo_vect, m.storage_sub, m.storage_pos_topo_vect,
                             m.line_or_sub, m.line_or_pos_topo_vect, m.line_ex_sub, m.line_ex_pos_topo_vect, m.shunt_sub)]
    topo, shb, off, row = i32(topo_vect), i32(shunt_bus), i32(offsets), np.ascontiguousarray(row, np.float32)
    cd = None if sub_cooldown is None else i32(sub_cooldown)
    NB = lay["NB"]
    idx, feat, dense = np.full(lay["width"], -7, np.int32), np.full((NB, 4), np.nan, np.float32), np.full((3, NB, NB), np.nan, np.float32)

    def p(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    emul_lib().graph_emul_lane(p(dims), *[p(t) for t in tabs], p(off), p(topo), p(shb), p(row), p(cd), int(bool(over)), p(idx), p(feat), p(dense))
    return dict(index=idx, features=feat, dense=dense)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the lane states of the GPU tests (tests/test_gpu_graph.py); tests/test_graph_cpu.py holds them to the CPU oracle's verdict ----
def split_substation(m, topo, sub, n_busbar):
    """`topo` with the line ends of substation `sub` dealt out over busbars 1 .. n_busbar in turn, and its other elements likewise"""
    topo = np.array(topo, np.int32)
    ends = np.concatenate([np.asarray(m.line_or_pos_topo_vect)[np.asarray(m.line_or_sub) == sub],
                           np.asarray(m.line_ex_pos_topo_vect)[np.asarray(m.line_ex_sub) == sub]])
    ends.sort()
    topo[ends] = 1 + np.arange(len(ends)) % n_busbar
    others = np.sort(np.concatenate([np.asarray(p)[np.asarray(s) == sub] for p, s in (
        (m.load_pos_topo_vect, m.load_sub), (m.gen_pos_topo_vect, m.gen_sub), (m.storage_pos_topo_vect, m.storage_sub))]))
    topo[others] = 1 + np.arange(len(others)) % min(n_busbar, max(len(ends), 1))
    return topo


def open_line(m, topo, l):
    topo = np.array(topo, np.int32)
    topo[m.line_or_pos_topo_vect[l]] = topo[m.line_ex_pos_topo_vect[l]] = -1
    return topo


def line_ends_of(m, sub):
    return int((np.asarray(m.line_or_sub) == sub).sum() + (np.asarray(m.line_ex_sub) == sub).sum())


def case5_lanes(m, n_busbar):
    """five lanes of rte_case5_example: [topo rows, shunt rows, load scale]"""
    base = np.asarray(m.initial_topo_vect(), np.int32)
    subs = sorted(range(m.n_sub), key=lambda s: -line_ends_of(m, s))
    one = split_substation(m, base, subs[0], n_busbar)
    away = [l for l in range(m.n_line) if subs[0] not in (m.line_or_sub[l], m.line_ex_sub[l])]
    rows = [base, one, open_line(m, one, away[0]), split_substation(m, base, subs[1], 2), open_line(m, base, away[-1])]
    return np.array(rows, np.int32), np.zeros((5, 0), np.int32), 1.0 + 0.02 * np.arange(5)


def wcci_lanes(m, fx):
    """six lanes of l2rpn_wcci_2022_dev from the recorded topologies: the reset topology, the thirteen splits (more than 128 buses), one
    line of a parallel pair open, another pair with a line open, the splits and one more substation with every shunt connected (that
    substation's on its busbar 2), the reset topology with every shunt on busbar 1"""
    base, splits, pair_open = fx["topo_vect"][0], fx["topo_vect"][1], fx["topo_vect"][2]
    sb0 = np.asarray(m.initial_shunt_bus(), np.int32)
    sb1 = np.ones_like(sb0)
    sb2 = sb1.copy()
    sh = next(i for i in range(m.n_shunt) if line_ends_of(m, m.shunt_sub[i]) >= 4 and (splits[np.asarray(m.line_or_pos_topo_vect)[
        np.asarray(m.line_or_sub) == m.shunt_sub[i]]] == 1).all())
    sb2[sh] = 2                                         # a shunt on busbar 2 of a substation split for it
    with_shunt = split_substation(m, splits, m.shunt_sub[sh], 2)
    rows = [base, splits, pair_open, open_line(m, base, 131), with_shunt, base]
    return np.array(rows, np.int32), np.array([sb0, sb0, sb0, sb0, sb2, sb1], np.int32), 1.0 + 0.01 * np.arange(6)
