"""Inputs of the parity tests of `gpf_ptdf_build_batch` (tests/test_gpu_ptdf_batch_parity.py) and of the conditions those inputs must
meet (tests/test_ptdf_batch_ref_cpu.py): small batches on the committed grids, every one seeded, every topology redrawn until the
oracle's DC power flow gives the verdict the case needs.  A case lists its topologies with the reduced dimension `nr` and the status it
claims for each; the CPU test proves the claims on the oracle alone.

Which kernel a build runs on is the host's rule restated (gridpf_capi_ptdf.hip): `ptdf_build_lds_kernel` ("resident") when the largest
n_pad = max(16, nr rounded up to 16) over ALL classes of the build is <= 128 and `GRIDPF_PTDFB_GLOBAL` is unset, else
`ptdf_build_kernel` ("global"); N = n_pad / 16 block rows per class.

The topology vector cannot put the two ends of a line on one bus (the ends belong to different substations, a bus id is
substation + (busbar - 1) * n_sub), so no case has such a row."""
import dataclasses
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Tuple

import numpy as np

from oracle.pf_oracle import LaneState

from ptdf_batch_ref import reduced_dim, state_of, verdict


def _pos_sub(m):
    """Substation of every position of the topology vector."""
    ps = np.empty(m.dim_topo, dtype=np.int64)
    ps[m.line_or_pos_topo_vect] = m.line_or_sub
    ps[m.line_ex_pos_topo_vect] = m.line_ex_sub
    ps[m.gen_pos_topo_vect] = m.gen_sub
    ps[m.load_pos_topo_vect] = m.load_sub
    if m.n_storage:
        ps[m.storage_pos_topo_vect] = m.storage_sub
    return ps


def _states(m, topos, lane_topo, rng):
    """One lane state per entry of `lane_topo`: that topology row, loads and generators jittered by 20 % (as tests/test_gpu_ptdf_batch.py)."""
    base = LaneState.from_model(m)
    states = []
    for ti in lane_topo:
        st = LaneState.from_model(m)
        st.topo = topos[ti].copy()
        st.load_p = base.load_p * (1 + 0.2 * rng.standard_normal(m.n_load))
        st.gen_p = base.gen_p * (1 + 0.2 * rng.standard_normal(m.n_gen))
        if m.n_storage:
            st.storage_p = rng.uniform(-2, 2, m.n_storage)
        states.append(st)
    return states


@dataclass
class BatchCase:
    id: str
    grid: str
    topos: List[np.ndarray]                 # distinct topology rows
    nr: List[int]                           # claimed reduced dimension of each
    status: List[int]                       # status the builder must report for each (0 ok, 1 singular pivot, 2 islanded, 3 no slack)
    builds: List[np.ndarray]                # lane -> topology of every build, in order, on ONE engine
    modes: Tuple[str, ...] = ("default",)   # "default" | "global" (GRIDPF_PTDFB_GLOBAL=1)
    seed: int = 0
    screen_lanes: Optional[int] = None      # lanes of a build whose screening is compared (None: all)
    claims: Tuple[str, ...] = ()            # special LODF columns the case must have: "nan", "stub", "off"
    patch: Optional[Callable] = None        # model -> model (a copy with changed data)
    extra: dict = field(default_factory=dict)

    def model(self, load_model):
        m = load_model(self.grid)
        return self.patch(m) if self.patch else m

    def states(self, m, build):
        """Lane states of build `build`: the topology rows with jittered injections."""
        rng = np.random.default_rng([self.seed, build])
        return _states(m, self.topos, self.builds[build], rng)

    def kernel(self, build, mode):
        used = sorted(set(self.builds[build].tolist()))
        npad_max = max(max(16, (self.nr[i] + 15) & ~15) for i in used)
        return "global" if (mode == "global" or npad_max > 128) else "resident"


def n_blocks(nr):
    return max(16, (nr + 15) & ~15) // 16


def line_out(m, topo, lines):
    t = topo.copy()
    for l in np.atleast_1d(lines):
        t[m.line_or_pos_topo_vect[l]] = -1
        t[m.line_ex_pos_topo_vect[l]] = -1
    return t


def split_subs(m, topo, subs, offs):
    """Every other element of each substation of `subs` to busbar 2, starting at element `off` (0 | 1)."""
    ps = _pos_sub(m)
    t = topo.copy()
    for s, off in zip(subs, offs):
        sel = np.nonzero(ps == s)[0][int(off)::2]
        t[sel] = np.where(t[sel] >= 1, 2, t[sel])
    return t


def big_subs(m):
    ps = _pos_sub(m)
    return [s for s in range(m.n_sub) if (ps == s).sum() >= 4]


def draw_split(m, n_split, rng, want=0, n_out=0, tries=400):
    """A topology with `n_split` substations (of >= 4 elements) split and `n_out` lines out whose oracle verdict is `want`."""
    big = big_subs(m)
    base = m.initial_topo_vect().astype(np.int32)
    for _ in range(tries):
        subs = rng.choice(big, n_split, replace=False) if n_split else []
        t = split_subs(m, base, subs, rng.integers(0, 2, n_split))
        if n_out:
            t = line_out(m, t, rng.choice(m.n_line, n_out, replace=False))
        if verdict(m, state_of(m, t)) == want:
            return t.astype(np.int32)
    raise AssertionError(f"no topology with {n_split} splits, {n_out} lines out and verdict {want}")


def ragged_lanes(n_topo, n_lanes, rng):
    """Every topology used, more lanes than topologies, shuffled."""
    lt = np.concatenate([np.arange(n_topo), rng.integers(0, n_topo, n_lanes - n_topo)])
    rng.shuffle(lt)
    return lt


def _finish(m, cid, grid, topos, status, builds, **kw):
    nr = [reduced_dim(m, state_of(m, t)) for t in topos]
    assert len({t.tobytes() for t in topos}) == len(topos), cid
    return BatchCase(id=cid, grid=grid, topos=[np.asarray(t, dtype=np.int32) for t in topos], nr=nr, status=list(status), builds=builds, **kw)


def leaf_line(m):
    """(line, substation) of the one substation that hangs on a single line, found from the model."""
    n_at = np.bincount(np.concatenate([m.line_or_sub, m.line_ex_sub]), minlength=m.n_sub)
    leaves = np.nonzero(n_at == 1)[0]
    assert len(leaves) == 1, leaves
    s = int(leaves[0])
    l = np.nonzero((m.line_or_sub == s) | (m.line_ex_sub == s))[0]
    return int(l[0]), s


def weak_leaf_model(m):
    """A copy of the model whose leaf line has br_bdc = 1e-14: the leaf bus's pivot of B' is 1e-14, below the kernels' 1e-12."""
    bdc = m.br_bdc.copy()
    bdc[leaf_line(m)[0]] = 1e-14
    return dataclasses.replace(m, br_bdc=bdc)


CASE_IDS = ["idf_over_128", "idf_switch", "idf_forced_global_vs_resident", "neurips_48_49", "case14_16_17", "case5_floor",
            "stub_and_bridge_case14", "stub_and_bridge_neurips", "singular_pivot"]
IDF = "l2rpn_idf_2023"

_CACHE = {}
_IDF_TOPO = {}


def _idf_topology(m, n_split):
    """The seeded connected idf topology with `n_split` split substations (nr = 117 + n_split), shared by the idf cases."""
    if n_split not in _IDF_TOPO:
        _IDF_TOPO[n_split] = draw_split(m, n_split, np.random.default_rng(2300 + n_split))
    return _IDF_TOPO[n_split]


def _idf_over_128(m):
    """Classes of nr = 128 (N = 8), 129 (N = 9), 144 (N = 9), 145 (N = 10) and 157 (N = 10) in ONE build: npad_max = 160, the global kernel
    handles all of them, each with its own leading dimension inside a work block of 160^2.  Two islanded topologies (status 2: a
    redrawn 20-split one; the nr = 129 one with the line of a leaf substation out) and one without a slack in service (status 3: the
    topology vector accepts -1 at the slack generator's position).  `extra["single"]`: the topology whose tables `gpf_ptdf_build`
    builds too (nr = 145)."""
    rng = np.random.default_rng(2301)
    live = [_idf_topology(m, s) for s in (11, 12, 27, 28, 40)]
    isl_a = draw_split(m, 20, rng, want=2, n_out=3)
    n_at = np.bincount(np.concatenate([m.line_or_sub, m.line_ex_sub]), minlength=m.n_sub)
    leaf = int(np.nonzero(n_at == 1)[0][0])
    isl_b = line_out(m, live[1], np.nonzero((m.line_or_sub == leaf) | (m.line_ex_sub == leaf))[0])
    no_slack = live[1].copy()
    no_slack[m.gen_pos_topo_vect[np.nonzero(m.gen_slack)[0]]] = -1
    topos = live + [isl_a, isl_b, no_slack]
    return _finish(m, "idf_over_128", IDF, topos, [0] * 5 + [2, 2, 3], [ragged_lanes(len(topos), 24, rng)], seed=2301, screen_lanes=6,
                   claims=("nan",), extra=dict(nr_live=[128, 129, 144, 145, 157], single=3))


def _idf_switch(m):
    """Three builds on one engine: classes of nr = 117 (one line out) and 128; then lane 0 moved to nr = 129 (npad_max 128 -> 144: the
    global kernel); then moved back.  Builds 1 and 3 run the resident kernel and must give bit-identical tables."""
    rng = np.random.default_rng(2302)
    topos = [draw_split(m, 0, rng, n_out=1), _idf_topology(m, 11), _idf_topology(m, 12)]
    lt = ragged_lanes(2, 8, rng)
    lt2 = lt.copy()
    lt2[0] = 2
    assert (lt2 == lt[0]).any()                      # the class lane 0 leaves keeps other lanes
    return _finish(m, "idf_switch", IDF, topos, [0, 0, 0], [lt, lt2, lt.copy()], seed=2302, screen_lanes=6, claims=("nan", "off"))


def _idf_forced(m):
    """Classes of nr = 117 and 128, built by the resident kernel and by the global one (N = 8, the most the resident kernel takes)."""
    rng = np.random.default_rng(2303)
    topos = [draw_split(m, 0, rng, n_out=1), _idf_topology(m, 11)]
    return _finish(m, "idf_forced_global_vs_resident", IDF, topos, [0, 0], [ragged_lanes(2, 8, rng)], modes=("default", "global"),
                   seed=2303, screen_lanes=6, claims=("nan", "off"))


def _boundary(m, cid, grid, n_splits, seed, n_lanes, extra_topos=()):
    rng = np.random.default_rng(seed)
    topos = [draw_split(m, s, rng) for s in n_splits] + list(extra_topos)
    return _finish(m, cid, grid, topos, [0] * len(topos), [ragged_lanes(len(topos), n_lanes, rng)], seed=seed, claims=("nan",) if m.n_sub > 5 else ())


def _case5_floor(m):
    """nr = 4, 5, 6 (N = 1: one worker wavefront of eight, no next pivot tile, 32 LODF stripes for 8 lines) and nr = 3: substation 2 carries
    lines only; with its four lines out it is no active bus -- every other substation has a generator or a load, so no outage set
    goes lower with the grid connected."""
    at2 = np.nonzero((m.line_or_sub == 2) | (m.line_ex_sub == 2))[0]
    assert not (m.gen_sub == 2).any() and not (m.load_sub == 2).any() and len(at2) == 4
    floor = line_out(m, m.initial_topo_vect().astype(np.int32), at2)
    return _boundary(m, "case5_floor", "rte_case5_example", (0, 1, 2), 501, 9, extra_topos=[floor])


def _stub_and_bridge(m, cid, grid, seed):
    """Crafted rows (base topology, then): (0) the origin end of a line ALONE on busbar 2 -- a stub: the bus carries nothing else, the
    line's LODF column is zero and its flow 0; (1) the same with the extremity end of another line; (2) a line end AND a load alone on
    busbar 2: a true bridge, NaN column; (3) one line out; (4) a stub, a line out and a split substation together.
    `extra["single"]`: the rows whose tables `gpf_ptdf_build` builds too (its dangling-line and islanding columns)."""
    rng = np.random.default_rng(seed)
    base = m.initial_topo_vect().astype(np.int32)

    def crafted(make):
        for _ in range(400):
            got = make()
            if got is not None and verdict(m, state_of(m, got[0])) == 0:
                return got
        raise AssertionError(cid)

    def stub(side, t0=None):
        t = (base if t0 is None else t0()).copy()
        l = int(rng.integers(m.n_line))
        pos = (m.line_or_pos_topo_vect if side == 0 else m.line_ex_pos_topo_vect)[l]
        if t[pos] != 1:
            return None
        t[pos] = 2
        return t, l

    def bridge():
        t = base.copy()
        i = int(rng.integers(m.n_load))
        at = np.nonzero(m.line_or_sub == m.load_sub[i])[0]
        if len(at) == 0:
            return None
        l = int(rng.choice(at))
        t[m.load_pos_topo_vect[i]] = 2
        t[m.line_or_pos_topo_vect[l]] = 2
        return t, l

    def one_out():
        l = int(rng.integers(m.n_line))
        return line_out(m, base, l), l

    rows = [crafted(lambda: stub(0)), crafted(lambda: stub(1)), crafted(bridge), crafted(one_out),
            crafted(lambda: stub(0, lambda: line_out(m, draw_split(m, 1, rng), int(rng.integers(m.n_line)))))]
    topos = [r[0] for r in rows]
    return _finish(m, cid, grid, topos, [0] * 5, [ragged_lanes(5, 11, rng)], seed=seed, claims=("nan", "stub", "off"),
                   extra=dict(stub_lines={0: rows[0][1], 1: rows[1][1], 4: rows[4][1]}, bridge_line=rows[2][1], out_line=rows[3][1], single=(0, 1, 2)))


def _singular_pivot(m0):
    """l2rpn_case14_sandbox with br_bdc = 1e-14 on the line of its leaf substation (a generator behind one transformer): the leaf bus's
    pivot is 1e-14.  Topologies with that line in service must come back with status 1 (NaN flows and screening) -- (0) the base
    topology: the leaf bus has compact index 6, the FIRST pivot of a 2 x 2 block (|a|); (1) the slack generator and one line of its
    substation on busbar 2: busbar 1 of substation 0 is no reference bus any more, the leaf bus has compact index 7, the SECOND pivot
    (|det / a|); (2) another line out; (3) a split substation.  (4) the leaf line out: its generator is islanded, status 2.  (5) the
    leaf line out and the generator disconnected: status 0, tables against the reference."""
    m = weak_leaf_model(m0)
    l_leaf, s_leaf = leaf_line(m)
    rng = np.random.default_rng(1404)
    base = m.initial_topo_vect().astype(np.int32)
    g_slack = int(np.nonzero(m.gen_slack)[0][0])
    s_slack = int(m.gen_sub[g_slack])
    moved = base.copy()
    moved[m.gen_pos_topo_vect[g_slack]] = 2
    moved[m.line_or_pos_topo_vect[int(np.nonzero(m.line_or_sub == s_slack)[0][0])]] = 2
    others = [l for l in range(m.n_line) if l != l_leaf]
    for _ in range(200):
        out1 = line_out(m, base, int(rng.choice(others)))
        if verdict(m, state_of(m, out1)) == 0:
            break
    else:
        raise AssertionError("singular_pivot: no other line whose outage leaves the grid connected")
    for _ in range(200):
        split = draw_split(m, 1, rng)
        if split[m.line_or_pos_topo_vect[l_leaf]] == 1 and split[m.line_ex_pos_topo_vect[l_leaf]] == 1:
            break
    else:
        raise AssertionError("singular_pivot: no split that keeps both ends of the leaf line on busbar 1")
    cut = line_out(m, base, l_leaf)
    cut_off = cut.copy()
    cut_off[m.gen_pos_topo_vect[np.nonzero(m.gen_sub == s_leaf)[0]]] = -1
    topos = [base, moved, out1, split, cut, cut_off]
    return _finish(m, "singular_pivot", "l2rpn_case14_sandbox", topos, [1, 1, 1, 1, 2, 0], [ragged_lanes(6, 13, rng)], modes=("default", "global"),
                   seed=1404, patch=weak_leaf_model, claims=("off",), extra=dict(leaf_line=l_leaf, leaf_sub=s_leaf, oracle_status=[0, 0, 0, 0, 2, 0]))


def batch_cases(load_model):
    """The cases by id."""
    if "all" in _CACHE:
        return _CACHE["all"]
    idf = load_model(IDF)
    neu = load_model("l2rpn_neurips_2020_track1")
    c14 = load_model("l2rpn_case14_sandbox")
    cases = {
        "idf_over_128": _idf_over_128(idf),
        "idf_switch": _idf_switch(idf),
        "idf_forced_global_vs_resident": _idf_forced(idf),
        "neurips_48_49": _boundary(neu, "neurips_48_49", "l2rpn_neurips_2020_track1", (12, 13, 14), 3603, 8),
        "case14_16_17": _boundary(c14, "case14_16_17", "l2rpn_case14_sandbox", (2, 3, 4), 1405, 8),
        "case5_floor": _case5_floor(load_model("rte_case5_example")),
        "stub_and_bridge_case14": _stub_and_bridge(c14, "stub_and_bridge_case14", "l2rpn_case14_sandbox", 1406),
        "stub_and_bridge_neurips": _stub_and_bridge(neu, "stub_and_bridge_neurips", "l2rpn_neurips_2020_track1", 3604),
        "singular_pivot": _singular_pivot(c14),
    }
    assert sorted(cases) == sorted(CASE_IDS)
    _CACHE["all"] = cases
    return cases


NR_CLAIMS = {"idf_over_128": [128, 129, 144, 145, 157], "idf_switch": [117, 128, 129], "idf_forced_global_vs_resident": [117, 128],
             "neurips_48_49": [47, 48, 49], "case14_16_17": [15, 16, 17], "case5_floor": [4, 5, 6, 3]}

_PARTS = {}


def class_reference(c, m, i):
    """`lodf_parts` of topology `i` of case `c` (model `m` = c.model(...)), computed once per process and shared, never written to."""
    key = (c.grid, c.patch is not None, c.topos[i].tobytes())
    if key not in _PARTS:
        from ptdf_batch_ref import lodf_parts
        p = lodf_parts(m, state_of(m, c.topos[i]))
        for v in p.values():
            v.setflags(write=False)
        _PARTS[key] = p
    return _PARTS[key]
