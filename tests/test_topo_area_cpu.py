"""Rules by area and composite actions (include/gridpf.h: gpf_set_topo_areas / gpf_set_topo_slots / gpf_get_topo_action_areas), the parts
that need no GPU: the library's shared rule core (run-time ambiguity, per-area mask evaluation, the impact of a composite's concatenated
item list; grid2op_amd/csrc/gridpf_topo_mask.hpp) compiled with g++ into a host emulator gives the verdicts the reference environment
recorded under ``RulesByArea`` (tests/golden/topo_area_*.npz); so does the Python restatement; the fixture separates the per-area rules
from the whole-grid ones; area sets and area validation through a header-only handle; ShardedEngine forwards the calls."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_path
from grid2op_amd.grid_model import GridModel
from grid2op_amd.sharding import ShardedEngine
from stub_engine import StubEngine
import topo_area_ref as A
import topo_mask_ref as R


@pytest.fixture(scope="module", params=sorted(A.FIXTURES))
def recorded(request, load_model):
    fix = A.load_fixture(request.param)
    assert str(fix["grid"]) == A.FIXTURES[request.param]
    m = load_model(A.FIXTURES[request.param])
    e = A.emul(m, fix["off"], fix["items"], fix["sub_area"], fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], comps=fix["comps"])
    return m, fix, e


def test_emulator_gives_the_reference_verdicts_on_entries_and_composites(recorded):
    m, fix, e = recorded
    assert list(fix["params"]) == [1, 1, 3, 3]
    A.check_against_reference(fix, e["mask"])
    A.check_against_reference(fix, e["comp_mask"], "comp_")
    assert np.array_equal(e["ambiguous"], fix["ambiguous"][0]) and np.array_equal(e["comp_ambiguous"], fix["comp_ambiguous"][0])
    # the composite played at every step: the environment's own flags
    t = np.arange(len(fix["played"]))
    played = e["comp_mask"][t, fix["played"]]
    assert np.array_equal((played & 0x0F) != 0, fix["is_illegal"]) and np.array_equal((played & 0x10) != 0, fix["is_ambiguous"])


def test_whole_grid_rules_fail_the_recording(recorded):
    """what makes the fixture a test of the feature: without areas the same core contradicts the recorded composite verdicts"""
    m, fix, e = recorded
    w = A.emul(m, fix["off"], fix["items"], None, fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], comps=fix["comps"])
    ok = ~fix["comp_ambiguous"]
    wrong = ((w["comp_mask"] & 0x03) != 0)[ok] != ~fix["comp_area_legal"][ok]
    assert wrong.mean() >= 0.1
    assert np.array_equal(((w["comp_mask"] & 0x03) != 0)[ok], ~fix["comp_look_legal"][ok])      # ... and agrees with whole-grid LookParam
    # the entries alone through the unchanged whole-grid emulator of the legality masks
    old, _ = R.emul_mask(m, fix["off"], fix["items"], fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], True, 1, 1)
    assert np.array_equal(old, w["mask"])


def test_fixture_separates_the_rules(recorded):
    _, fix, _ = recorded
    n = fix["comp_area_legal"].size
    assert fix["comp_area_legal"].shape[0] == 30 and fix["comp_area_legal"].shape[1] >= 40 and fix["ambiguous"].shape[1] >= 40
    assert 10 * int((fix["comp_area_legal"] & ~fix["comp_look_legal"]).sum()) >= n
    assert 10 * int((~fix["comp_area_legal"]).sum()) >= n
    assert fix["comp_ambiguous"].any() and not fix["comp_ambiguous"].all() and fix["is_illegal"].any() and fix["is_ambiguous"].any()
    assert (fix["comps"] >= 0).sum(1).max() == 3 and (fix["comps"] >= 0).sum(1).min() == 1


def test_restatement_gives_the_reference_verdicts_and_the_emulators_bytes(recorded):
    m, fix, e = recorded
    rules = A.AreaRules(m, fix["off"], fix["items"], fix["sub_area"])
    single = [[a] for a in range(rules.n_act)]
    mask = rules.masks(fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], single)
    A.check_against_reference(fix, mask)
    assert np.array_equal(mask, e["mask"])
    cmask = rules.masks(fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], fix["comps"])
    A.check_against_reference(fix, cmask, "comp_")
    assert np.array_equal(cmask, e["comp_mask"])
    assert np.array_equal(rules.action_areas(), e["areas"])


def test_factorisation_on_the_recorded_states(recorded):
    """entries with pairwise disjoint area sets: the composite is applied exactly when every entry's byte is 0"""
    m, fix, e = recorded
    rng = np.random.default_rng(1)
    areas, n_act = e["areas"], len(e["areas"])
    n_area = int(fix["sub_area"].max()) + 1
    draws = []
    while len(draws) < 60:
        c = rng.choice(n_act, size=min(3, n_area), replace=False)
        if all((areas[c[i]] & areas[c[j]]) == 0 for i in range(len(c)) for j in range(i)) and all(areas[c] != 0):
            draws.append(list(c) + [-1] * (3 - len(c)))
    draws = np.asarray(draws, np.int32)
    d = A.emul(m, fix["off"], fix["items"], fix["sub_area"], fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], comps=draws)
    each = np.stack([np.where(draws[:, k] >= 0, e["mask"][:, np.maximum(draws[:, k], 0)], 0) for k in range(3)])
    assert np.array_equal(d["comp_mask"] == 0, (each == 0).all(0))
    assert ((each != 0).any(0)).mean() >= 0.25 and (d["comp_mask"] == 0).any()


def test_one_index_in_several_slots(recorded):
    """nothing forbids it: the dense arrays of (a, a, a) and (a, -1, a) are those of `a`, so is the byte; (a, a, b) is (a, b); emulator
    and restatement agree on all of them"""
    m, fix, e = recorded
    n_act = len(e["areas"])
    a = np.arange(n_act, dtype=np.int32)
    b = np.roll(a, 7)
    dup = np.concatenate([np.stack([a, a, a], 1), np.stack([a, np.full(n_act, -1, np.int32), a], 1), np.stack([a, a, b], 1), np.stack([a, b, b], 1)])
    d = A.emul(m, fix["off"], fix["items"], fix["sub_area"], fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], comps=dup)
    assert np.array_equal(d["comp_mask"][:, :n_act], e["mask"]) and np.array_equal(d["comp_mask"][:, n_act:2 * n_act], e["mask"])
    pair = A.emul(m, fix["off"], fix["items"], fix["sub_area"], fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"],
                  comps=np.stack([a, b, np.full(n_act, -1, np.int32)], 1))
    assert np.array_equal(d["comp_mask"][:, 2 * n_act:3 * n_act], pair["comp_mask"]) and np.array_equal(d["comp_mask"][:, 3 * n_act:], pair["comp_mask"])
    rules = A.AreaRules(m, fix["off"], fix["items"], fix["sub_area"])
    rows = [0, len(fix["played"]) - 1]
    assert np.array_equal(rules.masks(fix["topo_vect"][rows], fix["cooldown_line"][rows], fix["cooldown_sub"][rows], dup), d["comp_mask"][rows])


def test_sanitized_stand_alone_emulator_runs_clean():
    p = subprocess.run([A.sanitized_program()], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert " 0 mismatches" in p.stdout


def test_area_sets_and_validation_through_a_header_only_handle(load_model):
    from grid2op_amd.engine import GridPFError, PowerFlowEngine
    fix = A.load_fixture("case14")
    m = load_model("l2rpn_case14_sandbox")
    eng = PowerFlowEngine(m, n_lanes=4, device=-1)
    acts = R.unpack_actions(fix["off"], fix["items"])
    with pytest.raises(GridPFError, match="no action table"):
        eng.topo_action_areas()
    amb = eng.upload_topo_actions(acts)
    assert np.array_equal(amb, fix["ambiguous"][0])
    assert set(np.unique(eng.topo_action_areas())) <= {0, 1}                       # no areas: one area, bit 0
    eng.set_topo_areas(fix["sub_area"])
    rules = A.AreaRules(m, fix["off"], fix["items"], fix["sub_area"])
    want = rules.action_areas()
    assert np.array_equal(eng.topo_action_areas(), want) and (want == 3).any() and (want == 1).any() and (want == 2).any()
    eng.set_topo_areas([list(range(0, 7)), list(range(7, 14))])                     # the list-of-lists form of the reference
    assert np.array_equal(eng.topo_action_areas(), want)
    eng.upload_topo_actions(acts[:5])                                               # areas set BEFORE an upload hold for it
    assert np.array_equal(eng.topo_action_areas(), want[:5])
    bad = fix["sub_area"].copy()
    bad[0] = 2
    with pytest.raises(GridPFError, match=r"outside \[0, n_area\)"):
        check_areas(eng, 2, bad)
    with pytest.raises(GridPFError, match="holds no substation"):
        check_areas(eng, 3, fix["sub_area"])
    with pytest.raises(GridPFError, match="at most 16"):
        check_areas(eng, 17, fix["sub_area"])
    with pytest.raises(GridPFError, match="negative"):
        check_areas(eng, -1, fix["sub_area"])
    with pytest.raises(ValueError, match="listed twice"):
        eng.set_topo_areas([[0, 1, 2], [2, 3]])
    assert np.array_equal(eng.topo_action_areas(), want[:5])                        # a refused call changes nothing
    eng.set_topo_areas(None)
    assert set(np.unique(eng.topo_action_areas())) <= {0, 1}
    for n in (0, 9):
        with pytest.raises(GridPFError, match="1..8"):
            eng.set_topo_slots(n)
    eng.close()


def check_areas(eng, n_area, sub_area):
    import ctypes as C
    from grid2op_amd.engine import check
    a = np.ascontiguousarray(sub_area, dtype=np.int32)
    check(eng._lib.gpf_set_topo_areas(eng._h, n_area, a.ctypes.data_as(C.POINTER(C.c_int32))), "gpf_set_topo_areas")


class _AreaStub(StubEngine):
    def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
        super().__init__(model, n_lanes, device, n_busbar)
        self.calls, self.idx = [], None

    def set_topo_areas(self, areas=None):
        self.calls.append(("areas", areas))

    def set_topo_slots(self, n_slot=1):
        self.calls.append(("slots", n_slot))

    def topo_action_areas(self):
        return np.array([1, 2, 3], np.uint32)

    def set_lane_topo_actions(self, index):
        self.idx = None if index is None else np.asarray(index).copy()


def test_sharded_engine_forwards_areas_slots_and_two_dimensional_indices():
    m = GridModel.load_npz(golden_path("l2rpn_case14_sandbox.grid.npz"))
    se = ShardedEngine(m, 37, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: _AreaStub(mm, n, dev, nbb))
    se.set_topo_areas([[0, 1], [2]])
    se.set_topo_slots(3)
    assert all(e.calls == [("areas", [[0, 1], [2]]), ("slots", 3)] for e in se.engines)
    assert list(se.topo_action_areas()) == [1, 2, 3]
    idx = np.arange(37 * 3, dtype=np.int32).reshape(37, 3)
    se.set_lane_topo_actions(idx)
    assert np.array_equal(np.concatenate([e.idx for e in se.engines]), idx) and all(e.idx.shape == (bn, 3) for e, (_, bn) in zip(se.engines, se.blocks))


def test_public_surface_is_declared():
    from grid2op_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "gridpf.h")).read()
    assert re.search(r"int gpf_set_topo_areas\(gpf_handle h, int32_t n_area, const int32_t\* sub_area", hdr)
    assert re.search(r"int gpf_set_topo_slots\(gpf_handle h, int32_t n_slot\);", hdr)
    assert re.search(r"int gpf_get_topo_action_areas\(gpf_handle h, uint32_t\* areas", hdr)
    for name in ("gpf_set_topo_areas", "gpf_set_topo_slots", "gpf_get_topo_action_areas"):
        assert name in _capi.EXPORTED_SYMBOLS
    assert "Factorisation guarantee" in hdr and "rulesByArea.py:120-140" in hdr
    assert "out of scope: RulesByArea" not in hdr
    core = open(os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_topo_mask.hpp")).read()
    assert len(re.findall(r"inline bool topo_dense_ambiguity\(", core)) == 1          # the ambiguity rules are stated once ...
    assert len(re.findall(r"unsigned topo_mask_rules\(", core)) == 1 and len(re.findall(r"TM_SUB_COOLDOWN;", core)) == 1   # so are the mask's
    pre = open(os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_topo.hpp")).read()
    assert "topo_dense_ambiguity(" in pre and "setv[po] == -1" not in pre             # ... and the pre-step kernel calls them
