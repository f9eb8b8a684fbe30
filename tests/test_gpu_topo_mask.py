"""Legality masks of the topology action table on the device (include/gridpf.h: gpf_topo_action_mask; kernel:
grid2op_amd/csrc/gridpf_topo_mask.hpp) against the verdicts recorded from the reference environment, the host emulator built from the same
rule core (tests/native/topo_mask_emul.cpp), and the flags the pre-step of an action launch gives when every entry is really played.
Grids: rte_case5_example (8 lines: bit sets shorter than a word), l2rpn_case14_sandbox, l2rpn_wcci_2022_dev (186 lines, 118 substations: three
and two 64-bit words)."""
import numpy as np
import pytest

from conftest import golden_path
from topo_rules_ref import random_topo_table
import topo_mask_ref as R

pytestmark = pytest.mark.gpu

RULES = dict(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=3)
GRIDS = ["rte_case5_example", "l2rpn_case14_sandbox", "l2rpn_wcci_2022_dev"]


def _engine(name, n):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path(f"{name}.grid.npz"))
    ch = dict(np.load(golden_path(f"{name}.chronics.npz")))
    if "prod_v" not in ch:                         # (fixtures without voltage set-points: the grid's own)
        ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    eng.set_lane_chronics(lane_offset=3 * np.arange(n))
    if "thermal_limits" in ch:                     # (rte_case5_example has none: its lanes run without the protections here)
        eng.set_thermal_limits(ch["thermal_limits"])
    return m, eng


def _set_states(eng, topo, lcd, scd, lane0=0):
    eng.set_topology(topo, lane0=lane0)
    eng.set_cooldown(lcd, lane0=lane0)
    eng.set_sub_cooldown(scd, lane0=lane0)


@pytest.mark.parametrize("tag", sorted(R.FIXTURES))
def test_device_mask_equals_reference_verdicts_and_emulator(tag):
    """the recorded states, one lane per recorded step"""
    fix = R.load_fixture(tag)
    n = fix["topo_vect"].shape[0]
    m, eng = _engine(R.FIXTURES[tag], n)
    amb = eng.upload_topo_actions(R.unpack_actions(fix["off"], fix["items"]))
    off, items = eng.pack_actions(R.unpack_actions(fix["off"], fix["items"]))
    assert np.array_equal(off, fix["off"]) and np.array_equal(items, fix["items"])
    eng.set_topo_rules(**RULES)
    _set_states(eng, fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"])
    mask = eng.topo_action_mask_host()
    assert np.array_equal(amb, fix["ambiguous"][0])
    R.check_against_reference(fix, mask)
    emu, _ = R.emul_mask(m, fix["off"], fix["items"], fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], True, 1, 1)
    assert np.array_equal(mask, emu)
    eng.close()


@pytest.mark.parametrize("name", GRIDS)
def test_mask_predicts_the_flags_of_the_action_launch(name):
    """every entry played from every source state in ONE one-step launch: is_illegal / is_ambiguous are what the mask said"""
    n, n_src = 130, 3
    rng = np.random.default_rng(11)
    m, eng = _engine(name, n)
    acts = random_topo_table(m, rng)
    n_act = len(acts)
    assert n_src * (n_act + 1) <= n
    eng.upload_topo_actions(acts)
    eng.set_topo_rules(**RULES)
    topo, lcd, scd = R.hand_set_states(m, rng, n_src)
    _set_states(eng, topo, lcd, scd)
    idx = np.full(n, -1, np.int32)
    for s in range(n_src):
        for j in range(n_act):
            eng.copy_lanes(s, n_src + s * n_act + j, 1)
        idx[n_src + s * n_act:n_src + (s + 1) * n_act] = np.arange(n_act)
    mask = eng.topo_action_mask_host()
    played = mask[np.arange(n), np.maximum(idx, 0)][idx >= 0]
    for bit in (R.TOO_MANY_LINES, R.TOO_MANY_SUBS, R.LINE_COOLDOWN, R.SUB_COOLDOWN, R.AMBIGUOUS):
        assert (played & bit).any(), bit
    assert (played == 0).any()
    for s in range(n_src):                                   # the copies have their source's mask rows
        assert (mask[n_src + s * n_act:n_src + (s + 1) * n_act] == mask[s]).all()
    eng.set_lane_topo_actions(idx)
    eng.step(1, nb_ts_reco=10)
    ill, amb = eng.topo_action_flags()
    assert np.array_equal(ill[idx >= 0], (played & 0x0F) != 0) and np.array_equal(amb[idx >= 0], (played & 0x10) != 0)
    assert not ill[idx < 0].any() and not amb[idx < 0].any()
    eng.close()


@pytest.mark.parametrize("name,n_act", [("l2rpn_wcci_2022_dev", 1), ("l2rpn_wcci_2022_dev", 63), ("l2rpn_wcci_2022_dev", 64), ("l2rpn_wcci_2022_dev", 65),
                                        ("l2rpn_wcci_2022_dev", 300), ("rte_case5_example", 65), ("l2rpn_case14_sandbox", 300)])
def test_shapes_strides_and_buffers(name, n_act):
    import torch
    n_lanes, lane0 = 140, 5
    rng = np.random.default_rng(n_act)
    m, eng = _engine(name, n_lanes)
    base = random_topo_table(m, rng)
    acts = (base[-3:] + base * 10)[:n_act]                    # (the tail first: the two-substation and the ambiguous entry are in every size > 1)
    eng.upload_topo_actions(acts)
    eng.set_topo_rules(**RULES)
    topo, lcd, scd = R.hand_set_states(m, rng, n_lanes)
    _set_states(eng, topo, lcd, scd)
    off, items = eng.pack_actions(acts)
    want, _ = R.emul_mask(m, off, items, topo, lcd, scd, True, 1, 1)
    stride = n_act + 7
    for n in (1, 3, 130):
        big = torch.full((n_lanes, stride), 0xEE, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        got = eng.topo_action_mask(lane0, n, out=big[lane0:lane0 + n])
        eng.sync()
        assert tuple(got.shape) == (n, n_act)
        h = big.cpu().numpy()
        assert np.array_equal(h[lane0:lane0 + n, :n_act], want[lane0:lane0 + n])
        assert (h[lane0:lane0 + n, n_act:] == 0xEE).all() and (h[:lane0] == 0xEE).all() and (h[lane0 + n:] == 0xEE).all()
        own = eng.topo_action_mask(lane0, n)                  # the engine-owned buffer ...
        eng.sync()
        assert tuple(own.shape) == (n, n_act) and np.array_equal(own.cpu().numpy(), want[lane0:lane0 + n])
        assert np.array_equal(eng.topo_action_mask_host(lane0, n), want[lane0:lane0 + n])     # ... and the host getter
    view = eng.device_views()["topo_mask"]
    assert tuple(view.shape) == (n_lanes, n_act) and view.dtype == torch.uint8
    # a table of another size: the buffer follows it
    acts2 = (base * 20)[:n_act + 70]
    assert len(acts2) == n_act + 70
    eng.upload_topo_actions(acts2)
    off2, items2 = eng.pack_actions(acts2)
    want2, _ = R.emul_mask(m, off2, items2, topo, lcd, scd, True, 1, 1)
    own = eng.topo_action_mask()
    eng.sync()
    assert tuple(own.shape) == (n_lanes, n_act + 70) and np.array_equal(own.cpu().numpy(), want2)
    assert tuple(eng.device_views()["topo_mask"].shape) == (n_lanes, n_act + 70)
    eng.close()


def test_always_legal_leaves_the_ambiguous_bit_alone():
    n = 12
    rng = np.random.default_rng(2)
    m, eng = _engine("l2rpn_wcci_2022_dev", n)
    acts = random_topo_table(m, rng)
    amb = eng.upload_topo_actions(acts)
    topo, lcd, scd = R.hand_set_states(m, rng, n)
    _set_states(eng, topo, lcd, scd)
    eng.set_topo_rules(**RULES)
    assert (eng.topo_action_mask_host() & 0x0F).any()
    eng.set_topo_rules(legal_rules=False, **RULES)
    mask = eng.topo_action_mask_host()
    assert amb.any() and np.array_equal(mask, np.tile(np.where(amb, R.AMBIGUOUS, 0).astype(np.uint8), (n, 1)))
    eng.close()


def test_mask_call_only_reads():
    """two engines through 8 acting steps, one of them taking a mask between handing the indices over and the launch"""
    n = 256
    rng = np.random.default_rng(4)
    m, a = _engine("l2rpn_case14_sandbox", n)
    _, b = _engine("l2rpn_case14_sandbox", n)
    acts = random_topo_table(m, rng)
    for e in (a, b):
        e.upload_topo_actions(acts)
        e.set_topo_rules(**RULES)
    n_ill = 0
    for t in range(1, 9):
        idx = rng.integers(-1, len(acts), size=n).astype(np.int32)
        a.set_lane_topo_actions(idx)
        b.set_lane_topo_actions(idx)
        mask = a.topo_action_mask_host()                       # (the pending indices must survive it)
        a.step(t, cascade=True, nb_ts_reco=10)
        b.step(t, cascade=True, nb_ts_reco=10)
        ra, rb = a.results(), b.results()
        assert np.array_equal(ra.out, rb.out, equal_nan=True) and np.array_equal(ra.status, rb.status), t
        assert np.array_equal(a.get_topology()[0], b.get_topology()[0]) and np.array_equal(a.cooldown(), b.cooldown()), t
        assert np.array_equal(a.sub_cooldown(), b.sub_cooldown()) and np.array_equal(a.last_bus(), b.last_bus()), t
        fa, fb = a.topo_action_flags(), b.topo_action_flags()
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]) and np.array_equal(a.episode()[0], b.episode()[0]), t
        played = mask[np.arange(n), np.maximum(idx, 0)]
        assert np.array_equal(fa[0][idx >= 0], (played[idx >= 0] & 0x0F) != 0) and np.array_equal(fa[1][idx >= 0], (played[idx >= 0] & 0x10) != 0), t
        n_ill += int(fa[0].sum())
    assert n_ill > 0
    a.close(); b.close()


def test_refusals_come_from_the_library_before_any_launch():
    import torch
    from grid2op_amd.engine import GridPFError
    n = 8
    m, eng = _engine("rte_case5_example", n)
    with pytest.raises(GridPFError, match="no action table"):
        eng.topo_action_mask()
    eng.set_topo_rules(**RULES)
    with pytest.raises(GridPFError, match="no action table"):
        eng.topo_action_mask_host()
    acts = random_topo_table(m, np.random.default_rng(0))
    eng.upload_topo_actions(acts)
    with pytest.raises(GridPFError, match="row_stride is smaller"):
        eng.topo_action_mask(0, 4, out=torch.zeros((4, len(acts) - 1), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(GridPFError, match="bad lane range"):
        eng.topo_action_mask(n - 1, 5)
    with pytest.raises(GridPFError, match="bad lane range"):
        eng.topo_action_mask_host(n - 1, 5)
    eng.upload_topo_actions([])                                 # an emptied table is no table
    with pytest.raises(GridPFError, match="no action table"):
        eng.topo_action_mask()
    eng.upload_topo_actions(acts)
    assert eng.topo_action_mask_host().shape == (n, len(acts))
    eng.close()
