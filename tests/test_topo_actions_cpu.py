"""Topology actions in the batched step, the parts that need no GPU: ShardedEngine routes the new calls by lane range, and the Python
restatement (tests/topo_rules_ref.py) of the reference's rules behaves as the reference on hand-made cases."""
import numpy as np

from conftest import golden_path
from grid2op_amd.grid_model import GridModel
from grid2op_amd.sharding import ShardedEngine
from stub_engine import StubEngine
from topo_rules_ref import TopoRules, pack_actions, random_topo_table, topo_pos_sub


class _TopoStub(StubEngine):
    """StubEngine + the acting-path calls, with per-lane state in numpy"""
    def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
        super().__init__(model, n_lanes, device, n_busbar)
        self.calls = []
        self.idx = None
        self.scd = np.zeros((self.n_lanes, model.n_sub), np.int32) + 100 * device
        self.lb = np.ones((self.n_lanes, model.dim_topo), np.int32)
        self.flags = np.zeros((self.n_lanes, 2), np.uint8)

    def set_topo_rules(self, *a, **kw):
        self.calls.append(("rules", a, kw))

    def upload_topo_actions(self, actions):
        self.calls.append(("table", len(actions)))
        return np.zeros(len(actions), bool)

    def set_lane_topo_actions(self, index):
        self.idx = None if index is None else np.asarray(index).copy()

    def topo_actions_on_device(self, on=True):
        self.calls.append(("device", on))

    def sub_cooldown(self, lane0=0, n=None):
        n = self.n_lanes - lane0 if n is None else n
        return self.scd[lane0:lane0 + n].copy()

    def set_sub_cooldown(self, c, lane0=0):
        self.scd[lane0:lane0 + len(c)] = c

    def last_bus(self, lane0=0, n=None):
        n = self.n_lanes - lane0 if n is None else n
        return self.lb[lane0:lane0 + n].copy()

    def set_last_bus(self, c, lane0=0):
        self.lb[lane0:lane0 + len(c)] = c

    def topo_action_flags(self, lane0=0, n=None):
        n = self.n_lanes - lane0 if n is None else n
        f = self.flags[lane0:lane0 + n]
        return f[:, 0].astype(bool), f[:, 1].astype(bool)


def test_sharded_engine_routes_topology_calls_by_lane_range():
    m = GridModel.load_npz(golden_path("l2rpn_case14_sandbox.grid.npz"))
    se = ShardedEngine(m, 37, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: _TopoStub(mm, n, dev, nbb))
    se.set_topo_rules(1, 1, 3, 3)
    assert se.upload_topo_actions([{}, {}]).shape == (2,)
    for e in se.engines:
        assert ("table", 2) in e.calls and e.calls[0][0] == "rules"
    idx = np.arange(37, dtype=np.int32)
    se.set_lane_topo_actions(idx)
    assert np.array_equal(np.concatenate([e.idx for e in se.engines]), idx)
    se.topo_actions_on_device()
    assert all(("device", True) in e.calls for e in se.engines)
    scd = se.sub_cooldown()
    assert scd.shape == (37, m.n_sub)
    assert np.array_equal(scd[:, 0], np.concatenate([np.full(bn, 100 * k) for k, (_, bn) in enumerate(se.blocks)]))
    new = np.arange(5 * m.n_sub, dtype=np.int32).reshape(5, m.n_sub)
    se.set_sub_cooldown(new, lane0=10)                       # crosses the first block boundary (13 lanes)
    assert np.array_equal(se.sub_cooldown(10, 5), new)
    lb = np.full((3, m.dim_topo), 2, np.int32)
    se.set_last_bus(lb, lane0=12)
    assert np.array_equal(se.last_bus(12, 3), lb) and (se.last_bus(0, 12) == 1).all()
    ill, amb = se.topo_action_flags(5, 20)
    assert ill.shape == (20,) and amb.shape == (20,)


def test_restatement_on_hand_made_cases():
    m = GridModel.load_npz(golden_path("l2rpn_case14_sandbox.grid.npz"))
    ps = topo_pos_sub(m)
    sub = int(np.argmax(np.bincount(ps)))
    pos = np.flatnonzero(ps == sub)
    lo, le = m.line_or_pos_topo_vect, m.line_ex_pos_topo_vect
    acts = [{"set_bus": {int(pos[0]): 2, int(pos[1]): 2}},           # 0 split
            {"set_line_status": [(0, -1)]},                          # 1 disconnect line 0
            {"set_line_status": [(0, 1)]},                           # 2 reconnect line 0
            {"set_bus": {int(pos[0]): 2}, "change_bus": [int(pos[0])]},  # 3 ambiguous (set + change of one element)
            {"set_line_status": [(0, -1), (1, -1)]}]                 # 4 two lines: illegal with MAX_LINE_STATUS_CHANGED = 1
    off, items = pack_actions(acts)
    R = TopoRules(m, off, items, True, 1, 1, 3, 3)
    assert list(R.ambiguous) == [False, False, False, True, False]
    row = np.asarray(m.initial_topo_vect(), np.int64)
    z_l, z_s, last = np.zeros(m.n_line, int), np.zeros(m.n_sub, int), np.ones(m.dim_topo, int)
    new, ill, amb, al, as_ = R.pre(row, z_l, z_s, last, 0)
    assert not ill and not amb and as_.sum() == 1 and as_[sub] and not al.any() and (new[pos[:2]] == 2).all()
    _, ill, _, _, _ = R.pre(row, z_l, as_.astype(int) * 3, last, 0)   # the substation is in its cooldown
    assert ill
    _, ill, _, _, _ = R.pre(row, z_l, z_s, last, 4)
    assert ill
    _, ill, amb, _, _ = R.pre(row, z_l, z_s, last, 3)
    assert amb and not ill
    _, _, amb, _, _ = R.pre(row, z_l, z_s, last, 99)
    assert amb
    off_row, ill, _, al, as_ = R.pre(row, z_l, z_s, last, 1)
    assert not ill and al[0] and not as_.any() and off_row[lo[0]] == -1 and off_row[le[0]] == -1
    last2 = last.copy()
    last2[lo[0]] = 2
    cd = z_l.copy()
    cd[0] = 2
    _, ill, _, _, _ = R.pre(off_row, cd, z_s, last2, 2)                # reconnection inside the line's cooldown
    assert ill
    back, ill, _, _, _ = R.pre(off_row, z_l, z_s, last2, 2)
    assert not ill and back[lo[0]] == 2 and back[le[0]] == 1           # back to the last known busbars
    lcd, scd, lb = R.post(back, z_l, np.array([0] * m.n_sub), last, al, as_)
    assert lcd[0] == 3 and not scd.any() and lb[lo[0]] == 2


def test_random_table_covers_the_kinds():
    m = GridModel.load_npz(golden_path("l2rpn_wcci_2022_dev.grid.npz"))
    acts = random_topo_table(m, np.random.default_rng(0))
    kinds = set(k for a in acts for k in a)
    assert {"set_bus", "change_bus", "set_line_status", "change_line_status"} <= kinds
    assert len(acts) >= 30
