"""`grid2op_amd.sharding.ShardedEngine`: the routing rules, checked name by name over one recording engine (CPU only).

Three engines hold 10 lanes in blocks of 4, 3 and 3; the global range ``lane0=2, n=7`` starts inside the first block and crosses both
boundaries.  An engine's answers are a function of (device, local lane), ``1000 * device + lane``, so the global-order concatenation
is known without any arithmetic of the engine."""
import dataclasses
import inspect
from types import SimpleNamespace

import numpy as np
import pytest

from grid2op_amd import sharding
from grid2op_amd.engine import CursorState, LaneResults, OpponentAreaState, OpponentState, PowerFlowEngine, OPP_STATE_INTS
from grid2op_amd.sharding import ROUTES, NOT_SHARDED, ShardedEngine, cut, every, first, gather, per_device, per_shard_tensor, scatter, scatter_state

MODEL = SimpleNamespace(n_line=5, n_sub=4, dim_topo=6, n_shunt=2, n_gen=3)
N_INJ = 3
LANE0, N = 2, 7
BLOCKS = [(0, 4), (4, 3), (7, 3)]
PARTS = [(0, 2, 2, 0), (1, 0, 3, 2), (2, 0, 2, 5)]          # (device, local lane0, count, offset into the caller's rows) of the range
HAND_WRITTEN = {"close", "runpf", "step", "upload_chronics", "upload_topo_actions", "set_opponent", "set_chronics_cursor", "fanout_n1",
                "simulate_candidates", "simulate_batch", "disconnect_line", "copy_lanes", "ptdf_build_batch", "ptdf_class", "counters",
                "specialize", "specialization", "results", "set_topology", "redispatch", "set_env_state"}


class Recorder:
    """Records ``(name, args, kwargs)`` of every call; ``reply(device, args, kwargs)`` makes the answer."""
    n_inj = N_INJ

    def __init__(self, model, n_lanes, device):
        self.model, self.n_lanes, self.device, self.log, self.reply = model, n_lanes, device, [], lambda device, args, kw: None

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kw):
            self.log.append((name, args, kw))
            return self.reply(self.device, args, kw)
        return call


def sharded(reply=None):
    se = ShardedEngine(MODEL, 10, devices=[0, 1, 2], engine_factory=lambda m, n, dev, nbb: Recorder(m, n, dev))
    assert se.blocks == BLOCKS
    for e in se.engines:
        e.log.clear()
        if reply is not None:
            e.reply = reply
    return se


def same(a, b):
    """Equality of nested answers / arguments: arrays by shape and value, dataclasses field by field."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    if dataclasses.is_dataclass(a):
        return type(a) is type(b) and all(same(getattr(a, f.name), getattr(b, f.name)) for f in dataclasses.fields(a))
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    return type(a) is type(b) and a == b


def logs(se):
    return [e.log for e in se.engines]


def public_methods(cls):
    return {k for k, v in vars(cls).items() if inspect.isfunction(v) and not k.startswith("_")}


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_every_engine_method_is_in_exactly_one_place():
    routed = [name for names in ROUTES.values() for name in names]
    unsharded = [name for name, reason in NOT_SHARDED if reason]
    places = routed + sorted(HAND_WRITTEN) + unsharded
    assert len(places) == len(set(places)), sorted(n for n in set(places) if places.count(n) > 1)
    assert len(unsharded) == len(NOT_SHARDED) == 14
    assert set(places) == public_methods(PowerFlowEngine)
    assert public_methods(ShardedEngine) == set(routed) | HAND_WRITTEN | {"owner"}
    assert public_methods(ShardedEngine) - set(routed) == HAND_WRITTEN | {"owner"}        # what is written out in the class body
    assert set(ROUTES) == {every, first, per_device, cut, gather, per_shard_tensor, scatter, scatter_state}
    for name, params in ROUTES[scatter].items():                                       # the row argument by the engine's name, then lane0
        assert list(inspect.signature(getattr(PowerFlowEngine, name)).parameters)[1:3] == [params["rows"], "lane0"], name
    for name in ROUTES[scatter_state]:
        assert list(inspect.signature(getattr(PowerFlowEngine, name)).parameters)[1:3] == ["state", "lane0"], name
    se = sharded()
    for name in unsharded:
        assert not hasattr(se, name)
        with pytest.raises(AttributeError):
            getattr(se, name)


def test_installed_methods_are_documented_attributes_of_the_class():
    for rule, names in ROUTES.items():
        for name in names:
            m = vars(ShardedEngine)[name]
            assert m.__name__ == name and name in dir(ShardedEngine)
            assert m.__doc__ and rule.__name__ in m.__doc__ and f"PowerFlowEngine.{name}" in m.__doc__
    for name in HAND_WRITTEN | {"owner"}:
        assert inspect.isfunction(vars(ShardedEngine)[name])
    assert "TRAJ_OBS" in vars(ShardedEngine) and "__getattr__" not in vars(ShardedEngine)


# ---- every / first / per_device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROUTES[every]))
def test_every(name):
    se = sharded(lambda dev, a, kw: dev)
    arr = np.arange(4)
    assert getattr(se, name)(1, arr, key="v") is None
    assert all(len(log) == 1 and log[0][0] == name and log[0][1][0] == 1 and log[0][1][1] is arr and log[0][2] == {"key": "v"} for log in logs(se))


@pytest.mark.parametrize("name", list(ROUTES[first]))
def test_first(name):
    se = sharded(lambda dev, a, kw: ("answer", dev))
    assert getattr(se, name)(3, n=2) == ("answer", 0)
    assert logs(se) == [[(name, (3,), {"n": 2})], [], []]


@pytest.mark.parametrize("name", list(ROUTES[per_device]))
def test_per_device(name):
    se = sharded(lambda dev, a, kw: {"device": dev})
    assert getattr(se, name)(key=1) == [{"device": 0}, {"device": 1}, {"device": 2}]
    assert logs(se) == [[(name, (), {"key": 1})]] * 3


# ---- cut -----------------------------------------------------------------------------------------------------------------
def cut_case(name):
    """(args, kw of the call, what block [b0, b0 + bn) must receive)"""
    a, b = np.arange(20).reshape(10, 2), np.arange(10.0)
    if name in ("upload_opponent_draws", "upload_cursor_draws"):                       # flat draws: [n_lanes, n_draw]
        return (np.arange(30.0),), {}, lambda b0, bn: ((np.arange(30.0).reshape(10, 3)[b0:b0 + bn],), {})
    if name == "upload_opponent_schedule":                                             # flat schedule, one count for all lanes
        sch = np.arange(40)
        return (sch, 2), {}, lambda b0, bn: ((sch.reshape(10, 2, 2)[b0:b0 + bn], np.full(bn, 2)), {})
    if name == "upload_opponent_area_schedule":                                        # one [n_area, k, 2] schedule for all lanes, counts per area
        sch, cnt = np.arange(12).reshape(2, 3, 2), np.array([3, 1])
        return (sch, cnt), {}, lambda b0, bn: ((np.tile(sch, (bn, 1, 1, 1)), np.tile(cnt, (bn, 1))), {})
    if name == "set_episode_limit":                                                    # [n_lanes, 1] limits; the scalars pass
        return (b.reshape(10, 1), 2.0), {"alert_end_bonus": 1.5}, lambda b0, bn: ((b[b0:b0 + bn], 2.0), {"alert_end_bonus": 1.5})
    return (a, None, True), {"key": b, "none": None}, lambda b0, bn: ((a[b0:b0 + bn], None, True), {"key": b[b0:b0 + bn], "none": None})


@pytest.mark.parametrize("name", list(ROUTES[cut]))
def test_cut(name):
    se = sharded()
    args, kw, want = cut_case(name)
    assert getattr(se, name)(*args, **kw) is None
    for log, (b0, bn) in zip(logs(se), BLOCKS):
        wa, wkw = want(b0, bn)
        assert len(log) == 1 and log[0][0] == name and same(log[0][1], wa) and same(log[0][2], wkw), (log, wa, wkw)


def test_cut_passes_none_and_scalars_through():
    se = sharded()
    se.set_lane_actions(None, 4.5, hold_storage=True)
    se.set_episode_limit(7, 2.0)
    se.set_episode_limit(None)
    area = np.arange(10 * 2 * 3 * 2).reshape(10, 2, 3, 2)                              # per-lane area schedules and counts
    se.upload_opponent_area_schedule(schedule=area, count=np.arange(20).reshape(10, 2))
    for log, (b0, bn) in zip(logs(se), BLOCKS):
        assert log[:3] == [("set_lane_actions", (None, 4.5), {"hold_storage": True}), ("set_episode_limit", (7, 2.0), {}), ("set_episode_limit", (None,), {})]
        assert same(log[3][1], (area[b0:b0 + bn], np.arange(20).reshape(10, 2)[b0:b0 + bn])) and log[3][2] == {}


# ---- gather --------------------------------------------------------------------------------------------------------------
def ids_of(dev, lane0, n):
    return 1000 * dev + lane0 + np.arange(n)


GLOBAL_IDS = np.concatenate([ids_of(dev, l0, k) for dev, l0, k, _ in PARTS])
TUPLES = {"get_topology": 2, "episode": 3, "step_outputs": 3, "topo_action_flags": 2}
DICTS = ("env_state", "episode_ends", "episode_stats")


def lane_results(ids, bus=True):
    two = np.tile(ids[:, None], (1, 2))
    return LaneResults(out=two.astype(np.float32), topo_vect=two, shunt_bus=two + 1, line_status=two % 2 == 0, status=two + 2,
                       bus_vm=two + 0.5 if bus else None, bus_va=two - 0.5 if bus else None, _slices={"rho": slice(0, 1)})


def answer(name, ids, n_steps=3):
    """The answer of ``name`` for the lanes ``ids``, in the shape of the engine's return type."""
    two = np.tile(ids[:, None], (1, 2))
    if name == "reset":
        return None
    if name in TUPLES:
        return tuple(two + i for i in range(TUPLES[name]))
    if name in DICTS:
        return {"a": two, "b": ids.astype(np.float32), "c": ids % 2 == 0}
    if name == "results":
        return lane_results(ids)
    if name == "opponent_state":
        return OpponentState.from_rows(ids + 0.25, np.tile(ids[:, None], (1, OPP_STATE_INTS)).astype(np.int32))
    if name == "opponent_area_state":
        return OpponentAreaState(*(np.tile(ids[:, None], (1, 2)).astype(np.int32) + i for i in range(6)))
    if name == "chronics_cursor_state":
        return CursorState(*(ids.astype(np.int32) + i for i in range(7)))
    if name == "trajectory":                                                            # the lanes are on axis 1
        return np.tile(two[None], (n_steps, 1, 1)), np.tile(ids[None], (n_steps, 1))
    if name == "trajectory_cooldown":
        return np.tile(two[None], (n_steps, 1, 1))
    if name == "trajectory_obs":
        return [lane_results(ids + s, bus=False) for s in range(n_steps)]
    return two


@pytest.mark.parametrize("name", list(ROUTES[gather]))
def test_gather(name):
    steps = ROUTES[gather][name].get("steps", False)
    head = (3, 1) if steps else ()
    se = sharded(lambda dev, a, kw: answer(name, ids_of(dev, a[-2], a[-1])))
    got = getattr(se, name)(*head, LANE0, N, key="v")
    assert [e.log for e in se.engines] == [[(name, head + (l0, k), {"key": "v"})] for _, l0, k, _ in PARTS]
    assert same(got, answer(name, GLOBAL_IDS))
    se = sharded(lambda dev, a, kw: answer(name, ids_of(dev, a[-2], a[-1])))
    got =getattr(se, name)(*head[:1], n=4, lane0=3) if steps else getattr(se, name)(n=4, lane0=3)         # by keyword: lanes 3 .. 6
    assert [e.log for e in se.engines] == [[(name, head[:1] + (0, 3, 1) if steps else (3, 1), {})], [(name, head[:1] + (0, 0, 3) if steps else (0, 3), {})], []]
    assert same(got, answer(name, np.array([3, 1000, 1001, 1002])))
    whole = getattr(se, name)(*head[:1])                                                                    # the whole batch
    assert same(whole, answer(name, np.concatenate([ids_of(dev, 0, bn) for dev, (_, bn) in enumerate(BLOCKS)])))
    with pytest.raises(ValueError, match="out of bounds"):
        getattr(se, name)(*head, 5, 6)


def test_results_joins_the_shards_and_forwards_pinned_only_when_set():
    se = sharded(lambda dev, a, kw: answer("results", ids_of(dev, a[0], a[1])))
    got = se.results(LANE0, N)
    assert logs(se) == [[("results", (l0, k), {"with_bus": True})] for _, l0, k, _ in PARTS]
    assert same(got, answer("results", GLOBAL_IDS)) and got._slices == {"rho": slice(0, 1)} and np.array_equal(got.rho[:, 0], GLOBAL_IDS)
    se.results(0, 4, with_bus=False, pinned=False)
    se.results(0, 4, pinned=True)
    assert se.engines[0].log[1:] == [("results", (0, 4), {"with_bus": False}), ("results", (0, 4), {"with_bus": True, "pinned": True})]


# ---- per_shard_tensor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROUTES[per_shard_tensor]))
def test_per_shard_tensor(name):
    keys, steps = ROUTES[per_shard_tensor][name]["keys"], ROUTES[per_shard_tensor][name].get("steps", False)
    head = (3, 1) if steps else ()
    none = dict.fromkeys(keys)

    def fresh():
        return sharded(lambda dev, a, kw: ("tensor", dev, a[-2], a[-1]))
    want = [("tensor", dev, l0, k) for dev, l0, k, _ in PARTS]
    se = fresh()
    assert getattr(se, name)(*head, LANE0, N, **none) == want                          # no tensors given: the engines make their own
    assert logs(se) == [[(name, head + (l0, k), none)] for _, l0, k, _ in PARTS]
    given = {key: [f"{key}{i}" for i in range(3)] for key in keys}
    se = fresh()
    assert getattr(se, name)(*head, LANE0, N, **given, other=5) == want
    assert logs(se) == [[(name, head + (l0, k), {"other": 5, **{key: f"{key}{i}" for key in keys}})] for i, (_, l0, k, _) in enumerate(PARTS)]
    se = fresh()
    assert getattr(se, name)(*head, LANE0, N, *given.values()) == want                 # the lists by position, as the engine takes its tensors
    assert logs(se) == [[(name, head + (l0, k), {key: f"{key}{i}" for key in keys})] for i, (_, l0, k, _) in enumerate(PARTS)]
    label = {"out": "output", "flags": "flag"}
    for key in keys:
        se = sharded()
        said = " / ".join(f"{2 if k == key else 3} {label[k]}" for k in keys)
        with pytest.raises(ValueError, match=f"ShardedEngine.{name}: 3 shards intersect the range, {said} tensors given"):
            getattr(se, name)(*head, LANE0, N, **{**given, key: ["x", "y"]})
        assert logs(se) == [[], [], []]
    assert len(getattr(se, name)(*head, 4, 3, **{keys[-1]: ["only"]})) == 1            # one shard: a list of one
    with pytest.raises(TypeError):
        getattr(se, name)(*head, LANE0, N, *given.values(), "one too many")
    with pytest.raises(TypeError):
        getattr(se, name)(*head, LANE0, N, given[keys[0]], **{keys[0]: given[keys[0]]})
    with pytest.raises(ValueError, match="out of bounds"):
        getattr(se, name)(*head, 8, 3)


# ---- scatter -------------------------------------------------------------------------------------------------------------
def scatter_case(name):
    """(rows of the call, the rows as the engines must see them before they are cut)"""
    if name == "set_opponent_state":
        st = OpponentState.from_rows(np.arange(7) + 0.5, np.tile(np.arange(7)[:, None], (1, OPP_STATE_INTS)).astype(np.int32))
        return [st], [st]
    if name == "set_opponent_area_state":
        st = OpponentAreaState(*(np.arange(14, dtype=np.int32).reshape(7, 2) + i for i in range(6)))
        return [st], [st]
    if name == "set_chronics_cursor_state":
        st = CursorState(*(np.arange(7, dtype=np.int32) + i for i in range(7)))
        return [st], [st]
    if name == "set_alert_state":                                                      # the last axis is kept
        a = np.arange(7 * 4).reshape(7, 4)
        return [a], [a]
    if name == "redispatch":                                                           # five flat row arrays and one value per lane
        rows = [np.arange(21.0) + i for i in range(5)]
        return rows + [4.0], [r.reshape(7, 3) for r in rows] + [np.full(7, 4.0)]
    size = {"n_inj": N_INJ, "model.dim_topo": 6, "model.n_line": 5, "model.n_sub": 4}[ROUTES[scatter][name]["width"]]
    rows = np.arange(7 * size)                                                         # flat rows: [-1, width]
    return [rows], [rows.reshape(7, size)]


def take(rows, a, b):
    if dataclasses.is_dataclass(rows):
        return type(rows)(*(getattr(rows, f.name)[a:b] for f in dataclasses.fields(rows)))
    return rows[a:b]


@pytest.mark.parametrize("name", list(ROUTES[scatter]) + list(ROUTES[scatter_state]) + ["redispatch"])
def test_scatter(name):
    rows, seen = scatter_case(name)
    routed = name != "redispatch"                                                      # redispatch: written out, its answers are gathered
    reply = None if routed else \
        (lambda dev, a, kw: (ids_of(dev, kw["lane0"], len(a[0])) % 2 == 0, np.tile(ids_of(dev, kw["lane0"], len(a[0]))[:, None], (1, 2))))
    extra = {"extra": "e"} if routed else {"apply": True}
    se = sharded(reply)
    got = getattr(se, name)(*rows, lane0=LANE0, **extra)
    for log, (_, l0, k, off) in zip(logs(se), PARTS):
        assert len(log) == 1 and log[0][0] == name and log[0][2] == {"lane0": l0, **extra}
        assert same(log[0][1], tuple(take(r, off, off + k) for r in seen)), (log, off, k)
    assert got is None if routed else same(got, (GLOBAL_IDS % 2 == 0, np.tile(GLOBAL_IDS[:, None], (1, 2))))
    se = sharded(reply)
    getattr(se, name)(*rows, LANE0)                                                    # lane0 by position
    assert [log[0][2]["lane0"] for log in logs(se)] == [l0 for _, l0, _, _ in PARTS]
    se = sharded(reply)
    getattr(se, name)(*(take(r, 0, 3) if np.ndim(r) or dataclasses.is_dataclass(r) else r for r in seen))   # lane0 = 0: three rows, one engine
    assert [len(log) for log in logs(se)] == [1, 0, 0] and se.engines[0].log[0][2]["lane0"] == 0
    if name in ROUTES[scatter]:                                                        # the rows by the engine's name for them
        se = sharded()
        getattr(se, name)(**{ROUTES[scatter][name]["rows"]: rows[0]}, lane0=LANE0)
        assert all(same(log, [(name, (seen[0][off:off + k],), {"lane0": l0})]) for log, (_, l0, k, off) in zip(logs(se), PARTS))
    with pytest.raises(ValueError, match="out of bounds"):
        getattr(se, name)(*rows, lane0=4)


def test_the_topology_and_the_dynamics_state_are_cut_by_rows():
    import torch
    se = sharded()
    topo = np.arange(42).reshape(7, 6)
    se.set_topology(topo, lane0=LANE0)
    se.set_topology(shunt_bus=np.arange(14), topo=np.arange(42), lane0=LANE0)          # flat rows get their width
    target, amount = np.arange(21.0).reshape(7, 3), np.arange(7.0)
    se.set_env_state(LANE0, target=target, charge=None, amount_prev=amount)            # the rows are the keywords; None fields are left out
    se.set_env_state(LANE0)                                                            # no rows: no call
    se.set_env_state(LANE0, target=torch.arange(21.0).reshape(7, 3), amount_prev=amount.tolist())     # any array-like is rows
    for log, (_, l0, k, off) in zip(logs(se), PARTS):
        assert len(log) == 4
        assert same(log[0], ("set_topology", (topo[off:off + k], None), {"lane0": l0}))
        assert same(log[1], ("set_topology", (topo[off:off + k], np.arange(14).reshape(7, 2)[off:off + k]), {"lane0": l0}))
        assert same(log[2], ("set_env_state", (l0,), {"target": target[off:off + k], "amount_prev": amount[off:off + k]}))
        assert same(log[3], ("set_env_state", (l0,), {"target": target[off:off + k].astype(np.float32), "amount_prev": amount[off:off + k]}))
    no_shunt = ShardedEngine(SimpleNamespace(dim_topo=6, n_shunt=0), 10, devices=[0, 1, 2], engine_factory=lambda m, n, dev, nbb: Recorder(m, n, dev))
    no_shunt.set_topology(topo, np.zeros((7, 0)), lane0=LANE0)                          # a grid without shunts: the engines get None
    assert all(same(e.log[-1][1], (topo[off:off + k], None)) for e, (_, _, k, off) in zip(no_shunt.engines, PARTS))


def test_a_hand_written_method_still_reaches_the_routed_ones():
    """`copy_lanes` across devices is built from the routed getters and setters"""
    se = sharded()
    wide = {"get_injections": N_INJ, "cooldown": MODEL.n_line, "get_topology": (MODEL.dim_topo, MODEL.n_shunt), "step_outputs": (MODEL.n_line,) * 3}

    def reply(eng):
        def make(dev, a, kw):
            name = eng.log[-1][0]
            if name == "env_state":
                return answer(name, ids_of(dev, a[0], a[1]))
            if name not in wide:
                return None
            rows = [np.tile(ids_of(dev, a[0], a[1])[:, None], (1, w)) for w in np.atleast_1d(wide[name])]
            return tuple(rows) if isinstance(wide[name], tuple) else rows[0]
        return make
    for e in se.engines:
        e.reply = reply(e)
    se.copy_lanes(3, 6, 2)                                                             # lanes 3, 4 (devices 0, 1) -> lanes 6, 7 (devices 1, 2)
    names = [[c[0] for c in log] for log in logs(se)]
    assert names[0] == ["get_topology", "get_injections", "step_outputs", "cooldown", "env_state"]
    assert names[2] == ["set_injections", "set_topology", "set_overflow_count", "set_cooldown", "set_env_state"]
    assert same(se.engines[2].log[0], ("set_injections", (np.full((1, N_INJ), 1000),), {"lane0": 0}))
    se.copy_lanes(0, 2, 2)                                                             # inside one device: the engine's own copy
    assert se.engines[0].log[-1] == ("copy_lanes", (0, 2, 2), {})


def test_a_rule_is_a_function_of_the_name_alone():
    """a new batched engine method is one name in one table: the rule needs nothing else"""
    m = sharding.gather("brand_new_getter")
    se = sharded(lambda dev, a, kw: ids_of(dev, a[0], a[1]))
    assert np.array_equal(m(se, LANE0, N), GLOBAL_IDS) and se.engines[1].log == [("brand_new_getter", (0, 3), {})]
