"""Static sharding of the lane batch over the GPUs of one node.

Lanes (environment copies / N-1 contingencies) never communicate, so the batch is cut into contiguous blocks, one
per rank (one process per GPU); there is NO collective on the data path.  ``torch.distributed`` (RCCL on the GPU
box, gloo in the CPU tests) is only used for the barrier and the max-over-ranks timing that ``bench.py`` reports.
"""
from __future__ import annotations

from dataclasses import fields, is_dataclass
from operator import attrgetter
from typing import Tuple

import numpy as np

__all__ = ["lane_range", "synthetic_lane_inputs", "max_over_ranks", "sum_over_ranks", "visible_devices", "ShardedEngine"]


def lane_range(total_lanes: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous block ``[lane0, lane0+n)`` of global lane ids owned by ``rank`` (sizes differ by at most 1)."""
    if not (0 <= rank < world):
        raise ValueError("rank out of range")
    base, rem = divmod(int(total_lanes), int(world))
    n = base + (1 if rank < rem else 0)
    lane0 = rank * base + min(rank, rem)
    return lane0, n


def synthetic_lane_inputs(n_load: int, T: int, lane_ids) -> Tuple[np.ndarray, np.ndarray]:
    """The synthetic workload of SURVEY.md 8(d) cfg 2, a pure function of the GLOBAL lane id (so that any
    sharding reproduces the same global batch): lane k reads chronics row ``(t + 7k) mod T`` and scales its loads by
    ``1 + 0.05 N(0,1)`` drawn from ``numpy.random.default_rng(k)``."""
    lane_ids = np.asarray(lane_ids, dtype=np.int64)
    offsets = ((7 * lane_ids) % T).astype(np.int32)
    scale = np.empty((lane_ids.size, 2 * n_load), dtype=np.float32)
    for i, k in enumerate(lane_ids):
        scale[i] = 1.0 + 0.05 * np.random.default_rng(int(k)).standard_normal(2 * n_load)
    return offsets, scale


def max_over_ranks(value: float, dist=None, device=None) -> float:
    """MAX-reduce a host scalar over the ranks (identity when not distributed)."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return float(value)
    import torch
    t = torch.tensor([value], dtype=torch.float64, device=device if device is not None else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(value: float, dist=None, device=None) -> float:
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return float(value)
    import torch
    t = torch.tensor([value], dtype=torch.float64, device=device if device is not None else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item())


def visible_devices() -> int:
    """Number of HIP devices this process sees (``gpf_device_count``; raises when the library is not built)."""
    import ctypes as C
    from . import _capi
    n = C.c_int32(0)
    _capi.check(_capi.lib().gpf_device_count(C.byref(n)), "gpf_device_count")
    return int(n.value)


class ShardedEngine:
    """Single-process multi-GPU engine: one `PowerFlowEngine` (own HIP stream) per device, the global lane batch cut
    into the contiguous blocks of `lane_range`.  Lanes never communicate, so there is no cross-device operation: every
    call is forwarded to the engines that own the addressed lanes (asynchronous calls stay asynchronous, i.e. one host
    thread keeps all the devices busy) and results are concatenated in global lane order.

    Most of the batched API is forwarded by one of the routing rules below the class: `ROUTES` names the rule of every
    such method and one loop installs them, so a new batched engine method is one name in one table.  The methods written
    out here are the ones that fit no rule; `NOT_SHARDED` lists the engine methods that are not forwarded at all.

    Counterpart in the reference: its only parallelism is one process per environment -- ``Runner._run_parrallel``
    (grid2op/Runner/runner.py:1071-1253, a ``multiprocessing.Pool`` over episodes) and ``BaseMultiProcessEnvironment``
    (grid2op/Environment/baseMultiProcessEnv.py:22, 293, one worker process per environment copy).  ``bench.py``
    uses the other form (one PROCESS per GPU, `lane_range` of the global batch per rank)."""

    TRAJ_RHO, TRAJ_OBS = 1, 2

    def __init__(self, model, n_lanes: int, devices=None, n_busbar: int = 2, engine_factory=None):
        if devices is None:
            devices = list(range(visible_devices()))
        devices = [int(d) for d in devices]
        if not devices:
            raise RuntimeError("ShardedEngine: no HIP device visible (there is no CPU fallback)")
        if n_lanes < len(devices):
            raise ValueError("ShardedEngine: fewer lanes than devices")
        if engine_factory is None:
            from .engine import PowerFlowEngine
            engine_factory = lambda m, n, dev, nbb: PowerFlowEngine(m, n_lanes=n, device=dev, n_busbar=nbb)  # noqa: E731
        self.model = model
        self.n_lanes = int(n_lanes)
        self.devices = devices
        self.blocks = [lane_range(self.n_lanes, len(devices), r) for r in range(len(devices))]
        self.engines = [engine_factory(model, n, dev, n_busbar) for dev, (_, n) in zip(devices, self.blocks)]
        e0 = self.engines[0]
        for k in ("n_inj", "n_out", "n_chron", "nb_total", "layout", "out_slices", "inj_slices", "init_inj"):
            if hasattr(e0, k):
                setattr(self, k, getattr(e0, k))

    # ---- routing ------------------------------------------------------------------------------------------------------
    def _parts(self, lane0: int = 0, n=None):
        """(engine, local lane0, count, offset into the caller's rows) of the shards that intersect [lane0, lane0+n)."""
        if n is None:
            n = self.n_lanes - lane0
        if lane0 < 0 or n < 0 or lane0 + n > self.n_lanes:
            raise ValueError("ShardedEngine: lane range out of bounds")
        out = []
        for eng, (b0, bn) in zip(self.engines, self.blocks):
            a, b = max(lane0, b0), min(lane0 + n, b0 + bn)
            if a < b:
                out.append((eng, a - b0, b - a, a - lane0))
        return out

    def owner(self, lane: int):
        (eng, l0, _, _), = self._parts(lane, 1)
        return eng, l0

    # ---- solve (asynchronous: queued on every device's stream) ----------------------------------------------------------------
    # One host thread per device: a launch call is planning + parameter upload + the launch itself (~10 us of host time on an
    # MI355X box) and the ctypes call releases the GIL, so the launches of the devices are issued CONCURRENTLY -- issued from one
    # thread, 8 devices x ~10 us serialised per step would be a third of a 26 us step.  The threads are created lazily and only with
    # more than one device; HIP handles are thread-compatible (one engine is only ever driven by one thread at a time: `_fan` joins
    # before it returns).
    def _fan(self, calls):
        if len(calls) <= 1:
            for fn in calls:
                fn()
            return
        if getattr(self, "_pool", None) is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=len(self.engines), thread_name_prefix="gridpf-dev")
        for f in [self._pool.submit(fn) for fn in calls]:
            f.result()                                   # re-raises a GridPFError of any device

    def runpf(self, lane0: int = 0, n=None, **kw):
        self._fan([(lambda e=eng, a=l0, b=k: e.runpf(a, b, **kw)) for eng, l0, k, _ in self._parts(lane0, n)])

    def step(self, t: int, **kw):
        self._fan([(lambda e=eng: e.step(t, **kw)) for eng in self.engines])

    # ---- what fits no rule -----------------------------------------------------------------------------------------------
    def upload_chronics(self, tables):                   # no rule: records the tables' length
        for eng in self.engines:                     # every device holds its own copy of the (small) tables
            eng.upload_chronics(tables)
        self.chron_T = self.engines[0].chron_T

    def upload_topo_actions(self, actions):              # no rule: every device gets the table, the first one's answer comes back
        return [eng.upload_topo_actions(actions) for eng in self.engines][0]

    def disconnect_line(self, lane: int, line_id: int):  # no rule: one lane of one device
        eng, l0 = self.owner(lane)
        eng.disconnect_line(l0, line_id)

    def results(self, lane0: int = 0, n=None, with_bus: bool = True, pinned: bool = False):
        """(``pinned``: every device's rows come over by DMA into its engine's pinned block; the concatenation below is the one host copy)"""
        # no rule: ``pinned`` is forwarded only when set (the engine of the launcher test has no such keyword)
        return _cat([eng.results(l0, k, with_bus=with_bus, **({"pinned": True} if pinned else {})) for eng, l0, k, _ in self._parts(lane0, n)])

    def set_topology(self, topo, shunt_bus=None, lane0: int = 0):        # no rule: two row arrays, the second optional and absent without shunts
        topo = np.asarray(topo).reshape(-1, self.model.dim_topo)
        sb = None if shunt_bus is None or not self.model.n_shunt else np.asarray(shunt_bus).reshape(-1, self.model.n_shunt)
        for eng, l0, n, off in self._parts(lane0, topo.shape[0]):
            eng.set_topology(topo[off:off + n], None if sb is None else sb[off:off + n], lane0=l0)

    def redispatch(self, new_p, prev_p, actual, target, modified, rhs, lane0: int = 0, apply: bool = False):
        # no rule: five row arrays and one value per lane go out, two arrays come back
        ng = self.model.n_gen
        rows = [np.asarray(a).reshape(-1, ng) for a in (new_p, prev_p, actual, target, modified)]
        n = rows[0].shape[0]
        rhs = np.broadcast_to(np.asarray(rhs, dtype=np.float64), (n,))
        oks, afters = [], []
        for eng, l0, k, off in self._parts(lane0, n):
            ok, after = eng.redispatch(*[r[off:off + k] for r in rows], rhs[off:off + k], lane0=l0, apply=apply)
            oks.append(ok)
            afters.append(after)
        return np.concatenate(oks), np.concatenate(afters)

    def set_env_state(self, lane0: int = 0, **fields):                   # no rule: the rows are whatever keywords are given
        """`PowerFlowEngine.set_env_state` on the global lane range starting at ``lane0``: every array is cut by device block."""
        arrs = {k: np.asarray(v) for k, v in fields.items() if v is not None}
        if not arrs:
            return
        n = next(iter(arrs.values())).shape[0]
        for eng, l0, k, off in self._parts(lane0, n):
            eng.set_env_state(l0, **{key: a[off:off + k] for key, a in arrs.items()})

    def counters(self) -> dict:
        """Step launches / kernel dispatches summed over the devices."""
        cs = [eng.counters() for eng in self.engines]
        return {k: sum(c[k] for c in cs) for k in cs[0]}

    # the opponent and the chronics cursor: the configuration goes to every device with the shard's lane_base (which makes the Philox
    # streams of the shards those of one engine) and has an "off" form
    def set_opponent(self, kind=0, lines=(), **kw):
        base = int(kw.pop("lane_base", 0))
        for eng, (b0, _) in zip(self.engines, self.blocks):
            if kind is None or int(kind) == 0:
                eng.set_opponent(None)
            else:
                eng.set_opponent(kind, lines, lane_base=base + b0, **kw)

    def set_chronics_cursor(self, order=None, policy="sequential", probabilities=None, first_row=0, next_pos=None, seed=None, lane_base: int = 0):
        def cut(v, b0, bn):
            return v if v is None or np.ndim(v) == 0 else np.asarray(v).reshape(self.n_lanes)[b0:b0 + bn]
        for eng, (b0, bn) in zip(self.engines, self.blocks):
            if order is False:
                eng.set_chronics_cursor(False)
            else:
                eng.set_chronics_cursor(order, policy, probabilities, cut(first_row, b0, bn), cut(next_pos, b0, bn), seed, lane_base=int(lane_base) + b0)

    # DC sensitivities of per-lane topologies: every device builds the tables of the topologies ITS lanes hold; class ids are per shard
    # (a class of shard s is reported as ``class_offset[s] + local id``), so that `ptdf_class` finds the owner again
    def ptdf_build_batch(self, lane0: int = 0, n=None, with_lodf: bool = True) -> dict:
        if n is None:
            n = self.n_lanes - lane0
        lc = np.empty(n, np.int32)
        st, cn, ms, self._ptdfb_owner = [], [], 0.0, []
        for eng, l0, k, off in self._parts(lane0, n):
            r = eng.ptdf_build_batch(l0, k, with_lodf=with_lodf)
            base = len(st)
            lc[off:off + k] = np.where(r["lane_class"] >= 0, r["lane_class"] + base, -1)
            st.extend(r["class_status"].tolist()); cn.extend(r["class_n"].tolist())
            self._ptdfb_owner.extend((eng, c) for c in range(r["n_classes"]))
            ms = max(ms, r["kernel_ms"])                      # the devices run concurrently
        return {"n_classes": len(st), "lane_class": lc, "class_status": np.asarray(st, np.int32), "class_n": np.asarray(cn, np.int32), "kernel_ms": ms}

    def ptdf_class(self, cls: int, lodf: bool = False):
        eng, c = self._ptdfb_owner[int(cls)]
        return eng.ptdf_class(c, lodf=lodf)

    def copy_lanes(self, src: int, dst: int, n: int = 1):
        """Device-side copy inside one shard; a copy that crosses devices goes through the host (inputs, protection counters and --
        when the injection dynamics are on -- the dispatch / storage / curtailment state: the results of the destination lanes are
        those of their next solve)."""
        ps, pd = self._parts(src, n), self._parts(dst, n)
        if len(ps) == 1 and len(pd) == 1 and ps[0][0] is pd[0][0]:
            ps[0][0].copy_lanes(ps[0][1], pd[0][1], n)
            return
        topo, sb = self.get_topology(src, n)
        self.set_injections(self.get_injections(src, n), lane0=dst)
        self.set_topology(topo, sb, lane0=dst)
        _, ovc, _ = self.step_outputs(src, n)
        self.set_overflow_count(ovc, lane0=dst)
        self.set_cooldown(self.cooldown(src, n), lane0=dst)
        if all(getattr(e, "env_dynamics_on", False) for e in self.engines):
            self.set_env_state(dst, **self.env_state(src, n))

    # the same-device calls: the source lanes and the lanes they are copied to must be on one device
    def fanout_n1(self, src_lane: int, dst_lane0: int, out_lines):
        """N-1 fan-out of one source lane; source and destinations must live on the same device (the contingencies of an
        environment sit next to it: SURVEY.md 8(e))."""
        ol = np.asarray(out_lines, dtype=np.int32)
        (es, ls, _, _), = self._parts(src_lane, 1)
        pd = self._parts(dst_lane0, ol.size)
        if len(pd) != 1 or pd[0][0] is not es:
            raise ValueError("ShardedEngine.fanout_n1: the source lane and its contingency lanes must be on the same device")
        es.fanout_n1(ls, pd[0][1], ol)

    def simulate_candidates(self, src_lane: int, dst_lane0: int, actions=None, topologies=None, **kw):
        (es, ls, _, _), = self._parts(src_lane, 1)
        n = len(actions) if topologies is None else np.asarray(topologies).reshape(-1, self.model.dim_topo).shape[0]
        pd = self._parts(dst_lane0, n)
        if len(pd) != 1 or pd[0][0] is not es:
            raise ValueError("ShardedEngine.simulate_candidates: the source lane and its candidate lanes must be on the same device")
        return es.simulate_candidates(ls, pd[0][1], actions=actions, topologies=topologies, **kw)

    def simulate_batch(self, t_obs: int, src_lanes, actions, dst_lane0: int, **kw):
        """`PowerFlowEngine.simulate_batch`; the source lanes and their candidate lanes must live on ONE device."""
        src = np.asarray(src_lanes, dtype=np.int64).reshape(-1)
        owners = {id(self.owner(int(k))[0]) for k in src}
        pd = self._parts(dst_lane0, src.size * len(actions))
        if len(owners) != 1 or len(pd) != 1 or id(pd[0][0]) not in owners:
            raise ValueError("ShardedEngine.simulate_batch: the source lanes and their candidate lanes must be on the same device")
        eng = pd[0][0]
        b0 = self.blocks[self.engines.index(eng)][0]
        return eng.simulate_batch(t_obs, src - b0, actions, pd[0][1], **kw)

    def specialize(self, enable: bool = True, cache_dir=None, verify: bool = True, features: bool = True):
        """`PowerFlowEngine.specialize` on every device's engine (same grid: the self-test runs once, the code objects are shared
        through the on-disk cache); returns one `specialization()` dict per device.  ``features=False``: grid-only kernels."""
        out = []
        kw = {} if features else {"features": False}
        for k, eng in enumerate(self.engines):
            out.append(eng.specialize(enable, cache_dir=cache_dir, verify=verify and k == 0, **kw) if hasattr(eng, "specialize") else None)
        return out

    def specialization(self):
        return [eng.specialization() if hasattr(eng, "specialization") else None for eng in self.engines]

    def close(self):
        if getattr(self, "_pool", None) is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        for eng in self.engines:
            eng.close()
        self.engines = []


# ---- the routing rules: each takes the name of an engine method and returns the method that forwards it ------------------------------
def _cat(parts, axis=0):
    """What the shards returned, joined in global lane order by the type of the first part: arrays are concatenated, tuples, lists and
    dicts element by element, dataclasses (`LaneResults`, the state classes) field by field with the underscore fields of the first."""
    p = parts[0] if parts else None
    if p is None:
        return None
    if isinstance(p, np.ndarray):
        return np.concatenate(parts, axis)
    if isinstance(p, (tuple, list)):
        return type(p)(_cat([q[i] for q in parts], axis) for i in range(len(p)))
    if isinstance(p, dict):
        return {key: _cat([q[key] for q in parts], axis) for key in p}
    if is_dataclass(p):
        names = [f.name for f in fields(p)]
        return type(p)(**{f: getattr(p, f) if f.startswith("_") else _cat([getattr(q, f) for q in parts], axis) for f in names})
    return np.concatenate(parts, axis)


def every(name):
    def method(self, *args, **kw):
        for eng in self.engines:
            getattr(eng, name)(*args, **kw)
    return method


def first(name):
    def method(self, *args, **kw):
        return getattr(self.engines[0], name)(*args, **kw)
    return method


def per_device(name):
    def method(self, *args, **kw):
        return [getattr(eng, name)(*args, **kw) for eng in self.engines]
    return method


def cut(name, by_lane=None):
    """Whole-batch arguments: every positional or keyword argument that is not None and not a scalar is cut ``[b0:b0+bn]`` by device
    block.  ``by_lane(n_lanes, *args, **kw) -> (args, kw)`` first brings arguments that may come flat or shared to ``[n_lanes, ...]``."""
    def block(a, b0, bn):
        return a if a is None or np.ndim(a) == 0 else np.asarray(a)[b0:b0 + bn]

    def method(self, *args, **kw):
        if by_lane is not None:
            args, kw = by_lane(self.n_lanes, *args, **kw)
        for eng, (b0, bn) in zip(self.engines, self.blocks):
            getattr(eng, name)(*[block(a, b0, bn) for a in args], **{key: block(v, b0, bn) for key, v in kw.items()})
    return method


def _draws_by_lane(n_lanes, draws):
    return (np.asarray(draws).reshape(n_lanes, -1),), {}


def _schedule_by_lane(n_lanes, schedule, count):
    return (np.asarray(schedule).reshape(n_lanes, -1, 2), np.broadcast_to(np.asarray(count), (n_lanes,))), {}


def _area_schedule_by_lane(n_lanes, schedule, count):
    sch = np.asarray(schedule)
    if sch.ndim == 3:
        sch = np.broadcast_to(sch, (n_lanes,) + sch.shape)
    return (sch, np.broadcast_to(np.asarray(count), (n_lanes, sch.shape[1]))), {}


def _episode_limit_by_lane(n_lanes, max_steps, *args, **kw):
    if max_steps is not None and np.ndim(max_steps) > 0:
        max_steps = np.asarray(max_steps).reshape(n_lanes)
    return (max_steps,) + args, kw


def _ranged(core, steps):
    """The method ``([n_steps, step0=0,] lane0=0, n=None, *args, **kw)`` around ``core(self, head, lane0, n, args, kw)``."""
    if steps:
        return lambda self, n_steps, step0=0, lane0=0, n=None, *args, **kw: core(self, (n_steps, step0), lane0, n, args, kw)
    return lambda self, lane0=0, n=None, *args, **kw: core(self, (), lane0, n, args, kw)


def gather(name, steps=False, axis=0):
    """A getter of the global lane range ``(lane0, n)``, after ``(n_steps, step0)`` if ``steps``: what the shards of `_parts` return
    goes through `_cat` on ``axis``."""
    def core(self, head, lane0, n, args, kw):
        return _cat([getattr(eng, name)(*head, l0, k, *args, **kw) for eng, l0, k, _ in self._parts(lane0, n)], axis)
    return _ranged(core, steps)


def per_shard_tensor(name, keys, steps=False):
    """A getter of the global lane range that leaves one tensor per intersecting shard on its device and returns them as a list; every
    argument of ``keys`` (after the range, or by keyword) is None or a list with one tensor per such shard (the rows of its lanes)."""
    label = {"out": "output", "flags": "flag"}

    def core(self, head, lane0, n, args, kw):
        if args:
            if len(args) > len(keys) or any(key in kw for key in keys[:len(args)]):
                raise TypeError(f"ShardedEngine.{name}: after the lane range, {' and '.join(keys)} once each")
            kw.update(zip(keys, args))
        parts = self._parts(lane0, n)
        lists = {key: list(kw.pop(key)) for key in keys if kw.get(key) is not None}
        if not lists:
            return [getattr(eng, name)(*head, l0, k, **kw) for eng, l0, k, _ in parts]
        if any(len(given) != len(parts) for given in lists.values()):
            given = " / ".join(f"{len(lists.get(key, parts))} {label.get(key, key)}" for key in keys)
            raise ValueError(f"ShardedEngine.{name}: {len(parts)} shards intersect the range, {given} tensors given")
        return [getattr(eng, name)(*head, l0, k, **kw, **{key: given[i] for key, given in lists.items()}) for i, (eng, l0, k, _) in enumerate(parts)]
    return _ranged(core, steps)


def scatter(name, rows, width=None):
    """A setter ``(rows, lane0=0)`` of the rows that start at global lane ``lane0``; ``rows`` is the engine's name of that argument.  The
    rows are reshaped ``[-1, width]``, ``width`` being an attribute path from the sharded engine, or keep their last axis (None)."""
    key, get_width = rows, attrgetter(width) if width else None

    def method(self, rows=None, lane0=0, **kw):
        rows = np.asarray(kw.pop(key) if rows is None else rows)
        rows = rows.reshape(-1, get_width(self) if get_width else rows.shape[-1])
        for eng, l0, k, off in self._parts(lane0, rows.shape[0]):
            getattr(eng, name)(rows[off:off + k], lane0=l0, **kw)
    return method


def scatter_state(name):
    """A setter ``(state, lane0=0)`` of one of the state dataclasses: every engine gets the lanes' slice of each field."""
    def method(self, state, lane0=0, **kw):
        names = [f.name for f in fields(state)]
        for eng, l0, k, off in self._parts(lane0, len(getattr(state, names[0]))):
            getattr(eng, name)(type(state)(*(getattr(state, f)[off:off + k] for f in names)), lane0=l0, **kw)
    return method


# ---- the table: the rule of every forwarded method (name -> the rule's parameters) ------------------------------------------------
ROUTES = {
    # the same call on every device: tables, rules and switches (every device holds its own copy)
    every: dict.fromkeys((
        "sync", "set_deterministic", "set_thermal_limits", "upload_maintenance", "upload_outage_durations", "upload_hazards", "upload_forecasts",
        "set_gen_limits", "set_gen_renewable", "set_storage_params", "set_env_dynamics", "set_trajectory", "set_obs_clock", "set_obs_spec",
        "lane_actions_on_device", "topo_actions_on_device", "alerts_on_device",        # each device's act_* buffers hold its own lanes
        "set_topo_rules", "set_topo_areas", "set_topo_slots", "set_opponent_areas", "set_alerts", "set_rewards", "set_combined_actions",
        "set_graph_obs", "set_n1_screen", "set_lookahead", "lookahead",         # (the look-ahead: one device block each)
        "set_lookahead_chain", "lookahead_chain"), {}),
    # host-side helpers that depend on the grid alone
    first: dict.fromkeys(("pack_injections", "pack_chronics", "topo_action_areas", "alert_state_fields", "graph_layout"), {}),
    # one entry per device; the views are zero-copy torch tensors (global lane order = concatenation over the list)
    per_device: dict.fromkeys(("device_views", "reward_views", "episode_views", "cursor_views", "combined_views", "plan", "n1_views", "lookahead_views",
                                "lookahead_chain_views"), {}),
    # whole-batch per-lane arrays, cut by device block
    cut: {**dict.fromkeys(("set_lane_chronics", "set_lane_redispatch", "set_lane_actions", "set_lane_curtailment", "set_lane_topo_actions",
                           "set_lane_alerts"), {}),
          "upload_opponent_draws": dict(by_lane=_draws_by_lane), "upload_cursor_draws": dict(by_lane=_draws_by_lane),
          "upload_opponent_schedule": dict(by_lane=_schedule_by_lane), "upload_opponent_area_schedule": dict(by_lane=_area_schedule_by_lane),
          "set_episode_limit": dict(by_lane=_episode_limit_by_lane)},
    # getters of a lane range
    gather: {**dict.fromkeys((
        "reset", "get_injections", "get_topology", "step_outputs", "episode", "cooldown", "sub_cooldown", "last_bus", "env_state",
        "observation_vector_host", "topo_action_flags", "topo_action_mask_host", "opponent_state", "opponent_area_state",
        "opponent_attack_lines", "alert_state", "alert_reward", "rewards", "episode_ends", "episode_stats", "chronics_cursor_state", "action_flags",
        "graph_observation_host", "n1_values", "n1_summary", "lookahead_values", "lookahead_chain_values"), {}),
        "trajectory": dict(steps=True, axis=1), "trajectory_cooldown": dict(steps=True, axis=1), "trajectory_obs": dict(steps=True)},
    # getters that leave their result on the devices: one tensor per shard, each on its own device and stream
    per_shard_tensor: {"observation_vector": dict(keys=("out",)), "topo_action_mask": dict(keys=("out",)),
                       "rewards_eval": dict(keys=("flags", "out")), "observation_trajectory": dict(keys=("out",), steps=True),
                       "graph_observation": dict(keys=("out",))},     # (out: one (index, features, dense) tuple per shard)
    # setters of the rows that start at a lane
    scatter: {"set_injections": dict(rows="inj", width="n_inj"), "set_cooldown": dict(rows="line_cooldown", width="model.n_line"),
              "set_overflow_count": dict(rows="counts", width="model.n_line"), "set_sub_cooldown": dict(rows="sub_cooldown", width="model.n_sub"),
              "set_last_bus": dict(rows="last_bus", width="model.dim_topo"), "set_alert_state": dict(rows="rows")},
    scatter_state: dict.fromkeys(("set_opponent_state", "set_opponent_area_state", "set_chronics_cursor_state"), {}),
}

# engine methods that `ShardedEngine` does not forward (calling one raises AttributeError), and why
NOT_SHARDED = (
    ("solve_lane", "one lane at a time: use `owner(lane)`"),
    ("candidate_topologies", "host-side helper of `simulate_candidates`: any engine answers"),
    ("pack_actions", "host-side helper of `simulate_batch`: any engine answers"),
    ("ptdf_build", "one lane's table: `ptdf_build_batch` is the sharded form"),
    ("ptdf", "reads the table of `ptdf_build`"),
    ("ptdf_batch_info", "`ptdf_build_batch` returns the info with the shards' class offsets applied"),
    ("ptdf_flows", "not forwarded yet: a `gather` over each device's own tables"),
    ("ptdf_flows_rows", "not forwarded yet: its lane range comes after four other arguments"),
    ("lodf_screen", "not forwarded yet: a `gather` whose ``cap_mw`` goes to every device"),
    ("set_profiling", "timing is per device: use `engines[k]`"),
    ("kernel_time", "timing is per device: use `engines[k]`"),
    ("feature_word", "describes one engine's launch: use `engines[k]`"),
    ("specialization_header", "describes one engine's kernels: use `engines[k]`"),
    ("algorithmic_bytes_per_step", "a per-engine figure of the benchmark, which runs one engine per process"),
)

for _rule, _names in ROUTES.items():
    for _name, _params in _names.items():
        assert _name not in vars(ShardedEngine), _name
        _method = _rule(_name, **_params)
        _method.__name__, _method.__qualname__ = _name, f"ShardedEngine.{_name}"
        _method.__doc__ = f"`PowerFlowEngine.{_name}` on the lanes of every device, forwarded by the rule `{_rule.__name__}`."
        setattr(ShardedEngine, _name, _method)
