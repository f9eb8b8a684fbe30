"""`PowerFlowEngine`: the batched MI355X power-flow engine (Python over the C ABI, no grid2op needed).

One engine = one grid (`GridModel`) x ``n_lanes`` independent grid instances ("lanes": environment
copies or N-1 contingencies) resident in the HBM of one GPU.  All arithmetic happens in
``libgridpf.so`` (hand-written HIP for gfx950); this module only marshals numpy arrays.

The single-environment drop-in `grid2op_amd.backend.HipBackend` is a one-lane view on such an engine;
the batched stepping API (`upload_chronics` / `step`) is what ``bench.py`` measures.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from . import _capi
from ._capi import GpfAlertDesc, GpfCombinedDesc, GpfCursorDesc, GpfEpisodeDesc, GpfRewardSlot, GpfGridDesc, GpfLayout, GpfOpponentDesc, GpfStepOpts, GridPFError, check, ptr
from .grid_model import GridModel

__all__ = ["PowerFlowEngine", "LaneResults", "GridPFError", "ST_CONVERGED", "STATUS_TEXT", "MASK_TOO_MANY_LINES", "MASK_TOO_MANY_SUBS",
           "MASK_LINE_COOLDOWN", "MASK_SUB_COOLDOWN", "MASK_AMBIGUOUS"]

ST_CONVERGED = 0
STATUS_TEXT = {
    0: "converged",
    1: "Newton-Raphson did not converge within max_iter iterations",
    2: "islanded grid (an active bus is not connected to the slack bus)",
    3: "no in-service slack generator",
    4: "singular matrix",
    5: "engine capacity exceeded",
    6: "infeasible redispatching (ImpossibleRedispatching: game over)",
    -1: "power flow not run",
}
# reason bits of `PowerFlowEngine.topo_action_mask` (include/gridpf.h GPF_MASK_*); 0: the entry would be applied
MASK_TOO_MANY_LINES, MASK_TOO_MANY_SUBS, MASK_LINE_COOLDOWN, MASK_SUB_COOLDOWN, MASK_AMBIGUOUS = 0x01, 0x02, 0x04, 0x08, 0x10

# the opponent of `PowerFlowEngine.set_opponent` (include/gridpf.h GPF_OPP_*)
OPP_NONE, OPP_RANDOM_LINE, OPP_WEIGHTED_RANDOM, OPP_GEOMETRIC = 0, 1, 2, 3
OPP_DRAWS_TABLE, OPP_DRAWS_PHILOX = 0, 1
OPP_STATE_INTS = 14
OPP_TIME_NONE = -2 ** 31
OPP_FLAG_DRAWS_EXHAUSTED, OPP_FLAG_SCHEDULE_CAPPED = 1, 2
OPP_MAX_AREAS, OPP_AREA_STATE_INTS = 16, 8
# the chronics cursor of `PowerFlowEngine.set_chronics_cursor` (include/gridpf.h GPF_CURSOR_*)
CURSOR_SEQUENTIAL, CURSOR_SAMPLED = 0, 1
CURSOR_FLAG_DRAWS_EXHAUSTED, CURSOR_FLAG_NEXT_POS_WRAPPED = 1, 2
CURSOR_STATE_INTS = 7
ALERT_MAX_LINES, ALERT_MAX_WINDOW = 64, 62
ALERT_OBS_SECTIONS = ("active_alert", "time_since_last_alert", "alert_duration", "time_since_last_attack", "attack_under_alert",
                      "was_alert_used_after_attack")      # sections of A of the lane's alert block; total_number_of_alert is its element 6 A
OPP_KIND_OF_CLASS = {"RandomLineOpponent": OPP_RANDOM_LINE, "WeightedRandomOpponent": OPP_WEIGHTED_RANDOM, "GeometricOpponent": OPP_GEOMETRIC}


@dataclass
class OpponentState:
    """Per-lane state of the opponent (`PowerFlowEngine.opponent_state`): the five values of ``OpponentSpace._get_state`` (the budget as
    float64 with the flag that it is still a numpy.float32), the opponent's own counters, and the two ``info`` values of the last launch.
    ``next_attack_time`` is `OPP_TIME_NONE` for None."""
    budget: np.ndarray
    budget_is_f32: np.ndarray
    attack_duration: np.ndarray
    attack_cooldown: np.ndarray
    attack_line: np.ndarray
    previous_fails: np.ndarray
    next_attack_time: np.ndarray
    attack_counter: np.ndarray
    n_schedule: np.ndarray
    cursor: np.ndarray
    episode: np.ndarray
    flags: np.ndarray
    opponent_attack_line: np.ndarray
    opponent_attack_duration: np.ndarray

    _COLS = ("budget_is_f32", "attack_duration", "attack_cooldown", "attack_line", "previous_fails", "next_attack_time", "attack_counter",
             "n_schedule", "cursor", "episode", "flags", "opponent_attack_line", "opponent_attack_duration")

    @classmethod
    def from_rows(cls, budget, rows):
        return cls(budget, *(rows[:, k].copy() for k in range(len(cls._COLS))))

    def rows(self) -> np.ndarray:
        out = np.zeros((len(self.budget), OPP_STATE_INTS), dtype=np.int32)
        for k, name in enumerate(self._COLS):
            out[:, k] = getattr(self, name)
        return out


@dataclass
class CursorState:
    """Per-lane state of the chronics cursor (`PowerFlowEngine.chronics_cursor_state`): the chronics table and offset the lane reads
    (``lane_table`` / ``lane_offset``), the position in the order of the episode under way (-1: none yet), the position the next episode
    takes (-1: none given), the episodes started, the draws consumed and the sticky `CURSOR_FLAG_DRAWS_EXHAUSTED` /
    `CURSOR_FLAG_NEXT_POS_WRAPPED` bits."""
    table: np.ndarray
    offset: np.ndarray
    pos: np.ndarray
    next_pos: np.ndarray
    n_started: np.ndarray
    draws_used: np.ndarray
    flags: np.ndarray

    _COLS = ("table", "offset", "pos", "next_pos", "n_started", "draws_used", "flags")

    @classmethod
    def from_rows(cls, rows):
        return cls(*(rows[:, k].copy() for k in range(len(cls._COLS))))

    def rows(self) -> np.ndarray:
        out = np.zeros((len(self.table), CURSOR_STATE_INTS), dtype=np.int32)
        for k, name in enumerate(self._COLS):
            out[:, k] = getattr(self, name)
        return out


def cursor_cdf(probabilities) -> np.ndarray:
    """The cumulative distribution ``Multifolder.sample_next_chronics`` and ``RandomState.choice`` search (Chronics/multiFolder.py:345-356):
    the probabilities as float32 over their float32 sum, then a float64 cumulative sum over its last entry."""
    p = np.array(probabilities, dtype=np.float32)
    tot = p.sum()
    if p.ndim != 1 or p.size == 0 or (p < 0).any() or not np.isfinite(tot) or abs(tot) <= 1e-5:
        raise ValueError("probabilities: a non-empty vector of non-negative numbers that does not sum to 0")
    p /= tot
    cdf = p.astype(np.float64).cumsum()
    cdf /= cdf[-1]
    return cdf


@dataclass
class OpponentAreaState:
    """Per-(lane, area) state of the multi-area opponent (`PowerFlowEngine.opponent_area_state`), every field ``[n, n_area]``: the area's
    ``_new_attack_time_counters`` entry (-1: free), its ``_previous_attacks`` line (-1: None), its sub-opponent's ``_next_attack_time``
    (`OPP_TIME_NONE` for None), ``_attack_counter`` and ``_number_of_attacks``, and the area's line in the accepted attack of the last
    launch (-1: none)."""
    counter: np.ndarray
    line: np.ndarray
    next_attack_time: np.ndarray
    attack_counter: np.ndarray
    n_schedule: np.ndarray
    opponent_attack_line: np.ndarray

    _COLS = ("counter", "line", "next_attack_time", "attack_counter", "n_schedule", "opponent_attack_line")

    @classmethod
    def from_rows(cls, rows):
        return cls(*(rows[:, :, k].copy() for k in range(len(cls._COLS))))

    def rows(self) -> np.ndarray:
        out = np.zeros(np.shape(self.counter) + (OPP_AREA_STATE_INTS,), dtype=np.int32)
        for k, name in enumerate(self._COLS):
            out[:, :, k] = getattr(self, name)
        return out


def opponent_config(model, opponent_class, kwargs_opponent=None, opponent_init_budget=0.0, opponent_budget_per_ts=0.0,
                    opponent_attack_duration=0, opponent_attack_cooldown=99999, delta_time_seconds=300.0, max_episode_duration=None,
                    draw_source=OPP_DRAWS_PHILOX, seed=0, lane_base=0, schedule_cap=None) -> dict:
    """The keyword arguments of `PowerFlowEngine.set_opponent` from a reference-style configuration: the ``opponent_class`` (the class or
    its name), ``kwargs_opponent`` and the four ``opponent_*`` numbers of ``grid2op.make``; line names are resolved through the model's
    ``name_line`` (BaseOpponent._set_line_id, Opponent/baseOpponent.py:139-161), the Geometric rates are derived as
    GeometricOpponent.init does (Opponent/geometricOpponent.py:111-135) and its errors are raised with its reasons."""
    name = opponent_class if isinstance(opponent_class, str) else getattr(opponent_class, "__name__", str(opponent_class))
    if name not in OPP_KIND_OF_CLASS:
        raise ValueError(f"opponent_config: {name} is not one of {sorted(OPP_KIND_OF_CLASS)} (the single-area line opponents; "
                         "GeometricOpponentMultiArea: opponent_area_config)")
    kw = dict(kwargs_opponent or {})
    names = [str(x) for x in np.asarray(model.name_line)]
    lines = []
    for l_name in kw.get("lines_attacked", ()):
        if str(l_name) not in names:
            raise ValueError(f'opponent_config: unable to find the powerline named "{l_name}" on the grid')
        lines.append(names.index(str(l_name)))
    out = dict(kind=OPP_KIND_OF_CLASS[name], lines=lines, init_budget=opponent_init_budget, budget_per_ts=opponent_budget_per_ts,
               attack_duration=int(opponent_attack_duration), attack_cooldown=int(opponent_attack_cooldown), draw_source=draw_source,
               seed=seed, lane_base=lane_base)
    if name == "WeightedRandomOpponent":
        norm = list(kw.get("rho_normalization", ()))
        if norm and len(norm) != len(lines):
            raise ValueError("opponent_config: the usage rate normalization must have the same length as the number of attacked lines")
        out.update(rho_normalization=norm or None, attack_period=int(kw.get("attack_period", 12 * 24)))
    if name == "GeometricOpponent":
        every, avg = kw.get("attack_every_xxx_hour", 24), kw.get("average_attack_duration_hour", 4)
        mini = kw.get("minimum_attack_duration_hour", 2)
        ts_per_hour = 3600.0 / float(delta_time_seconds)
        if avg < mini:
            raise ValueError("opponent_config: the average duration of an attack cannot be lower than the minimum time of an attack")
        if avg == mini:
            raise ValueError("opponent_config: average_attack_duration_hour == minimum_attack_duration_hour is not supported")
        if every <= avg:
            raise ValueError("opponent_config: attack_every_xxx_hour <= average_attack_duration_hour is not supported")
        if max_episode_duration is None or not np.isfinite(max_episode_duration):
            raise ValueError("opponent_config: the Geometric opponent only works with a known finite episode duration (max_episode_duration)")
        hazard = 1.0 / (ts_per_hour * (every - avg))
        if schedule_cap is None:            # expected attacks of an episode with a wide margin (the schedule ends where the capacity does)
            schedule_cap = int(min(max(16, 4 * int(max_episode_duration) * hazard + 16), int(max_episode_duration)))
        out.update(attack_hazard_rate=hazard, recovery_rate=1.0 / (ts_per_hour * (avg - mini)),
                   recovery_minimum_duration=int(mini * ts_per_hour), pmax_pmin_ratio=float(kw.get("pmax_pmin_ratio", 4)),
                   episode_max_time=int(max_episode_duration), schedule_cap=int(schedule_cap))
    return out


# the sections of the bus-graph index row, in the order of include/gridpf.h GPF_GRAPH_* (PowerFlowEngine.graph_layout)
GRAPH_SECTIONS = ("n_bus", "load_bus", "gen_bus", "storage_bus", "line_or_bus", "line_ex_bus", "shunt_bus", "bus_global")
GRAPH_N_BUS, GRAPH_LOAD_BUS, GRAPH_GEN_BUS, GRAPH_STORAGE_BUS, GRAPH_LINE_OR_BUS, GRAPH_LINE_EX_BUS, GRAPH_SHUNT_BUS, GRAPH_BUS_GLOBAL = range(8)

RW_REDISP, RW_L2RPN, RW_LINES_CAPACITY, RW_ECONOMIC, RW_GAMEPLAY = 1, 2, 3, 4, 5      # include/gridpf.h GPF_RW_*
LA_ILLEGAL, LA_AMBIGUOUS, LA_DONE = 1, 2, 4      # include/gridpf.h GPF_LA_*: the flag bits of `PowerFlowEngine.lookahead`
RW_N1 = 7                            # include/gridpf.h GPF_RW_N1: p[0] = index into the watched lines of `PowerFlowEngine.set_n1_screen`
REWARD_MAX_SLOTS = 8
REWARD_KINDS = {"RedispReward": RW_REDISP, "L2RPNReward": RW_L2RPN, "LinesCapacityReward": RW_LINES_CAPACITY, "EconomicReward": RW_ECONOMIC,
                "GameplayReward": RW_GAMEPLAY}


def reward_config(kind, gen_cost_per_MW=None, gen_pmax=None, delta_time_seconds=300.0, **meta) -> dict:
    """One slot of `PowerFlowEngine.set_rewards` from a reference-style configuration: ``kind`` is a ``RW_*`` constant or the reference
    class's name (``"RedispReward"`` ...); ``meta`` are the class's meta-parameters with the reference's defaults.  ``max_regret`` of
    ``RedispReward`` and ``worst_cost`` of ``EconomicReward`` are derived as the two ``initialize`` methods derive them
    (Reward/redispReward.py:141-167, Reward/economicReward.py:49-55), float32 where the reference uses ``dt_float``.  Returns
    ``dict(kind=..., p=[...])`` plus the derived values by name (``reward_max`` of ``RedispReward`` among them)."""
    f32 = np.float32
    k = REWARD_KINDS.get(kind, kind) if isinstance(kind, str) else int(kind)
    dts = float(delta_time_seconds) / 3600.0

    def take(name, default):
        return meta.pop(name, default)
    out = dict(kind=k)
    if k == RW_REDISP:
        if gen_cost_per_MW is None or gen_pmax is None:
            raise ValueError("reward_config: RedispReward needs gen_cost_per_MW and gen_pmax")
        cost, pmax = np.asarray(gen_cost_per_MW, f32), np.asarray(gen_pmax, f32)
        alpha, min_load_ratio = f32(take("alpha_redisph", 5.0)), f32(take("min_load_ratio", 0.1))
        worst_losses_ratio, min_reward = f32(take("worst_losses_ratio", 0.05)), f32(take("min_reward", -10.0))
        least_losses_ratio, ria = f32(take("least_losses_ratio", 0.015)), f32(take("reward_illegal_ambiguous", 0.0))
        worst_marginal_cost = np.max(cost)
        worst_load = pmax.sum(dtype=f32)
        worst_losses = f32(worst_losses_ratio) * worst_load
        worst_redisp = alpha * pmax.sum()
        max_regret = (worst_losses + worst_redisp) * worst_marginal_cost * float(delta_time_seconds) / 3600.0
        least_loads = f32(worst_load * min_load_ratio)
        least_losses = f32(least_losses_ratio * least_loads * float(delta_time_seconds) / 3600.0)
        base_marginal_cost = np.min(cost[cost > 0.0])
        min_regret = (least_losses + f32(0.0)) * base_marginal_cost
        reward_max = f32((max_regret - min_regret) / least_loads)
        out.update(p=[float(alpha), float(max_regret), float(min_reward), float(ria), dts], max_regret=float(max_regret),
                   reward_min=float(min_reward), reward_max=float(reward_max))
    elif k == RW_ECONOMIC:
        if gen_cost_per_MW is None or gen_pmax is None:
            raise ValueError("reward_config: EconomicReward needs gen_cost_per_MW and gen_pmax")
        cost, pmax = np.asarray(gen_cost_per_MW, f32), np.asarray(gen_pmax, f32)
        worst_cost = f32((cost * pmax).sum() * float(delta_time_seconds) / 3600.0)
        rmin, rmax = f32(take("reward_min", 0.0)), f32(take("reward_max", 1.0))
        out.update(p=[float(worst_cost), float(rmin), float(rmax), dts], worst_cost=float(worst_cost), reward_min=float(rmin), reward_max=float(rmax))
    elif k == RW_GAMEPLAY:
        rmin, rmax = f32(take("reward_min", -1.0)), f32(take("reward_max", 1.0))
        out.update(p=[float(rmin), float(rmax)], reward_min=float(rmin), reward_max=float(rmax))
    elif k in (RW_L2RPN, RW_LINES_CAPACITY):
        out.update(p=[])
    else:
        raise ValueError(f"reward_config: unknown reward kind {kind!r}")
    if meta:
        raise ValueError(f"reward_config: unknown meta-parameters {sorted(meta)}")
    return out


def alert_end_bonus(alert_reward=None) -> float:
    """``reward_end_episode_bonus`` of an ``AlertReward`` instance (anything with that attribute), or the class's default 1.0
    (Reward/alertReward.py:75-91): the ``alert_end_bonus`` of `PowerFlowEngine.set_episode_limit`."""
    if alert_reward is None:
        return 1.0
    return float(alert_reward.reward_end_episode_bonus)


def alert_config(parameters=None, reward_min_no_blackout=-1.0, reward_min_blackout=-10.0, reward_max_no_blackout=1.0, reward_max_blackout=2.0) -> dict:
    """Keyword arguments of `PowerFlowEngine.set_alerts` from a reference-style configuration: ``parameters`` is a ``grid2op.Parameters``
    (or anything with ``ALERT_TIME_WINDOW``, or a dict, or None for the default 12); the four constants are ``AlertReward``'s
    (Reward/alertReward.py:75-91).  ``reward_end_episode_bonus`` belongs to the episode limit: `alert_end_bonus` returns it for
    `PowerFlowEngine.set_episode_limit`."""
    if parameters is None:
        w = 12
    elif isinstance(parameters, dict):
        w = parameters.get("ALERT_TIME_WINDOW", 12)
    else:
        w = getattr(parameters, "ALERT_TIME_WINDOW", 12)
    w = int(w)
    if not 1 <= w <= ALERT_MAX_WINDOW:
        raise ValueError(f"alert_config: ALERT_TIME_WINDOW {w} is outside [1, {ALERT_MAX_WINDOW}] (AlertReward needs a window > 0; the rings hold 64 rows)")
    return dict(time_window=w, reward_min_no_blackout=float(reward_min_no_blackout), reward_min_blackout=float(reward_min_blackout),
                reward_max_no_blackout=float(reward_max_no_blackout), reward_max_blackout=float(reward_max_blackout))


def opponent_area_config(model, kwargs_opponent=None, opponent_init_budget=0.0, opponent_budget_per_ts=0.0, opponent_attack_duration=0,
                         opponent_attack_cooldown=99999, **kw):
    """A reference-style configuration of ``GeometricOpponentMultiArea`` (``lines_attacked``: a list of lists, one per area) as
    ``(set_opponent keywords, area_of_line)``: the lines of all areas in area order with the rates `opponent_config` derives for a
    GeometricOpponent, and the area of each of them for `PowerFlowEngine.set_opponent_areas`.  ``lines_attacked`` None is the reference's
    warning case (Opponent/geometricOpponentMultiArea.py:69-71): the opponent is deactivated, ``(dict(kind=OPP_NONE), None)``.  Further
    keywords are those of `opponent_config`."""
    kwo = dict(kwargs_opponent or {})
    areas = kwo.get("lines_attacked")
    if areas is None:
        import warnings
        warnings.warn("opponent_area_config: GeometricOpponentMultiArea: no area provided, the opponent will be deactivated.")
        return dict(kind=OPP_NONE), None
    areas = [list(a) for a in areas]
    if any(isinstance(a, str) for a in kwo["lines_attacked"]):
        raise ValueError("opponent_area_config: lines_attacked must be a list of lists of line names, one list per area")
    kwo["lines_attacked"] = [l for a in areas for l in a]
    out = opponent_config(model, "GeometricOpponent", kwo, opponent_init_budget, opponent_budget_per_ts, opponent_attack_duration,
                          opponent_attack_cooldown, **kw)
    return out, [a for a, names in enumerate(areas) for _ in names]


_OUT_FIELDS = [
    ("p_or", "n_line"), ("q_or", "n_line"), ("v_or", "n_line"), ("a_or", "n_line"), ("theta_or", "n_line"),
    ("p_ex", "n_line"), ("q_ex", "n_line"), ("v_ex", "n_line"), ("a_ex", "n_line"), ("theta_ex", "n_line"),
    ("gen_p", "n_gen"), ("gen_q", "n_gen"), ("gen_v", "n_gen"), ("gen_theta", "n_gen"),
    ("load_p", "n_load"), ("load_q", "n_load"), ("load_v", "n_load"), ("load_theta", "n_load"),
    ("storage_p", "n_storage"), ("storage_q", "n_storage"), ("storage_v", "n_storage"), ("storage_theta", "n_storage"),
    ("shunt_p", "n_shunt"), ("shunt_q", "n_shunt"), ("shunt_v", "n_shunt"),
]
_INJ_FIELDS = [("gen_p", "n_gen"), ("gen_vm", "n_gen"), ("load_p", "n_load"), ("load_q", "n_load"),
               ("storage_p", "n_storage"), ("storage_q", "n_storage"), ("shunt_p", "n_shunt"), ("shunt_q", "n_shunt")]


@dataclass
class LaneResults:
    """Results of ``n`` lanes; every float field is a float32 ``[n, n_el]`` view of one ``out`` block."""
    out: np.ndarray
    topo_vect: np.ndarray
    shunt_bus: np.ndarray
    line_status: np.ndarray
    status: np.ndarray           # [n, 4] {status, n_iter, n_active_bus, n_cascade_rounds}
    bus_vm: np.ndarray           # float64 [n, nb_total] (pu), NaN for inactive buses
    bus_va: np.ndarray           # float64 [n, nb_total] (deg)
    _slices: Dict[str, slice]

    def __getattr__(self, name):
        sl = self.__dict__.get("_slices", {}).get(name)
        if sl is None:
            raise AttributeError(name)
        return self.out[:, sl]

    @property
    def converged(self) -> np.ndarray:
        return self.status[:, 0] == ST_CONVERGED

    @property
    def n_iter(self) -> np.ndarray:
        return self.status[:, 1]


def _ptr(a: Optional[np.ndarray]):
    """`ptr` with the ctypes element type of the array's own dtype."""
    return None if a is None else ptr(a, np.ctypeslib.as_ctypes_type(a.dtype))


def _fill_pointers(desc, arrays: dict):
    """Point the pointer fields of a ctypes descriptor at the arrays of ``{field: array or None}``, each as the field's own pointer type
    (an array of another element type is an error).  The CALLER keeps ``arrays`` referenced until the C call that reads ``desc`` returned."""
    types = dict(desc._fields_)
    for field, a in arrays.items():
        if a is not None:
            assert a.flags.c_contiguous and a.dtype == np.dtype(types[field]._type_), field
            setattr(desc, field, a.ctypes.data_as(types[field]))


class PowerFlowEngine:
    def __init__(self, model: GridModel, n_lanes: int = 1, device: int = 0, n_busbar: int = 2, deterministic: bool = False):
        self.model = model
        self.n_busbar = int(n_busbar)
        self._lib = _capi.lib()
        self._h = C.c_void_p()
        # Feature state: every private attribute the methods below read is declared HERE, with the setter that owns it.  The three cached
        # views alias engine-owned device buffers; the setter named drops the view because the library re-allocates the buffer there.
        self._has_maint = self._has_hazard = self._has_outages = False      # upload_maintenance / upload_hazards
        self._n_topo_act = 0                 # upload_topo_actions: entries of the action table
        self._n_topo_slot = 1                # set_topo_slots
        self._mask_view = None               # topo_action_mask's cache of device_views()["topo_mask"]; dropped by upload_topo_actions
        self._opp_n_lines = self._opp_cap = 0     # set_opponent: attackable lines, schedule capacity (Geometric)
        self._opp_n_area = 0                 # set_opponent_areas (set_opponent: back to 0)
        self._alert = None                   # set_alerts: (A, W) while alerts are on; set_opponent / set_opponent_areas turn them off
        self._traj_cap = 0                   # set_trajectory
        self._n_reward_slot = 0              # set_rewards
        self._n1 = None                      # set_n1_screen: (n_env, K)
        self._la = None                      # set_lookahead: (n_env, K)
        self._lc = None                      # set_lookahead_chain: max_steps
        self._rw_view = None                 # rewards_eval's cache of reward_views()["rewards"]; dropped by set_rewards
        self._ep_on = self._cb_on = self._cur_on = False      # set_episode_limit / set_combined_actions / set_chronics_cursor
        self._obs_spec = None                # set_obs_spec
        self._obs_view = None                # observation_vector's cache of device_views()["obs"]; dropped by set_obs_spec
        self._graph_on = False               # set_graph_obs
        m = model
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        br_y = np.empty((m.n_line, 8), dtype=np.float64)
        for k, y in enumerate((m.br_yff, m.br_yft, m.br_ytf, m.br_ytt)):
            br_y[:, 2 * k] = y.real
            br_y[:, 2 * k + 1] = y.imag
        init_inj = np.concatenate([f64(m.gen_p0), f64(m.gen_vm0), f64(m.load_p0), f64(m.load_q0), f64(m.storage_p0),
                                   f64(m.storage_q0), f64(m.shunt_p0), f64(m.shunt_q0)])
        d = GpfGridDesc(n_sub=m.n_sub, n_busbar=self.n_busbar, n_line=m.n_line, n_gen=m.n_gen, n_load=m.n_load, n_storage=m.n_storage,
                        n_shunt=m.n_shunt, dim_topo=m.dim_topo, sn_mva=m.sn_mva)
        arrays = dict(                       # descriptor field -> array; referenced until gpf_create (which copies them) has returned
            sub_vn_kv=f64(m.sub_vn_kv), line_or_sub=i32(m.line_or_sub), line_ex_sub=i32(m.line_ex_sub),
            line_or_pos_topo_vect=i32(m.line_or_pos_topo_vect), line_ex_pos_topo_vect=i32(m.line_ex_pos_topo_vect), br_y=br_y,
            br_bdc=f64(m.br_bdc), gen_sub=i32(m.gen_sub), gen_pos_topo_vect=i32(m.gen_pos_topo_vect), gen_min_q=f64(m.gen_min_q),
            gen_max_q=f64(m.gen_max_q), gen_slack=np.ascontiguousarray(m.gen_slack, dtype=np.uint8),
            load_sub=i32(m.load_sub), load_pos_topo_vect=i32(m.load_pos_topo_vect), storage_sub=i32(m.storage_sub),
            storage_pos_topo_vect=i32(m.storage_pos_topo_vect), shunt_sub=i32(m.shunt_sub), shunt_fact=f64(m.shunt_fact),
            init_inj=init_inj, init_topo=i32(m.initial_topo_vect()), init_shunt_bus=i32(m.initial_shunt_bus()))
        _fill_pointers(d, arrays)
        check(self._lib.gpf_create(C.byref(d), int(n_lanes), int(device), C.byref(self._h)), "gpf_create")
        self._pid = os.getpid()          # HIP handles belong to the creating process (a forked child must not destroy them)
        if deterministic:
            self.set_deterministic(True)
        self.n_lanes = int(n_lanes)
        self.device = int(device)
        lay = GpfLayout()
        self._call("gpf_get_layout", C.byref(lay))
        self.layout = lay
        self.n_inj, self.n_out, self.n_chron, self.nb_total = lay.n_inj, lay.n_out, lay.n_chron, lay.nb_total
        sizes = dict(n_line=m.n_line, n_gen=m.n_gen, n_load=m.n_load, n_storage=m.n_storage, n_shunt=m.n_shunt)
        self.out_slices = {}
        for name, sz in _OUT_FIELDS:
            key = "out_" + name
            off = getattr(lay, key)
            self.out_slices[name] = slice(off, off + sizes[sz])
        self.inj_slices = {}
        for name, sz in _INJ_FIELDS:
            off = getattr(lay, "inj_" + name)
            self.inj_slices[name] = slice(off, off + sizes[sz])
        self.init_inj = init_inj.copy()
        self.env_dynamics_on = False

    # ------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if getattr(self, "_pid", None) == os.getpid():
                self._lib.gpf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_deterministic(self, flag: bool = True):
        """Results are bit-identical from run to run on every grid by default; ``True`` additionally forces one wavefront per lane
        on grids with >= 64 substations (cross-check variant, ~20 % slower there)."""
        self._call("gpf_set_deterministic", int(bool(flag)))

    # ---- the plumbing every method below shares ------------------------------------------------------
    def _call(self, name, *args):
        """``name(handle, *args)`` of the library; `GridPFError` with the library's message when it fails."""
        check(getattr(self._lib, name)(self._h, *args), name)

    def _range(self, lane0, n):
        if n is None:
            n = self.n_lanes - lane0
        return int(lane0), int(n)

    def _get_rows(self, name, lane0, n, *specs, zeros=False):
        """A row getter ``name(handle, lane0, n, out...)``: one ``[n, cols]`` array (``cols`` None: ``[n]``) per ``(cols, dtype)`` of
        ``specs``, uninitialised or (``zeros``) zeroed before the call.  Returns the array, or the list of them."""
        lane0, n = self._range(lane0, n)
        outs = [(np.zeros if zeros else np.empty)(n if cols is None else (n, cols), dtype=dtype) for cols, dtype in specs]
        self._call(name, lane0, n, *[_ptr(a) for a in outs])
        return outs[0] if len(outs) == 1 else outs

    def _set_rows(self, name, rows, cols, dtype, lane0):
        """A row setter ``name(handle, lane0, n, rows)``: ``rows`` as contiguous ``[n, cols]`` of ``dtype``."""
        rows = np.ascontiguousarray(rows, dtype=dtype).reshape(-1, cols)
        self._call(name, int(lane0), rows.shape[0], _ptr(rows))

    def _device_pointers(self, name, count):
        """The pointer array of a ``gpf_*_device_pointers(handle, out, count)`` call."""
        ptrs = (C.c_void_p * count)()
        self._call(name, ptrs, count)
        return ptrs

    def _view(self, p, shape, typestr, steps=None):
        """The engine-owned buffer at device pointer ``p`` as a torch tensor that ALIASES it (no copy): ``shape`` is a lane's, the buffer
        holds one per lane of the engine's capacity (``steps``: per step and lane, as the trajectory buffers do) and the view is cut to
        ``n_lanes``.  None for an absent buffer (null pointer) or an empty one."""
        import torch
        if not p or 0 in shape:
            return None
        full = (self._lib.gpf_lane_capacity(self._h),) + tuple(shape)
        iface = {"shape": full if steps is None else (steps,) + full, "typestr": typestr, "data": (int(p), False), "version": 2, "strides": None}
        holder = type("_Arr", (), {"__cuda_array_interface__": iface})()      # v2: torch.as_tensor wraps it without a copy
        t = torch.as_tensor(holder, device=torch.device("cuda", self.device))
        return t[:self.n_lanes] if steps is None else t[:, :self.n_lanes]

    def _views(self, ptrs, table):
        """``{key: view}`` of a table of (key, pointer index, lane shape, typestr) over the pointer array ``ptrs``."""
        return {key: self._view(ptrs[idx], shape, typestr) for key, idx, shape, typestr in table}

    def _out_rows(self, what, out, dtype, n, width, narrow_to_library):
        """Pointer and row stride of a caller's ``out=`` tensor: 2-d CUDA of ``dtype`` ("uint8" / "float32") on this device, ``n`` rows,
        unit column stride; ValueError otherwise.  Rows narrower than ``width`` (or, with several rows, a row stride below it) are the one
        point the callers differ on: ``narrow_to_library`` passes the rows' width down as the stride, which the library refuses with its
        own message; without it they are refused here."""
        import torch
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == getattr(torch, dtype) and out.dim() == 2):
            raise ValueError(f"{what}: out must be a 2-d {dtype} CUDA tensor")
        ok = out.device.index == self.device and out.shape[0] == n and out.stride(1) == 1
        if narrow_to_library:
            if not ok:
                raise ValueError(f"{what}: out must live on cuda:{self.device} and have {n} rows with unit column stride")
            stride = int(out.stride(0)) if n > 1 and out.shape[1] >= width else int(out.shape[1])
        else:
            if not ok or out.shape[1] < width or (n > 1 and out.stride(0) < width):
                raise ValueError(f"{what}: out must live on cuda:{self.device}, have {n} rows of >= {width} contiguous columns and a row stride >= {width}")
            stride = int(out.stride(0)) if n > 1 else max(int(out.stride(0)), width)
        return C.cast(out.data_ptr(), C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), stride

    # ---- state --------------------------------------------------------------------------------------
    def pack_injections(self, n: int = 1, **fields) -> np.ndarray:
        """``[n, n_inj]`` float64 rows starting from the pristine injections; override by field name."""
        inj = np.tile(self.init_inj, (n, 1))
        for k, v in fields.items():
            inj[:, self.inj_slices[k]] = v
        return inj

    def set_injections(self, inj: np.ndarray, lane0: int = 0):
        self._set_rows("gpf_set_injections", inj, self.n_inj, np.float64, lane0)

    def get_injections(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        return self._get_rows("gpf_get_injections", lane0, n, (self.n_inj, np.float64))

    def set_topology(self, topo: np.ndarray, shunt_bus: Optional[np.ndarray] = None, lane0: int = 0):
        topo = np.ascontiguousarray(topo, dtype=np.int32).reshape(-1, self.model.dim_topo)
        sb = None
        if shunt_bus is not None and self.model.n_shunt:
            sb = np.ascontiguousarray(shunt_bus, dtype=np.int32).reshape(-1, self.model.n_shunt)
            assert sb.shape[0] == topo.shape[0]
        self._call("gpf_set_topology", lane0, topo.shape[0], _ptr(topo), _ptr(sb))

    def get_topology(self, lane0: int = 0, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        topo, sb = self._get_rows("gpf_get_topology", lane0, n, (self.model.dim_topo, np.int32), (self.model.n_shunt, np.int32))
        return topo, sb

    def disconnect_line(self, lane: int, line_id: int):
        self._call("gpf_disconnect_line", lane, line_id)

    def reset(self, lane0: int = 0, n: Optional[int] = None):
        lane0, n = self._range(lane0, n)
        self._call("gpf_reset_lanes", lane0, n)

    def copy_lanes(self, src: int, dst: int, n: int = 1):
        self._call("gpf_copy_lanes", src, dst, n)

    def fanout_n1(self, src_lane: int, dst_lane0: int, out_lines):
        ol = np.ascontiguousarray(out_lines, dtype=np.int32)
        self._call("gpf_fanout_n1", src_lane, dst_lane0, ol.size, _ptr(ol))

    def candidate_topologies(self, base_topo, actions, last_bus=None) -> np.ndarray:
        """``[len(actions), dim_topo]`` topology rows = ``base_topo`` modified by each candidate action, described as grid2op
        describes them (Action/baseAction.py ``set_bus`` / ``set_line_status`` / ``change_bus``): a dict with any of
        ``"set_bus": {topo_vect position: bus}``, ``"lines_or_bus" / "lines_ex_bus" / "loads_bus" / "gens_bus" / "storages_bus":
        [(element id, bus)]``, ``"set_line_status": [(line id, +1 | -1)]``, ``"change_bus": [positions]`` (1 <-> 2; refused with
        more than 2 busbars per substation, as grid2op refuses it).  A reconnection without an explicit bus puts each end back on
        its LAST KNOWN busbar (``last_bus``: the ``[dim_topo]`` row _BackendAction keeps in ``last_topo_registered``,
        Action/_backendAction.py; busbar 1 where it is unknown or not given).  An empty dict is the do-nothing candidate."""
        m = self.model
        base = np.asarray(base_topo, dtype=np.int32).reshape(m.dim_topo)
        last = None if last_bus is None else np.asarray(last_bus, dtype=np.int32).reshape(m.dim_topo)
        pos_of = {"lines_or_bus": m.line_or_pos_topo_vect, "lines_ex_bus": m.line_ex_pos_topo_vect, "loads_bus": m.load_pos_topo_vect,
                  "gens_bus": m.gen_pos_topo_vect, "storages_bus": m.storage_pos_topo_vect}
        out = np.tile(base, (len(actions), 1))
        for k, act in enumerate(actions):
            row = out[k]
            for line, st in act.get("set_line_status", ()):
                po, pe = m.line_or_pos_topo_vect[line], m.line_ex_pos_topo_vect[line]
                if st < 0:
                    row[po] = row[pe] = -1
                elif st > 0 and (row[po] < 1 or row[pe] < 1):
                    for p_ in (po, pe):
                        if row[p_] < 1:
                            row[p_] = last[p_] if (last is not None and last[p_] >= 1) else 1
            for key, pos in pos_of.items():
                for el, bus in act.get(key, ()):
                    row[pos[el]] = bus
            for p_, bus in dict(act.get("set_bus", {})).items():
                row[p_] = bus
            if act.get("change_bus", ()) and self.n_busbar > 2:
                raise ValueError("change_bus is only defined for 2 busbars per substation (grid2op refuses it otherwise)")
            for p_ in act.get("change_bus", ()):
                if row[p_] >= 1:
                    row[p_] = 2 if row[p_] == 1 else 1
        return out

    def simulate_candidates(self, src_lane: int, dst_lane0: int, actions=None, topologies=None, is_dc: bool = False,
                            max_iter: int = 10, tol_mva: float = 1e-8) -> int:
        """Batched ``obs.simulate`` (Observation/_obsEnv.py:321-503, Reward/n1Reward.py:70-99): lanes ``dst_lane0 ...`` become
        copies of ``src_lane`` (injections, shunts) with one candidate topology each -- built from ``actions``
        (`candidate_topologies`) or given as rows -- and are solved in ONE launch (asynchronous; read them with `results`).
        Returns the number of candidate lanes."""
        if topologies is None:
            base, _ = self.get_topology(src_lane, 1)
            topologies = self.candidate_topologies(base[0], actions)
        topologies = np.ascontiguousarray(topologies, dtype=np.int32).reshape(-1, self.model.dim_topo)
        n = topologies.shape[0]
        self.fanout_n1(src_lane, dst_lane0, np.full(n, -1, dtype=np.int32))      # device-side copy of the source lane's state
        self.set_topology(topologies, lane0=dst_lane0)
        self.runpf(dst_lane0, n, is_dc=is_dc, max_iter=max_iter, tol_mva=tol_mva)
        return n

    ACT_SET_BUS, ACT_SET_LINE_STATUS, ACT_CHANGE_BUS, ACT_CHANGE_LINE_STATUS, ACT_SET_SHUNT_BUS = 0, 1, 2, 3, 4

    def upload_forecasts(self, tables):
        """The ``*_forecasted`` tables of the uploaded chronics (`grid2op_amd.chronics` loads them with ``forecasts=True``;
        `pack_chronics` packs them like the chronics): ``[n_tables, T, n_chron]`` (one horizon, the reference's default) or
        ``[n_tables, T, n_horizons, n_chron]``; None removes them.  Row ``r`` holds the forecast made at chronics row ``r``
        (Chronics/gridStateFromFileWithForecasts.py:311-353)."""
        if tables is None:
            self._call("gpf_upload_forecasts", 0, 0, 0, None)
            return
        t = np.ascontiguousarray(tables, dtype=np.float32)
        if t.ndim == 2:
            t = t[None]
        if t.ndim == 3:
            t = t[:, :, None, :]
        assert t.ndim == 4 and t.shape[3] == self.n_chron, t.shape
        self._call("gpf_upload_forecasts", t.shape[0], t.shape[1], t.shape[2], _ptr(t))

    def pack_actions(self, actions):
        """Candidate actions (dicts as `candidate_topologies` takes them, plus ``"change_line_status": [line ids]`` and
        ``"shunts_bus": [(shunt id, bus)]``) -> (offsets ``[n + 1]``, items ``[n_items, 3]``) of `gpf_simulate_batch`."""
        m = self.model
        pos_of = {"lines_or_bus": m.line_or_pos_topo_vect, "lines_ex_bus": m.line_ex_pos_topo_vect, "loads_bus": m.load_pos_topo_vect,
                  "gens_bus": m.gen_pos_topo_vect, "storages_bus": m.storage_pos_topo_vect}
        off, items = [0], []
        for act in actions:
            for line, st in act.get("set_line_status", ()):
                items.append((self.ACT_SET_LINE_STATUS, int(line), int(st)))
            for line in act.get("change_line_status", ()):
                items.append((self.ACT_CHANGE_LINE_STATUS, int(line), 0))
            for key, pos in pos_of.items():
                for el, bus in act.get(key, ()):
                    items.append((self.ACT_SET_BUS, int(pos[el]), int(bus)))
            for p_, bus in dict(act.get("set_bus", {})).items():
                items.append((self.ACT_SET_BUS, int(p_), int(bus)))
            for p_ in act.get("change_bus", ()):
                items.append((self.ACT_CHANGE_BUS, int(p_), 0))
            for sh, bus in act.get("shunts_bus", ()):
                items.append((self.ACT_SET_SHUNT_BUS, int(sh), int(bus)))
            off.append(len(items))
        return np.asarray(off, dtype=np.int32), np.asarray(items, dtype=np.int32).reshape(-1, 3)

    def simulate_batch(self, t_obs: int, src_lanes, actions, dst_lane0: int, time_step: int = 1, last_bus=None, max_iter: int = 10,
                       tol_mva: float = 1e-8, rebalance: float = 0.0, cascade: bool = False, hard_overflow: float = 2.0,
                       soft_overflow: float = 1.0, nb_ts_allowed: int = 2, max_rounds: int = 16, is_dc: bool = False) -> int:
        """Batched ``obs.simulate(action, time_step)`` (Observation/baseObservation.py:3365-3670): for every source lane ``b``
        (an environment whose current observation is the step at time index ``t_obs``) and every candidate action ``k``, lane
        ``dst_lane0 + b * len(actions) + k`` becomes a copy of lane ``b`` with the action applied as ``_BackendAction`` applies it
        and is stepped ONCE on the injections forecast ``time_step`` steps ahead (0: the observation's own injections) -- all
        ``len(src_lanes) * len(actions)`` candidates in one launch (asynchronous).  Read them with `results` / `step_outputs`
        on the destination range.  ``last_bus``: ``[len(src_lanes), dim_topo]`` last known busbars (reconnections), default 1.
        Returns the number of destination lanes."""
        src = np.ascontiguousarray(src_lanes, dtype=np.int32).reshape(-1)
        off, items = self.pack_actions(actions)
        lb = None if last_bus is None else np.ascontiguousarray(last_bus, dtype=np.int32).reshape(src.size, self.model.dim_topo)
        o = GpfStepOpts(int(max_iter), float(tol_mva), float(rebalance), int(bool(cascade)), float(hard_overflow), float(soft_overflow),
                        int(nb_ts_allowed), int(max_rounds), int(bool(is_dc)), 0, 0, 0, 0)
        self._call("gpf_simulate_batch", int(t_obs), int(time_step), src.size, _ptr(src), len(actions), _ptr(off),
                   _ptr(items if items.size else None), _ptr(lb), int(dst_lane0), C.byref(o))
        return src.size * len(actions)

    # ---- solve --------------------------------------------------------------------------------------
    def runpf(self, lane0: int = 0, n: Optional[int] = None, is_dc: bool = False, max_iter: int = 10,
              tol_mva: float = 1e-8):
        lane0, n = self._range(lane0, n)
        self._call("gpf_runpf", lane0, n, int(bool(is_dc)), int(max_iter), float(tol_mva))

    def _result_arrays(self, n, with_bus=True):
        """out, topo_vect, shunt_bus, line_status (uint8), status, bus_vm, bus_va of ``n`` lanes, uninitialised (the last two None without
        ``with_bus``): what `gpf_get_results` / `gpf_solve_lane` fill."""
        m = self.model
        arrs = [np.empty((n, cols), dtype=dt) for cols, dt in ((self.n_out, np.float32), (m.dim_topo, np.int32), (m.n_shunt, np.int32),
                                                               (m.n_line, np.uint8), (4, np.int32))]
        return arrs + [np.empty((n, self.nb_total), dtype=np.float64) if with_bus else None for _ in range(2)]

    def solve_lane(self, lane: int, inj: np.ndarray, topo: np.ndarray, shunt_bus: Optional[np.ndarray] = None, is_dc: bool = False,
                   max_iter: int = 10, tol_mva: float = 1e-8) -> LaneResults:
        """`set_injections` + `set_topology` + `runpf` + `results` of ONE lane in one C call with a single synchronisation: the
        whole of a Backend's ``runpf`` (what `HipBackend` uses)."""
        m = self.model
        inj = np.ascontiguousarray(inj, dtype=np.float64).reshape(self.n_inj)
        topo = np.ascontiguousarray(topo, dtype=np.int32).reshape(m.dim_topo)
        sb_in = None if not m.n_shunt else np.ascontiguousarray(shunt_bus, dtype=np.int32).reshape(m.n_shunt)
        out, tv, sb, ls, st, bvm, bva = self._result_arrays(1)
        self._call("gpf_solve_lane", int(lane), _ptr(inj), _ptr(topo), _ptr(sb_in), int(bool(is_dc)), int(max_iter), float(tol_mva),
                   _ptr(out), _ptr(tv), _ptr(sb), _ptr(ls), _ptr(st), _ptr(bvm), _ptr(bva))
        return LaneResults(out=out, topo_vect=tv, shunt_bus=sb, line_status=ls.astype(bool), status=st, bus_vm=bvm, bus_va=bva,
                           _slices=self.out_slices)

    def results(self, lane0: int = 0, n: Optional[int] = None, with_bus: bool = True, pinned: bool = False) -> LaneResults:
        """The result rows of lanes ``[lane0, lane0 + n)`` on the host.  ``pinned=True``: the arrays ALIAS a pinned block the engine owns
        (gpf_get_results_pinned: DMA at the PCIe rate, no second host copy) and are only valid until the next ``results(pinned=True)``
        call -- for a host agent that reads every lane at every step; copy what must outlive the step."""
        lane0, n = self._range(lane0, n)
        m = self.model
        if pinned:
            ptrs = (C.c_void_p * 8)()
            what = 0b0011111 | (0b1100000 if with_bus else 0)
            self._call("gpf_get_results_pinned", lane0, n, what, ptrs)

            def arr(k, cols, ctype, dtype):
                if not ptrs[k] or cols == 0:
                    return np.empty((n, cols), dtype=dtype)
                return np.ctypeslib.as_array(C.cast(ptrs[k], C.POINTER(ctype)), shape=(n, cols))
            return LaneResults(out=arr(0, self.n_out, C.c_float, np.float32), topo_vect=arr(1, m.dim_topo, C.c_int32, np.int32),
                               shunt_bus=arr(2, m.n_shunt, C.c_int32, np.int32), line_status=arr(3, m.n_line, C.c_uint8, np.uint8).view(np.bool_),
                               status=arr(4, 4, C.c_int32, np.int32), bus_vm=arr(5, self.nb_total, C.c_double, np.float64) if with_bus else None,
                               bus_va=arr(6, self.nb_total, C.c_double, np.float64) if with_bus else None, _slices=self.out_slices)
        out, tv, sb, ls, st, bvm, bva = self._result_arrays(n, with_bus)
        self._call("gpf_get_results", lane0, n, _ptr(out), _ptr(tv), _ptr(sb), _ptr(ls), _ptr(st), _ptr(bvm), _ptr(bva))
        return LaneResults(out=out, topo_vect=tv, shunt_bus=sb, line_status=ls.astype(bool), status=st, bus_vm=bvm,
                           bus_va=bva, _slices=self.out_slices)

    # ---- batched stepping -----------------------------------------------------------------------------
    def pack_chronics(self, load_p, load_q, prod_p, prod_v) -> np.ndarray:
        """``[..., T, n_chron]`` float32 table from the four ``[..., T, n]`` chronics arrays."""
        return np.ascontiguousarray(np.concatenate([load_p, load_q, prod_p, prod_v], axis=-1), dtype=np.float32)

    def upload_chronics(self, tables: np.ndarray):
        tables = np.ascontiguousarray(tables, dtype=np.float32)
        if tables.ndim == 2:
            tables = tables[None]
        assert tables.shape[2] == self.n_chron, (tables.shape, self.n_chron)
        self._call("gpf_upload_chronics", tables.shape[0], tables.shape[1], _ptr(tables))
        self.chron_T = tables.shape[1]
        self.chron_tables = tables.shape[0]

    def _upload_line_table(self, name, table, dtype):
        """A per-line table of the uploaded chronics, ``[n_tables, T, n_line]`` (or ``[T, n_line]``); None removes it."""
        if table is None:
            self._call(name, 0, 0, None)
            return
        t = np.ascontiguousarray(table, dtype=dtype)
        if t.ndim == 2:
            t = t[None]
        assert t.shape[2] == self.model.n_line
        self._call(name, t.shape[0], t.shape[1], _ptr(t))

    def upload_maintenance(self, maintenance):
        """Scheduled maintenance of the uploaded tables: ``[n_tables, T, n_line]`` (or ``[T, n_line]``) 0/1; None removes it."""
        self._has_maint = maintenance is not None
        self._has_outages = self._has_maint or self._has_hazard
        self._upload_line_table("gpf_upload_maintenance", maintenance, np.uint8)

    def upload_outage_durations(self, durations):
        """Remaining duration of the maintenance / hazard under way at every row, ``[n_tables, T, n_line]`` (or ``[T, n_line]``): what the line
        cooldowns are held at during an outage.  Only needed when the uploaded tables are a window of longer chronics (the library derives
        the durations from the outage tables otherwise); None: derived again."""
        self._upload_line_table("gpf_upload_outage_durations", None if durations is None else np.minimum(np.asarray(durations), 65535), np.uint16)

    def upload_hazards(self, hazards):
        """Hazards of the uploaded tables (``hazards.csv``: unplanned outages): ``[n_tables, T, n_line]`` (or ``[T, n_line]``) 0/1; None
        removes them.  Independent of the maintenance table; a line is out of service where either flags it."""
        self._has_hazard = hazards is not None
        self._has_outages = self._has_hazard or self._has_maint
        self._upload_line_table("gpf_upload_hazards", hazards, np.uint8)

    def set_lane_chronics(self, lane_table=None, lane_offset=None, lane_scale=None):
        lt = None if lane_table is None else np.ascontiguousarray(lane_table, dtype=np.int32)
        lo = None if lane_offset is None else np.ascontiguousarray(lane_offset, dtype=np.int32)
        ls = None if lane_scale is None else np.ascontiguousarray(lane_scale, dtype=np.float32)
        if lt is not None:
            assert lt.size == self.n_lanes
        if lo is not None:
            assert lo.size == self.n_lanes
        if ls is not None:
            assert ls.shape == (self.n_lanes, 2 * self.model.n_load)
        self._call("gpf_set_lane_chronics", _ptr(lt), _ptr(lo), _ptr(ls))

    def set_thermal_limits(self, limit_a):
        lim = np.ascontiguousarray(limit_a, dtype=np.float32)
        assert lim.size == self.model.n_line
        self._call("gpf_set_thermal_limits", _ptr(lim))

    def step(self, t: int, max_iter: int = 10, tol_mva: float = 1e-8, rebalance: float = 0.0, cascade: bool = False,
             hard_overflow: float = 2.0, soft_overflow: float = 1.0, nb_ts_allowed: int = 2, max_rounds: int = 16,
             is_dc: bool = False, n_steps: int = 1, auto_reset: bool = False, warm_start: bool = False, nb_ts_reco: Optional[int] = None):
        """``n_steps`` consecutive DoNothing ``env.step`` (t, t+1, ...) for every lane in ONE launch (asynchronous).  Every step
        writes its results; the getters return the last one, `trajectory` the rho / status of each when requested.
        ``warm_start`` (opt-in, NOT the reference's algorithm) starts Newton of steps 2..n from the previous step's voltages
        while a lane's topology stands: same solution within ``tol_mva``, fewer iterations, ``n_iter`` differs.
        ``nb_ts_reco`` (Parameters.NB_TIMESTEP_RECONNECTION): the environment's line cooldowns (`cooldown`, obs.time_before_cooldown_line) are
        maintained at every step -- default: 10 (the reference's default) when lines can go out by themselves (``cascade`` or uploaded
        maintenance / hazard tables), else not tracked; -1 switches the tracking off."""
        if nb_ts_reco is None:
            nb_ts_reco = 10 if (cascade or self._has_outages) else -1
        o = GpfStepOpts(int(max_iter), float(tol_mva), float(rebalance), int(bool(cascade)), float(hard_overflow), float(soft_overflow),
                        int(nb_ts_allowed), int(max_rounds), int(bool(is_dc)), int(bool(auto_reset)), int(bool(warm_start)), int(nb_ts_reco >= 0), max(int(nb_ts_reco), 0))
        self._call("gpf_step_n", int(t), int(n_steps), C.byref(o))

    def set_lane_redispatch(self, delta_mw):
        """Per-lane additive generator set-point delta (MW, ``[n_lanes, n_gen]``; None switches it off): the redispatch the
        environment adds to the chronics' prod_p."""
        d = None if delta_mw is None else np.ascontiguousarray(delta_mw, dtype=np.float32)
        if d is not None:
            assert d.shape == (self.n_lanes, self.model.n_gen)
        self._call("gpf_set_lane_redispatch", _ptr(d))

    def set_gen_limits(self, pmin, pmax, ramp_up, ramp_down, redispatchable, eps_poly: float = 1e-4):
        """Generator characteristics (``prods_charac.csv``: Pmin, Pmax, max_ramp_up, max_ramp_down, redispatchable) for
        `redispatch`."""
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        a = [f64(pmin), f64(pmax), f64(ramp_up), f64(ramp_down)]
        r = np.ascontiguousarray(redispatchable, dtype=np.uint8)
        assert all(x.size == self.model.n_gen for x in a) and r.size == self.model.n_gen
        self._call("gpf_set_gen_limits", *[_ptr(x) for x in a], _ptr(r), float(eps_poly))

    def redispatch(self, new_p, prev_p, actual, target, modified, rhs, lane0: int = 0, apply: bool = False):
        """The environment's redispatching automaton for a batch of lanes (``BaseEnv._compute_dispatch_vect``): rows
        ``[n, n_gen]`` of new_p / prev_p / actual dispatch / target dispatch / modified mask, ``rhs[n]`` = storage - curtailment
        + detached MW.  Returns ``(ok[n] bool, actual_dispatch_after[n, n_gen] float32)``; ``apply`` also installs the result as
        the lanes' redispatch delta for the next `step`."""
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1, self.model.n_gen)  # noqa: E731
        new_p, prev_p, actual, target = f64(new_p), f64(prev_p), f64(actual), f64(target)
        n = new_p.shape[0]
        mod = np.ascontiguousarray(modified, dtype=np.uint8).reshape(n, self.model.n_gen)
        rhs = np.ascontiguousarray(np.broadcast_to(np.asarray(rhs, dtype=np.float64), (n,)))
        ok = np.empty(n, dtype=np.uint8)
        after = np.empty((n, self.model.n_gen), dtype=np.float32)
        self._call("gpf_redispatch", int(lane0), n, _ptr(new_p), _ptr(prev_p), _ptr(actual), _ptr(target), _ptr(mod), _ptr(rhs),
                   int(bool(apply)), _ptr(ok), _ptr(after))
        return ok.astype(bool), after

    TRAJ_RHO, TRAJ_OBS = 1, 2

    # ---- injection dynamics of the environment (storage state of charge, redispatch projection) inside the stepped batch ------
    def set_storage_params(self, emax, emin, loss, eff_charge, eff_discharge, charge0, delta_time_seconds: float = 300.0,
                           activate_loss: bool = True):
        """Storage characteristics (``storage_Emax / Emin / loss / charging_efficiency / discharging_efficiency``, initial charge
        in MWh), the step length and ``Parameters.ACTIVATE_STORAGE_LOSS``."""
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(self.model.n_storage)  # noqa: E731
        a = [f64(emax), f64(emin), f64(loss), f64(eff_charge), f64(eff_discharge)]
        c0 = np.ascontiguousarray(charge0, dtype=np.float32).reshape(self.model.n_storage)
        self._call("gpf_set_storage_params", *[_ptr(x) for x in a], _ptr(c0), float(delta_time_seconds), int(bool(activate_loss)))

    def set_env_dynamics(self, on: bool = True, tol_poly: float = 1e-2):
        """Switch the environment's injection dynamics on: every step of `step` then evolves the storage state of charge and
        re-solves the ramp-limited redispatch (BaseEnv.step's path between the chronics and the backend); needs `set_gen_limits`
        (and `set_storage_params` on a grid with storage units).  Resets the dynamics of every lane."""
        self._call("gpf_set_env_dynamics", int(bool(on)), float(tol_poly))
        self.env_dynamics_on = bool(on)

    def set_lane_actions(self, redispatch=None, storage_power=None, hold_storage: bool = False):
        """The agents' actions of the NEXT launch: redispatch ``[n_lanes, n_gen]`` MW (consumed by its first step), storage power
        ``[n_lanes, n_storage]`` MW (first step only, or every step until replaced with ``hold_storage``)."""
        r = None if redispatch is None else np.ascontiguousarray(redispatch, dtype=np.float32).reshape(self.n_lanes, self.model.n_gen)
        s_ = None if storage_power is None or not self.model.n_storage else \
            np.ascontiguousarray(storage_power, dtype=np.float32).reshape(self.n_lanes, self.model.n_storage)
        self._call("gpf_set_lane_actions", _ptr(r), _ptr(s_), int(bool(hold_storage)))

    def lane_actions_on_device(self, redispatch: bool = False, storage_power: bool = False, curtailment: bool = False,
                               hold_storage: bool = False):
        """The actions of the NEXT launch were written ON THE DEVICE, into ``device_views()["act_redispatch" / "act_storage" /
        "act_curtail"]`` (on ``views["stream"]`` or ordered before the launch): say which buffers hold an action.  Same semantics as
        `set_lane_actions` / `set_lane_curtailment`, no PCIe transfer, no synchronisation -- the hand-over of an agent that lives next
        to the engine (curtailment ratios are NOT range-checked on this path)."""
        self._call("gpf_lane_actions_on_device", int(bool(redispatch)), int(bool(storage_power)), int(bool(curtailment)), int(bool(hold_storage)))

    # ---- topology actions in the batched step (include/gridpf.h: gpf_upload_topo_actions) ------------------------------------
    def set_topo_rules(self, max_sub_changed: int = 1, max_line_status_changed: int = 1, cooldown_sub: int = 0, cooldown_line: int = 0,
                       legal_rules: bool = True):
        """Parameters.MAX_SUB_CHANGED / MAX_LINE_STATUS_CHANGED (DefaultRules; ``legal_rules=False``: AlwaysLegal) and
        NB_TIMESTEP_COOLDOWN_SUB / NB_TIMESTEP_COOLDOWN_LINE of the topology actions of the batched step."""
        self._call("gpf_set_topo_rules", int(bool(legal_rules)), int(max_sub_changed), int(max_line_status_changed), int(cooldown_sub), int(cooldown_line))

    def upload_topo_actions(self, actions) -> np.ndarray:
        """The action table of the topology actions (dicts as `pack_actions` takes them); returns the static ambiguity flags (bool ``[n]``).
        Lanes then pick an entry per launch: `set_lane_topo_actions` (host) or ``device_views()["act_topo"]`` + `topo_actions_on_device`."""
        off, items = self.pack_actions(actions)
        n = len(off) - 1
        amb = np.zeros(max(n, 1), dtype=np.uint8)
        items = np.ascontiguousarray(items, dtype=np.int32)
        self._call("gpf_upload_topo_actions", n, _ptr(off), _ptr(items if items.size else None), _ptr(amb))
        self._n_topo_act = n
        self._mask_view = None               # (the engine-owned mask buffer is re-allocated with the table)
        return amb[:n].astype(bool)

    def set_topo_areas(self, areas=None):
        """The areas of the reference's ``RulesByArea``: ``sub_area`` (int ``[n_sub]``, the area of every substation) or a list of lists
        of substation ids, one per area (at most 16).  The two limits of `set_topo_rules` then hold per area, a line counting in the
        area of its origin substation.  None: whole-grid limits again (the default)."""
        n_sub = self.model.n_sub
        if areas is None or len(areas) == 0:
            self._call("gpf_set_topo_areas", 0, None)
            return
        if np.ndim(areas[0]) == 0:
            sub_area = np.ascontiguousarray(areas, dtype=np.int32)
            if sub_area.shape != (n_sub,):
                raise ValueError(f"set_topo_areas: sub_area must have {n_sub} entries")
            n_area = int(sub_area.max()) + 1 if (sub_area >= 0).all() else 1     # (the library refuses a negative id)
        else:
            sub_area = np.full(n_sub, -1, dtype=np.int32)
            for k, subs in enumerate(areas):
                subs = np.asarray(subs, dtype=np.int64)
                if ((subs < 0) | (subs >= n_sub)).any() or (sub_area[subs] >= 0).any():
                    raise ValueError("set_topo_areas: a substation id is out of range or listed twice")
                sub_area[subs] = k
            n_area = len(areas)
        self._call("gpf_set_topo_areas", n_area, _ptr(sub_area))

    def set_topo_slots(self, n_slot: int = 1):
        """Table entries a lane plays per step (1..8): the concatenation, in slot order, of the non-empty slots' item lists is played as
        ONE action.  Changing it drops pending indices; ``device_views()["act_topo"]`` becomes ``[n_lanes, n_slot]``."""
        self._call("gpf_set_topo_slots", int(n_slot))
        self._n_topo_slot = int(n_slot)

    def topo_action_areas(self) -> np.ndarray:
        """uint32 ``[n_act]``: bit k set when the table entry can touch area k (every substation it names, both ends of every line it
        names).  Entries of the slots of one lane with pairwise disjoint area sets are applied exactly when each has mask byte 0."""
        out = np.zeros(max(int(self._n_topo_act), 1), dtype=np.uint32)
        self._call("gpf_get_topo_action_areas", _ptr(out))
        return out[:int(self._n_topo_act)]

    def set_lane_topo_actions(self, index):
        """Entries of the action table every lane plays at the NEXT launch (int ``[n_lanes]`` with one slot, ``[n_lanes, n_slot]`` else;
        -1 = empty slot, all empty = do nothing; None: none) -- that launch must be a one-step launch."""
        a = None if index is None else np.ascontiguousarray(index, dtype=np.int32).reshape(self.n_lanes * int(self._n_topo_slot))
        self._call("gpf_set_lane_topo_actions", _ptr(a))

    def topo_actions_on_device(self, on: bool = True):
        """The NEXT launch takes the indices written into ``device_views()["act_topo"]`` (on ``views["stream"]`` or ordered before it)."""
        self._call("gpf_topo_actions_on_device", int(bool(on)))

    def sub_cooldown(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """obs.time_before_cooldown_sub of the lanes, int32 ``[n, n_sub]``."""
        return self._get_rows("gpf_get_sub_cooldown", lane0, n, (self.model.n_sub, np.int32))

    def set_sub_cooldown(self, sub_cooldown, lane0: int = 0):
        self._set_rows("gpf_set_sub_cooldown", sub_cooldown, self.model.n_sub, np.int32, lane0)

    def last_bus(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Last known busbar of every element (where a reconnected line end goes back to), int32 ``[n, dim_topo]``."""
        return self._get_rows("gpf_get_last_bus", lane0, n, (self.model.dim_topo, np.int32))

    def set_last_bus(self, last_bus, lane0: int = 0):
        self._set_rows("gpf_set_last_bus", last_bus, self.model.dim_topo, np.int32, lane0)

    def topo_action_flags(self, lane0: int = 0, n: Optional[int] = None):
        """(is_illegal, is_ambiguous) bool ``[n]`` of the last launch that carried topology actions."""
        f = self._get_rows("gpf_get_topo_flags", lane0, n, (2, np.uint8))
        return f[:, 0].astype(bool), f[:, 1].astype(bool)

    def topo_action_mask(self, lane0: int = 0, n: Optional[int] = None, out=None):
        """Which entries of the uploaded action table lanes ``[lane0, lane0 + n)`` may play right now: a uint8 torch tensor
        ``[n, n_act]`` in device memory, 0 where a launch that carried the entry would apply it, else the OR of the reasons
        (`MASK_TOO_MANY_LINES` ... `MASK_AMBIGUOUS`).  One kernel queued on the engine's stream (asynchronous: order the consumer on
        ``device_views()["stream"]``, or `sync`); it only reads the lanes' state.  Without ``out`` the tensor ALIASES the engine-owned buffer
        ``device_views()["topo_mask"]`` (rewritten by the next call); ``out`` may be a caller's uint8 CUDA tensor ``[n, >= n_act]`` with unit
        column stride and any row stride >= n_act -- only the first ``n_act`` columns of its rows are written."""
        lane0, n = self._range(lane0, n)
        if out is None:
            self._call("gpf_topo_action_mask", lane0, n, None, 0)
            if self._mask_view is None:
                self._mask_view = self.device_views()["topo_mask"]
            return self._mask_view[lane0:lane0 + n]
        self._call("gpf_topo_action_mask", lane0, n, *self._out_rows("topo_action_mask", out, "uint8", n, self._n_topo_act, True))
        return out[:, :self._n_topo_act]

    def topo_action_mask_host(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """`topo_action_mask` copied to the host: uint8 ``[n, n_act]`` (synchronous)."""
        lane0, n = self._range(lane0, n)
        out = np.empty((n, int(self._n_topo_act)), dtype=np.uint8)
        self._call("gpf_get_topo_action_mask", lane0, n, _ptr(out if out.size else None))
        return out

    # ---- the opponent (include/gridpf.h gpf_set_opponent; grid2op_amd/csrc/gridpf_opponent.hpp) -------
    def set_opponent(self, kind=OPP_NONE, lines=(), *, init_budget=0.0, budget_per_ts=0.0, attack_duration=0, attack_cooldown=0,
                     rho_normalization=None, attack_period=12 * 24, attack_hazard_rate=0.0, recovery_rate=0.0, recovery_minimum_duration=0,
                     pmax_pmin_ratio=4.0, episode_max_time=0, draw_source=OPP_DRAWS_PHILOX, seed=0, lane_base=0, schedule_cap=64):
        """The reference's OpponentSpace with a RandomLine / WeightedRandom / Geometric opponent on every lane of the one-step launches
        (`opponent_config` builds these arguments from a ``grid2op.make``-style configuration).  ``kind`` None or `OPP_NONE`: off.
        ``lines``: attackable line ids in the order of ``lines_attacked``.  ``seed``: 64-bit key of the Philox source; ``lane_base``: the
        global index of lane 0.  Launches then need ``n_steps = 1`` and ``track_cooldown``."""
        self._alert = None                   # gpf_set_opponent turns alerts off
        self._opp_n_lines = 0
        if kind is None or int(kind) == OPP_NONE:
            self._call("gpf_set_opponent", None)
            self._opp_cap = self._opp_n_area = 0
            return
        ids = np.ascontiguousarray(lines, dtype=np.int32).reshape(-1)
        norm = None if rho_normalization is None else np.ascontiguousarray(rho_normalization, dtype=np.float64).reshape(-1)
        if norm is not None and norm.size != ids.size:
            raise ValueError("set_opponent: rho_normalization must have one entry per attackable line")
        self._opp_n_lines = int(ids.size)
        d = GpfOpponentDesc()
        d.kind, d.n_lines, d.line_ids, d.rho_normalization = int(kind), int(ids.size), _ptr(ids if ids.size else None), _ptr(norm)
        d.attack_period, d.attack_hazard_rate, d.recovery_rate = int(attack_period), float(attack_hazard_rate), float(recovery_rate)
        d.recovery_minimum_duration, d.pmax_pmin_ratio, d.episode_max_time = int(recovery_minimum_duration), float(pmax_pmin_ratio), int(episode_max_time)
        d.init_budget, d.budget_per_ts = float(np.float32(init_budget)), float(np.float32(budget_per_ts))
        d.attack_duration, d.attack_cooldown, d.draw_source = int(attack_duration), int(attack_cooldown), int(draw_source)
        d.seed_lo, d.seed_hi, d.lane_base, d.schedule_cap = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(lane_base), int(schedule_cap)
        self._call("gpf_set_opponent", C.byref(d))
        self._opp_cap, self._opp_n_area = (int(schedule_cap) if int(kind) == OPP_GEOMETRIC else 0), 0

    def upload_opponent_draws(self, draws):
        """Table source: float64 ``[n_lanes, n_draw]`` uniforms in [0, 1), consumed per lane in event order; the cursors go back to 0."""
        u = np.ascontiguousarray(draws, dtype=np.float64).reshape(self.n_lanes, -1)
        self._call("gpf_upload_opponent_draws", u.shape[1], _ptr(u if u.size else None))

    def upload_opponent_schedule(self, schedule, count):
        """Geometric opponent, table source: int32 ``[n_lanes, k, 2]`` {waiting time, duration} (``k`` <= the schedule capacity) and the
        number of entries of every lane -- what the opponent's reset sampled."""
        cap = int(self._opp_cap)
        sch = np.asarray(schedule, dtype=np.int32).reshape(self.n_lanes, -1, 2)
        if sch.shape[1] > cap:
            raise ValueError(f"upload_opponent_schedule: {sch.shape[1]} entries per lane exceed the schedule capacity {cap}")
        full = np.zeros((self.n_lanes, max(cap, 1), 2), dtype=np.int32)
        full[:, :sch.shape[1]] = sch
        cnt = np.ascontiguousarray(np.broadcast_to(np.asarray(count, dtype=np.int32), (self.n_lanes,)))
        self._call("gpf_upload_opponent_schedule", _ptr(full), _ptr(cnt))

    def opponent_state(self, lane0: int = 0, n: Optional[int] = None) -> "OpponentState":
        """The lanes' opponent state with ``opponent_attack_line`` (-1: none) / ``opponent_attack_duration`` of the last launch (synchronous)."""
        return OpponentState.from_rows(*self._get_rows("gpf_get_opponent_state", lane0, n, (None, np.float64), (OPP_STATE_INTS, np.int32), zeros=True))

    def set_opponent_state(self, state: "OpponentState", lane0: int = 0):
        bud = np.ascontiguousarray(state.budget, dtype=np.float64)
        rows = np.ascontiguousarray(state.rows())
        self._call("gpf_set_opponent_state", int(lane0), len(bud), _ptr(bud), _ptr(rows))

    # ---- the multi-area opponent (include/gridpf.h gpf_set_opponent_areas) ----------------------------
    def set_opponent_areas(self, area_of_line):
        """GeometricOpponentMultiArea: ``area_of_line[i]`` is the area of entry ``i`` of the ``lines`` of `set_opponent` (kind
        `OPP_GEOMETRIC`); every area is a Geometric opponent of its own on the lane's one stream of draws (`opponent_area_config` builds
        both from a reference-style configuration).  None (or empty): back to the single-area opponent.  Every lane's opponent starts reset."""
        a = np.zeros(0, np.int32) if area_of_line is None else np.ascontiguousarray(area_of_line, dtype=np.int32).reshape(-1)
        n_area = int(a.max()) + 1 if a.size else 0
        self._alert = None                   # ... and so does gpf_set_opponent_areas
        self._call("gpf_set_opponent_areas", n_area, _ptr(a if a.size else None))
        self._opp_n_area = n_area

    def upload_opponent_area_schedule(self, schedule, count):
        """Table source: int32 ``[n_lanes, n_area, k, 2]`` {waiting time, duration} (``k`` <= the schedule capacity) and ``[n_lanes, n_area]``
        entries -- what every area's reset sampled."""
        cap, na = int(self._opp_cap), int(self._opp_n_area)
        sch = np.asarray(schedule, dtype=np.int32)
        sch = np.broadcast_to(sch, (self.n_lanes,) + sch.shape[-3:]) if sch.ndim == 3 else sch.reshape(self.n_lanes, na, -1, 2)
        if sch.shape[2] > cap:
            raise ValueError(f"upload_opponent_area_schedule: {sch.shape[2]} entries per area exceed the schedule capacity {cap}")
        full = np.zeros((self.n_lanes, na, max(cap, 1), 2), dtype=np.int32)
        full[:, :, :sch.shape[2]] = sch
        cnt = np.ascontiguousarray(np.broadcast_to(np.asarray(count, dtype=np.int32), (self.n_lanes, na)))
        self._call("gpf_upload_opponent_area_schedule", _ptr(full), _ptr(cnt))

    def opponent_area_state(self, lane0: int = 0, n: Optional[int] = None) -> "OpponentAreaState":
        lane0, n = self._range(lane0, n)
        rows = np.zeros((n, max(int(self._opp_n_area), 1), OPP_AREA_STATE_INTS), dtype=np.int32)
        self._call("gpf_get_opponent_area_state", lane0, n, _ptr(rows))
        return OpponentAreaState.from_rows(rows)

    def set_opponent_area_state(self, state: "OpponentAreaState", lane0: int = 0):
        rows = np.ascontiguousarray(state.rows())
        self._call("gpf_set_opponent_area_state", int(lane0), rows.shape[0], _ptr(rows))

    def opponent_attack_lines(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """bool ``[n, n_line]``: ``info["opponent_attack_line"]`` of the last launch, with or without areas (synchronous)."""
        return self._get_rows("gpf_get_opponent_attack_lines", lane0, n, (self.model.n_line, np.uint8), zeros=True).astype(bool)

    # ---- alerts and AlertReward (include/gridpf.h gpf_set_alerts; grid2op_amd/csrc/gridpf_alert.hpp) ----
    def set_alerts(self, time_window: Optional[int] = 12, reward_min_no_blackout=-1.0, reward_min_blackout=-10.0, reward_max_no_blackout=1.0,
                   reward_max_blackout=2.0):
        """The alert bookkeeping of ``BaseEnv.step`` and ``AlertReward`` on every lane of the one-step launches (`alert_config` builds the
        arguments from the reference's ``Parameters``).  The alertable lines are the current opponent's ``lines`` (with areas: grouped by
        area), so call it after `set_opponent` / `set_opponent_areas`, which turn alerts off.  ``time_window`` None: off.  Every lane
        starts reset.  The end-of-episode bonus of ``AlertReward`` is paid on a step truncated by `set_episode_limit`, which carries it."""
        if time_window is None:
            self._call("gpf_set_alerts", None)
            self._alert = None
            return
        d = GpfAlertDesc(int(time_window), float(reward_min_no_blackout), float(reward_min_blackout), float(reward_max_no_blackout),
                         float(reward_max_blackout))
        self._alert = None
        self._call("gpf_set_alerts", C.byref(d))
        self._alert = (self._opp_n_lines, int(time_window))

    def _alert_dims(self, what):
        if self._alert is None:
            raise GridPFError(f"{what}: alerts are off (set_alerts)")
        return self._alert

    def set_lane_alerts(self, alerts):
        """The agent's alerts of the NEXT launch: bool ``[n_lanes, A]`` (A alertable lines, in the opponent's order) or uint64 ``[n_lanes]``
        masks (bit i = alertable line i); None: none.  Consumed by the launch."""
        if alerts is None:
            self._call("gpf_set_lane_alerts", None)
            return
        a = np.asarray(alerts)
        if a.ndim == 2:
            if a.shape[1] > 64:
                raise ValueError("set_lane_alerts: at most 64 alertable lines")
            a = (a.astype(bool).astype(np.uint64) << np.arange(a.shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(self.n_lanes)
        self._call("gpf_set_lane_alerts", _ptr(a))

    def alerts_on_device(self, on: bool = True):
        """The NEXT launch takes the masks written into ``device_views()["act_alert"]`` (int64 ``[n_lanes]``: the bits of the uint64 mask; bits at
        or above A are dropped by the kernel)."""
        self._call("gpf_alerts_on_device", int(bool(on)))

    def alert_state(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """int32 ``[n, 8 A + 3 + 2 (W + 2) A]`` rows (include/gridpf.h gpf_get_alert_state; `alert_state_fields` names their parts)."""
        A, W = self._alert_dims("alert_state")
        return self._get_rows("gpf_get_alert_state", lane0, n, (8 * A + 3 + 2 * (W + 2) * A, np.int32), zeros=True)

    def set_alert_state(self, rows, lane0: int = 0):
        A, W = self._alert_dims("set_alert_state")
        self._set_rows("gpf_set_alert_state", rows, 8 * A + 3 + 2 * (W + 2) * A, np.int32, lane0)

    def alert_state_fields(self, rows) -> dict:
        """views of the parts of `alert_state` rows: the seven environment arrays ``[n, A]``, ``total_number_of_alert`` / ``current_id`` /
        ``ran`` ``[n]``, ``lines_currently_attacked`` ``[n, A]``, ``ts_attack`` / ``alert_launched`` ``[n, W + 2, A]``"""
        A, W = self._alert_dims("alert_state_fields")
        R = W + 2
        names = ("last_alert", "is_already_attacked", "time_since_last_alert", "alert_duration", "time_since_last_attack", "attack_under_alert",
                 "was_alert_used_after_attack")
        out = {k: rows[:, i * A:(i + 1) * A] for i, k in enumerate(names)}
        out.update(total_number_of_alert=rows[:, 7 * A], current_id=rows[:, 7 * A + 1], ran=rows[:, 7 * A + 2],
                   lines_currently_attacked=rows[:, 7 * A + 3:8 * A + 3], ts_attack=rows[:, 8 * A + 3:8 * A + 3 + R * A].reshape(-1, R, A),
                   alert_launched=rows[:, 8 * A + 3 + R * A:].reshape(-1, R, A))
        return out

    def alert_reward(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """float32 ``[n]``: ``AlertReward`` of the last launch (0 on a lane that was reset or left alone); synchronous."""
        self._alert_dims("alert_reward")
        return self._get_rows("gpf_get_alert_reward", lane0, n, (None, np.float32), zeros=True)

    def set_gen_renewable(self, renewable):
        """``gen_renewable`` mask (curtailment only acts on these generators); None switches curtailment off."""
        r = None if renewable is None else np.ascontiguousarray(renewable, dtype=np.uint8).reshape(self.model.n_gen)
        self._call("gpf_set_gen_renewable", _ptr(r))

    def set_lane_curtailment(self, limit):
        """Curtailment action of the NEXT launch: ``[n_lanes, n_gen]`` ratios of pmax in [0, 1], -1 = no change (consumed by the
        launch's first step; the limits then stay in the lanes' state until changed)."""
        a = None if limit is None else np.ascontiguousarray(limit, dtype=np.float32).reshape(self.n_lanes, self.model.n_gen)
        self._call("gpf_set_lane_curtailment", _ptr(a))

    def env_state(self, lane0: int = 0, n: Optional[int] = None) -> dict:
        """``target`` / ``actual`` dispatch, ``prev_p``, ``already_modified`` ``[n, n_gen]``, ``charge`` ``[n, n_storage]``,
        ``amount_prev`` ``[n]`` of the lanes' environment dynamics; ``illegal`` ``[n]``: actions cancelled as illegal redispatch since the reset."""
        lane0, n = self._range(lane0, n)
        ng, ns = self.model.n_gen, self.model.n_storage
        d = dict(target=np.empty((n, ng), np.float32), actual=np.empty((n, ng), np.float32), prev_p=np.empty((n, ng), np.float32),
                 already_modified=np.empty((n, ng), np.uint8), charge=np.empty((n, ns), np.float32), amount_prev=np.empty(n, np.float32),
                 curtail_limit=np.empty((n, ng), np.float32), curtail_prev=np.empty(n, np.float32))
        self._call("gpf_get_env_state", lane0, n, _ptr(d["target"]), _ptr(d["actual"]), _ptr(d["prev_p"]), _ptr(d["already_modified"]),
                   _ptr(d["charge"] if ns else None), _ptr(d["amount_prev"]), _ptr(d["curtail_limit"]), _ptr(d["curtail_prev"]))
        d["already_modified"] = d["already_modified"].astype(bool)
        d["illegal"] = np.empty(n, np.int32)             # steps whose action BaseEnv.step would have cancelled as an illegal redispatch
        self._call("gpf_get_env_illegal", lane0, n, _ptr(d["illegal"]))
        return d

    def set_env_state(self, lane0: int = 0, target=None, actual=None, prev_p=None, already_modified=None, charge=None, amount_prev=None,
                      curtail_limit=None, curtail_prev=None, illegal=None):
        """Overwrite (parts of) the lanes' environment dynamics, e.g. to restore them from an observation.  Accepts every key
        `env_state` returns (``eng.set_env_state(l0, **eng.env_state(l1, n))`` moves the complete state of n lanes)."""
        f = lambda a, w: None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(-1, w)  # noqa: E731
        ng, ns = self.model.n_gen, max(self.model.n_storage, 1)
        arrs = [f(target, ng), f(actual, ng), f(prev_p, ng)]
        am = None if already_modified is None else np.ascontiguousarray(already_modified, dtype=np.uint8).reshape(-1, ng)
        ch = None if charge is None or not self.model.n_storage else f(charge, ns)
        ap = None if amount_prev is None else np.ascontiguousarray(amount_prev, dtype=np.float32).reshape(-1)
        cl = f(curtail_limit, ng)
        cp = None if curtail_prev is None else np.ascontiguousarray(curtail_prev, dtype=np.float32).reshape(-1)
        il = None if illegal is None else np.ascontiguousarray(illegal, dtype=np.int32).reshape(-1)
        n = next((x.shape[0] for x in arrs + [am, ch, ap, cl, cp] if x is not None), None)
        if il is not None:
            self._call("gpf_set_env_illegal", int(lane0), il.shape[0], _ptr(il))
        if n is None:
            return
        self._call("gpf_set_env_state", int(lane0), n, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), _ptr(am), _ptr(ch), _ptr(ap), _ptr(cl), _ptr(cp))

    def set_trajectory(self, n_steps_cap: int, what: int = 1):
        """Trajectory buffers of multi-step launches: ``what`` = `TRAJ_RHO` (rho + status of every step) or `TRAJ_OBS` (in
        addition the complete backend observation of every step: results row, topo_vect, shunt buses, line status).
        ``n_steps_cap = 0`` releases them."""
        self._call("gpf_set_trajectory", int(n_steps_cap), int(what))
        self._traj_cap = int(n_steps_cap) if what else 0

    def trajectory(self, n_steps: int, step0: int = 0, lane0: int = 0, n: Optional[int] = None):
        """(rho ``[n_steps, n, n_line]`` float32, status ``[n_steps, n]`` int8) of the steps of the last multi-step launch."""
        lane0, n = self._range(lane0, n)
        rho = np.empty((n_steps, n, self.model.n_line), dtype=np.float32)
        st = np.empty((n_steps, n), dtype=np.int8)
        self._call("gpf_get_trajectory", int(step0), int(n_steps), lane0, n, _ptr(rho), _ptr(st))
        return rho, st

    def trajectory_obs(self, n_steps: int, step0: int = 0, lane0: int = 0, n: Optional[int] = None):
        """The backend observation of every step of the last multi-step launch (`set_trajectory(cap, TRAJ_OBS)`): a list of
        `LaneResults` (one per step; ``status`` column 0 from the status trajectory, bus voltages are not part of it)."""
        lane0, n = self._range(lane0, n)
        m = self.model
        out = np.empty((n_steps, n, self.n_out), dtype=np.float32)
        tv = np.empty((n_steps, n, m.dim_topo), dtype=np.int32)
        sb = np.empty((n_steps, n, m.n_shunt), dtype=np.int32)
        ls = np.empty((n_steps, n, m.n_line), dtype=np.uint8)
        self._call("gpf_get_trajectory_obs", int(step0), int(n_steps), lane0, n, _ptr(out), _ptr(tv), _ptr(sb), _ptr(ls))
        _, st = self.trajectory(n_steps, step0, lane0, n)
        res = []
        for k in range(n_steps):
            st4 = np.full((n, 4), -1, dtype=np.int32)
            st4[:, 0] = st[k]
            res.append(LaneResults(out=out[k], topo_vect=tv[k], shunt_bus=sb[k], line_status=ls[k].astype(bool), status=st4,
                                   bus_vm=None, bus_va=None, _slices=self.out_slices))
        return res

    def episode(self, lane0: int = 0, n: Optional[int] = None):
        """(done ``[n]`` bool, steps survived since the last reset ``[n]``, auto-resets ``[n]``)."""
        done, sr = self._get_rows("gpf_get_episode", lane0, n, (None, np.uint8), (2, np.int32))
        return done.astype(bool), sr[:, 0].copy(), sr[:, 1].copy()

    # ---- the environment's rewards (include/gridpf.h gpf_set_rewards; grid2op_amd/csrc/gridpf_reward.hpp) ----
    def set_rewards(self, slots, gen_cost_per_MW=None):
        """The rewards of ``env.step`` on every lane of the one-step launches: ``slots`` is a list of up to 8 slots, each a `reward_config`
        result, a ``(kind, p)`` pair or a bare ``RW_*`` kind (the reference's ``reward_class`` first, then its ``other_rewards``);
        ``gen_cost_per_MW`` ``[n_gen]`` is needed by `RW_REDISP` / `RW_ECONOMIC`.  None or an empty list: off."""
        self._rw_view = None                 # (the engine-owned rewards are re-allocated for the new slot count)
        if not slots:
            self._call("gpf_set_rewards", 0, None, None)
            self._n_reward_slot = 0
            return
        arr = (GpfRewardSlot * len(slots))()
        for i, s_ in enumerate(slots):
            if isinstance(s_, dict):
                kind, p = s_["kind"], s_.get("p", ())
            elif isinstance(s_, (tuple, list)):
                kind, p = s_
            else:
                kind, p = s_, ()
            p = [float(x) for x in p]
            if len(p) > 6:
                raise ValueError("set_rewards: a slot has at most 6 parameters")
            arr[i].kind = int(kind)
            for j, x in enumerate(p):
                arr[i].p[j] = x
        cost = None
        if gen_cost_per_MW is not None:
            cost = np.ascontiguousarray(gen_cost_per_MW, dtype=np.float32).reshape(self.model.n_gen)
        self._n_reward_slot = 0
        self._call("gpf_set_rewards", len(slots), arr, _ptr(cost))
        self._n_reward_slot = len(slots)

    def _reward_slots(self, what):
        n = int(self._n_reward_slot)
        if n == 0:
            raise GridPFError(f"{what}: rewards are off (set_rewards)")
        return n

    def rewards(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """float32 ``[n, n_slot]``: the rewards of the last one-step launch (0 on a lane that was reset since); synchronous.  Refused after
        a multi-step launch, which computes none."""
        return self._get_rows("gpf_get_rewards", lane0, n, (self._reward_slots("rewards"), np.float32), zeros=True)

    def reward_views(self) -> dict:
        """``{"rewards": float32 torch tensor [n_lanes, n_slot]}`` ALIASING the engine-owned rewards (what a device-resident learner reads,
        no copy; order the reader on ``device_views()["stream"]``)."""
        ns = self._reward_slots("reward_views")
        return self._views(self._device_pointers("gpf_reward_device_pointers", _capi.N_REWARD_POINTERS), [("rewards", 0, (ns,), "<f4")])

    def rewards_eval(self, lane0: int = 0, n: Optional[int] = None, flags=None, out=None):
        """The rewards of lanes ``[lane0, lane0 + n)`` on their CURRENT state (results row, rho, line status, done / status, dispatch, storage
        set-points), one read-only kernel queued on the engine's stream: for a state restored or copied into a lane.  ``flags``: a uint8
        CUDA tensor ``[n, 2]`` {illegal, ambiguous} (None: none).  Without ``out`` the result ALIASES the lanes' rows of the engine-owned
        rewards; ``out`` may be a float32 CUDA tensor ``[n, >= n_slot]`` with unit column stride."""
        import torch
        ns = self._reward_slots("rewards_eval")
        lane0, n = self._range(lane0, n)
        fp = None
        if flags is not None:
            if not (isinstance(flags, torch.Tensor) and flags.is_cuda and flags.dtype == torch.uint8 and tuple(flags.shape) == (n, 2)
                    and flags.is_contiguous() and flags.device.index == self.device):
                raise ValueError(f"rewards_eval: flags must be a contiguous uint8 CUDA tensor [{n}, 2] on cuda:{self.device}")
            fp = C.cast(flags.data_ptr(), C.POINTER(C.c_uint8))
        if out is None:
            self._call("gpf_rewards_eval", lane0, n, fp, None, 0)
            if self._rw_view is None:
                self._rw_view = self.reward_views()["rewards"]
            return self._rw_view[lane0:lane0 + n]
        self._call("gpf_rewards_eval", lane0, n, fp, *self._out_rows("rewards_eval", out, "float32", n, ns, True))
        return out[:, :ns]

    # ---- episode time limits (include/gridpf.h gpf_set_episode_limit; grid2op_amd/csrc/gridpf_episode.hpp) ----
    def set_episode_limit(self, max_steps, per_timestep: float = 1.0, alert_end_bonus: float = 0.0):
        """The reference's ``done`` without an error on every lane of the one-step launches: ``max_steps`` is one step count for all lanes
        or an array ``[n_lanes]`` (0: no limit for that lane; after `reset` the N-th launch of a lane with limit N is the truncated one,
        as after ``env.reset(options={"max step": N})``); None, or 0, turns the feature off.  ``per_timestep`` is
        ``EpisodeDurationReward``'s, ``alert_end_bonus`` ``AlertReward.reward_end_episode_bonus`` (`alert_end_bonus` reads it).  Under
        ``auto_reset`` a truncated lane restarts as a failed one does; while a limit is set multi-step launches are refused."""
        self._ep_on = False
        if max_steps is None:
            self._call("gpf_set_episode_limit", None)
            return
        d = GpfEpisodeDesc(0, None, float(per_timestep), float(alert_end_bonus))
        arrays = {}                          # referenced until the call has returned
        if np.ndim(max_steps) > 0:
            arrays["lane_max_steps"] = np.ascontiguousarray(max_steps, dtype=np.int32).reshape(self.n_lanes)
        else:
            d.max_steps = int(max_steps)
        _fill_pointers(d, arrays)
        self._call("gpf_set_episode_limit", C.byref(d))
        self._ep_on = bool(arrays) or d.max_steps > 0

    def _episode_on(self, what):
        if not self._ep_on:
            raise GridPFError(f"{what}: episode limits are off (set_episode_limit)")

    def episode_ends(self, lane0: int = 0, n: Optional[int] = None) -> dict:
        """``terminated`` / ``truncated`` bool ``[n]``, ``length`` int32 ``[n]`` (``nb_time_step`` of the episode that ended in the last
        launch, else 0), ``duration_reward`` float32 ``[n]`` (``EpisodeDurationReward``); synchronous."""
        self._episode_on("episode_ends")
        te, tr, ln, du = self._get_rows("gpf_get_episode_ends", lane0, n, (None, np.uint8), (None, np.uint8), (None, np.int32), (None, np.float32),
                                        zeros=True)
        return dict(terminated=te.astype(bool), truncated=tr.astype(bool), length=ln, duration_reward=du)

    def episode_stats(self, lane0: int = 0, n: Optional[int] = None) -> dict:
        """``return_running`` / ``return_last`` float64 ``[n, n_slot]`` (sequential sums of the launches' float32 rewards; the episode under
        way / the last one that ended), ``length_last`` / ``n_episodes`` int32 ``[n]``; synchronous."""
        self._episode_on("episode_stats")
        ns = self._n_reward_slot
        run, last, ll, ne = self._get_rows("gpf_get_episode_stats", lane0, n, (REWARD_MAX_SLOTS, np.float64), (REWARD_MAX_SLOTS, np.float64),
                                           (None, np.int32), (None, np.int32), zeros=True)
        return dict(return_running=run[:, :ns].copy(), return_last=last[:, :ns].copy(), length_last=ll, n_episodes=ne)

    def episode_views(self) -> dict:
        """Zero-copy torch tensors ALIASING the episode buffers (order the reader on ``device_views()["stream"]``): ``limit`` int32
        ``[n_lanes]`` (writable: the next launch reads it), ``terminated`` / ``truncated`` uint8 ``[n_lanes]``, ``length``,
        ``duration_reward``, ``return_running`` / ``return_last`` float64 ``[n_lanes, n_slot]``, ``length_last``, ``n_episodes``."""
        self._episode_on("episode_views")
        v = self._views(self._device_pointers("gpf_episode_device_pointers", _capi.N_EPISODE_POINTERS),
                        [("limit", 0, (), "<i4"), ("flags", 1, (2,), "|u1"), ("length", 2, (), "<i4"), ("duration_reward", 3, (), "<f4"),
                         ("running", 4, (REWARD_MAX_SLOTS,), "<f8"), ("last", 5, (REWARD_MAX_SLOTS,), "<f8"), ("length_last", 6, (), "<i4"),
                         ("n_episodes", 7, (), "<i4")])
        ns = self._n_reward_slot
        return {"limit": v["limit"], "terminated": v["flags"][:, 0], "truncated": v["flags"][:, 1], "length": v["length"],
                "duration_reward": v["duration_reward"], "return_running": v["running"][:, :ns], "return_last": v["last"][:, :ns],
                "length_last": v["length_last"], "n_episodes": v["n_episodes"]}

    # ---- the N-1 screen (include/gridpf.h gpf_set_n1_screen; grid2op_amd/csrc/gridpf_n1.hpp) ----
    def set_n1_screen(self, lines, n_env: Optional[int] = None):
        """``N1Reward`` for the watched ``lines`` on every environment lane of the one-step launches: lanes ``[0, n_env)`` are the
        environments (the only lanes `step` then steps), lane ``n_env + i * K + k`` is environment ``i`` with ``lines[k]`` out, solved in
        the same launch.  ``n_env`` None: as many as fit, ``n_lanes // (1 + K)``.  None or an empty list: off.  A reward slot
        ``(RW_N1, [k])`` of `set_rewards` is the value of ``lines[k]``; while the screen is on multi-step launches are refused."""
        if lines is None or len(lines) == 0:
            self._call("gpf_set_n1_screen", 0, None, 0)
            self._n1 = None
            return
        ln = np.ascontiguousarray(lines, dtype=np.int32).reshape(-1)
        ne = self.n_lanes // (1 + ln.size) if n_env is None else int(n_env)
        self._call("gpf_set_n1_screen", ne, _ptr(ln), ln.size)      # (a refused call leaves the screen as it was)
        self._n1 = (ne, int(ln.size))

    def _n1_range(self, what, lane0, n):
        """The environments among lanes ``[lane0, lane0 + n)`` (the whole range by default): first environment, count, K."""
        if getattr(self, "_n1", None) is None:
            raise GridPFError(f"{what}: the N-1 screen is off (set_n1_screen)")
        ne, K = self._n1
        lane0, n = self._range(lane0, n)
        a, b = min(max(lane0, 0), ne), min(max(lane0 + n, 0), ne)
        return a, max(b - a, 0), K

    def n1_values(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """float32 ``[n_env', K]``: the ``N1Reward`` values of the last one-step launch for the environment lanes inside lanes
        ``[lane0, lane0 + n)`` (0: the step ended the episode, -1: the contingency's power flow diverged); synchronous."""
        a, m, K = self._n1_range("n1_values", lane0, n)
        out = np.zeros((m, K), np.float32)
        self._call("gpf_get_n1_values", a, m, _ptr(out))
        return out

    def n1_summary(self, lane0: int = 0, n: Optional[int] = None) -> dict:
        """``worst`` float32, ``arg_worst`` / ``n_insecure`` / ``n_diverged`` int32, each ``[n_env']``, of the environment lanes inside
        lanes ``[lane0, lane0 + n)``: the contingency that ranks first (a diverged one outranks every value, the lowest index wins a tie)
        and its value, the contingencies above 1 or diverged, the diverged ones; synchronous."""
        a, m, _ = self._n1_range("n1_summary", lane0, n)
        w, aw, ni, nd = np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        self._call("gpf_get_n1_summary", a, m, _ptr(w), _ptr(aw), _ptr(ni), _ptr(nd))
        return dict(worst=w, arg_worst=aw, n_insecure=ni, n_diverged=nd)

    def n1_views(self) -> dict:
        """Zero-copy torch tensors ALIASING the screen's buffers (order the reader on ``device_views()["stream"]``): ``values`` float32
        ``[n_env, K]``, ``worst`` float32 ``[n_env]``, ``arg_worst`` / ``n_insecure`` / ``n_diverged`` int32 ``[n_env]``, ``lines`` int32
        ``[K]``."""
        import torch
        _, _, K = self._n1_range("n1_views", 0, None)
        ptrs = self._device_pointers("gpf_n1_device_pointers", _capi.N_N1_POINTERS)

        def view(p, shape, typestr):
            iface = {"shape": shape, "typestr": typestr, "data": (int(p), False), "version": 2, "strides": None}
            return torch.as_tensor(type("_Arr", (), {"__cuda_array_interface__": iface})(), device=torch.device("cuda", self.device))
        ne = self._n1[0]
        info = view(ptrs[2], (ne, 3), "<i4")
        return {"values": view(ptrs[0], (ne, K), "<f4"), "worst": view(ptrs[1], (ne,), "<f4"), "arg_worst": info[:, 0], "n_insecure": info[:, 1],
                "n_diverged": info[:, 2], "lines": view(ptrs[3], (K,), "<i4")}

    # ---- the look-ahead screen (include/gridpf.h gpf_set_lookahead; grid2op_amd/csrc/gridpf_lookahead.hpp) ----
    def set_lookahead(self, n_cand: int, n_env: Optional[int] = None):
        """``obs.simulate`` of ``n_cand`` action-table entries per environment in one call (`lookahead`): lanes ``[0, n_env)`` are the
        environments (the only lanes `step` then steps), lane ``n_env + i * n_cand + k`` is the scratch lane of candidate ``k`` of
        environment ``i``.  ``n_env`` None: as many as fit, ``n_lanes // (1 + n_cand)``.  0 or None: off.  Needs an uploaded action
        table; refused with composite slots, areas or the N-1 screen on; while it is set multi-step launches are refused."""
        self._lc = None                      # (the chain's buffers have the look-ahead's shape: the library releases them)
        if not n_cand:
            self._call("gpf_set_lookahead", 0, 0)
            self._la = None
            return
        K = int(n_cand)
        ne = self.n_lanes // (1 + K) if n_env is None else int(n_env)
        self._la = None
        try:
            self._call("gpf_set_lookahead", ne, K)
        except GridPFError as exc:
            if "header-only handle" in str(exc):     # (the library keeps a valid setting there, so that every later refusal can be shown)
                self._la = (ne, K)
            raise
        self._la = (ne, K)

    def _la_range(self, what, lane0, n):
        """The environments among lanes ``[lane0, lane0 + n)`` (the whole range by default): first environment, count, K."""
        if getattr(self, "_la", None) is None:
            raise GridPFError(f"{what}: the look-ahead is off (set_lookahead)")
        ne, K = self._la
        lane0, n = self._range(lane0, n)
        a, b = min(max(lane0, 0), ne), min(max(lane0 + n, 0), ne)
        return a, max(b - a, 0), K

    def lookahead(self, t_obs: int, time_step: int = 1, candidates=None, max_iter: int = 10, tol_mva: float = 1e-8, rebalance: float = 0.0,
                  cascade: bool = False, hard_overflow: float = 2.0, soft_overflow: float = 1.0, nb_ts_allowed: int = 2, max_rounds: int = 16,
                  is_dc: bool = False):
        """Environment ``i``'s candidates -- ``candidates`` int32 ``[n_env, K]`` of table indices (-1: do nothing), or None: what was
        written into ``lookahead_views()["cand"]`` on ``device_views()["stream"]`` -- are played under the environment's rules on copies of
        lane ``i`` and stepped once on the forecast ``time_step`` steps ahead (0: the observation's own injections), as `simulate_batch`
        steps its candidates, and reduced on the device (asynchronous): ``value`` (the simulated ``rho.max()``, +inf when the step ended
        the episode), ``flags`` (`LA_ILLEGAL` | `LA_AMBIGUOUS` | `LA_DONE`), ``best`` (the playable slot with the lowest value, -1: none)
        -- `lookahead_views` / `lookahead_values`.  The environments are not touched and nothing plays the choice::

            v, la = eng.device_views(), eng.lookahead_views()
            pick = la["cand"].gather(1, la["best"].clamp(min=0).long()[:, None])[:, 0]
            v["act_topo"][:n_env, 0] = torch.where(la["best"] >= 0, pick, -1)
        """
        cand = None
        if candidates is not None:
            if getattr(self, "_la", None) is None:
                raise GridPFError("lookahead: the look-ahead is off (set_lookahead)")
            cand = np.ascontiguousarray(candidates, dtype=np.int32)
            if cand.shape != self._la:
                raise ValueError(f"lookahead: candidates must be [n_env, K] = {list(self._la)}, got {list(cand.shape)}")
        o = GpfStepOpts(int(max_iter), float(tol_mva), float(rebalance), int(bool(cascade)), float(hard_overflow), float(soft_overflow),
                        int(nb_ts_allowed), int(max_rounds), int(bool(is_dc)), 0, 0, 0, 0)
        self._call("gpf_lookahead", int(t_obs), int(time_step), _ptr(cand), C.byref(o))

    def lookahead_values(self, lane0: int = 0, n: Optional[int] = None) -> dict:
        """``value`` float32 / ``flags`` uint8 ``[n_env', K]``, ``best`` int32 / ``best_value`` float32 ``[n_env']``, ``n_playable`` /
        ``n_done`` int32 ``[n_env']`` of the last `lookahead`, for the environment lanes inside lanes ``[lane0, lane0 + n)``; synchronous."""
        a, m, K = self._la_range("lookahead_values", lane0, n)
        value, flags = np.zeros((m, K), np.float32), np.zeros((m, K), np.uint8)
        best, bv, info = np.zeros(m, np.int32), np.zeros(m, np.float32), np.zeros((m, 2), np.int32)
        self._call("gpf_get_lookahead", a, m, _ptr(value), _ptr(flags), _ptr(best), _ptr(bv), _ptr(info))
        return dict(value=value, flags=flags, best=best, best_value=bv, n_playable=info[:, 0].copy(), n_done=info[:, 1].copy())

    def lookahead_views(self) -> dict:
        """Zero-copy torch tensors ALIASING the look-ahead's buffers (order the reader or writer on ``device_views()["stream"]``): ``cand``
        int32 ``[n_env, K]`` (the candidates a `lookahead` without ``candidates`` plays), ``value`` float32 / ``flags`` uint8
        ``[n_env, K]``, ``best`` int32 / ``best_value`` float32 ``[n_env]``, ``n_playable`` / ``n_done`` int32 ``[n_env]``."""
        import torch
        _, _, K = self._la_range("lookahead_views", 0, None)
        ptrs = self._device_pointers("gpf_lookahead_device_pointers", _capi.N_LOOKAHEAD_POINTERS)

        def view(p, shape, typestr):
            iface = {"shape": shape, "typestr": typestr, "data": (int(p), False), "version": 2, "strides": None}
            return torch.as_tensor(type("_Arr", (), {"__cuda_array_interface__": iface})(), device=torch.device("cuda", self.device))
        ne = self._la[0]
        info = view(ptrs[5], (ne, 2), "<i4")
        return {"cand": view(ptrs[0], (ne, K), "<i4"), "value": view(ptrs[1], (ne, K), "<f4"), "flags": view(ptrs[2], (ne, K), "|u1"),
                "best": view(ptrs[3], (ne,), "<i4"), "best_value": view(ptrs[4], (ne,), "<f4"), "n_playable": info[:, 0], "n_done": info[:, 1]}

    # ---- the look-ahead chain (include/gridpf.h gpf_set_lookahead_chain; grid2op_amd/csrc/gridpf_lookahead.hpp) ----
    def set_lookahead_chain(self, max_steps: int):
        """Chains of up to ``max_steps`` forecast steps on the scratch lanes of `set_lookahead` (`lookahead_chain`).  0 or None: off;
        `set_lookahead` switches it off as well."""
        self._lc = None
        if not max_steps:
            self._call("gpf_set_lookahead_chain", 0)
            return
        try:
            self._call("gpf_set_lookahead_chain", int(max_steps))
        except GridPFError as exc:
            if "header-only handle" in str(exc):     # (the library keeps a valid setting there, so that every later refusal can be shown)
                self._lc = int(max_steps)
            raise
        self._lc = int(max_steps)

    def _lc_range(self, what, lane0, n):
        if getattr(self, "_lc", None) is None or getattr(self, "_la", None) is None:
            raise GridPFError(f"{what}: the chain is off (set_lookahead_chain)")
        return self._la_range(what, lane0, n) + (self._lc,)

    def lookahead_chain(self, t_obs: int, n_steps: int, candidates=None, play: int = 0, max_iter: int = 10, tol_mva: float = 1e-8,
                        rebalance: float = 0.0, cascade: bool = False, hard_overflow: float = 2.0, soft_overflow: float = 1.0,
                        nb_ts_allowed: int = 2, max_rounds: int = 16, is_dc: bool = False):
        """``obs.get_forecast_env()`` for every candidate of every environment in one call: `lookahead` ``(t_obs, 1)``, then do-nothing
        steps on forecast horizons 2 .. ``n_steps`` of the same observation, the lines of a maintenance that begins on the way taken out,
        overflow counters and protections running (asynchronous).  ``value`` / ``flags`` / ``best`` of `lookahead_values` then speak of
        the chain (``value``: the maximum of ``rho.max()`` over the steps, +inf and `LA_DONE` when any step ended the episode);
        `lookahead_chain_values` / `lookahead_chain_views` hold ``survived``, ``peak``, ``value_h``, ``fallback``.  ``play``: 1 writes the
        table index of the best slot (-1 without one) into ``device_views()["act_topo"]`` of the environment's lane and arms it as
        `topo_actions_on_device` does, 2 falls back on ``fallback`` before -1; 0 leaves the acting path alone."""
        cand = None
        if candidates is not None:
            if getattr(self, "_la", None) is None:
                raise GridPFError("lookahead_chain: the look-ahead is off (set_lookahead)")
            cand = np.ascontiguousarray(candidates, dtype=np.int32)
            if cand.shape != self._la:
                raise ValueError(f"lookahead_chain: candidates must be [n_env, K] = {list(self._la)}, got {list(cand.shape)}")
        o = GpfStepOpts(int(max_iter), float(tol_mva), float(rebalance), int(bool(cascade)), float(hard_overflow), float(soft_overflow),
                        int(nb_ts_allowed), int(max_rounds), int(bool(is_dc)), 0, 0, 0, 0)
        self._call("gpf_lookahead_chain", int(t_obs), int(n_steps), _ptr(cand), int(play), C.byref(o))

    def lookahead_chain_values(self, lane0: int = 0, n: Optional[int] = None) -> dict:
        """``survived`` int32 / ``peak`` float32 ``[n_env', K]``, ``value_h`` float32 ``[n_env', K, max_steps]`` (columns below the last
        call's ``n_steps``), ``fallback`` / ``fallback_steps`` int32 ``[n_env']`` of the last `lookahead_chain`, for the environment lanes
        inside lanes ``[lane0, lane0 + n)``; synchronous."""
        a, m, K, H = self._lc_range("lookahead_chain_values", lane0, n)
        survived, peak, value_h = np.zeros((m, K), np.int32), np.zeros((m, K), np.float32), np.zeros((m, K, H), np.float32)
        fb, fbs = np.zeros(m, np.int32), np.zeros(m, np.int32)
        self._call("gpf_get_lookahead_chain", a, m, _ptr(survived), _ptr(peak), _ptr(value_h), _ptr(fb), _ptr(fbs))
        return dict(survived=survived, peak=peak, value_h=value_h, fallback=fb, fallback_steps=fbs)

    def lookahead_chain_views(self) -> dict:
        """Zero-copy torch tensors ALIASING the chain's buffers (order the reader on ``device_views()["stream"]``): ``survived`` int32 /
        ``peak`` float32 ``[n_env, K]``, ``value_h`` float32 ``[n_env, K, max_steps]``, ``fallback`` / ``fallback_steps`` int32 ``[n_env]``."""
        import torch
        _, _, K, H = self._lc_range("lookahead_chain_views", 0, None)
        ptrs = self._device_pointers("gpf_lookahead_chain_device_pointers", _capi.N_LOOKAHEAD_CHAIN_POINTERS)

        def view(p, shape, typestr):
            iface = {"shape": shape, "typestr": typestr, "data": (int(p), False), "version": 2, "strides": None}
            return torch.as_tensor(type("_Arr", (), {"__cuda_array_interface__": iface})(), device=torch.device("cuda", self.device))
        ne = self._la[0]
        return {"survived": view(ptrs[0], (ne, K), "<i4"), "peak": view(ptrs[1], (ne, K), "<f4"), "value_h": view(ptrs[2], (ne, K, H), "<f4"),
                "fallback": view(ptrs[3], (ne,), "<i4"), "fallback_steps": view(ptrs[4], (ne,), "<i4")}

    # ---- combined topology + injection actions (include/gridpf.h gpf_set_combined_actions; grid2op_amd/csrc/gridpf_combined.hpp) ----
    def set_combined_actions(self, on: bool = True, check_values: bool = True, storage_max_p_prod=None, storage_max_p_absorb=None):
        """One-step launches take topology actions and injection actions (redispatch / storage / curtailment) together, lane by lane, as
        ``BaseEnv.step`` does: a verdict on either part voids both, ``PreventDiscoStorageModif`` joins the rules, a redispatch the step
        cancels books no cooldown.  ``check_values``: the reference's value rules on every lane of the launch (``storage_max_p_prod`` /
        ``storage_max_p_absorb`` ``[n_storage]``: the storage range; None: not checked).  Needs `set_env_dynamics` and the acting path;
        ``on=False`` brings the refusal of combined launches back."""
        self._cb_on = False
        if not on:
            self._call("gpf_set_combined_actions", None)
            return
        d = GpfCombinedDesc(1, 1 if check_values else 0, None, None)
        arrays = {name: None if v is None else np.ascontiguousarray(v, dtype=np.float32).reshape(self.model.n_storage)
                  for name, v in (("storage_max_p_prod", storage_max_p_prod), ("storage_max_p_absorb", storage_max_p_absorb))}
        _fill_pointers(d, arrays)            # (referenced until the call has returned)
        self._call("gpf_set_combined_actions", C.byref(d))
        self._cb_on = True

    def _combined_on(self, what):
        if not self._cb_on:
            raise GridPFError(f"{what}: combined actions are off (set_combined_actions)")

    def action_flags(self, lane0: int = 0, n: Optional[int] = None) -> dict:
        """``is_illegal`` / ``is_ambiguous`` / ``is_illegal_redisp`` bool ``[n]`` and ``reason`` uint8 ``[n]`` (``GPF_CB_*``) of the whole
        step of the last one-step launch in combined mode; synchronous."""
        self._combined_on("action_flags")
        f = self._get_rows("gpf_get_action_flags", lane0, n, (4, np.uint8), zeros=True)
        return dict(is_illegal=f[:, 0].astype(bool), is_ambiguous=f[:, 1].astype(bool), is_illegal_redisp=f[:, 2].astype(bool), reason=f[:, 3].copy())

    def combined_views(self) -> dict:
        """``{"flags": uint8 torch tensor [n_lanes, 4]}`` {is_illegal, is_ambiguous, is_illegal_redisp, reason} ALIASING the engine-owned
        flags of the last one-step launch (no copy; order the reader on ``device_views()["stream"]``)."""
        self._combined_on("combined_views")
        return self._views(self._device_pointers("gpf_combined_device_pointers", _capi.N_COMBINED_POINTERS), [("flags", 0, (4,), "|u1")])

    # ---- the chronics cursor (include/gridpf.h gpf_set_chronics_cursor; grid2op_amd/csrc/gridpf_cursor.hpp) ----
    def set_chronics_cursor(self, order=None, policy="sequential", probabilities=None, first_row=0, next_pos=None, seed=None, lane_base: int = 0):
        """Every lane that starts an episode in a one-step launch starts a scenario, as ``env.reset()`` does (``next_chronics``).
        ``order``: table indices (``Multifolder._order``; None: every uploaded table in order), or False to turn the feature off.
        ``policy`` "sequential" walks the order; "sampled" draws a position with ``probabilities`` (None: uniform) as
        ``sample_next_chronics`` does.  ``first_row``: the row the first launch of an episode reads, one value or ``[n_lanes]`` (0 for a
        loop that spends a launch on the reset observation, 1 for one that does not, ``k`` / ``k + 1`` for ``options={"init ts": k}``).
        ``next_pos``: the position the first episode takes, one value or ``[n_lanes]`` (None: 0 when sequential, a draw when sampled);
        later ones are written through `cursor_views` (``env.set_id``).  ``seed`` None: the uniforms come from `upload_cursor_draws`;
        an integer: Philox on (episodes started, lane + ``lane_base``).  While it is on multi-step launches are refused."""
        self._cur_on = False
        if order is False:
            self._call("gpf_set_chronics_cursor", None)
            return
        if order is None:
            order = np.arange(int(getattr(self, "chron_tables", 1)))
        order = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
        pol = {"sequential": CURSOR_SEQUENTIAL, "sampled": CURSOR_SAMPLED}.get(policy, policy)
        d = GpfCursorDesc(n_order=len(order), policy=int(pol), lane_base=int(lane_base))
        arrays = dict(order=order)           # descriptor field -> array, referenced until the call has returned
        if pol == CURSOR_SAMPLED:
            arrays["cdf"] = cursor_cdf(np.ones(len(order)) if probabilities is None else probabilities)
            if len(arrays["cdf"]) != len(order):
                raise ValueError("probabilities: one per position of the order")
        for name, val, default in (("first_row", first_row, 0), ("next_pos", next_pos, 0 if pol == CURSOR_SEQUENTIAL else -1)):
            val = default if val is None else val
            if np.ndim(val) > 0:
                arrays["lane_" + name] = np.ascontiguousarray(val, dtype=np.int32).reshape(self.n_lanes)
            else:
                setattr(d, name, int(val))
        _fill_pointers(d, arrays)
        if seed is None:
            d.draw_source = OPP_DRAWS_TABLE
        else:
            d.draw_source, d.seed_lo, d.seed_hi = OPP_DRAWS_PHILOX, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        self._call("gpf_set_chronics_cursor", C.byref(d))
        self._cur_on = True

    def _cursor_on(self, what):
        if not self._cur_on:
            raise GridPFError(f"{what}: the chronics cursor is off (set_chronics_cursor)")

    def upload_cursor_draws(self, draws):
        """``[n_lanes, n_draw]`` float64 uniforms in [0, 1) of the sampled policy, one per episode start and lane, consumed in order."""
        self._cursor_on("upload_cursor_draws")
        u = np.ascontiguousarray(draws, dtype=np.float64).reshape(self.n_lanes, -1)
        self._call("gpf_upload_cursor_draws", u.shape[1], _ptr(u))

    def chronics_cursor_state(self, lane0: int = 0, n: Optional[int] = None) -> "CursorState":
        self._cursor_on("chronics_cursor_state")
        return CursorState.from_rows(self._get_rows("gpf_get_cursor_state", lane0, n, (CURSOR_STATE_INTS, np.int32), zeros=True))

    def set_chronics_cursor_state(self, state: "CursorState", lane0: int = 0):
        self._cursor_on("set_chronics_cursor_state")
        self._set_rows("gpf_set_cursor_state", state.rows(), CURSOR_STATE_INTS, np.int32, lane0)

    def cursor_views(self) -> dict:
        """Zero-copy torch tensors ALIASING the cursor's buffers (order the reader on ``device_views()["stream"]``), int32 ``[n_lanes]``:
        ``next_pos`` (writable: ``env.set_id`` on the device), ``pos``, ``n_started``."""
        self._cursor_on("cursor_views")
        return self._views(self._device_pointers("gpf_cursor_device_pointers", _capi.N_CURSOR_POINTERS),
                           [("next_pos", 0, (), "<i4"), ("pos", 1, (), "<i4"), ("n_started", 2, (), "<i4")])

    # ---- zero-copy device views ------------------------------------------------------------------------------------------
    def device_views(self):
        """The engine's result buffers as torch tensors that ALIAS the device memory (no copy, no PCIe): ``out`` float32
        ``[n_lanes, n_out]`` (columns: `out_slices`), ``rho`` ``[n_lanes, n_line]``, ``status`` int32 ``[n_lanes, 4]``,
        ``topo_vect``, ``line_status`` uint8, ``overflow_count``, ``done`` uint8, ``episode`` int32 ``[n_lanes, 2]``, ``inj``
        float64, ``bus_vm`` / ``bus_va`` float64; with the environment dynamics on also the action buffers ``act_redispatch`` /
        ``act_curtail`` ``[n_lanes, n_gen]``, ``act_storage`` ``[n_lanes, n_storage]`` (`lane_actions_on_device`) and
        ``target_dispatch`` / ``actual_dispatch`` / ``storage_charge`` float32 (obs.target_dispatch, ...); once topology actions are enabled
        (`set_topo_rules` / `upload_topo_actions`) also ``act_topo`` int32 ``[n_lanes, n_slot]`` (`topo_actions_on_device`), ``sub_cooldown``
        ``[n_lanes, n_sub]``, ``topo_flags`` uint8 ``[n_lanes, 2]`` and ``last_bus`` ``[n_lanes, dim_topo]``; once an observation spec is set
        (`set_obs_spec`) also ``obs`` float32 ``[n_lanes, dim]`` (what `observation_vector` without ``out`` writes); once an action table is
        uploaded also ``topo_mask`` uint8 ``[n_lanes, n_act]`` (what `topo_action_mask` without ``out`` writes).  The engine works on its own HIP stream: call `sync` (or make the consumer's
        stream wait on ``views["stream"]``, a ``torch.cuda.ExternalStream``) before reading."""
        import torch
        ptrs = (C.c_void_p * _capi.N_DEVICE_POINTERS)()
        stream = C.c_void_p()
        self._call("gpf_device_pointers_n", ptrs, _capi.N_DEVICE_POINTERS, C.byref(stream))
        m = self.model
        v = self._views(ptrs, [
            ("inj", 0, (self.n_inj,), "<f8"), ("topo", 1, (m.dim_topo,), "<i4"), ("out", 3, (self.n_out,), "<f4"),
            ("topo_vect", 4, (m.dim_topo,), "<i4"), ("line_status", 5, (m.n_line,), "|u1"), ("status", 6, (4,), "<i4"),
            ("rho", 8, (m.n_line,), "<f4"), ("overflow_count", 9, (m.n_line,), "<i4"), ("done", 10, (1,), "|u1"),
            ("episode", 11, (2,), "<i4"), ("bus_vm", 12, (self.nb_total,), "<f8"), ("bus_va", 13, (self.nb_total,), "<f8"),
            ("disc_round", 15, (m.n_line,), "<i4"),
            ("act_redispatch", 22, (m.n_gen,), "<f4"), ("act_storage", 23, (m.n_storage,), "<f4"), ("act_curtail", 24, (m.n_gen,), "<f4"),
            ("target_dispatch", 25, (m.n_gen,), "<f4"), ("actual_dispatch", 26, (m.n_gen,), "<f4"),
            ("storage_charge", 27, (m.n_storage,), "<f4"),
            ("act_topo", 28, (self._n_topo_slot,), "<i4"), ("sub_cooldown", 29, (m.n_sub,), "<i4"), ("topo_flags", 30, (2,), "|u1"),
            ("last_bus", 31, (m.dim_topo,), "<i4"),
            ("obs", 32, (self._obs_spec.dim if self._obs_spec is not None else 0,), "<f4"),
            ("topo_mask", 33, (self._n_topo_act,), "|u1")])
        for key, idx, cols, typestr in (("traj_rho", 16, m.n_line, "<f4"), ("traj_status", 17, 1, "|i1"), ("traj_out", 18, self.n_out, "<f4"),
                                        ("traj_topo_vect", 19, m.dim_topo, "<i4"), ("traj_shunt_bus", 20, m.n_shunt, "<i4"),
                                        ("traj_line_status", 21, m.n_line, "|u1")):      # trajectory buffers: [cap_steps][cap][cols]
            v[key] = self._view(ptrs[idx], (cols,), typestr, steps=self._traj_cap) if self._traj_cap else None
        if self._alert is not None:          # alerts on: the masks of the next launch, the rewards, the observation block
            v.update(self._views(self._device_pointers("gpf_alert_device_pointers", _capi.N_ALERT_POINTERS),
                                 [("act_alert", 0, (), "<i8"), ("alert_reward", 1, (), "<f4"), ("alert_obs", 2, (6 * self._alert[0] + 1,), "<i4")]))
        v["stream"] = torch.cuda.ExternalStream(stream.value, device=torch.device("cuda", self.device))
        return v


    # ---- observation vectors assembled on the device (include/gridpf.h: gpf_set_obs_spec; grid2op_amd/obs_spec.py) ----------------------
    def set_obs_clock(self, start, step_minutes: int = 5, max_step: Optional[int] = None):
        """The calendar of row 0 of each chronics table: ``start`` is a naive ``datetime`` (or a list with one per table); ``step_minutes``
        is the length of a step (obs.delta_time), ``max_step`` what obs.max_step reports (default: the rows of the uploaded tables - 1,
        as the reference's ``max_episode_duration`` of a chronics of that length)."""
        import datetime as _dt
        starts = list(start) if isinstance(start, (list, tuple)) else [start]
        mins = []
        for s_ in starts:
            if not isinstance(s_, _dt.datetime):
                raise TypeError("set_obs_clock: start must be a datetime (or a list of them)")
            d = s_.replace(tzinfo=None) - _dt.datetime(1970, 1, 1)
            if d.seconds % 60 or d.microseconds:
                raise ValueError("set_obs_clock: start must fall on a whole minute")
            mins.append(d.days * 1440 + d.seconds // 60)
        if max_step is None:
            max_step = max(int(getattr(self, "chron_T", 1)) - 1, 0)
        a = np.ascontiguousarray(mins, dtype=np.int64)
        self._call("gpf_set_obs_clock", a.size, _ptr(a), int(step_minutes), int(max_step))

    def set_obs_spec(self, spec, game_over_fill: bool = True):
        """The layout of the observation vectors (`grid2op_amd.obs_spec.ObsSpec`).  ``game_over_fill``: a lane whose last step ended its
        episode gets the reference's game-over vector (``BaseObservation.set_game_over``: zeros, topo_vect / _shunt_bus /
        time_next_maintenance -1, curtailment_limit 1, calendar and counters kept) instead of the NaN rows of the failed power flow."""
        from .obs_spec import out_offsets
        oo = out_offsets(self.model)
        assert all(self.out_slices[k].start == v for k, v in oo.items()), "obs_spec.out_offsets disagrees with the library's layout"
        seg = np.ascontiguousarray(spec.segments, dtype=np.int32)
        sub = np.ascontiguousarray(spec.subtract, dtype=np.float32)
        div = np.ascontiguousarray(spec.divide, dtype=np.float32)
        assert sub.size == spec.dim and div.size == spec.dim
        self._call("gpf_set_obs_spec", seg.shape[0], _ptr(seg), int(spec.dim), _ptr(sub), _ptr(div), int(bool(game_over_fill)))
        self._obs_spec = spec
        self._obs_view = None                # (the engine-owned observation buffer is re-allocated for the new dim)

    def _obs_dim(self):
        if self._obs_spec is None:
            raise GridPFError("no observation spec is set (set_obs_spec)")
        return self._obs_spec.dim

    def observation_vector(self, lane0: int = 0, n: Optional[int] = None, out=None):
        """The observation vectors of lanes ``[lane0, lane0 + n)`` as a float32 torch tensor ``[n, dim]`` in device memory, written by one
        gather kernel queued on the engine's stream (asynchronous: order the consumer on ``device_views()["stream"]``, or `sync`).
        Without ``out`` the tensor ALIASES the engine-owned buffer ``device_views()["obs"]`` (rewritten by the next call); ``out`` may be
        a caller's float32 CUDA tensor ``[n, >= dim]`` with unit column stride and any row stride >= dim -- only the first ``dim``
        columns of its rows are written."""
        lane0, n = self._range(lane0, n)
        dim = self._obs_dim()
        if out is None:
            self._call("gpf_obs_vector", lane0, n, None, 0)
            if self._obs_view is None:
                self._obs_view = self.device_views()["obs"]
            return self._obs_view[lane0:lane0 + n]
        self._call("gpf_obs_vector", lane0, n, *self._out_rows("observation_vector", out, "float32", n, dim, False))
        return out[:, :dim]

    def observation_trajectory(self, n_steps: int, step0: int = 0, lane0: int = 0, n: Optional[int] = None, out=None):
        """The observation vectors of steps ``[step0, step0 + n_steps)`` of the last multi-step launch, ``[n_steps, n, dim]`` float32 on the
        device, from the per-step copies of `set_trajectory(cap, TRAJ_OBS)`.  Calendar and maintenance attributes advance with the
        steps; attributes without a per-step copy (timestep_overflow, time_before_cooldown_sub, the dispatch / charge / curtailment
        state, current_step) must not be in the spec.  Asynchronous, as `observation_vector`."""
        import torch
        lane0, n = self._range(lane0, n)
        dim = self._obs_dim()
        if out is None:
            out = torch.empty((int(n_steps), n, dim), dtype=torch.float32, device=torch.device("cuda", self.device))
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (int(n_steps), n, dim)):
            raise ValueError(f"observation_trajectory: out must be a contiguous float32 CUDA tensor of shape {(int(n_steps), n, dim)}")
        torch.cuda.current_stream(out.device).synchronize()      # (a fresh allocation may still be in use by work queued on torch's stream)
        self._call("gpf_obs_vector_trajectory", int(step0), int(n_steps), lane0, n, C.cast(out.data_ptr(), C.POINTER(C.c_float)))
        return out

    def observation_vector_host(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """`observation_vector` copied to the host: float32 ``[n, dim]`` (synchronous)."""
        return self._get_rows("gpf_get_obs_vector", lane0, n, (self._obs_dim(), np.float32))

    # ---- the observation as a bus graph (include/gridpf.h: gpf_set_graph_obs; grid2op_amd/csrc/gridpf_graph.hpp) ------------------------
    def set_graph_obs(self, on: bool = True, game_over_fill: bool = True):
        """Turns the bus-graph observation on (the static tables are built from the grid) or off.  ``game_over_fill``: a lane whose last
        step ended its episode gets the reference's game-over graph (one bus, every element on it, zeros) instead of what its rows give."""
        self._call("gpf_set_graph_obs", int(bool(on)), int(bool(game_over_fill)))
        self._graph_on = bool(on)

    def graph_layout(self) -> dict:
        """The sections of the index row as slices, by name in `GRAPH_SECTIONS` order, with ``"width"`` (ints per row), ``"NB"``
        (``n_sub * n_busbar``: rows of the feature table, side of the dense planes) and ``"n_features"``."""
        off, wid = np.zeros(_capi.GRAPH_N_SECTIONS, np.int32), np.zeros(_capi.GRAPH_N_SECTIONS, np.int32)
        width, nb = C.c_int32(0), C.c_int32(0)
        self._call("gpf_graph_layout", _ptr(off), _ptr(wid), C.byref(width), C.byref(nb))
        lay = {name: slice(int(o), int(o + w)) for name, o, w in zip(GRAPH_SECTIONS, off, wid)}
        lay.update(width=int(width.value), NB=int(nb.value), n_features=_capi.GRAPH_N_FEATURES)
        return lay

    def _graph_shapes(self, n, dense):
        if not self._graph_on:
            raise GridPFError("the graph observation is off (set_graph_obs)")
        lay = self.graph_layout()
        nb = lay["NB"]
        return (n, lay["width"]), (n, nb, _capi.GRAPH_N_FEATURES), (n, 3, nb, nb) if dense else None

    def graph_observation(self, lane0: int = 0, n: Optional[int] = None, out_index=None, out_features=None, out_dense=None, dense: bool = False,
                          out=None):
        """The bus graph of lanes ``[lane0, lane0 + n)`` as torch tensors in device memory: ``(index, features, dense)`` -- int32
        ``[n, width]`` (sections: `graph_layout`), float32 ``[n, NB, 4]`` (p, q, v, cooldown) and, with ``dense`` or an ``out_dense``, float32
        ``[n, 3, NB, NB]`` (bus_connectivity_matrix, flow_bus_matrix active / reactive), else None.  One kernel queued on the engine's stream
        (asynchronous: order the consumer on ``device_views()["stream"]``, or `sync`); it only reads the lanes' current rows.  An output is
        allocated only when none is given; a given one must be a contiguous CUDA tensor of exactly that shape and dtype on the engine's
        device.  ``out``: the three as one tuple ``(index, features, dense or None)`` -- the form `ShardedEngine` takes, one per shard."""
        import torch
        lane0, n = self._range(lane0, n)
        if out is not None:
            if out_index is not None or out_features is not None or out_dense is not None:
                raise TypeError("graph_observation: out is the three outputs as one tuple; give it or the separate ones")
            out_index, out_features, out_dense = out
        shapes = self._graph_shapes(n, dense or out_dense is not None)
        dev = torch.device("cuda", self.device)
        outs, fresh = [], False
        for name, t, shape, dtype in zip(("out_index", "out_features", "out_dense"), (out_index, out_features, out_dense), shapes,
                                         (torch.int32, torch.float32, torch.float32)):
            if shape is None:
                outs.append(None)
                continue
            if t is None:
                t, fresh = torch.empty(shape, dtype=dtype, device=dev), True
            elif not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype == dtype and t.is_contiguous()
                      and tuple(t.shape) == tuple(shape)):
                raise ValueError(f"graph_observation: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on cuda:{self.device}")
            outs.append(t)
        if fresh:
            torch.cuda.current_stream(dev).synchronize()      # (a fresh allocation may still be in use by work queued on torch's stream)
        ip, fp, dp = (None if t is None else C.cast(t.data_ptr(), C.POINTER(ct)) for t, ct in zip(outs, (C.c_int32, C.c_float, C.c_float)))
        self._call("gpf_graph_obs", lane0, n, ip, fp, dp)
        return tuple(outs)

    def graph_observation_host(self, lane0: int = 0, n: Optional[int] = None, dense: bool = False) -> dict:
        """`graph_observation` copied to the host (synchronous): ``{"index", "features", "dense"}`` numpy arrays (``dense`` None without it)."""
        lane0, n = self._range(lane0, n)
        si, sf, sd = self._graph_shapes(n, dense)
        idx, feat, dn = np.empty(si, np.int32), np.empty(sf, np.float32), np.empty(sd, np.float32) if dense else None
        self._call("gpf_graph_obs_host", lane0, n, _ptr(idx), _ptr(feat), _ptr(dn))
        return {"index": idx, "features": feat, "dense": dn}

    def set_overflow_count(self, counts, lane0: int = 0):
        """The protection counters (consecutive steps above the thermal limit, ``obs.timestep_overflow``) of lanes
        ``lane0 ...``: ``[n, n_line]`` ints."""
        self._set_rows("gpf_set_overflow_count", counts, self.model.n_line, np.int32, lane0)

    def cooldown(self, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The environment's line cooldowns of the lanes (obs.time_before_cooldown_line; `step(nb_ts_reco=...)`), int32 ``[n, n_line]``."""
        return self._get_rows("gpf_get_cooldown", lane0, n, (self.model.n_line, np.int32))

    def set_cooldown(self, line_cooldown, lane0: int = 0):
        """Restore the line cooldowns (an environment restored from an observation hands over obs.time_before_cooldown_line)."""
        self._set_rows("gpf_set_cooldown", line_cooldown, self.model.n_line, np.int32, lane0)

    def trajectory_cooldown(self, n_steps: int, step0: int = 0, lane0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Line cooldowns after every step of the last multi-step launch, int16 ``[n_steps, n, n_line]`` (needs `set_trajectory`)."""
        lane0, n = self._range(lane0, n)
        out = np.empty((n_steps, n, self.model.n_line), dtype=np.int16)
        self._call("gpf_get_trajectory_cooldown", int(step0), int(n_steps), lane0, n, _ptr(out))
        return out

    def step_outputs(self, lane0: int = 0, n: Optional[int] = None):
        nl = self.model.n_line
        return tuple(self._get_rows("gpf_get_step_outputs", lane0, n, (nl, np.float32), (nl, np.int32), (nl, np.int32)))

    # ---- measurement -------------------------------------------------------------------------------------
    # ---- DC sensitivity (PTDF) path: fixed topology, flows = PTDF * P_bus as one FP64 MFMA GEMM ----------------------
    def ptdf_build(self, lane: int = 0):
        """Factorise the DC system of the topology currently held by ``lane`` (once per topology)."""
        self._call("gpf_ptdf_build", int(lane))

    def ptdf_build_batch(self, lane0: int = 0, n: Optional[int] = None, with_lodf: bool = True, info: bool = True) -> dict:
        """PTDF (and LODF) tables of EVERY distinct topology the lanes ``[lane0, lane0 + n)`` hold right now, built on the device in
        one launch (gpf_ptdf_build_batch: one workgroup per topology class, blocked Gauss-Jordan on the FP64 matrix cores).  Afterwards
        `ptdf_flows` / `ptdf_flows_rows` / `lodf_screen` evaluate every lane against the tables of its own class.  Returns
        ``lane_class`` [n], ``class_status`` [n_classes] (0 ok, 1 singular, 2 islanded, 3 no slack: the lanes of such a class get NaN
        flows), ``class_n`` (dimension of each reduced B'), ``kernel_ms``."""
        lane0, n = self._range(lane0, n)
        nc = C.c_int32(0)
        self._call("gpf_ptdf_build_batch", lane0, n, 1 if with_lodf else 0, C.byref(nc))
        if not info:                                        # asynchronous: the build kernel is queued, nobody waits (`ptdf_batch_info()` later)
            return {"n_classes": int(nc.value)}
        return self.ptdf_batch_info(n, nc.value)

    def ptdf_batch_info(self, n: Optional[int] = None, n_classes: Optional[int] = None) -> dict:
        """Lane -> class map, class status / dimension and the kernel time of the last `ptdf_build_batch` (waits for its kernel)."""
        if n is None or n_classes is None:
            raise ValueError("ptdf_batch_info: pass the lane count and the class count of the build call")
        nc = C.c_int32(int(n_classes))
        lc, st, cn = np.empty(n, np.int32), np.empty(nc.value, np.int32), np.empty(nc.value, np.int32)
        ms = C.c_double(0.0)
        self._call("gpf_ptdf_batch_info", _ptr(lc), _ptr(st), _ptr(cn), C.byref(ms))
        return {"n_classes": int(nc.value), "lane_class": lc, "class_status": st, "class_n": cn, "kernel_ms": float(ms.value)}

    def ptdf_class(self, cls: int, lodf: bool = False):
        """PTDF [n_line, n_sub * n_busbar] of topology class ``cls`` of the last `ptdf_build_batch` (and its LODF [n_line, n_line])."""
        out = np.empty((self.model.n_line, self.nb_total), dtype=np.float64)
        lo = np.empty((self.model.n_line, self.model.n_line), dtype=np.float64) if lodf else None
        self._call("gpf_ptdf_batch_get", int(cls), _ptr(out), _ptr(lo))
        return (out, lo) if lodf else out

    def ptdf(self) -> np.ndarray:
        """PTDF [n_line, n_sub * n_busbar] (MW of origin-side flow per MW injected at the bus, slack-referenced)."""
        out = np.empty((self.model.n_line, self.nb_total), dtype=np.float64)
        self._call("gpf_ptdf_get", _ptr(out))
        return out

    def ptdf_flows(self, lane0: int = 0, n: Optional[int] = None, fetch: bool = True) -> Optional[np.ndarray]:
        """DC active-power flows (MW, float32 [n, n_line]) of the lanes' current injection rows (asynchronous launch;
        ``fetch=False`` leaves the result on the device)."""
        lane0, n = self._range(lane0, n)
        self._call("gpf_ptdf_flows", lane0, n)
        if not fetch:
            return None
        out = np.empty((n, self.model.n_line), dtype=np.float32)
        self._call("gpf_get_ptdf_flows", lane0, n, _ptr(out))
        return out

    def ptdf_flows_rows(self, t0: int, n_rows: int, rebalance: float = 0.0, fetch: bool = True, lane0: int = 0, n: Optional[int] = None):
        """DC active-power flows of ``n_rows`` consecutive chronics rows of EVERY lane in ONE launch (the GEMM has
        ``n_lanes * n_rows`` rows): row ``j`` of lane ``k`` is chronics row ``(t0 + j + lane_offset[k]) mod T`` turned into injections
        as `step` does.  Returns float32 ``[n_rows, n, n_line]`` (MW at the origin side) of lanes ``[lane0, lane0 + n)``, or None with
        ``fetch=False`` (asynchronous)."""
        self._call("gpf_ptdf_flows_rows", int(t0), int(n_rows), float(rebalance))
        if not fetch:
            return None
        lane0, n = self._range(lane0, n)
        out = np.empty((n_rows, n, self.model.n_line), dtype=np.float32)
        self._call("gpf_get_ptdf_flows_rows", 0, int(n_rows), lane0, n, _ptr(out))
        return out

    def lodf_screen(self, lane0: int = 0, n: Optional[int] = None, cap_mw: Optional[np.ndarray] = None) -> np.ndarray:
        """DC N-1 screening from the flows of the last ``ptdf_flows``: [n, n_line] largest post-outage loading
        max_l |f_l + LODF[l, k] f_k| / cap_mw[l] for every single-line outage k (MW if ``cap_mw`` is None; inf: the
        outage islands the grid)."""
        lane0, n = self._range(lane0, n)
        out = np.empty((n, self.model.n_line), dtype=np.float32)
        cap = None if cap_mw is None else np.ascontiguousarray(cap_mw, dtype=np.float32)
        self._call("gpf_lodf_screen", lane0, n, _ptr(cap), _ptr(out))
        return out

    def sync(self):
        self._call("gpf_sync")

    def set_profiling(self, mode):
        """0/False: off; 1/True: one HIP event pair around the window of launches up to the next ``kernel_time()``;
        2: an event pair per launch (exact per-kernel durations, costs ~7 us of stream time per launch); 3 (inside a window): the
        window ends at this point of the stream (recorded asynchronously behind the launches issued so far)."""
        self._call("gpf_set_profiling", int(mode))

    def kernel_time(self) -> Tuple[float, int]:
        ms = C.c_double(0.0)
        n = C.c_int64(0)
        self._call("gpf_get_kernel_time", C.byref(ms), C.byref(n))
        return ms.value, n.value

    def specialize(self, enable: bool = True, cache_dir: str = None, verify: bool = True, features: bool = True) -> dict:
        """Switch the engine's solver launches (`step`, `simulate_batch`, `runpf`, `solve_lane`) to kernels compiled AT RUN TIME FOR THIS GRID
        (gpf_jit_enable): every size and table offset of the grid is a literal in them instead of a value read from the
        launch parameter block.  The first launch of each kernel variant compiles it (hipcc, about a second; cached on disk per
        grid in ``cache_dir`` / $GRIDPF_JIT_CACHE / ``grid2op_amd/_jit_cache``); results are bit-identical to the shipped kernels.
        ``verify`` (default): before this engine is switched, a 64-lane twin engine of the same grid runs two 8-step launches
        (synthetic chronics around the grid's own injections, load jitter, generation rebalancing) and an AC + a DC `runpf` with the
        shipped and with the specialised kernels, and every result must agree bit for bit -- a specialised kernel is a new binary, and a binary
        is only trusted after it reproduced the validated one; on a mismatch the engine keeps the shipped kernels and
        `GridPFError` is raised.  Raises `GridPFError` too when no hipcc is available (shipped kernels stay).
        ``features`` (default on): a step launch first looks for a kernel compiled for its LAUNCH FEATURES as well -- which of cascade,
        auto-reset, cooldowns, outage tables, kept state, lane lists, trajectory ... the launch uses at all (`feature_word`) -- then for the
        grid-only kernel.  At most 4 feature words per kernel variant and engine are compiled at run time (further words run on the grid-only
        kernel; kernels built ahead of time do not count); without a compiler a missing feature kernel is silently the grid-only one.
        ``features=False``: grid-only kernels.  The self-test runs its launches both ways."""
        self._call("gpf_jit_features", int(bool(features)))
        if not enable:
            self._call("gpf_jit_disable")
            return self.specialization()
        if verify:
            self._verify_specialization(cache_dir)
        # (the kernel sources beside this package; $GRIDPF_JIT_SRC: those of another build -- same-box A/B runs of a library selected with $GRIDPF_LIB)
        src = (os.environ.get("GRIDPF_JIT_SRC") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")).encode()
        self._call("gpf_jit_enable", src, cache_dir.encode() if cache_dir else None)
        return self.specialization()

    def _verify_specialization(self, cache_dir=None, n_lanes: int = 64, n_steps: int = 8, T: int = 24):
        twin = PowerFlowEngine(self.model, n_lanes=n_lanes, device=self.device, n_busbar=self.n_busbar)
        try:
            sl, inj = twin.inj_slices, twin.init_inj
            m = self.model
            w = 1.0 + 0.04 * np.sin(0.7 * np.arange(T))[:, None]
            load_p = inj[sl["load_p"]][None, :] * w
            load_q = inj[sl["load_q"]][None, :] * w
            prod_p = inj[sl["gen_p"]][None, :] * w
            prod_v = np.tile((inj[sl["gen_vm"]] * m.sub_vn_kv[m.gen_sub])[None, :], (T, 1))
            twin.upload_chronics(twin.pack_chronics(load_p, load_q, prod_p, prod_v))
            rng = np.random.default_rng(0)
            twin.set_lane_chronics(lane_offset=(5 * np.arange(n_lanes) % T).astype(np.int32),
                                   lane_scale=(1.0 + 0.03 * rng.standard_normal((n_lanes, 2 * m.n_load))).astype(np.float32))

            def run():
                twin.reset()
                twin.set_trajectory(n_steps, twin.TRAJ_OBS)
                got = []
                for k in range(2):
                    twin.step(k * n_steps, n_steps=n_steps, rebalance=1.02, auto_reset=True)
                    r = twin.results()
                    got += [r.out, r.topo_vect, r.status, r.bus_vm, r.bus_va] + [x.out for x in twin.trajectory_obs(n_steps)]
                twin.runpf()                                        # the one-power-flow-per-lane kernels (runpf / solve_lane), AC and DC
                r = twin.results()
                got += [r.out, r.status, r.bus_vm, r.bus_va]
                twin.runpf(is_dc=True)
                got += [twin.results().out]
                return got

            ref = run()
            src = (os.environ.get("GRIDPF_JIT_SRC") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")).encode()
            twin._call("gpf_jit_features", 0)            # the grid-only kernels ...
            twin._call("gpf_jit_enable", src, cache_dir.encode() if cache_dir else None)
            got = run()
            twin._call("gpf_jit_features", 1)            # ... and the same launches under their feature kernels
            got += run()
            ref = ref + ref
            info = twin.specialization()
            if info["launches"] == 0:
                raise GridPFError(f"specialised kernels could not be built for this grid ({info['variants']}): the shipped kernels stay")
            bad = [i for i, (a, b) in enumerate(zip(ref, got)) if not np.array_equal(a, b, equal_nan=True)]
            if bad:
                raise GridPFError(f"specialised kernels {info['variants']} do NOT reproduce the shipped kernels on the {n_lanes}-lane self-test "
                                  f"({len(bad)} of {len(ref)} result arrays differ): the shipped kernels stay")
        finally:
            twin.close()

    def specialization(self) -> dict:
        """State of the run-time specialised kernels (gpf_jit_info): enabled, variants compiled / taken from the cache / failed,
        launches that went through them, seconds spent compiling + loading, the variants' template arguments."""
        counts = (C.c_int64 * 6)()
        sec = C.c_double()
        text = C.create_string_buffer(2048)
        self._call("gpf_jit_info", counts, C.byref(sec), text, len(text))
        return {"enabled": bool(counts[0]), "compiled": int(counts[1]), "cached": int(counts[2]), "failed": int(counts[3]),
                "launches": int(counts[4]), "aot": int(counts[5]), "seconds": float(sec.value), "variants": text.value.decode()}

    def feature_word(self, n_steps: int = 1, lane_scale: bool = False, outages: bool = False, gen_delta: bool = False,
                     trajectory_obs: bool = False, **step_kw) -> int:
        """The launch-feature word (gpf_jit_feature_word) of ``step(t, n_steps=n_steps, **step_kw)`` on this engine as it stands, plus the
        optional inputs the flags say the launch will have (a header-only engine has none of its own): what names the feature kernel of that
        launch in `specialization()["variants"]` and in ``grid2op_amd/aot/manifest.json``.  Needs no device."""
        kw = dict(max_iter=10, tol_mva=1e-8, rebalance=0.0, cascade=False, hard_overflow=2.0, soft_overflow=1.0, nb_ts_allowed=2, max_rounds=16,
                  is_dc=False, auto_reset=False, warm_start=False, nb_ts_reco=None)
        kw.update(step_kw)
        reco = kw["nb_ts_reco"]
        if reco is None:
            reco = 10 if (kw["cascade"] or outages or self._has_outages) else -1
        o = GpfStepOpts(int(kw["max_iter"]), float(kw["tol_mva"]), float(kw["rebalance"]), int(bool(kw["cascade"])), float(kw["hard_overflow"]),
                        float(kw["soft_overflow"]), int(kw["nb_ts_allowed"]), int(kw["max_rounds"]), int(bool(kw["is_dc"])), int(bool(kw["auto_reset"])),
                        int(bool(kw["warm_start"])), int(reco >= 0), max(int(reco), 0))
        have = (1 if lane_scale else 0) | (4 if outages else 0) | (8 if gen_delta else 0) | (16 if trajectory_obs else 0)     # GPF_HAVE_*
        word = C.c_uint32(0)
        self._call("gpf_jit_feature_word", int(n_steps), C.byref(o), have, C.byref(word))
        return int(word.value)

    def specialization_header(self) -> str:
        """The generated header the specialised kernels are compiled with (gpf_jit_source): this grid's numbers as C literals."""
        need = C.c_size_t()
        self._call("gpf_jit_source", None, 0, C.byref(need))
        buf = C.create_string_buffer(need.value + 1)
        self._call("gpf_jit_source", buf, len(buf), None)
        return buf.value.decode()

    def counters(self) -> dict:
        """Step launches issued since the engine was created and the kernel dispatches they took (a batch of a few residency rounds goes
        out as one dispatch per round)."""
        out = (C.c_int64 * 2)()
        self._call("gpf_get_counters", out)
        return {"step_launches": int(out[0]), "kernel_dispatches": int(out[1])}

    def plan(self) -> dict:
        """Diagnostics: the kernel configuration a launch over all lanes would use right now (gpf_get_plan)."""
        out = (C.c_int32 * 8)()
        self._call("gpf_get_plan", out)
        keys = ("busbars_per_block", "instances_per_wavefront", "wavefronts_per_instance", "staging_tier", "ybus_in_registers",
                "dc_factors_kept", "lds_bytes", "topology_classes")
        return dict(zip(keys, [int(v) for v in out]))

    def algorithmic_bytes_per_step(self) -> int:
        """inputs at API dtype + outputs at API dtype, topology unchanged."""
        m = self.model
        bytes_in = 4 * (2 * m.n_load + 2 * m.n_gen + m.n_storage)
        bytes_out = 4 * (8 * m.n_line + 3 * m.n_gen + 3 * m.n_load + 3 * m.n_storage
                         + (2 * m.n_line + m.n_load + m.n_gen + m.n_storage) + 4 * m.n_shunt) + 4 * m.dim_topo + m.n_line
        return bytes_in + bytes_out
