"""`ObsSpec`: the layout of the observation vector the engine assembles on the device (no GPU needed to build one).

What a policy reads in the reference is ``obs.to_vect()``: the attributes of ``CompleteObservation.attr_list_vect``
(Observation/completeObservation.py:140-212) concatenated as float32 (Space/GridObjects.py ``to_vect``), usually behind
``gym_compat.BoxGymObsSpace(attr_to_keep, subtract, divide)`` which maps every element to ``(x - subtract) / divide`` in float32.
An `ObsSpec` names the attributes, in any order, and compiles them into the segment table of ``gpf_set_obs_spec`` (include/gridpf.h):
one ``{source kind, source offset, length, destination offset, flags}`` row per attribute plus per-element subtract / divide arrays.

Sources (``PowerFlowEngine.observation_vector``):

* ``gen_p/q/v``, ``load_p/q/v``, ``p/q/v/a_or``, ``p/q/v/a_ex``, ``storage_power``, ``_shunt_p/q/v``: the float32 results row;
* ``rho``, ``timestep_overflow``: the buffers the STEP launches maintain -- `runpf` does NOT refresh them (they keep the values of the
  lane's last step; zeros before any);
* ``timestep_protection_engaged``: the same counter as ``timestep_overflow`` (the engine keeps one protection counter per line; the
  reference's two coincide under its default protection parameters);
* ``line_status``, ``topo_vect``, ``_shunt_bus``: the result rows of the last power flow;
* ``time_before_cooldown_line`` / ``time_before_cooldown_sub``: the cooldown counters (zeros while the engine does not track them);
* ``target_dispatch``, ``actual_dispatch``, ``storage_charge``, ``curtailment_limit``: the state of the injection dynamics
  (zeros, ``curtailment_limit`` 1, while they are off);
* ``gen_margin_up/down``: ``min(pmax - gen_p, ramp_up)`` / ``min(gen_p - pmin, ramp_down)`` in float32, 0 on renewables, clamped at 0
  (baseObservation.py:4393-4410); zeros until `set_gen_limits` was called;
* ``year`` .. ``day_of_week``, ``max_step``, ``delta_time``: the clock of `set_obs_clock` at the chronics row the lane's last step read;
  ``current_step``: the lane's steps survived (+1 on a lane whose last step ended its episode, as ``BaseEnv.nb_time_step`` counts it);
  NOT the reference's on a reset row: the engine has no launch-free observation, a launch at ``t = 0`` that reproduces the reset state
  counts as a step and reads 1 where the reference's reset observation has 0;
* ``time_next_maintenance`` / ``duration_next_maintenance``: ``GridValue.get_maintenance_time_1d`` / ``get_maintenance_duration_1d``
  (Chronics/gridValue.py:264-410) of the uploaded maintenance table at that row; -1 / 0 without a table;
* ``gen_p_before_curtail`` (renewables: the generator set-point the last launch left in the injection row, others 0) and ``gen_p_delta``
  (``gen_p`` minus that set-point: what the slack absorbed) -- the reference's values while no curtailment limit acts on the lane;
  under an acting limit ``gen_p_before_curtail`` shows the CURTAILED set-point: a caller who curtails covers it with a ``const`` entry;
* with ``dim_alerts=A``: ``active_alert``, ``time_since_last_alert``, ``alert_duration``, ``time_since_last_attack``, ``attack_under_alert``,
  ``was_alert_used_after_attack`` (A elements each) and ``total_number_of_alert`` (ONE element): the lanes' alert state
  (`PowerFlowEngine.set_alerts`, which must be on when the spec is set); without the keyword these names are refused as before;
* ``thermal_limit`` (not part of the reference vector; ``BoxGymObsSpace`` keeps it);
* ``("const", size, value)``: a fill -- how a caller covers attributes of features the engine does not model.

`ObsSpec.complete(model, fill=True)` is the full reference layout for an environment without alarms, alerts and detachment, with
``const`` segments at the values the reference gives there (`ATTR_TABLE`)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

__all__ = ["ObsSpec", "ATTR_TABLE", "KIND", "out_offsets"]

# source kinds = GPF_OBS_* of include/gridpf.h
KIND = dict(const=0, out=1, rho=2, line_status=3, topo_vect=4, shunt_bus=5, overflow=6, cooldown_line=7, cooldown_sub=8, target_dispatch=9,
            actual_dispatch=10, storage_charge=11, curtailment_limit=12, margin_up=13, margin_down=14, calendar=15, current_step=16,
            max_step=17, delta_time=18, time_next_maintenance=19, duration_next_maintenance=20, thermal_limit=21, gen_p_before_curtail=22,
            gen_p_delta=23, active_alert=24, time_since_last_alert=25, alert_duration=26, total_number_of_alert=27, time_since_last_attack=28,
            attack_under_alert=29, was_alert_used_after_attack=30)
GO_ZERO, GO_KEEP, GO_MINUS1, GO_ONE = 0, 1, 2, 3       # what a game-over lane writes (BaseObservation.set_game_over, baseObservation.py:1551-1700)
MAX_SEGMENTS = 64

# CompleteObservation.attr_list_vect in order: (name, size rule, dtype class, fill).  `fill` is None for an attribute the engine assembles
# itself; otherwise the value the reference gives in an environment WITHOUT that feature (BaseObservation.reset, baseObservation.py:1576-1700,
# and _update_obs_complete :4464-4540) -- what `complete(fill=True)` writes.  Size rules are keys of `_sizes`; alarm / alert / detachment
# attributes have size 0 in such an environment (the reference drops them from the vector).  tests/golden/obs_attr_list.json is this table.
ATTR_TABLE = [
    ("year", "one", "int", None), ("month", "one", "int", None), ("day", "one", "int", None), ("hour_of_day", "one", "int", None),
    ("minute_of_hour", "one", "int", None), ("day_of_week", "one", "int", None),
    ("gen_p", "n_gen", "float", None), ("gen_q", "n_gen", "float", None), ("gen_v", "n_gen", "float", None),
    ("load_p", "n_load", "float", None), ("load_q", "n_load", "float", None), ("load_v", "n_load", "float", None),
    ("p_or", "n_line", "float", None), ("q_or", "n_line", "float", None), ("v_or", "n_line", "float", None), ("a_or", "n_line", "float", None),
    ("p_ex", "n_line", "float", None), ("q_ex", "n_line", "float", None), ("v_ex", "n_line", "float", None), ("a_ex", "n_line", "float", None),
    ("rho", "n_line", "float", None), ("line_status", "n_line", "bool", None), ("timestep_overflow", "n_line", "int", None),
    ("topo_vect", "dim_topo", "int", None), ("time_before_cooldown_line", "n_line", "int", None),
    ("time_before_cooldown_sub", "n_sub", "int", None), ("time_next_maintenance", "n_line", "int", None),
    ("duration_next_maintenance", "n_line", "int", None), ("target_dispatch", "n_gen", "float", None),
    ("actual_dispatch", "n_gen", "float", None), ("storage_charge", "n_storage", "float", None),
    ("storage_power_target", "n_storage", "float", 0.0), ("storage_power", "n_storage", "float", None),
    ("gen_p_before_curtail", "n_gen", "float", None), ("curtailment", "n_gen", "float", 0.0), ("curtailment_limit", "n_gen", "float", None),
    ("curtailment_limit_effective", "n_gen", "float", 1.0),
    ("is_alarm_illegal", "one", "bool", 0.0), ("time_since_last_alarm", "one", "int", -1.0), ("last_alarm", "dim_alarms", "int", 0.0),
    ("attention_budget", "one", "float", 0.0), ("was_alarm_used_after_game_over", "one", "bool", 0.0),
    ("_shunt_p", "n_shunt", "float", None), ("_shunt_q", "n_shunt", "float", None), ("_shunt_v", "n_shunt", "float", None),
    ("_shunt_bus", "n_shunt", "int", None),
    ("current_step", "one", "int", None), ("max_step", "one", "int", None), ("delta_time", "one", "float", None),
    ("gen_margin_up", "n_gen", "float", None), ("gen_margin_down", "n_gen", "float", None),
    ("active_alert", "dim_alerts", "bool", 0.0), ("attack_under_alert", "dim_alerts", "int", 0.0),
    ("time_since_last_alert", "dim_alerts", "int", 0.0), ("alert_duration", "dim_alerts", "int", 0.0),
    ("total_number_of_alert", "dim_alerts", "int", 0.0), ("time_since_last_attack", "dim_alerts", "int", -1.0),
    ("was_alert_used_after_attack", "dim_alerts", "int", 0.0),
    ("gen_p_delta", "n_gen", "float", None),
    ("load_detached", "detach_n_load", "bool", 0.0), ("gen_detached", "detach_n_gen", "bool", 0.0),
    ("storage_detached", "detach_n_storage", "bool", 0.0), ("load_p_detached", "detach_n_load", "float", 0.0),
    ("load_q_detached", "detach_n_load", "float", 0.0), ("gen_p_detached", "detach_n_gen", "float", 0.0),
    ("storage_p_detached", "detach_n_storage", "float", 0.0),
    ("timestep_protection_engaged", "n_line", "int", None),
]
_EXTRA = [("thermal_limit", "n_line", "float", None)]       # kept by BoxGymObsSpace, not in attr_list_vect

_OUT_ATTR = {"gen_p": "gen_p", "gen_q": "gen_q", "gen_v": "gen_v", "load_p": "load_p", "load_q": "load_q", "load_v": "load_v",
             "p_or": "p_or", "q_or": "q_or", "v_or": "v_or", "a_or": "a_or", "p_ex": "p_ex", "q_ex": "q_ex", "v_ex": "v_ex", "a_ex": "a_ex",
             "storage_power": "storage_p", "_shunt_p": "shunt_p", "_shunt_q": "shunt_q", "_shunt_v": "shunt_v"}
_CALENDAR = ["year", "month", "day", "hour_of_day", "minute_of_hour", "day_of_week"]
# attribute -> (source kind, game-over value)
_DIRECT = {"rho": ("rho", GO_ZERO), "line_status": ("line_status", GO_ZERO), "topo_vect": ("topo_vect", GO_MINUS1),
           "_shunt_bus": ("shunt_bus", GO_MINUS1), "timestep_overflow": ("overflow", GO_ZERO),
           "time_before_cooldown_line": ("cooldown_line", GO_ZERO), "time_before_cooldown_sub": ("cooldown_sub", GO_ZERO),
           "target_dispatch": ("target_dispatch", GO_ZERO), "actual_dispatch": ("actual_dispatch", GO_ZERO),
           "storage_charge": ("storage_charge", GO_ZERO), "curtailment_limit": ("curtailment_limit", GO_ONE),
           "gen_margin_up": ("margin_up", GO_ZERO), "gen_margin_down": ("margin_down", GO_ZERO),
           "current_step": ("current_step", GO_KEEP), "max_step": ("max_step", GO_KEEP), "delta_time": ("delta_time", GO_KEEP),
           "time_next_maintenance": ("time_next_maintenance", GO_MINUS1), "duration_next_maintenance": ("duration_next_maintenance", GO_ZERO),
           "thermal_limit": ("thermal_limit", GO_KEEP), "gen_p_before_curtail": ("gen_p_before_curtail", GO_ZERO),
           "gen_p_delta": ("gen_p_delta", GO_ZERO), "timestep_protection_engaged": ("overflow", GO_ZERO)}


# the alert attributes (``ObsSpec(..., dim_alerts=A)``, `PowerFlowEngine.set_alerts`): attribute -> (source kind, game-over value); a
# game-over observation keeps the environment's attack_under_alert / was_alert_used_after_attack (baseObservation.py:1681-1687).
# ``total_number_of_alert`` has ONE element (baseObservation.py:5142-5143), whatever `ATTR_TABLE`'s size rule for the alert-free layout says.
_ALERT = {"active_alert": ("active_alert", GO_ZERO), "time_since_last_alert": ("time_since_last_alert", GO_ZERO),
          "alert_duration": ("alert_duration", GO_ZERO), "total_number_of_alert": ("total_number_of_alert", GO_ZERO),
          "time_since_last_attack": ("time_since_last_attack", GO_MINUS1), "attack_under_alert": ("attack_under_alert", GO_KEEP),
          "was_alert_used_after_attack": ("was_alert_used_after_attack", GO_KEEP)}
MAX_ALERTS = 64


def _check_dim_alerts(dim_alerts) -> int:
    a = int(dim_alerts)
    if not 0 <= a <= MAX_ALERTS:
        raise ValueError(f"dim_alerts {a} is outside [0, {MAX_ALERTS}]")
    return a


def _sizes(model, dim_alerts: int = 0) -> Dict[str, int]:
    return dict(one=1, n_gen=model.n_gen, n_load=model.n_load, n_line=model.n_line, n_sub=model.n_sub, dim_topo=model.dim_topo,
                n_storage=model.n_storage, n_shunt=model.n_shunt, dim_alarms=0, dim_alerts=dim_alerts, detach_n_load=0, detach_n_gen=0,
                detach_n_storage=0)


def out_offsets(model) -> Dict[str, int]:
    """Column offsets of the engine's float32 results row (``gpf_layout`` of include/gridpf.h, `PowerFlowEngine.out_slices`)."""
    off, k = {}, 0
    for grp, n in ((("p_or", "q_or", "v_or", "a_or", "theta_or", "p_ex", "q_ex", "v_ex", "a_ex", "theta_ex"), model.n_line),
                   (("gen_p", "gen_q", "gen_v", "gen_theta"), model.n_gen), (("load_p", "load_q", "load_v", "load_theta"), model.n_load),
                   (("storage_p", "storage_q", "storage_v", "storage_theta"), model.n_storage),
                   (("shunt_p", "shunt_q", "shunt_v"), model.n_shunt)):
        for name in grp:
            off[name] = k
            k += n
    return off


class ObsSpec:
    """``attrs``: ordered attribute names, or ``("const", size, value)`` fills.  ``subtract`` / ``divide``: name -> scalar or per-element
    array (a const entry is addressed as ``"const<k>"``, k counting the const entries from 0); the value written is
    ``(x - subtract) / divide`` in float32, a plain cast where both are the defaults 0 and 1."""

    def __init__(self, model, attrs: Sequence, subtract: Optional[dict] = None, divide: Optional[dict] = None, dim_alerts: int = 0):
        self.dim_alerts = _check_dim_alerts(dim_alerts)
        sizes = _sizes(model, self.dim_alerts)
        known = {name: rule for name, rule, _, _ in ATTR_TABLE + _EXTRA}
        filled = {name for name, _, _, fill in ATTR_TABLE if fill is not None and not (self.dim_alerts > 0 and name in _ALERT)}
        oo = out_offsets(model)
        self.model = model
        self.attrs: List = []
        self.names: List[str] = []
        self.offsets: Dict[str, slice] = {}
        segs = []
        pos, n_const = 0, 0
        for a in attrs:
            if isinstance(a, (tuple, list)):
                if len(a) != 3 or a[0] != "const":
                    raise ValueError(f"observation attribute {a!r}: a tuple entry must be ('const', size, value)")
                size, value = int(a[1]), float(a[2])
                if size <= 0:
                    raise ValueError(f"observation attribute {a!r}: the size of a const entry must be positive")
                name = f"const{n_const}"
                n_const += 1
                kind, src, go = KIND["const"], int(np.float32(value).view(np.int32)), GO_KEEP
            else:
                name = str(a)
                if name not in known or name in filled:
                    raise ValueError(f"observation attribute {name!r} is not assembled by the engine"
                                     + (" (a feature it does not model)" if name in filled else "")
                                     + ": cover it with a ('const', size, value) entry")
                if name in self.offsets:
                    raise ValueError(f"observation attribute {name!r} is listed twice")
                size = 1 if name == "total_number_of_alert" and self.dim_alerts > 0 else sizes[known[name]]
                if size == 0:
                    raise ValueError(f"observation attribute {name!r} has no element on this grid")
                if name in _OUT_ATTR:
                    kind, src, go = KIND["out"], oo[_OUT_ATTR[name]], GO_ZERO
                elif name in _CALENDAR:
                    kind, src, go = KIND["calendar"], _CALENDAR.index(name), GO_KEEP
                elif name in _ALERT:
                    kind, src, go = KIND[_ALERT[name][0]], 0, _ALERT[name][1]
                else:
                    kind, src, go = KIND[_DIRECT[name][0]], 0, _DIRECT[name][1]
            self.attrs.append(a if not isinstance(a, list) else tuple(a))
            self.names.append(name)
            self.offsets[name] = slice(pos, pos + size)
            segs.append((kind, src, size, pos, go))
            pos += size
        if not segs:
            raise ValueError("an observation spec needs at least one attribute")
        if len(segs) > MAX_SEGMENTS:
            raise ValueError(f"an observation spec holds at most {MAX_SEGMENTS} entries ({len(segs)} given)")
        self.dim = pos
        self.segments = np.asarray(segs, dtype=np.int32).reshape(-1, 5)
        self.subtract = self._per_element(subtract, 0.0, "subtract")
        self.divide = self._per_element(divide, 1.0, "divide")
        if np.any(self.divide == 0.0):
            bad = [n for n in self.names if np.any(self.divide[self.offsets[n]] == 0.0)]
            raise ValueError(f"divide is zero for {bad}")
        check_segments(self.segments, self.dim)

    def _per_element(self, d, default, what):
        out = np.full(self.dim, default, dtype=np.float32)
        for name, v in (d or {}).items():
            if name not in self.offsets:
                raise ValueError(f"{what}: {name!r} is not an attribute of this spec")
            sl = self.offsets[name]
            v = np.asarray(v, dtype=np.float32)
            if v.ndim > 1 or (v.ndim == 1 and v.size != sl.stop - sl.start):
                raise ValueError(f"{what}[{name!r}]: a scalar or {sl.stop - sl.start} values are needed, got shape {v.shape}")
            if not np.all(np.isfinite(v)):
                raise ValueError(f"{what}[{name!r}] is not finite")
            out[sl] = v
        return out

    @classmethod
    def complete(cls, model, fill: bool = False, subtract=None, divide=None, dim_alerts: int = 0) -> "ObsSpec":
        """The reference's ``CompleteObservation.attr_list_vect`` order.  ``fill=False``: the attributes the engine assembles;
        ``fill=True``: the reference's full layout, the others as ``const`` entries at the reference's values (`ATTR_TABLE`).
        ``dim_alerts=A`` (an environment with A alertable lines, `PowerFlowEngine.set_alerts`): the seven alert attributes at their
        positions, assembled by the engine."""
        dim_alerts = _check_dim_alerts(dim_alerts)
        sizes = _sizes(model, dim_alerts)
        attrs = []
        for name, rule, _, fillv in ATTR_TABLE:
            if sizes[rule] == 0:
                continue
            if fillv is None or (dim_alerts > 0 and name in _ALERT):
                attrs.append(name)
            elif fill:
                if attrs and isinstance(attrs[-1], tuple) and attrs[-1][2] == fillv:      # neighbours with one value: one segment
                    attrs[-1] = ("const", attrs[-1][1] + sizes[rule], fillv)
                else:
                    attrs.append(("const", sizes[rule], fillv))
        return cls(model, attrs, subtract, divide, dim_alerts=dim_alerts)


def check_segments(segments, dim):
    """The destination ranges must tile ``[0, dim)``: no overlap, no gap (what ``gpf_set_obs_spec`` verifies again on its side)."""
    seg = np.asarray(segments, dtype=np.int64).reshape(-1, 5)
    cover = np.zeros(int(dim), dtype=np.int32)
    for kind, _, length, d0, _ in seg:
        if length <= 0 or d0 < 0 or d0 + length > dim:
            raise ValueError(f"observation segment (kind {kind}) writes [{d0}, {d0 + length}) outside [0, {dim})")
        cover[d0:d0 + length] += 1
    if np.any(cover > 1):
        raise ValueError(f"observation segments overlap at element {int(np.argmax(cover > 1))}")
    if np.any(cover == 0):
        raise ValueError(f"observation segments leave a gap at element {int(np.argmax(cover == 0))}")
