"""TEST INFRASTRUCTURE: numpy restatement of the observation vector the engine assembles on the device (grid2op_amd/obs_spec.py,
grid2op_amd/csrc/gridpf_obs.hpp) -- `compose` -- and of the derived attributes, written from the reference's definitions:

* calendar: ``datetime`` arithmetic (``env.time_stamp``; ``day_of_week`` = ``weekday()``), Observation/baseObservation.py:4464-4480;
* generator margins: baseObservation.py:4393-4410, in float32;
* maintenance look-ahead: ``GridValue.get_maintenance_time_1d`` / ``get_maintenance_duration_1d``, Chronics/gridValue.py:264-410;
* game over: ``BaseObservation.set_game_over``, baseObservation.py:1551-1700.

`engine_state` collects the inputs of `compose` from the engine's existing getters."""
import datetime as dt

import numpy as np

from grid2op_amd.obs_spec import GO_KEEP, GO_MINUS1, GO_ONE, KIND, _OUT_ATTR

CALENDAR = ("year", "month", "day", "hour_of_day", "minute_of_hour", "day_of_week")


def calendar(start, step_minutes, rows):
    """``[len(rows), 6]`` int: year, month, day, hour, minute, weekday of ``start + rows * step_minutes``."""
    out = np.empty((len(rows), 6), dtype=np.int64)
    for i, r in enumerate(rows):
        t = start + dt.timedelta(minutes=int(step_minutes) * int(r))
        out[i] = (t.year, t.month, t.day, t.hour, t.minute, t.weekday())
    return out


def margins(gen_p, pmin, pmax, ramp_up, ramp_down, renewable):
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)  # noqa: E731
    gen_p = np.asarray(gen_p, dtype=np.float32)
    ren = np.asarray(renewable, dtype=bool) if renewable is not None else np.zeros(gen_p.shape[-1], dtype=bool)
    with np.errstate(invalid="ignore"):
        up = np.minimum(f32(pmax) - gen_p, f32(ramp_up))
        down = np.minimum(gen_p - f32(pmin), f32(ramp_down))
        up[..., ren] = 0.0
        down[..., ren] = 0.0
        up[up < 0.0] = 0.0
        down[down < 0.0] = 0.0
    return up, down


def maintenance_lookahead(maintenance):
    """(time_next_maintenance, duration_next_maintenance), each ``[T, n_line]`` int32, of a ``[T, n_line]`` 0/1 table: per column the
    reference's two scans (a diff of the column padded with two zeros gives the starts and ends of the outages)."""
    m = np.asarray(maintenance).astype(np.int64)
    T, nl = m.shape
    nxt = np.full((T, nl), -1, dtype=np.int32)
    dur = np.zeros((T, nl), dtype=np.int32)
    for l in range(nl):
        a = np.diff(np.concatenate((m[:, l], (0, 0))))
        start = (a == 1).nonzero()[0] + 1
        end = (a == -1).nonzero()[0] + 1
        if m[0, l]:                                         # (an outage at row 0 has no rising edge in the diff: the reference's own
            start = np.concatenate(([0], start))             #  tables never start inside one; the engine counts it as under way)
        prev = 0
        for b, e in zip(start, end):
            nxt[prev:b, l] = np.arange(b - prev, 0, -1)
            nxt[b:e, l] = 0
            dur[prev:b, l] = e - b
            dur[b:e, l] = np.arange(e - b, 0, -1)
            prev = e
    return nxt, dur


def compose(spec, state, game_over_fill=True):
    """float32 ``[n, spec.dim]``: every attribute of the spec from ``state[name]`` (``[n, size]``, any dtype; const entries from the
    spec) cast to float32, game-over rows (``state["done"]``) replaced, then ``(x - subtract) / divide`` in float32 where either is
    not the default."""
    n = len(np.asarray(state["done"]))
    done = np.asarray(state["done"], dtype=bool) if game_over_fill else np.zeros(n, dtype=bool)
    vec = np.empty((n, spec.dim), dtype=np.float32)
    for name, (kind, src, size, d0, go) in zip(spec.names, spec.segments.tolist()):
        if kind == KIND["const"]:
            x = np.full((n, size), np.int32(src).view(np.float32), dtype=np.float32)
        else:
            x = np.asarray(state[name]).reshape(n, size).astype(np.float32)
        go &= 3
        if go != GO_KEEP and done.any():
            x = x.copy()
            x[done] = -1.0 if go == GO_MINUS1 else 1.0 if go == GO_ONE else 0.0
        sl = slice(d0, d0 + size)
        sub, div = spec.subtract[sl], spec.divide[sl]
        if np.any(sub != 0.0) or np.any(div != 1.0):
            with np.errstate(invalid="ignore", over="ignore"):
                x = (x - sub[None, :]) / div[None, :]
        vec[:, sl] = x
    return vec


def engine_state(eng, spec, clock=None, gen_limits=None, renewable=None, maintenance=None, lane_table=None, lane_offset=None, t=0,
                 lane0=0, n=None, acting=False):
    """The inputs of `compose` for lanes ``[lane0, lane0 + n)`` from the engine's getters.  ``clock`` = (list of start datetimes,
    step_minutes, max_step); ``gen_limits`` = (pmin, pmax, ramp_up, ramp_down) or None; ``maintenance``: the uploaded
    ``[n_tables, T, n_line]`` table or None; ``t``: time index of the lanes' last step; ``acting``: the topology acting path is
    enabled (the substation cooldowns exist; asking for them would enable it)."""
    m = eng.model
    n = eng.n_lanes - lane0 if n is None else n
    r = eng.results(lane0, n, with_bus=False)
    rho, ovc, _ = eng.step_outputs(lane0, n)
    done, steps, _ = eng.episode(lane0, n)
    st = {"done": done, "rho": rho, "timestep_overflow": ovc, "timestep_protection_engaged": ovc, "line_status": r.line_status, "topo_vect": r.topo_vect,
          "_shunt_bus": r.shunt_bus, "time_before_cooldown_line": eng.cooldown(lane0, n),
          "current_step": (steps + done.astype(steps.dtype))[:, None]}
    for attr, field in _OUT_ATTR.items():
        st[attr] = r.out[:, eng.out_slices[field]]
    st["time_before_cooldown_sub"] = eng.sub_cooldown(lane0, n) if acting else np.zeros((n, m.n_sub), dtype=np.int32)
    if getattr(eng, "env_dynamics_on", False):
        es = eng.env_state(lane0, n)
        st.update(target_dispatch=es["target"], actual_dispatch=es["actual"], storage_charge=es["charge"], curtailment_limit=es["curtail_limit"])
    else:
        st.update(target_dispatch=np.zeros((n, m.n_gen), np.float32), actual_dispatch=np.zeros((n, m.n_gen), np.float32),
                  storage_charge=np.zeros((n, m.n_storage), np.float32), curtailment_limit=np.ones((n, m.n_gen), np.float32))
    setp = eng.get_injections(lane0, n)[:, eng.inj_slices["gen_p"]].astype(np.float32)
    ren = np.zeros(m.n_gen, dtype=bool) if renewable is None else np.asarray(renewable, dtype=bool)
    st["gen_p_before_curtail"] = np.where(ren[None, :], setp, np.float32(0.0))
    with np.errstate(invalid="ignore"):
        st["gen_p_delta"] = np.asarray(st["gen_p"], dtype=np.float32) - setp
    if gen_limits is not None:
        st["gen_margin_up"], st["gen_margin_down"] = margins(st["gen_p"], *gen_limits, renewable)
    else:
        st["gen_margin_up"] = st["gen_margin_down"] = np.zeros((n, m.n_gen), np.float32)
    T = getattr(eng, "chron_T", 0)
    tab = np.zeros(n, dtype=np.int64) if lane_table is None else np.asarray(lane_table)[lane0:lane0 + n]
    off = np.zeros(n, dtype=np.int64) if lane_offset is None else np.asarray(lane_offset)[lane0:lane0 + n]
    rows = (int(t) + off) % T if T else np.zeros(n, dtype=np.int64)
    if clock is not None:
        starts, step_minutes, max_step = clock
        cal = np.stack([calendar(starts[int(k)], step_minutes, [rw])[0] for k, rw in zip(tab, rows)])
        for i, name in enumerate(CALENDAR):
            st[name] = cal[:, i:i + 1]
        st["max_step"] = np.full((n, 1), max_step)
        st["delta_time"] = np.full((n, 1), step_minutes)
    if maintenance is not None:
        look = [maintenance_lookahead(tb) for tb in np.asarray(maintenance)]
        st["time_next_maintenance"] = np.stack([look[int(k)][0][rw] for k, rw in zip(tab, rows)])
        st["duration_next_maintenance"] = np.stack([look[int(k)][1][rw] for k, rw in zip(tab, rows)])
    else:
        st["time_next_maintenance"] = np.full((n, m.n_line), -1, np.int32)
        st["duration_next_maintenance"] = np.zeros((n, m.n_line), np.int32)
    return st
