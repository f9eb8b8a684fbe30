"""Plain-numpy statement of what `gpf_ptdf_flows_rows` computes: the DC flows of `n_rows` consecutive chronics rows of every lane.

For pair (row j, lane k) the injections follow the rule of the step kernel's chronics phase (gridpf_sparse.hpp, the block marked K9;
Environment/baseEnv.py:2516-2563 feeds float32 vectors, pandaPowerBackend.py:927), with its float32 roundings at the same places:

  1. table `lane_table[k]`, row `(t0 + j + lane_offset[k]) mod T` (a non-negative remainder, also for a negative sum);
  2. loads: float32(load_p * scale);
  3. sp = float32(rebalance * sum_load / sum_prod), both sums in float64 over the float32 values, sum_prod over the non-slack
     generators; sp = 1 when rebalance <= 0 or sum_prod <= 0;
  4. non-slack generators: float32(float32(prod_p * sp) + delta);
  5. storage and shunt set-points: the lane's own injection row.

The flows are `oracle.pf_oracle.ptdf(m, state) @ oracle.pf_oracle.dc_bus_injection(m, state)` on lane k's own topology; a lane whose
topology the oracle's DC power flow rejects (islanded, no slack) gets all-NaN rows.  Nothing of the kernel under test is in this file.

Injection rows are float64 `[n_inj]` in the layout of include/gridpf.h:
gen_p | gen_vm | load_p | load_q | storage_p | storage_q | shunt_p | shunt_q."""
import numpy as np

from oracle.pf_oracle import LaneState, dc_bus_injection, ptdf, solve


def inj_offsets(m):
    """Start of every field of an injection row."""
    o, k = {}, 0
    for name, n in (("gen_p", m.n_gen), ("gen_vm", m.n_gen), ("load_p", m.n_load), ("load_q", m.n_load), ("storage_p", m.n_storage),
                    ("storage_q", m.n_storage), ("shunt_p", m.n_shunt), ("shunt_q", m.n_shunt)):
        o[name] = k
        k += n
    o["n_inj"] = k
    return o


def _per_lane(a, n_lanes, width, dtype):
    if a is None:
        return None
    a = np.asarray(a, dtype=dtype)
    return np.broadcast_to(a, (n_lanes, width)) if a.ndim == 1 else a


def rows_injections(m, inj_row, tables, lane_table, lane_offset, lane_scale, gen_delta, t0, n_rows, rebalance):
    """Injection rows float64 `[n_rows, n_lanes, n_inj]` of every pair: rules 1-5 above (load_q, gen_vm as the lane's row holds them:
    the DC flows do not depend on them)."""
    inj_row = np.asarray(inj_row, dtype=np.float64)
    n_lanes = inj_row.shape[0]
    tables = np.asarray(tables, dtype=np.float32)
    if tables.ndim == 2:
        tables = tables[None]
    T = tables.shape[1]
    nl, ng = m.n_load, m.n_gen
    o = inj_offsets(m)
    lane_table = np.zeros(n_lanes, np.int64) if lane_table is None else np.asarray(lane_table, dtype=np.int64)
    lane_offset = np.zeros(n_lanes, np.int64) if lane_offset is None else np.asarray(lane_offset, dtype=np.int64)
    scale = _per_lane(lane_scale, n_lanes, 2 * nl, np.float32)
    delta = _per_lane(gen_delta, n_lanes, ng, np.float32)
    ns = ~np.asarray(m.gen_slack, dtype=bool)
    out = np.empty((n_rows, n_lanes, o["n_inj"]))
    for j in range(n_rows):
        for k in range(n_lanes):
            row = tables[lane_table[k], (int(t0) + j + int(lane_offset[k])) % T]
            lp = row[:nl].astype(np.float32)
            if scale is not None:
                lp = (lp * scale[k, :nl]).astype(np.float32)
            pp = row[2 * nl:2 * nl + ng].astype(np.float32)
            sum_load = lp.astype(np.float64).sum()
            sum_prod = pp[ns].astype(np.float64).sum()
            sp = np.float32(rebalance * sum_load / sum_prod) if (rebalance > 0 and sum_prod > 0) else np.float32(1.0)
            gp = pp.copy()
            gp[ns] = (pp[ns] * sp).astype(np.float32)
            if delta is not None:
                gp[ns] = (gp[ns] + delta[k, ns]).astype(np.float32)
            x = inj_row[k].copy()
            x[o["load_p"]:o["load_p"] + nl] = lp
            x[o["gen_p"]:o["gen_p"] + ng] = gp
            out[j, k] = x
    return out


def lane_state(m, x, topo, shunt_bus):
    """LaneState of one injection row on one topology."""
    o = inj_offsets(m)
    st = LaneState.from_model(m)
    st.topo = np.asarray(topo).copy()
    if m.n_shunt and shunt_bus is not None:
        st.shunt_bus = np.asarray(shunt_bus).copy()
    for f, n in (("gen_p", m.n_gen), ("gen_vm", m.n_gen), ("load_p", m.n_load), ("load_q", m.n_load), ("storage_p", m.n_storage),
                 ("storage_q", m.n_storage), ("shunt_p", m.n_shunt), ("shunt_q", m.n_shunt)):
        setattr(st, f, np.asarray(x[o[f]:o[f] + n], dtype=np.float64).copy())
    return st


def rows_reference(m, topo, shunt_bus, inj_row, tables, lane_table, lane_offset, lane_scale, gen_delta, t0, n_rows, rebalance):
    """float64 `[n_rows, n_lanes, n_line]`: DC flows (MW, origin side) of every (row, lane) pair on the lane's own topology.
    `topo` `[dim_topo]` (one topology for all lanes) or `[n_lanes, dim_topo]`; `shunt_bus` likewise (None: the model's)."""
    x = rows_injections(m, inj_row, tables, lane_table, lane_offset, lane_scale, gen_delta, t0, n_rows, rebalance)
    n_lanes = x.shape[1]
    topo = np.asarray(topo)
    topo = np.broadcast_to(topo, (n_lanes, m.dim_topo)) if topo.ndim == 1 else topo
    sb = np.asarray(m.initial_shunt_bus() if shunt_bus is None else shunt_bus)
    sb = np.broadcast_to(sb, (n_lanes, m.n_shunt)) if sb.ndim == 1 else sb
    out = np.full((n_rows, n_lanes, m.n_line), np.nan)
    tables_of = {}                                       # PTDF per distinct (topology, shunt buses); None: the DC power flow rejects it
    for k in range(n_lanes):
        key = topo[k].tobytes() + sb[k].tobytes()
        if key not in tables_of:
            st = lane_state(m, x[0, k], topo[k], sb[k])
            tables_of[key] = ptdf(m, st) if solve(m, st, is_dc=True).converged else None
        ptdf_k = tables_of[key]
        if ptdf_k is None:
            continue
        for j in range(n_rows):
            out[j, k] = ptdf_k @ dc_bus_injection(m, lane_state(m, x[j, k], topo[k], sb[k]))
    return out
