// gridpf_capi_obs.hip -- the observation-vector entry points of the C ABI (include/gridpf.h: gpf_set_obs_clock, gpf_set_obs_spec,
// gpf_obs_vector, gpf_obs_vector_trajectory, gpf_get_obs_vector): the host side of the gather kernel of gridpf_obs.hpp, on the engine of
// gridpf_engine.hpp.  Everything a spec can get wrong is refused here, before the device is touched.
#include <hip/hip_runtime.h>

#include <cstring>

#include "gridpf_engine.hpp"
#include "gridpf_obs.hpp"

namespace {

const char* const kKindName[GPF_OBS_N_KINDS] = {
    "const", "out", "rho", "line_status", "topo_vect", "_shunt_bus", "timestep_overflow", "time_before_cooldown_line", "time_before_cooldown_sub",
    "target_dispatch", "actual_dispatch", "storage_charge", "curtailment_limit", "gen_margin_up", "gen_margin_down", "calendar", "current_step",
    "max_step", "delta_time", "time_next_maintenance", "duration_next_maintenance", "thermal_limit", "gen_p_before_curtail", "gen_p_delta",
    "active_alert", "time_since_last_alert", "alert_duration", "total_number_of_alert", "time_since_last_attack", "attack_under_alert",
    "was_alert_used_after_attack"};

bool alert_kind(int kind) { return kind >= GPF_OBS_ACTIVE_ALERT && kind <= GPF_OBS_WAS_ALERT_USED_AFTER_ATTACK; }

// width of the source a segment of `kind` reads (-1: any offset, the segment is a fill)
int source_width(const gpf_engine* e, int kind) {
  const gpf::GridDev& g = e->g;
  if (kind == GPF_OBS_TOTAL_NUMBER_OF_ALERT) return 1;
  if (alert_kind(kind)) return e->al_A;
  switch (kind) {
    case GPF_OBS_OUT: return g.n_out;
    case GPF_OBS_RHO: case GPF_OBS_LINE_STATUS: case GPF_OBS_OVERFLOW: case GPF_OBS_COOLDOWN_LINE: case GPF_OBS_TIME_NEXT_MAINTENANCE:
    case GPF_OBS_DURATION_NEXT_MAINTENANCE: case GPF_OBS_THERMAL_LIMIT: return g.n_line;
    case GPF_OBS_TOPO_VECT: return g.dim_topo;
    case GPF_OBS_SHUNT_BUS: return g.n_shunt;
    case GPF_OBS_COOLDOWN_SUB: return g.n_sub;
    case GPF_OBS_TARGET_DISPATCH: case GPF_OBS_ACTUAL_DISPATCH: case GPF_OBS_CURTAILMENT_LIMIT: case GPF_OBS_MARGIN_UP: case GPF_OBS_MARGIN_DOWN:
    case GPF_OBS_GEN_P_BEFORE_CURTAIL: case GPF_OBS_GEN_P_DELTA:
      return g.n_gen;
    case GPF_OBS_STORAGE_CHARGE: return g.n_sto;
    default: return -1;
  }
}

bool spec_uses(const gpf_engine* e, int kind) {
  for (int s = 0; s < e->obs_n_seg; ++s) if (e->h_obs_seg[gpf::OBS_SEG_INTS * s] == kind) return true;
  return false;
}

// GridValue.get_maintenance_time_1d / get_maintenance_duration_1d (Chronics/gridValue.py:264-410) of every line of every uploaded maintenance
// table: one backward scan per column.  Rows after the last outage: -1 / 0; during an outage: 0 / the remaining steps (a caller's
// gpf_upload_outage_durations is not consulted: the look-ahead is that of the table as uploaded).
int refresh_maintenance(gpf_engine* e) {
  if (e->obs_maint_gen == e->maint_gen) return GPF_OK;
  e->obs_maint_next.release(); e->obs_maint_durn.release();
  e->obs_maint_gen = e->maint_gen;
  if (e->h_maint.empty()) return GPF_OK;
  const size_t nl = e->g.n_line, T = (size_t)e->chron_T, nt = (size_t)e->chron_tables;
  std::vector<int> nx(nt * T * nl), du(nt * T * nl);
  for (size_t k = 0; k < nt; ++k)
    for (size_t l = 0; l < nl; ++l) {
      int next = -1, dur = 0, run = 0;      // distance to / length of the next outage seen from row t + 1, outage run that covers row t + 1
      for (size_t t = T; t-- > 0;) {
        const size_t i = (k * T + t) * nl + l;
        if (e->h_maint[i]) { ++run; nx[i] = 0; du[i] = run; next = 0; dur = run; }
        else { run = 0; next = next >= 0 ? next + 1 : -1; nx[i] = next; du[i] = next >= 0 ? dur : 0; }
      }
    }
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(e->obs_maint_next.upload(nx.data(), nx.size()));
  HIP_TRY(e->obs_maint_durn.upload(du.data(), du.size()));
  return GPF_OK;
}

int launch_obs(gpf_engine* e, bool traj, int step0, int n_steps, int lane0, int n, float* dst, long long row_stride, const char* who) {
  if (e->dry) return fail(GPF_E_DEVICE, std::string(who) + ": header-only handle");
  if (!e->obs_spec_on) return fail(GPF_E_INVALID, std::string(who) + ": no observation spec (gpf_set_obs_spec)");
  if (spec_uses(e, GPF_OBS_CALENDAR) || spec_uses(e, GPF_OBS_MAX_STEP) || spec_uses(e, GPF_OBS_DELTA_TIME)) {
    if (!e->obs_clock_on)
      return fail(GPF_E_INVALID, std::string(who) + ": the spec has calendar attributes (year .. day_of_week, max_step, delta_time) but no clock is set (gpf_set_obs_clock)");
    if (e->obs_clock_tables < std::max(e->chron_tables, 1))
      return fail(GPF_E_INVALID, std::string(who) + ": the clock has fewer start times than there are chronics tables (gpf_set_obs_clock)");
  }
  if (n == 0 || n_steps == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  const bool maint = spec_uses(e, GPF_OBS_TIME_NEXT_MAINTENANCE) || spec_uses(e, GPF_OBS_DURATION_NEXT_MAINTENANCE);
  if (maint) { int rc = refresh_maintenance(e); if (rc != GPF_OK) return rc; }
  const gpf::GridDev& g = e->g;
  gpf::ObsSrc S{};
  S.out = traj ? e->traj_out.p : e->out.p; S.rho = traj ? e->traj_rho.p : e->rho.p;
  S.line_status = traj ? e->traj_lstat.p : e->line_status.p; S.topo_vect = traj ? e->traj_topo.p : e->topo_out.p;
  S.shunt_bus = traj ? e->traj_shb.p : e->shunt_bus_out.p;
  S.inj = e->inj.p; S.n_inj = g.n_inj; S.inj_gen_p_off = e->oo.inj_gen_p;
  S.overflow = e->overflow_count.p; S.cooldown = e->cooldown.p; S.cooldown16 = traj && e->last_track_cooldown ? e->traj_cool.p : nullptr;
  S.sub_cd = e->ta_on ? e->ta_sub_cd.p : nullptr;
  S.target = e->env_on ? e->env_target.p : nullptr; S.actual = e->env_on ? e->env_actual.p : nullptr;
  S.charge = e->env_on ? e->env_charge.p : nullptr; S.limit = e->env_on ? e->env_limit.p : nullptr;
  if (e->rd_ready) { S.pmin = e->rd_pmin.p; S.pmax = e->rd_pmax.p; S.ramp_up = e->rd_ru.p; S.ramp_down = e->rd_rd.p; }
  S.renewable = e->env_has_ren ? e->env_renewable.p : nullptr;
  S.done = e->done.p; S.traj_status = traj ? e->traj_status.p : nullptr; S.episode = e->episode.p;
  S.lane_table = e->lane_table.p; S.lane_offset = e->lane_offset.p;
  S.clock_start = e->obs_clock_on ? e->obs_clock.p : nullptr;
  S.maint_next = maint && e->obs_maint_next.n ? e->obs_maint_next.p : nullptr;
  S.maint_durn = maint && e->obs_maint_durn.n ? e->obs_maint_durn.p : nullptr;
  S.thermal_limit = e->thermal_limit.p;
  for (int kind = GPF_OBS_ACTIVE_ALERT; kind <= GPF_OBS_WAS_ALERT_USED_AFTER_ATTACK; ++kind)
    if (spec_uses(e, kind) && !e->al_on)
      return fail(GPF_E_INVALID, std::string(who) + ": " + kKindName[kind] + " is in the spec but alerts were turned off since (gpf_set_alerts)");
  for (int s = 0; s < e->obs_n_seg; ++s) {                 // (alerts set again on another opponent: the spec's ranges may not fit any more)
    const int* q = &e->h_obs_seg[gpf::OBS_SEG_INTS * s];
    if (alert_kind(q[0]) && q[1] + q[2] > source_width(e, q[0]))
      return fail(GPF_E_INVALID, std::string(who) + ": " + kKindName[q[0]] + ": the spec was set for more alertable lines than there are now: set it again");
  }
  S.alert = e->al_on ? e->al_obs.p : nullptr; S.alert_A = e->al_A;
  S.T = e->chron.p ? e->chron_T : 0;
  S.t = traj ? e->last_t0 : e->last_t0 + e->last_n_steps - 1;
  S.step_minutes = e->obs_step_minutes; S.max_step = e->obs_max_step;
  S.n_out = g.n_out; S.n_line = g.n_line; S.dim_topo = g.dim_topo; S.n_shunt = g.n_shunt; S.n_sub = g.n_sub; S.n_gen = g.n_gen; S.n_sto = g.n_sto;
  S.gen_p_off = e->oo.gen_p;
  S.lane_stride = e->cap_lanes; S.traj = traj ? 1 : 0;
  const long long n_rows = (long long)n * n_steps;
  if (n_rows > 0x7fffffffLL) return fail(GPF_E_INVALID, std::string(who) + ": too many rows");
  const unsigned blocks = (unsigned)std::min<long long>((n_rows + gpf::OBS_WPB - 1) / gpf::OBS_WPB, 65535LL * 16);
  hipLaunchKernelGGL(gpf::obs_gather_kernel, dim3(blocks), dim3(64 * gpf::OBS_WPB), 0, e->stream, S, e->obs_seg.p, e->obs_n_seg, e->obs_sub.p,
                     e->obs_div.p, dst, row_stride, lane0, n, (int)n_rows, step0, e->obs_gof ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

}  // namespace

extern "C" {

int gpf_set_obs_clock(gpf_handle e, int32_t n_tables, const int64_t* start_minutes, int32_t step_minutes, int32_t max_step) {
  if (!e || n_tables <= 0 || !start_minutes || step_minutes <= 0 || max_step < 0)
    return fail(GPF_E_INVALID, "gpf_set_obs_clock: bad arguments (n_tables > 0, start times, step_minutes > 0, max_step >= 0)");
  for (int k = 0; k < n_tables; ++k)
    if (start_minutes[k] < 0 || start_minutes[k] > (int64_t)1 << 40) return fail(GPF_E_INVALID, "gpf_set_obs_clock: start time before 1970-01-01 or out of range");
  if (e->dry) return fail(GPF_E_DEVICE, "gpf_set_obs_clock: header-only handle");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::vector<long long> st(start_minutes, start_minutes + n_tables);
  HIP_TRY(e->obs_clock.upload(st.data(), st.size()));
  e->obs_clock_tables = n_tables; e->obs_step_minutes = step_minutes; e->obs_max_step = max_step; e->obs_clock_on = true;
  return GPF_OK;
}

int gpf_set_obs_spec(gpf_handle e, int32_t n_seg, const int32_t* segments, int32_t dim, const float* subtract, const float* divide,
                     int32_t game_over_fill) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_obs_spec: null");
  if (n_seg <= 0 || n_seg > GPF_OBS_MAX_SEGMENTS || !segments || dim <= 0)
    return fail(GPF_E_INVALID, "gpf_set_obs_spec: 1 .. " + std::to_string(GPF_OBS_MAX_SEGMENTS) + " segments and dim > 0 are required");
  const gpf::GridDev& g = e->g;
  std::vector<int> seg(segments, segments + (size_t)n_seg * gpf::OBS_SEG_INTS);
  std::vector<char> covered(dim, 0);
  for (int s = 0; s < n_seg; ++s) {
    int* q = &seg[(size_t)s * gpf::OBS_SEG_INTS];
    const int kind = q[0], so = q[1], len = q[2], d0 = q[3];
    const std::string at = "gpf_set_obs_spec: segment " + std::to_string(s);
    if (kind < 0 || kind >= GPF_OBS_N_KINDS) return fail(GPF_E_INVALID, at + ": unknown source kind " + std::to_string(kind));
    if (len <= 0) return fail(GPF_E_INVALID, at + " (" + kKindName[kind] + "): length must be positive");
    if (alert_kind(kind) && !e->al_on && !(e->dry && e->al_host_A > 0))
      return fail(GPF_E_INVALID, at + " (" + kKindName[kind] + "): alerts are off (gpf_set_alerts)");
    const int w = alert_kind(kind) && e->dry ? (kind == GPF_OBS_TOTAL_NUMBER_OF_ALERT ? 1 : e->al_host_A) : source_width(e, kind);
    if (w >= 0 && (so < 0 || (long long)so + len > w))
      return fail(GPF_E_INVALID, at + " (" + kKindName[kind] + "): source range [" + std::to_string(so) + ", " + std::to_string((long long)so + len) +
                                     ") is outside the " + std::to_string(w) + " elements this grid has");
    if (kind == GPF_OBS_CALENDAR && (so < 0 || so > 5)) return fail(GPF_E_INVALID, at + ": calendar field must be 0 .. 5");
    if (d0 < 0 || (long long)d0 + len > dim) return fail(GPF_E_INVALID, at + " (" + kKindName[kind] + "): destination range leaves [0, dim)");
    for (int i = d0; i < d0 + len; ++i) {
      if (covered[i]) return fail(GPF_E_INVALID, at + " (" + kKindName[kind] + "): destination element " + std::to_string(i) + " is written twice (segments overlap)");
      covered[i] = 1;
    }
    if (q[4] & ~3) return fail(GPF_E_INVALID, at + ": flags beyond the game-over mode (bits 0-1)");
    bool affine = false;
    for (int i = d0; i < d0 + len; ++i) affine |= (subtract && subtract[i] != 0.f) || (divide && divide[i] != 1.f);
    if (affine) q[4] |= gpf::OBS_F_AFFINE;
  }
  for (int i = 0; i < dim; ++i) if (!covered[i]) return fail(GPF_E_INVALID, "gpf_set_obs_spec: destination element " + std::to_string(i) + " is written by no segment (gap)");
  std::vector<float> sb(dim, 0.f), dv(dim, 1.f);
  if (subtract) std::copy(subtract, subtract + dim, sb.begin());
  if (divide) std::copy(divide, divide + dim, dv.begin());
  for (int i = 0; i < dim; ++i)
    if (dv[i] == 0.f || dv[i] != dv[i] || sb[i] != sb[i]) return fail(GPF_E_INVALID, "gpf_set_obs_spec: divide[" + std::to_string(i) + "] is zero (or an entry is NaN)");
  if (e->dry) return fail(GPF_E_DEVICE, "gpf_set_obs_spec: header-only handle");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->obs_spec_on = false;
  HIP_TRY(e->obs_seg.upload(seg.data(), seg.size()));
  HIP_TRY(e->obs_sub.upload(sb.data(), sb.size()));
  HIP_TRY(e->obs_div.upload(dv.data(), dv.size()));
  HIP_TRY(e->obs_vec.alloc((size_t)e->cap_lanes * dim));
  HIP_TRY(hipMemset(e->obs_vec.p, 0, (size_t)e->cap_lanes * dim * sizeof(float)));
  e->h_obs_seg = seg; e->obs_n_seg = n_seg; e->obs_dim = dim; e->obs_gof = game_over_fill != 0; e->obs_spec_on = true;
  return GPF_OK;
}

int gpf_obs_vector(gpf_handle e, int32_t lane0, int32_t n, float* out_dev, int64_t row_stride) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_obs_vector: bad lane range");
  if (!e->obs_spec_on) return fail(GPF_E_INVALID, "gpf_obs_vector: no observation spec (gpf_set_obs_spec)");
  if (out_dev && row_stride < e->obs_dim) return fail(GPF_E_INVALID, "gpf_obs_vector: row_stride is smaller than the spec's dim");
  float* dst = out_dev ? out_dev : e->obs_vec.p + (size_t)lane0 * e->obs_dim;
  return launch_obs(e, false, 0, 1, lane0, n, dst, out_dev ? (long long)row_stride : (long long)e->obs_dim, "gpf_obs_vector");
}

int gpf_obs_vector_trajectory(gpf_handle e, int32_t step0, int32_t n_steps, int32_t lane0, int32_t n, float* out_dev) {
  if (!check_range(e, lane0, n) || !out_dev) return fail(GPF_E_INVALID, "gpf_obs_vector_trajectory: bad lane range or null output");
  if (!e->obs_spec_on) return fail(GPF_E_INVALID, "gpf_obs_vector_trajectory: no observation spec (gpf_set_obs_spec)");
  if (!(e->traj_cap && (e->traj_what & GPF_TRAJ_OBS)))
    return fail(GPF_E_INVALID, "gpf_obs_vector_trajectory: no observation trajectory (gpf_set_trajectory(.., GPF_TRAJ_OBS))");
  if (step0 < 0 || n_steps < 0 || step0 + n_steps > e->traj_valid)
    return fail(GPF_E_INVALID, "gpf_obs_vector_trajectory: bad step range (only the steps of the last gpf_step_n are retrievable)");
  for (int kind : {GPF_OBS_OVERFLOW, GPF_OBS_COOLDOWN_SUB, GPF_OBS_TARGET_DISPATCH, GPF_OBS_ACTUAL_DISPATCH, GPF_OBS_STORAGE_CHARGE,
                   GPF_OBS_CURTAILMENT_LIMIT, GPF_OBS_CURRENT_STEP, GPF_OBS_GEN_P_BEFORE_CURTAIL, GPF_OBS_GEN_P_DELTA,
                   GPF_OBS_ACTIVE_ALERT, GPF_OBS_TIME_SINCE_LAST_ALERT, GPF_OBS_ALERT_DURATION, GPF_OBS_TOTAL_NUMBER_OF_ALERT,
                   GPF_OBS_TIME_SINCE_LAST_ATTACK, GPF_OBS_ATTACK_UNDER_ALERT, GPF_OBS_WAS_ALERT_USED_AFTER_ATTACK})
    if (spec_uses(e, kind))
      return fail(GPF_E_INVALID, std::string("gpf_obs_vector_trajectory: ") + kKindName[kind] + " has no per-step copy in the trajectory buffers: "
                                 "take it out of the spec for this mode");
  // traj_cool is written by the converged steps of a launch that maintains the line cooldowns (gridpf_sparse.hpp, K8); a launch that does
  // not leaves them standing, so launch_obs reads the lanes' own counters for every step of it.  A failed step has no copy at all:
  if (spec_uses(e, GPF_OBS_COOLDOWN_LINE) && e->last_track_cooldown && !e->obs_gof)
    return fail(GPF_E_INVALID, "gpf_obs_vector_trajectory: time_before_cooldown_line: a failed step leaves no per-step copy of the line cooldowns; "
                               "with game_over_fill off take it out of the spec for this mode");
  return launch_obs(e, true, step0, n_steps, lane0, n, out_dev, (long long)e->obs_dim, "gpf_obs_vector_trajectory");
}

int gpf_get_obs_vector(gpf_handle e, int32_t lane0, int32_t n, float* host_out) {
  if (!check_range(e, lane0, n) || !host_out) return fail(GPF_E_INVALID, "gpf_get_obs_vector: bad arguments");
  int rc = gpf_obs_vector(e, lane0, n, nullptr, 0);
  if (rc != GPF_OK) return rc;
  if (n > 0)
    HIP_TRY(hipMemcpyAsync(host_out, e->obs_vec.p + (size_t)lane0 * e->obs_dim, (size_t)n * e->obs_dim * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

}  // extern "C"
