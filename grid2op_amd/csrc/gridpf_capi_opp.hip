// gridpf_capi_opp.hip -- the opponent's entry points of the C ABI (include/gridpf.h: gpf_set_opponent, gpf_upload_opponent_draws,
// gpf_upload_opponent_schedule, gpf_get_opponent_state, gpf_set_opponent_state, and gpf_set_opponent_areas with the four calls of the
// multi-area opponent) and the host side of opponent_prestep_kernel / opponent_area_prestep_kernel (gridpf_opponent.hpp), on the engine of
// gridpf_engine.hpp.  Everything a descriptor can get wrong is refused here, before the device is
// touched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#define GPF_OPPONENT_KERNEL
#include "gridpf_engine.hpp"
#include "gridpf_opponent.hpp"

namespace {

const char* const kKindName[4] = {"none", "RandomLineOpponent", "WeightedRandomOpponent", "GeometricOpponent"};

// the state every lane starts from: as after a reset that has not happened yet (the lane's first launch resets it)
int opponent_clear_lanes(gpf_engine* e) {
  const size_t cap = (size_t)e->cap_lanes;
  std::vector<int> st(cap * gpf::OPP_STATE_INTS, 0);
  std::vector<double> bud(cap, (double)e->opp_desc.init_budget);
  for (size_t k = 0; k < cap; ++k) {
    int* s = &st[k * gpf::OPP_STATE_INTS];
    s[gpf::OS_F32] = 1; s[gpf::OS_COOLDOWN] = e->opp_desc.attack_cooldown; s[gpf::OS_LINE] = -1; s[gpf::OS_NEXT_TIME] = gpf::OPP_TIME_NONE;
    s[gpf::OS_INFO_LINE] = -1;
  }
  HIP_TRY(e->opp_state.upload(st.data(), st.size()));
  HIP_TRY(e->opp_budget.upload(bud.data(), bud.size()));
  return GPF_OK;
}

gpf::OppCfg opponent_cfg(const gpf_engine* e) {
  const gpf_opponent_desc& d = e->opp_desc;
  gpf::OppCfg c{};
  c.kind = d.kind; c.n_att = d.n_lines; c.lines = e->opp_lines.p; c.norm = e->opp_norm.p;
  c.attack_period = d.attack_period; c.hazard = d.attack_hazard_rate; c.recovery = d.recovery_rate; c.min_dur = d.recovery_minimum_duration;
  c.log_ratio = d.kind == GPF_OPP_GEOMETRIC ? std::log(d.pmax_pmin_ratio) : 0.0; c.episode_len = d.episode_max_time;
  c.init_budget = d.init_budget; c.budget_per_ts = d.budget_per_ts; c.max_duration = d.attack_duration; c.attack_cooldown = d.attack_cooldown;
  c.source = d.draw_source; c.seed_lo = d.seed_lo; c.seed_hi = d.seed_hi; c.lane_base = d.lane_base;
  c.sched_cap = d.kind == GPF_OPP_GEOMETRIC ? d.schedule_cap : 0; c.n_draw = e->opp_n_draw;
  return c;
}

bool areas_on(const gpf_engine* e) { return e->opp_n_area > 0; }

// the area rows every lane starts from: free, nothing held, nothing scheduled
int opponent_clear_areas(gpf_engine* e) {
  const size_t rows = (size_t)e->cap_lanes * e->opp_n_area;
  std::vector<int> st(rows * gpf::OPP_AREA_STATE_INTS, 0);
  for (size_t k = 0; k < rows; ++k) {
    int* r = &st[k * gpf::OPP_AREA_STATE_INTS];
    r[gpf::OAS_COUNTER] = -1; r[gpf::OAS_LINE] = -1; r[gpf::OAS_NEXT_TIME] = gpf::OPP_TIME_NONE; r[gpf::OAS_INFO_LINE] = -1;
  }
  HIP_TRY(e->opp_area_state.upload(st.data(), st.size()));
  const size_t n = rows * e->opp_desc.schedule_cap * 2;
  HIP_TRY(e->opp_area_sched.alloc(n));
  HIP_TRY(hipMemset(e->opp_area_sched.p, 0, n * sizeof(int)));
  return GPF_OK;
}

void opponent_areas_off(gpf_engine* e) {
  e->opp_n_area = 0;
  e->opp_area_lines_host.clear(); e->opp_area_off.clear();
  e->opp_area_lines.release(); e->opp_area_tab.release(); e->opp_area_state.release(); e->opp_area_sched.release();
}

}  // namespace

int opponent_prestep(gpf_engine* e) {
  const gpf::GridDev& g = e->g;
  gpf::OppDev d{};
  d.budget = e->opp_budget.p; d.state = e->opp_state.p;
  d.draws = e->opp_desc.draw_source == GPF_OPP_DRAWS_TABLE && e->opp_n_draw > 0 ? e->opp_draws.p : nullptr;
  d.sched = e->opp_kind == GPF_OPP_GEOMETRIC ? e->opp_sched.p : nullptr;
  d.rho = e->rho.p; d.line_status = e->line_status.p; d.done = e->done.p; d.episode = e->episode.p;
  d.topo = e->topo.p; d.cooldown = e->cooldown.p; d.or_pos = e->line_or_pos.p; d.ex_pos = e->line_ex_pos.p;
  d.n_line = g.n_line; d.dim_topo = g.dim_topo;
  e->dev_topo_dirty = true;                 // the kernel may force lines out of topology rows: the host mirrors are not the device rows any more
  const unsigned blocks = (unsigned)((e->n_lanes + gpf::OPP_WPB - 1) / gpf::OPP_WPB);
  if (areas_on(e)) {
    d.sched = nullptr;
    gpf::OppAreas A{};
    A.n_area = e->opp_n_area; A.lines = e->opp_area_lines.p; A.offset = e->opp_area_tab.p; A.count = e->opp_area_tab.p + e->opp_n_area;
    gpf::OppAreaDev ad{e->opp_area_state.p, e->opp_area_sched.p};
    hipLaunchKernelGGL(gpf::opponent_area_prestep_kernel, dim3(blocks), dim3(64 * gpf::OPP_WPB), 0, e->stream, opponent_cfg(e), d, A, ad, e->n_lanes);
  } else {
    hipLaunchKernelGGL(gpf::opponent_prestep_kernel, dim3(blocks), dim3(64 * gpf::OPP_WPB), 0, e->stream, opponent_cfg(e), d, e->n_lanes);
  }
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

hipError_t opponent_copy_lanes(gpf_engine* e, int src, int dst, int n) {
  auto cp = [&](auto* p, size_t stride) {
    return hipMemcpyAsync(p + (size_t)dst * stride, p + (size_t)src * stride, (size_t)n * stride * sizeof(*p), hipMemcpyDeviceToDevice, e->stream);
  };
  hipError_t err = cp(e->opp_budget.p, 1);
  if (err == hipSuccess) err = cp(e->opp_state.p, gpf::OPP_STATE_INTS);
  if (err == hipSuccess && e->opp_kind == GPF_OPP_GEOMETRIC) err = cp(e->opp_sched.p, (size_t)e->opp_desc.schedule_cap * 2);
  if (err == hipSuccess && areas_on(e)) err = cp(e->opp_area_state.p, (size_t)e->opp_n_area * gpf::OPP_AREA_STATE_INTS);
  if (err == hipSuccess && areas_on(e)) err = cp(e->opp_area_sched.p, (size_t)e->opp_n_area * e->opp_desc.schedule_cap * 2);
  return err;
}

extern "C" {

int gpf_set_opponent(gpf_handle e, const gpf_opponent_desc* d) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_opponent: null");
  if (!d || d->kind == GPF_OPP_NONE) {
    if (e->opp_kind && !e->dry) { HIP_TRY(hipSetDevice(e->device)); HIP_TRY(hipStreamSynchronize(e->stream)); }
    e->opp_kind = GPF_OPP_NONE;
    e->opp_host_kind = GPF_OPP_NONE;
    e->opp_host_lines.clear();
    opponent_areas_off(e);
    alerts_off(e);                            // (the alertable lines were this opponent's)
    return GPF_OK;
  }
  const std::string at = "gpf_set_opponent: ";
  if (d->kind < 0 || d->kind > GPF_OPP_GEOMETRIC) return fail(GPF_E_INVALID, at + "unknown opponent kind " + std::to_string(d->kind));
  const std::string who = at + kKindName[d->kind] + ": ";
  if (d->n_lines <= 0 || !d->line_ids) return fail(GPF_E_INVALID, who + "no attackable line (lines_attacked is empty)");
  std::vector<char> seen(e->g.n_line, 0);
  for (int i = 0; i < d->n_lines; ++i) {
    const int l = d->line_ids[i];
    if (l < 0 || l >= e->g.n_line)
      return fail(GPF_E_INVALID, who + "attackable line id " + std::to_string(l) + " is outside [0, n_line = " + std::to_string(e->g.n_line) + ")");
    if (seen[l]) return fail(GPF_E_INVALID, who + "attackable line id " + std::to_string(l) + " is listed twice");
    seen[l] = 1;
  }
  if (!(d->init_budget >= 0.f) || !std::isfinite(d->init_budget))
    return fail(GPF_E_INVALID, who + "an opponent should at least have a positive (or null) budget (init_budget)");
  if (!std::isfinite(d->budget_per_ts)) return fail(GPF_E_INVALID, who + "budget_per_ts is not finite");
  if (d->attack_duration < 0 || d->attack_cooldown < 0) return fail(GPF_E_INVALID, who + "attack_duration and attack_cooldown must not be negative");
  if (d->draw_source != GPF_OPP_DRAWS_TABLE && d->draw_source != GPF_OPP_DRAWS_PHILOX)
    return fail(GPF_E_INVALID, who + "unknown draw source " + std::to_string(d->draw_source));
  if (d->lane_base < 0) return fail(GPF_E_INVALID, who + "lane_base must not be negative");
  if (d->kind == GPF_OPP_WEIGHTED_RANDOM) {
    if (d->attack_period <= 0) return fail(GPF_E_INVALID, who + "attack_period needs to be > 0");
    if (d->rho_normalization)
      for (int i = 0; i < d->n_lines; ++i)
        if (!(d->rho_normalization[i] > 0.0) || !std::isfinite(d->rho_normalization[i]))
          return fail(GPF_E_INVALID, who + "rho_normalization[" + std::to_string(i) + "] must be finite and > 0");
  }
  if (d->kind == GPF_OPP_GEOMETRIC) {
    if (!(d->recovery_rate > 0.0 && d->recovery_rate <= 1.0))
      return fail(GPF_E_INVALID, who + "recovery_rate must be in (0, 1] (the average duration of an attack must exceed its minimum by at least one step)");
    if (!(d->attack_hazard_rate > 0.0 && d->attack_hazard_rate <= 1.0))
      return fail(GPF_E_INVALID, who + "attack_hazard_rate must be in (0, 1] (attack_every_xxx_hour must exceed average_attack_duration_hour by at least one step)");
    if (d->recovery_minimum_duration < 0) return fail(GPF_E_INVALID, who + "recovery_minimum_duration must not be negative");
    if (!(d->pmax_pmin_ratio > 0.0) || !std::isfinite(d->pmax_pmin_ratio)) return fail(GPF_E_INVALID, who + "pmax_pmin_ratio must be finite and > 0");
    if (d->episode_max_time <= 0 || d->episode_max_time == INT32_MAX)
      return fail(GPF_E_INVALID, who + "only works with a known finite episode duration (episode_max_time)");
    if (d->schedule_cap <= 0 || d->schedule_cap > (1 << 20)) return fail(GPF_E_INVALID, who + "schedule_cap must be in [1, 2^20]");
  }
  // the host's copy of a descriptor that passed (a header-only handle keeps it too: gpf_set_opponent_areas validates against it)
  e->opp_host_kind = d->kind;
  e->opp_host_lines.assign(d->line_ids, d->line_ids + d->n_lines);
  if (e->dry) {
    alerts_off(e);
    e->opp_desc = *d;
    e->opp_desc.line_ids = nullptr; e->opp_desc.rho_normalization = nullptr;
    e->opp_n_area = 0; e->opp_area_lines_host.clear(); e->opp_area_off.clear();
    return fail(GPF_E_DEVICE, "gpf_set_opponent: header-only handle: no HIP device");
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->opp_kind = GPF_OPP_NONE;
  opponent_areas_off(e);
  alerts_off(e);                              // a new opponent: a new alertable list (gpf_set_alerts comes after it)
  std::vector<double> norm(d->n_lines, 1.0);
  if (d->kind == GPF_OPP_WEIGHTED_RANDOM && d->rho_normalization) std::copy(d->rho_normalization, d->rho_normalization + d->n_lines, norm.begin());
  HIP_TRY(e->opp_lines.upload(d->line_ids, (size_t)d->n_lines));
  HIP_TRY(e->opp_norm.upload(norm.data(), norm.size()));
  e->opp_desc = *d;
  e->opp_desc.line_ids = nullptr; e->opp_desc.rho_normalization = nullptr;
  e->opp_n_draw = 0;
  e->opp_draws.release();
  e->opp_sched.release();
  if (d->kind == GPF_OPP_GEOMETRIC) {
    const size_t n = (size_t)e->cap_lanes * d->schedule_cap * 2;
    HIP_TRY(e->opp_sched.alloc(n));
    HIP_TRY(hipMemset(e->opp_sched.p, 0, n * sizeof(int)));
  }
  int rc = opponent_clear_lanes(e);
  if (rc != GPF_OK) return rc;
  e->opp_kind = d->kind;
  return GPF_OK;
}

int gpf_upload_opponent_draws(gpf_handle e, int32_t n_draw, const double* draws) {
  if (!e) return fail(GPF_E_INVALID, "gpf_upload_opponent_draws: null");
  if (!e->opp_kind) return fail(GPF_E_INVALID, "gpf_upload_opponent_draws: no opponent (gpf_set_opponent)");
  if (e->opp_desc.draw_source != GPF_OPP_DRAWS_TABLE) return fail(GPF_E_INVALID, "gpf_upload_opponent_draws: the opponent's draw source is not GPF_OPP_DRAWS_TABLE");
  if (n_draw < 0 || (n_draw > 0 && !draws)) return fail(GPF_E_INVALID, "gpf_upload_opponent_draws: bad arguments");
  for (size_t i = 0; i < (size_t)e->n_lanes * n_draw; ++i)
    if (!(draws[i] >= 0.0 && draws[i] < 1.0)) return fail(GPF_E_INVALID, "gpf_upload_opponent_draws: draw " + std::to_string(i) + " is outside [0, 1)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->opp_n_draw = 0;
  HIP_TRY(e->opp_draws.alloc((size_t)e->cap_lanes * n_draw));
  if (n_draw) {
    HIP_TRY(hipMemset(e->opp_draws.p, 0, (size_t)e->cap_lanes * n_draw * sizeof(double)));
    HIP_TRY(hipMemcpy(e->opp_draws.p, draws, (size_t)e->n_lanes * n_draw * sizeof(double), hipMemcpyHostToDevice));
  }
  const std::vector<int> zeros((size_t)e->cap_lanes, 0);      // the cursors
  HIP_TRY(hipMemcpy2D(e->opp_state.p + gpf::OS_CURSOR, gpf::OPP_STATE_INTS * sizeof(int), zeros.data(), sizeof(int), sizeof(int), zeros.size(), hipMemcpyHostToDevice));
  e->opp_n_draw = n_draw;
  return GPF_OK;
}

int gpf_upload_opponent_schedule(gpf_handle e, const int32_t* schedule, const int32_t* count) {
  if (!e || !schedule || !count) return fail(GPF_E_INVALID, "gpf_upload_opponent_schedule: null");
  if (e->opp_kind != GPF_OPP_GEOMETRIC) return fail(GPF_E_INVALID, "gpf_upload_opponent_schedule: the opponent is not a GeometricOpponent (gpf_set_opponent)");
  if (e->opp_desc.draw_source != GPF_OPP_DRAWS_TABLE)
    return fail(GPF_E_INVALID, "gpf_upload_opponent_schedule: the opponent's draw source is not GPF_OPP_DRAWS_TABLE (with GPF_OPP_DRAWS_PHILOX the kernel samples the schedule)");
  const int cap = e->opp_desc.schedule_cap;
  for (int k = 0; k < e->n_lanes; ++k) {
    if (count[k] < 0 || count[k] > cap)
      return fail(GPF_E_INVALID, "gpf_upload_opponent_schedule: lane " + std::to_string(k) + ": count is outside [0, schedule_cap = " + std::to_string(cap) + "]");
    for (int i = 0; i < count[k]; ++i)
      if (schedule[((size_t)k * cap + i) * 2] < 1 || schedule[((size_t)k * cap + i) * 2 + 1] < 1)
        return fail(GPF_E_INVALID, "gpf_upload_opponent_schedule: lane " + std::to_string(k) + ": waiting times and durations must be >= 1");
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(e->opp_sched.p, schedule, (size_t)e->n_lanes * cap * 2 * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy2D(e->opp_state.p + gpf::OS_N_SCHED, gpf::OPP_STATE_INTS * sizeof(int), count, sizeof(int), sizeof(int), (size_t)e->n_lanes, hipMemcpyHostToDevice));
  return GPF_OK;
}

int gpf_get_opponent_state(gpf_handle e, int32_t lane0, int32_t n, double* budget, int32_t* state) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_get_opponent_state: bad lane range");
  if (!e->opp_kind) return fail(GPF_E_INVALID, "gpf_get_opponent_state: no opponent (gpf_set_opponent)");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  if (budget) HIP_TRY(hipMemcpyAsync(budget, e->opp_budget.p + lane0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (state)
    HIP_TRY(hipMemcpyAsync(state, e->opp_state.p + (size_t)lane0 * gpf::OPP_STATE_INTS, (size_t)n * gpf::OPP_STATE_INTS * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_set_opponent_state(gpf_handle e, int32_t lane0, int32_t n, const double* budget, const int32_t* state) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_set_opponent_state: bad lane range");
  if (!e->opp_kind && !(e->dry && e->opp_host_kind)) return fail(GPF_E_INVALID, "gpf_set_opponent_state: no opponent (gpf_set_opponent)");
  const gpf_opponent_desc& d = e->opp_desc;
  if (state)
    for (int k = 0; k < n; ++k) {
      const int32_t* s = state + (size_t)k * gpf::OPP_STATE_INTS;
      const std::string at = "gpf_set_opponent_state: lane " + std::to_string(lane0 + k) + ": ";
      if (s[gpf::OS_LINE] < -1 || s[gpf::OS_LINE] >= e->g.n_line) return fail(GPF_E_INVALID, at + "the attacked line is outside [-1, n_line)");
      if (s[gpf::OS_DURATION] < 0 || s[gpf::OS_COOLDOWN] < 0) return fail(GPF_E_INVALID, at + "negative attack duration or cooldown");
      if (s[gpf::OS_CURSOR] < 0) return fail(GPF_E_INVALID, at + "negative draw cursor");
      if (d.kind == GPF_OPP_GEOMETRIC && (s[gpf::OS_N_SCHED] < 0 || s[gpf::OS_N_SCHED] > d.schedule_cap || s[gpf::OS_COUNTER] < 0))
        return fail(GPF_E_INVALID, at + "the schedule length is outside [0, schedule_cap] or the attack counter is negative");
      if (areas_on(e) && s[gpf::OS_DURATION] > 1)
        return fail(GPF_E_INVALID, at + "with areas set (gpf_set_opponent_areas) the attack duration is 0 or 1 (GeometricOpponentMultiArea.attack always "
                                        "returns duration 1, geometricOpponentMultiArea.py:149)");
    }
  if (e->dry) return fail(GPF_E_DEVICE, "gpf_set_opponent_state: header-only handle: no HIP device");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  if (budget) HIP_TRY(hipMemcpyAsync(e->opp_budget.p + lane0, budget, (size_t)n * sizeof(double), hipMemcpyHostToDevice, e->stream));
  if (state)
    HIP_TRY(hipMemcpyAsync(e->opp_state.p + (size_t)lane0 * gpf::OPP_STATE_INTS, state, (size_t)n * gpf::OPP_STATE_INTS * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_set_opponent_areas(gpf_handle e, int32_t n_area, const int32_t* area_of_line) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_opponent_areas: null");
  const std::string at = "gpf_set_opponent_areas: ";
  if (!e->opp_host_kind || (!e->dry && !e->opp_kind)) return fail(GPF_E_INVALID, at + "no opponent (gpf_set_opponent)");
  if (e->opp_host_kind != GPF_OPP_GEOMETRIC)
    return fail(GPF_E_INVALID, at + "the opponent is not a GeometricOpponent (gpf_set_opponent): areas are those of GeometricOpponentMultiArea");
  if (n_area < 0 || n_area > GPF_OPP_MAX_AREAS)
    return fail(GPF_E_INVALID, at + "n_area " + std::to_string(n_area) + " is outside [0, GPF_OPP_MAX_AREAS = " + std::to_string(GPF_OPP_MAX_AREAS) + "]");
  const int n_lines = (int)e->opp_host_lines.size();
  std::vector<int> off(n_area + 1, 0), grouped(n_lines, 0);
  if (n_area > 0) {
    if (!area_of_line) return fail(GPF_E_INVALID, at + "area_of_line is null");
    for (int i = 0; i < n_lines; ++i) {
      if (area_of_line[i] < 0 || area_of_line[i] >= n_area)
        return fail(GPF_E_INVALID, at + "area_of_line[" + std::to_string(i) + "] = " + std::to_string(area_of_line[i]) + " is outside [0, n_area = " + std::to_string(n_area) + ")");
      ++off[area_of_line[i] + 1];
    }
    for (int a = 0; a < n_area; ++a) {
      if (off[a + 1] == 0) return fail(GPF_E_INVALID, at + "area " + std::to_string(a) + " has no attackable line (an empty lines_attacked list)");
      off[a + 1] += off[a];
    }
    if (e->opp_desc.attack_cooldown > 1)
      return fail(GPF_E_INVALID, at + "attack_cooldown " + std::to_string(e->opp_desc.attack_cooldown) + " > 1 cannot be played: two consecutive attacking steps leave "
                  "current_attack_cooldown = 2 c, and 2 c - 1 > c sends OpponentSpace.attack into its minimum-time-between-attacks branch, whose call of "
                  "GeometricOpponentMultiArea.tell_attack_continues is RuntimeError(\"I should not get there !\") (geometricOpponentMultiArea.py:152-153)");
    std::vector<int> fill(off.begin(), off.end() - 1);
    for (int i = 0; i < n_lines; ++i) grouped[fill[area_of_line[i]]++] = e->opp_host_lines[i];     // descriptor order inside an area: it decides the cdf
  }
  if (e->dry) {                              // (kept, so that the state setters can refuse on a header-only handle too)
    alerts_off(e);
    e->opp_n_area = n_area; e->opp_area_lines_host = grouped; e->opp_area_off = off;
    return fail(GPF_E_DEVICE, "gpf_set_opponent_areas: header-only handle: no HIP device");
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  opponent_areas_off(e);
  alerts_off(e);                             // areas regroup the alertable list
  int rc = opponent_clear_lanes(e);          // every lane's opponent starts reset, with or without areas
  if (rc != GPF_OK || n_area == 0) return rc;
  std::vector<int> tab(2 * (size_t)n_area);
  for (int a = 0; a < n_area; ++a) { tab[a] = off[a]; tab[n_area + a] = off[a + 1] - off[a]; }
  HIP_TRY(e->opp_area_lines.upload(grouped.data(), grouped.size()));
  HIP_TRY(e->opp_area_tab.upload(tab.data(), tab.size()));
  e->opp_area_lines_host = grouped; e->opp_area_off = off;
  e->opp_n_area = n_area;
  rc = opponent_clear_areas(e);
  if (rc != GPF_OK) opponent_areas_off(e);
  return rc;
}

int gpf_upload_opponent_area_schedule(gpf_handle e, const int32_t* schedule, const int32_t* count) {
  if (!e || !schedule || !count) return fail(GPF_E_INVALID, "gpf_upload_opponent_area_schedule: null");
  const std::string at = "gpf_upload_opponent_area_schedule: ";
  if (!areas_on(e)) return fail(GPF_E_INVALID, at + "no areas (gpf_set_opponent_areas)");
  if (e->opp_desc.draw_source != GPF_OPP_DRAWS_TABLE)
    return fail(GPF_E_INVALID, at + "the opponent's draw source is not GPF_OPP_DRAWS_TABLE (with GPF_OPP_DRAWS_PHILOX the kernel samples the schedules)");
  const int cap = e->opp_desc.schedule_cap, na = e->opp_n_area;
  for (size_t k = 0; k < (size_t)e->n_lanes * na; ++k) {
    const std::string who = at + "lane " + std::to_string(k / na) + ", area " + std::to_string(k % na) + ": ";
    if (count[k] < 0 || count[k] > cap) return fail(GPF_E_INVALID, who + "count is outside [0, schedule_cap = " + std::to_string(cap) + "]");
    for (int i = 0; i < count[k]; ++i)
      if (schedule[(k * cap + i) * 2] < 1 || schedule[(k * cap + i) * 2 + 1] < 1) return fail(GPF_E_INVALID, who + "waiting times and durations must be >= 1");
  }
  if (e->dry) return fail(GPF_E_DEVICE, "gpf_upload_opponent_area_schedule: header-only handle: no HIP device");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(e->opp_area_sched.p, schedule, (size_t)e->n_lanes * na * cap * 2 * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy2D(e->opp_area_state.p + gpf::OAS_N_SCHED, gpf::OPP_AREA_STATE_INTS * sizeof(int), count, sizeof(int), sizeof(int), (size_t)e->n_lanes * na, hipMemcpyHostToDevice));
  return GPF_OK;
}

int gpf_get_opponent_area_state(gpf_handle e, int32_t lane0, int32_t n, int32_t* state) {
  if (!check_range(e, lane0, n) || !state) return fail(GPF_E_INVALID, "gpf_get_opponent_area_state: bad lane range or null");
  if (!areas_on(e) || !e->opp_kind) return fail(GPF_E_INVALID, "gpf_get_opponent_area_state: no areas (gpf_set_opponent_areas)");
  if (n == 0) return GPF_OK;
  const size_t row = (size_t)e->opp_n_area * gpf::OPP_AREA_STATE_INTS;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(state, e->opp_area_state.p + (size_t)lane0 * row, (size_t)n * row * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_set_opponent_area_state(gpf_handle e, int32_t lane0, int32_t n, const int32_t* state) {
  if (!check_range(e, lane0, n) || !state) return fail(GPF_E_INVALID, "gpf_set_opponent_area_state: bad lane range or null");
  if (!areas_on(e)) return fail(GPF_E_INVALID, "gpf_set_opponent_area_state: no areas (gpf_set_opponent_areas)");
  const int na = e->opp_n_area, cap = e->opp_desc.schedule_cap;
  for (int k = 0; k < n; ++k)
    for (int a = 0; a < na; ++a) {
      const int32_t* r = state + ((size_t)k * na + a) * gpf::OPP_AREA_STATE_INTS;
      const std::string at = "gpf_set_opponent_area_state: lane " + std::to_string(lane0 + k) + ", area " + std::to_string(a) + ": ";
      for (int f : {gpf::OAS_LINE, gpf::OAS_INFO_LINE}) {
        bool in = r[f] == -1;
        for (int i = e->opp_area_off[a]; i < e->opp_area_off[a + 1] && !in; ++i) in = e->opp_area_lines_host[i] == r[f];
        if (!in) return fail(GPF_E_INVALID, at + "line " + std::to_string(r[f]) + " is outside the area's list (and not -1)");
      }
      if (r[gpf::OAS_COUNTER] < -1) return fail(GPF_E_INVALID, at + "the counter is below -1");
      if (r[gpf::OAS_N_SCHED] < 0 || r[gpf::OAS_N_SCHED] > cap || r[gpf::OAS_ATTACK_COUNTER] < 0)
        return fail(GPF_E_INVALID, at + "the schedule length is outside [0, schedule_cap] or the attack counter is negative");
    }
  if (e->dry) return fail(GPF_E_DEVICE, "gpf_set_opponent_area_state: header-only handle: no HIP device");
  if (n == 0) return GPF_OK;
  const size_t row = (size_t)na * gpf::OPP_AREA_STATE_INTS;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(e->opp_area_state.p + (size_t)lane0 * row, state, (size_t)n * row * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_opponent_attack_lines(gpf_handle e, int32_t lane0, int32_t n, uint8_t* attacked) {
  if (!check_range(e, lane0, n) || !attacked) return fail(GPF_E_INVALID, "gpf_get_opponent_attack_lines: bad lane range or null");
  if (!e->opp_kind) return fail(GPF_E_INVALID, "gpf_get_opponent_attack_lines: no opponent (gpf_set_opponent)");
  const int n_line = e->g.n_line;
  std::memset(attacked, 0, (size_t)n * n_line);
  if (n == 0) return GPF_OK;
  // the accepted lines of the last launch: one per area (OAS_INFO_LINE), or the lane's one line without areas
  const bool areas = areas_on(e);
  const size_t per = areas ? (size_t)e->opp_n_area : 1, stride = areas ? gpf::OPP_AREA_STATE_INTS : gpf::OPP_STATE_INTS;
  const int field = areas ? gpf::OAS_INFO_LINE : gpf::OS_INFO_LINE;
  std::vector<int> rows((size_t)n * per * stride);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(rows.data(), (areas ? e->opp_area_state.p : e->opp_state.p) + (size_t)lane0 * per * stride, rows.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < n; ++k)
    for (size_t a = 0; a < per; ++a) {
      const int l = rows[((size_t)k * per + a) * stride + field];
      if (l >= 0 && l < n_line) attacked[(size_t)k * n_line + l] = 1;
    }
  return GPF_OK;
}

}  // extern "C"
