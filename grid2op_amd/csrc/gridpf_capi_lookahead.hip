// gridpf_capi_lookahead.hip -- the look-ahead screen's entry points of the C ABI (include/gridpf.h: gpf_set_lookahead, gpf_lookahead,
// gpf_get_lookahead, gpf_lookahead_device_pointers; the chain: gpf_set_lookahead_chain, gpf_lookahead_chain, gpf_get_lookahead_chain,
// gpf_lookahead_chain_device_pointers) and the host side of the kernels of gridpf_lookahead.hpp, on the engine of
// gridpf_engine.hpp.  Everything a call can get wrong is refused here, before the device is touched.  A call in which no scratch lane
// changed its topology class does no host work that grows with n_env x K: the candidates are played on the device, the plans of the
// two lane ranges are cached (fan_plans) and the play kernel's list of moved lanes is read back count first.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#define GPF_LA_KERNEL
#include "gridpf_engine.hpp"
#include "gridpf_lookahead.hpp"

static_assert(gpf::LA_ILLEGAL == GPF_LA_ILLEGAL && gpf::LA_AMBIGUOUS == GPF_LA_AMBIGUOUS && gpf::LA_DONE == GPF_LA_DONE, "flags");

namespace {
constexpr size_t LA_LDS_LIMIT = 64 * 1024;        // LDS of one workgroup
constexpr FanOwner LA = FanOwner::lookahead;

void la_chain_release(gpf_engine* e) {
  e->lc_on = e->lc_host_on = false;
  e->lc_max = 0;
  e->lc_survived.release(); e->lc_fallback.release(); e->lc_fallback_steps.release(); e->lc_peak.release(); e->lc_value_h.release();
}

void la_release(gpf_engine* e) {
  la_chain_release(e);                      // (its buffers have the look-ahead's shape)
  e->la_noted_gen = e->la_maint_gen = -1;
  e->la_cand.release(); e->la_best.release(); e->la_info.release(); e->la_moved_list.release(); e->la_noted.release();
  e->la_src.release(); e->la_value.release(); e->la_best_value.release(); e->la_flags.release(); e->la_maint.release();
  e->fan.release();
}

gpf::LaDev la_dev(const gpf_engine* e, int t_obs, int time_step) {
  gpf::LaDev d{};
  d.cand = e->la_cand.p; d.flags = e->la_flags.p; d.value = e->la_value.p; d.best = e->la_best.p; d.best_value = e->la_best_value.p;
  d.info = e->la_info.p; d.list = e->la_moved_list.list.p; d.list_rows = e->la_moved_list.rows.p; d.noted = e->la_noted.p;
  d.maint = e->la_maint.n ? e->la_maint.p : nullptr; d.lane_table = e->lane_table.p; d.lane_offset = e->lane_offset.p;
  d.rho = e->rho.p; d.done = e->done.p;
  d.n_env = e->fan.n_env; d.K = e->fan.K; d.T = e->chron_T; d.t_obs = t_obs; d.time_step = time_step;
  return d;
}

gpf::LaChainDev la_chain_dev(const gpf_engine* e) {
  gpf::LaChainDev c{};
  c.survived = e->lc_survived.p; c.peak = e->lc_peak.p; c.value_h = e->lc_value_h.p; c.fallback = e->lc_fallback.p;
  c.fallback_steps = e->lc_fallback_steps.p; c.lane_offset = e->lane_offset.p; c.topo = e->topo.p; c.topo0 = e->topo0.p;
  c.line_or_pos = e->g.line_or_pos; c.line_ex_pos = e->g.line_ex_pos; c.act = e->ta_act.p;
  c.dim_topo = e->g.dim_topo; c.n_line = e->g.n_line; c.n_h = e->fc_h; c.max_steps = e->lc_max;
  return c;
}

// what composite slots and areas are refused with
int la_check_table(const gpf_engine* e, const std::string& at) {
  if (e->ta_n_act == 0) return fail(GPF_E_INVALID, at + "no action table (gpf_upload_topo_actions): the candidates are indices into it");
  if (e->ta_n_slot > 1)
    return fail(GPF_E_INVALID, at + "composite actions (gpf_set_topo_slots > 1) are not supported: a candidate is one table entry");
  if (e->ta_n_area > 0)
    return fail(GPF_E_INVALID, at + "rules by area (gpf_set_topo_areas) are not supported: a candidate is one table entry under whole-grid limits");
  return GPF_OK;
}

// the rows the host last noted for the scratch lanes -> la_noted (an unknown mirror stays INT_MIN in front: the play kernel lists the lane)
int la_upload_noted(gpf_engine* e) {
  const gpf::GridDev& g = e->g;
  const size_t w = (size_t)g.dim_topo + g.n_shunt, nc = (size_t)e->fan.n_sec();
  std::vector<int> rows(nc * w);
  for (size_t q = 0; q < nc; ++q) {
    const size_t lane = (size_t)e->fan.n_env + q;
    std::copy_n(e->h_lane_topo.begin() + lane * g.dim_topo, g.dim_topo, rows.begin() + q * w);
    if (g.n_shunt) std::copy_n(e->h_lane_sb.begin() + lane * g.n_shunt, g.n_shunt, rows.begin() + q * w + g.dim_topo);
  }
  HIP_TRY(hipMemcpyAsync(e->la_noted.p, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));                 // (the host vector goes out of scope)
  return GPF_OK;
}

// what gpf_lookahead and gpf_lookahead_chain refuse alike, before the device is touched
int la_check(const gpf_engine* e, const char* who, int time_step) {
  const std::string at = std::string(who) + ": ";
  if (!e->fan.owned_by(LA)) return fail(GPF_E_INVALID, at + "the look-ahead is off (gpf_set_lookahead)");
  int rc = la_check_table(e, at);
  if (rc != GPF_OK) return rc;
  if (time_step < 0 || time_step > e->fc_h)                 // (fc_h: 0 without uploaded forecasts)
    return fail(GPF_E_INVALID, at + "no forecast for that horizon (gpf_upload_forecasts; NoForecastAvailable in the reference)");
  if (!e->dry && (!e->chron.p || e->chron_T <= 0)) return fail(GPF_E_INVALID, at + "no chronics uploaded");
  if (e->cb_on && (e->env_act_r || e->env_act_s || e->env_act_c))
    return fail(GPF_E_INVALID, at + "in combined mode (gpf_set_combined_actions) injection actions are pending: the candidates are topology "
                                    "actions alone, injection candidates are not supported");
  return GPF_OK;
}

// steps 1-4 of a look-ahead call: the scratch lanes become their environments, the candidates are played, the host notes the lanes
// that changed class, and the scratch range is stepped ONCE
int la_play_and_step(gpf_engine* e, const char* who, int t_obs, int time_step, const int32_t* cand, const gpf_step_opts* o) {
  const std::string at = std::string(who) + ": ";
  int rc = GPF_OK;
  const gpf::GridDev& g = e->g;
  const int ne = e->fan.n_env, K = e->fan.K, nc = e->fan.n_sec();
  for (int i = 0; i < ne; ++i)
    if (e->h_lane_forecast[i])
      return fail(GPF_E_INVALID, at + "an environment lane is itself a scratch lane of an earlier gpf_simulate_batch (its chronics cursor is an absolute "
                                      "row): send gpf_set_lane_chronics again");
  HIP_TRY(hipSetDevice(e->device));
  if (cand) {
    HIP_TRY(hipMemcpyAsync(e->la_cand.p, cand, (size_t)nc * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));               // (the caller may reuse `cand`)
  }
  const bool maint = !e->h_maint.empty() && e->h_maint.size() == (size_t)e->chron_tables * e->chron_T * e->g.n_line;
  if (maint && e->la_maint_gen != e->maint_gen) {           // the scheduled maintenance alone, once per uploaded table
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(e->la_maint.upload(e->h_maint.data(), e->h_maint.size()));
  } else if (!maint && e->la_maint.n) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->la_maint.release();
  }
  e->la_maint_gen = e->maint_gen;
  // whatever invalidated the plans may have re-keyed scratch lanes on the host (gpf_set_topology, gpf_reset_lanes, gpf_copy_lanes ...)
  if (e->la_noted_gen != e->fan.plans_gen || !(e->plan_valid && e->fan.plans_valid)) { rc = la_upload_noted(e); if (rc != GPF_OK) return rc; }
  // 1. everything of the environments that is not topology, and the chronics / forecast row to step on
  rc = simulate_prepare(e, e->la_src.p, K, nc, ne, t_obs, time_step);
  if (rc != GPF_OK) return rc;
  // 2. the topology side and the candidates, under the environments' rules
  HIP_TRY(hipMemsetAsync(e->la_moved_list.list.p, 0, sizeof(int), e->stream));
  const gpf::TopoTab tab{e->ta_off.p, e->ta_items.p, e->ta_amb.p, e->ta_n_act};
  const size_t lds = gpf::topo_prestep_lds_ints(g.dim_topo, g.n_line, g.n_sub, g.n_shunt, g.n_busbar) * sizeof(int);
  const gpf::LaDev d = la_dev(e, t_obs, time_step);
  hipLaunchKernelGGL(gpf::la_play_kernel, dim3((unsigned)nc), dim3(64), lds, e->stream, topo_dev(e), tab, topo_lanes(e), e->ta_rules, d);
  HIP_TRY(hipGetLastError());
  e->dev_topo_dirty = true;
  if (e->env_on) { rc = env_copy_from(e, e->la_src.p, K, nc, ne); if (rc != GPF_OK) return rc; }
  // 3. the scratch lanes whose topology class or busbar count left the one the host noted: ONE compact read-back (no per-lane work: a
  // scratch lane is never auto-reset)
  rc = moved_list_readback(e, e->la_moved_list, ne, ne + nc, "gpf_lookahead: internal (read-back", nullptr);
  if (rc != GPF_OK) return rc;
  rc = fan_plans(e);
  if (rc != GPF_OK) return rc;
  e->la_noted_gen = e->fan.plans_gen;       // (la_noted and the host's mirrors of the scratch lanes agree: the read-back noted what the kernel wrote)
  // 4. ONE step of the scratch range, as gpf_simulate_batch steps it
  return simulate_step(e, ne, nc, time_step, o, who, &e->fan.sec.p, &e->fan.sec.pb);
}

}  // namespace

int la_mark_lanes(gpf_engine* e) {
  const LaneFan& f = e->fan;
  for (int i = 0; i < f.n_env; ++i)
    for (int k = 0; k < f.K; ++k) e->h_lane_table[f.lane(i, k)] = e->h_lane_table[i];      // (their offsets are absolute rows: not mirrored)
  return fan_mark_lanes(e, e->h_lane_forecast, 1);     // (gpf_simulate_batch refuses them as sources: chained horizons are out of scope)
}

extern "C" {

int gpf_set_lookahead(gpf_handle e, int32_t n_env, int32_t n_cand) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_lookahead: null");
  const std::string at = "gpf_set_lookahead: ";
  if (n_cand == 0) {
    if (!e->fan.owned_by(LA)) return GPF_OK;
    if (e->fan.on(LA)) {
      HIP_TRY(hipSetDevice(e->device));
      HIP_TRY(hipStreamSynchronize(e->stream));
      int rc = fan_mark_lanes(e, e->h_lane_forecast, 0);   // the scratch lanes are ordinary lanes again
      if (rc != GPF_OK) return rc;
      e->plan_valid = false;
    }
    la_release(e);
    return GPF_OK;
  }
  if (n_cand < 0) return fail(GPF_E_INVALID, at + "negative n_cand");
  if (n_env <= 0) return fail(GPF_E_INVALID, at + "n_env must be positive");
  if (e->fan.owned_by(FanOwner::n1_screen))
    return fail(GPF_E_INVALID, at + "the N-1 screen (gpf_set_n1_screen) is on and claims the lanes behind the environments: switch it off first");
  int rc = la_check_table(e, at);
  if (rc != GPF_OK) return rc;
  if ((long long)n_env * (1 + (long long)n_cand) > (long long)e->n_lanes)
    return fail(GPF_E_CAPACITY, at + std::to_string(n_env) + " environments x (1 + " + std::to_string(n_cand) + " candidates) need " +
                                std::to_string((long long)n_env * (1 + (long long)n_cand)) + " lanes, the engine has " + std::to_string(e->n_lanes));
  const gpf::GridDev& g = e->g;
  if (gpf::topo_prestep_lds_ints(g.dim_topo, g.n_line, g.n_sub, g.n_shunt, g.n_busbar) * sizeof(int) > LA_LDS_LIMIT)
    return fail(GPF_E_CAPACITY, at + "the grid's rows do not fit the 64 KiB of LDS of the play kernel");
  if (e->dry) {
    la_release(e);
    e->fan.claim(LA, n_env, n_cand, true);
    return fail(GPF_E_DEVICE, "gpf_set_lookahead: header-only handle: no HIP device");
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->fan.on(LA)) { rc = fan_mark_lanes(e, e->h_lane_forecast, 0); if (rc != GPF_OK) return rc; }
  la_release(e);
  const size_t ne = (size_t)n_env, nc = ne * (size_t)n_cand, w = (size_t)g.dim_topo + g.n_shunt;
  std::vector<int> none(nc, -1), iota(ne);
  for (size_t i = 0; i < ne; ++i) iota[i] = (int)i;
  hipError_t err = e->la_cand.upload(none.data(), nc);       // every slot starts as the do-nothing candidate
  if (err == hipSuccess) err = e->la_src.upload(iota.data(), ne);
  if (err == hipSuccess) err = e->la_value.alloc(nc);
  if (err == hipSuccess) err = e->la_flags.alloc(nc);
  if (err == hipSuccess) err = e->la_best.alloc(ne);
  if (err == hipSuccess) err = e->la_best_value.alloc(ne);
  if (err == hipSuccess) err = e->la_info.alloc(ne * 2);
  if (err == hipSuccess) err = e->la_moved_list.alloc(nc, w);
  if (err == hipSuccess) err = e->la_noted.alloc(nc * w);
  if (err == hipSuccess) err = hipMemset(e->la_value.p, 0, nc * sizeof(float));
  if (err == hipSuccess) err = hipMemset(e->la_flags.p, 0, nc);
  if (err == hipSuccess) err = hipMemset(e->la_best.p, 0xff, ne * sizeof(int));
  if (err == hipSuccess) err = hipMemset(e->la_best_value.p, 0, ne * sizeof(float));
  if (err == hipSuccess) err = hipMemset(e->la_info.p, 0, ne * 2 * sizeof(int));
  if (err == hipSuccess) err = hipMemset(e->la_moved_list.list.p, 0, (nc + 1) * sizeof(int));
  if (err != hipSuccess) { la_release(e); HIP_TRY(err); }
  e->fan.claim(LA, n_env, n_cand, false);
  rc = la_mark_lanes(e);
  if (rc == GPF_OK) rc = la_upload_noted(e);
  if (rc != GPF_OK) la_release(e);
  e->plan_valid = false;                    // (the first call plans the two ranges)
  return rc;
}

int gpf_lookahead(gpf_handle e, int32_t t_obs, int32_t time_step, const int32_t* cand, const gpf_step_opts* o) {
  if (!e || !o) return fail(GPF_E_INVALID, "gpf_lookahead: null");
  int rc = la_check(e, "gpf_lookahead", time_step);
  if (rc != GPF_OK) return rc;
  if (e->dry) return fail(GPF_E_DEVICE, "gpf_lookahead: header-only handle: no HIP device");
  rc = la_play_and_step(e, "gpf_lookahead", t_obs, time_step, cand, o);
  if (rc != GPF_OK) return rc;
  // 5. values, flags, the best playable slot
  const int ne = e->fan.n_env, nc = e->fan.n_sec();
  const gpf::LaDev d = la_dev(e, t_obs, time_step);
  hipLaunchKernelGGL(gpf::la_reduce_kernel, dim3((unsigned)((nc + gpf::LA_WPB - 1) / gpf::LA_WPB)), dim3(64 * gpf::LA_WPB), 0, e->stream, d, e->g.n_line);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(gpf::la_summary_kernel, dim3((unsigned)((ne + gpf::LA_WPB - 1) / gpf::LA_WPB)), dim3(64 * gpf::LA_WPB), 0, e->stream, d);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

int gpf_set_lookahead_chain(gpf_handle e, int32_t max_steps) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_lookahead_chain: null");
  const std::string at = "gpf_set_lookahead_chain: ";
  if (max_steps == 0) {
    if (e->lc_on) { HIP_TRY(hipSetDevice(e->device)); HIP_TRY(hipStreamSynchronize(e->stream)); }
    la_chain_release(e);
    return GPF_OK;
  }
  if (max_steps < 0) return fail(GPF_E_INVALID, at + "negative max_steps");
  if (!e->fan.owned_by(LA)) return fail(GPF_E_INVALID, at + "the look-ahead is off (gpf_set_lookahead): the chain runs on its scratch lanes");
  if (e->dry) {
    la_chain_release(e);
    e->lc_host_on = true; e->lc_max = max_steps;
    return fail(GPF_E_DEVICE, "gpf_set_lookahead_chain: header-only handle: no HIP device");
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  la_chain_release(e);
  const size_t ne = (size_t)e->fan.n_env, nc = (size_t)e->fan.n_sec();
  hipError_t err = e->lc_survived.alloc(nc);
  if (err == hipSuccess) err = e->lc_peak.alloc(nc);
  if (err == hipSuccess) err = e->lc_value_h.alloc(nc * (size_t)max_steps);
  if (err == hipSuccess) err = e->lc_fallback.alloc(ne);
  if (err == hipSuccess) err = e->lc_fallback_steps.alloc(ne);
  if (err == hipSuccess) err = hipMemset(e->lc_survived.p, 0, nc * sizeof(int));
  if (err == hipSuccess) err = hipMemset(e->lc_peak.p, 0, nc * sizeof(float));
  if (err == hipSuccess) err = hipMemset(e->lc_value_h.p, 0, nc * (size_t)max_steps * sizeof(float));
  if (err == hipSuccess) err = hipMemset(e->lc_fallback.p, 0xff, ne * sizeof(int));
  if (err == hipSuccess) err = hipMemset(e->lc_fallback_steps.p, 0, ne * sizeof(int));
  if (err != hipSuccess) { la_chain_release(e); HIP_TRY(err); }
  e->lc_max = max_steps; e->lc_on = true;
  return GPF_OK;
}

int gpf_lookahead_chain(gpf_handle e, int32_t t_obs, int32_t n_steps, const int32_t* cand, int32_t play, const gpf_step_opts* o) {
  if (!e || !o) return fail(GPF_E_INVALID, "gpf_lookahead_chain: null");
  const char* who = "gpf_lookahead_chain";
  const std::string at = "gpf_lookahead_chain: ";
  if (!e->fan.owned_by(LA)) return fail(GPF_E_INVALID, at + "the look-ahead is off (gpf_set_lookahead)");
  if (!e->lc_on && !e->lc_host_on) return fail(GPF_E_INVALID, at + "the chain is off (gpf_set_lookahead_chain)");
  if (n_steps < 1) return fail(GPF_E_INVALID, at + "n_steps must be at least 1");
  if (n_steps > e->lc_max)
    return fail(GPF_E_INVALID, at + "n_steps = " + std::to_string(n_steps) + " exceeds max_steps = " + std::to_string(e->lc_max) + " of gpf_set_lookahead_chain");
  if (play < 0 || play > 2) return fail(GPF_E_INVALID, at + "play must be 0 (nothing), 1 (the best slot) or 2 (the best slot, else the fall-back)");
  if (play && e->ta_n_slot != 1)
    return fail(GPF_E_INVALID, at + "play needs one action slot per lane (gpf_set_topo_slots is " + std::to_string(e->ta_n_slot) +
                                    "): the choice is one table index in the lane's action buffer");
  int rc = la_check(e, who, n_steps);       // (a horizon beyond the uploaded forecasts: gpf_lookahead's refusal of that horizon)
  if (rc != GPF_OK) return rc;
  if (e->dry) return fail(GPF_E_DEVICE, "gpf_lookahead_chain: header-only handle: no HIP device");
  if (play && !e->ta_act.p) return fail(GPF_E_INVALID, at + "internal (no action buffer)");
  // step 1: gpf_lookahead(t_obs, 1) up to its step
  rc = la_play_and_step(e, who, t_obs, 1, cand, o);
  if (rc != GPF_OK) return rc;
  const int ne = e->fan.n_env, nc = e->fan.n_sec();
  const gpf::LaDev d = la_dev(e, t_obs, 1);
  const gpf::LaChainDev c = la_chain_dev(e);
  const dim3 grid_q((unsigned)((nc + gpf::LA_WPB - 1) / gpf::LA_WPB)), grid_e((unsigned)((ne + gpf::LA_WPB - 1) / gpf::LA_WPB)), block(64 * gpf::LA_WPB);
  for (int h = 1; h <= n_steps; ++h) {
    // the sticky reduce of step h and, but for the last, the lanes' move to the forecast row and the maintenance of step h + 1
    hipLaunchKernelGGL(gpf::la_chain_kernel, grid_q, block, 0, e->stream, d, c, h, h < n_steps ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (h == n_steps) break;
    // a do-nothing step on the cached plan: a line outage never changes a lane's planning class
    rc = simulate_step(e, ne, nc, h + 1, o, who, &e->fan.sec.p, &e->fan.sec.pb);
    if (rc != GPF_OK) return rc;
  }
  hipLaunchKernelGGL(gpf::la_chain_summary_kernel, grid_e, block, 0, e->stream, d, c, (int)play);
  HIP_TRY(hipGetLastError());
  if (play) e->ta_dev = true;               // (as gpf_topo_actions_on_device(1): the next gpf_step_n plays what the kernel wrote)
  return GPF_OK;
}

int gpf_get_lookahead_chain(gpf_handle e, int32_t env0, int32_t n, int32_t* survived, float* peak, float* value_h, int32_t* fallback, int32_t* fallback_steps) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_lookahead_chain: null");
  if (!e->lc_on) return fail(GPF_E_INVALID, "gpf_get_lookahead_chain: the chain is off (gpf_set_lookahead_chain)");
  if (env0 < 0 || n < 0 || env0 + n > e->fan.n_env) return fail(GPF_E_INVALID, "gpf_get_lookahead_chain: bad environment range");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  const size_t K = (size_t)e->fan.K, H = (size_t)e->lc_max;
  if (survived) HIP_TRY(hipMemcpyAsync(survived, e->lc_survived.p + env0 * K, n * K * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (peak) HIP_TRY(hipMemcpyAsync(peak, e->lc_peak.p + env0 * K, n * K * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (value_h) HIP_TRY(hipMemcpyAsync(value_h, e->lc_value_h.p + env0 * K * H, n * K * H * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (fallback) HIP_TRY(hipMemcpyAsync(fallback, e->lc_fallback.p + env0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (fallback_steps) HIP_TRY(hipMemcpyAsync(fallback_steps, e->lc_fallback_steps.p + env0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_lookahead_chain_device_pointers(gpf_handle e, void** out, int32_t n) {
  if (!e || !out || n != GPF_N_LOOKAHEAD_CHAIN_POINTERS)
    return fail(GPF_E_INVALID, "gpf_lookahead_chain_device_pointers: null, or n is not GPF_N_LOOKAHEAD_CHAIN_POINTERS");
  if (!e->lc_on) return fail(GPF_E_INVALID, "gpf_lookahead_chain_device_pointers: the chain is off (gpf_set_lookahead_chain)");
  out[0] = e->lc_survived.p; out[1] = e->lc_peak.p; out[2] = e->lc_value_h.p; out[3] = e->lc_fallback.p; out[4] = e->lc_fallback_steps.p;
  return GPF_OK;
}

int gpf_get_lookahead(gpf_handle e, int32_t env0, int32_t n, float* value, uint8_t* flags, int32_t* best, float* best_value, int32_t* info) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_lookahead: null");
  if (!e->fan.on(LA)) return fail(GPF_E_INVALID, "gpf_get_lookahead: the look-ahead is off (gpf_set_lookahead)");
  if (env0 < 0 || n < 0 || env0 + n > e->fan.n_env) return fail(GPF_E_INVALID, "gpf_get_lookahead: bad environment range");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  const size_t K = (size_t)e->fan.K;
  if (value) HIP_TRY(hipMemcpyAsync(value, e->la_value.p + env0 * K, n * K * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (flags) HIP_TRY(hipMemcpyAsync(flags, e->la_flags.p + env0 * K, n * K, hipMemcpyDeviceToHost, e->stream));
  if (best) HIP_TRY(hipMemcpyAsync(best, e->la_best.p + env0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (best_value) HIP_TRY(hipMemcpyAsync(best_value, e->la_best_value.p + env0, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (info) HIP_TRY(hipMemcpyAsync(info, e->la_info.p + (size_t)env0 * 2, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_lookahead_device_pointers(gpf_handle e, void** out, int32_t n) {
  if (!e || !out || n != GPF_N_LOOKAHEAD_POINTERS) return fail(GPF_E_INVALID, "gpf_lookahead_device_pointers: null, or n is not GPF_N_LOOKAHEAD_POINTERS");
  if (!e->fan.on(LA)) return fail(GPF_E_INVALID, "gpf_lookahead_device_pointers: the look-ahead is off (gpf_set_lookahead)");
  out[0] = e->la_cand.p; out[1] = e->la_value.p; out[2] = e->la_flags.p; out[3] = e->la_best.p; out[4] = e->la_best_value.p; out[5] = e->la_info.p;
  return GPF_OK;
}

}  // extern "C"
