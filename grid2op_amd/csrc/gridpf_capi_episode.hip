// gridpf_capi_episode.hip -- the episode limits' entry points of the C ABI (include/gridpf.h: gpf_set_episode_limit, gpf_get_episode_ends,
// gpf_get_episode_stats, gpf_episode_device_pointers) and the host side of episode_kernel (gridpf_episode.hpp), on the engine of
// gridpf_engine.hpp.  Everything a descriptor can get wrong is refused here, before the device is touched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#define GPF_EPISODE_KERNEL
#include "gridpf_engine.hpp"
#include "gridpf_episode.hpp"

static_assert(gpf::EP_MAX_SLOTS == GPF_REWARD_MAX_SLOTS, "the returns' rows hold every reward slot");

namespace {

void episode_off(gpf_engine* e) {
  e->ep_on = e->ep_host_on = false;
  e->ep_limit.release(); e->ep_flags.release(); e->ep_length.release(); e->ep_duration.release(); e->ep_steps_prev.release();
  e->ep_ret_run.release(); e->ep_ret_last.release(); e->ep_length_last.release(); e->ep_n_episodes.release();
}

// every buffer but the limits of lanes [lane0, lane0 + n) to zero; steps_prev takes the lanes' episode[0] (from_episode) or 0
hipError_t episode_clear(gpf_engine* e, int lane0, int n, bool from_episode) {
  const size_t l0 = (size_t)lane0, k = (size_t)n;
  hipError_t err = hipMemsetAsync(e->ep_flags.p + l0 * 2, 0, k * 2, e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(e->ep_length.p + l0, 0, k * sizeof(int), e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(e->ep_duration.p + l0, 0, k * sizeof(float), e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(e->ep_ret_run.p + l0 * gpf::EP_MAX_SLOTS, 0, k * gpf::EP_MAX_SLOTS * sizeof(double), e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(e->ep_ret_last.p + l0 * gpf::EP_MAX_SLOTS, 0, k * gpf::EP_MAX_SLOTS * sizeof(double), e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(e->ep_length_last.p + l0, 0, k * sizeof(int), e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(e->ep_n_episodes.p + l0, 0, k * sizeof(int), e->stream);
  if (err == hipSuccess)
    err = from_episode ? hipMemcpy2DAsync(e->ep_steps_prev.p + l0, sizeof(int), e->episode.p + l0 * 2, 2 * sizeof(int), sizeof(int), k,
                                          hipMemcpyDeviceToDevice, e->stream)
                       : hipMemsetAsync(e->ep_steps_prev.p + l0, 0, k * sizeof(int), e->stream);
  return err;
}

}  // namespace

int episode_poststep(gpf_engine* e, bool auto_reset, bool track_cooldown, bool list_resets) {
  const gpf::GridDev& g = e->g;
  gpf::EpisodeDev d{};
  d.limit = e->ep_limit.p; d.episode = e->episode.p; d.done = e->done.p; d.flags = e->ep_flags.p; d.length = e->ep_length.p;
  d.duration = e->ep_duration.p; d.steps_prev = e->ep_steps_prev.p;
  d.reward = e->rw_on ? e->rw_out.p : nullptr; d.n_slot = e->rw_n_slot;
  d.ret_run = e->ep_ret_run.p; d.ret_last = e->ep_ret_last.p; d.length_last = e->ep_length_last.p; d.n_episodes = e->ep_n_episodes.p;
  d.per_timestep = e->ep_per_timestep;
  d.auto_reset = auto_reset ? 1 : 0;
  d.dim_topo = g.dim_topo; d.n_line = g.n_line; d.n_sub = g.n_sub; d.n_gen = g.n_gen; d.n_sto = g.n_sto; d.n_shunt = g.n_shunt;
  d.topo = e->topo.p; d.topo0 = e->topo0.p; d.overflow_count = e->overflow_count.p;
  d.cooldown = track_cooldown ? e->cooldown.p : nullptr;
  if (e->env_on) {
    d.env_target = e->env_target.p; d.env_actual = e->env_actual.p; d.env_prev = e->env_prev.p; d.env_limit = e->env_limit.p;
    d.env_amount_prev = e->env_amount_prev.p; d.env_curt_prev = e->env_curt_prev.p; d.env_charge = e->env_charge.p;
    d.env_charge0 = e->sto_charge0.n ? e->sto_charge0.p : nullptr;
    d.env_already = e->env_already.p; d.env_fresh = e->env_fresh.p; d.env_illegal = e->env_illegal.p;
  }
  if (e->ta_on) { d.sub_cd = e->ta_sub_cd.p; d.last_bus = e->ta_last_bus.p; }
  if (list_resets) { d.list = e->ta_moved_list.list.p; d.list_rows = e->ta_moved_list.rows.p; d.shunt_bus = e->shunt_bus.p; }
  const unsigned blocks = (unsigned)((e->n_lanes + gpf::EP_WPB - 1) / gpf::EP_WPB);
  hipLaunchKernelGGL(gpf::episode_kernel, dim3(blocks), dim3(64 * gpf::EP_WPB), 0, e->stream, d, e->n_lanes);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

int episode_reset_lanes(gpf_engine* e, int lane0, int n) {
  HIP_TRY(episode_clear(e, lane0, n, false));
  return GPF_OK;
}

hipError_t episode_copy_lanes(gpf_engine* e, int src, int dst, int n) {
  auto cp = [&](auto* p, size_t stride) {
    return hipMemcpyAsync(p + (size_t)dst * stride, p + (size_t)src * stride, (size_t)n * stride * sizeof(*p), hipMemcpyDeviceToDevice, e->stream);
  };
  hipError_t err = cp(e->ep_limit.p, 1);
  if (err == hipSuccess) err = cp(e->ep_flags.p, 2);
  if (err == hipSuccess) err = cp(e->ep_length.p, 1);
  if (err == hipSuccess) err = cp(e->ep_duration.p, 1);
  if (err == hipSuccess) err = cp(e->ep_steps_prev.p, 1);
  if (err == hipSuccess) err = cp(e->ep_ret_run.p, gpf::EP_MAX_SLOTS);
  if (err == hipSuccess) err = cp(e->ep_ret_last.p, gpf::EP_MAX_SLOTS);
  if (err == hipSuccess) err = cp(e->ep_length_last.p, 1);
  if (err == hipSuccess) err = cp(e->ep_n_episodes.p, 1);
  return err;
}

int episode_rewards_changed(gpf_engine* e) {
  const size_t bytes = (size_t)e->cap_lanes * gpf::EP_MAX_SLOTS * sizeof(double);
  HIP_TRY(hipMemsetAsync(e->ep_ret_run.p, 0, bytes, e->stream));
  HIP_TRY(hipMemsetAsync(e->ep_ret_last.p, 0, bytes, e->stream));
  return GPF_OK;
}

extern "C" {

int gpf_set_episode_limit(gpf_handle e, const gpf_episode_desc* d) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_episode_limit: null");
  const std::string at = "gpf_set_episode_limit: ";
  bool any = false;
  if (d) {
    if (d->max_steps < 0) return fail(GPF_E_INVALID, at + "negative max_steps");
    if (d->lane_max_steps)
      for (int k = 0; k < e->n_lanes; ++k)
        if (d->lane_max_steps[k] < 0) return fail(GPF_E_INVALID, at + "lane " + std::to_string(k) + ": negative limit");
    if (!std::isfinite(d->per_timestep) || !(d->per_timestep > 0.f)) return fail(GPF_E_INVALID, at + "per_timestep must be finite and positive");
    if (!std::isfinite(d->alert_end_bonus)) return fail(GPF_E_INVALID, at + "alert_end_bonus is not finite");
    any = d->max_steps > 0 || d->lane_max_steps != nullptr;
  }
  if (!any) {
    if (e->ep_on && !e->dry) { HIP_TRY(hipSetDevice(e->device)); HIP_TRY(hipStreamSynchronize(e->stream)); }
    episode_off(e);
    return GPF_OK;
  }
  if (e->dry) {
    e->ep_host_on = true;
    return fail(GPF_E_DEVICE, "gpf_set_episode_limit: header-only handle: no HIP device");
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t cap = (size_t)e->cap_lanes;
  std::vector<int> lim(cap, 0);
  for (int k = 0; k < e->n_lanes; ++k) lim[k] = d->lane_max_steps ? d->lane_max_steps[k] : d->max_steps;
  if (!e->ep_on) {                    // a new limit on a running feature keeps the lanes' statistics
    episode_off(e);
    hipError_t err = e->ep_limit.alloc(cap);
    if (err == hipSuccess) err = e->ep_flags.alloc(cap * 2);
    if (err == hipSuccess) err = e->ep_length.alloc(cap);
    if (err == hipSuccess) err = e->ep_duration.alloc(cap);
    if (err == hipSuccess) err = e->ep_steps_prev.alloc(cap);
    if (err == hipSuccess) err = e->ep_ret_run.alloc(cap * gpf::EP_MAX_SLOTS);
    if (err == hipSuccess) err = e->ep_ret_last.alloc(cap * gpf::EP_MAX_SLOTS);
    if (err == hipSuccess) err = e->ep_length_last.alloc(cap);
    if (err == hipSuccess) err = e->ep_n_episodes.alloc(cap);
    if (err == hipSuccess) err = episode_clear(e, 0, e->cap_lanes, true);
    if (err != hipSuccess) { episode_off(e); HIP_TRY(err); }
  }
  hipError_t err = hipMemcpyAsync(e->ep_limit.p, lim.data(), cap * sizeof(int), hipMemcpyHostToDevice, e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);        // (lim is on this frame)
  if (err != hipSuccess) { episode_off(e); HIP_TRY(err); }
  e->ep_per_timestep = d->per_timestep; e->ep_alert_bonus = d->alert_end_bonus;
  e->ep_on = true;
  return GPF_OK;
}

int gpf_get_episode_ends(gpf_handle e, int32_t lane0, int32_t n, uint8_t* terminated, uint8_t* truncated, int32_t* length, float* duration_reward) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_episode_ends: null");
  if (!e->ep_on) return fail(GPF_E_INVALID, "gpf_get_episode_ends: episode limits are off (gpf_set_episode_limit)");
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_get_episode_ends: bad lane range");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  std::vector<unsigned char> fl((size_t)n * 2);
  HIP_TRY(hipMemcpyAsync(fl.data(), e->ep_flags.p + (size_t)lane0 * 2, fl.size(), hipMemcpyDeviceToHost, e->stream));
  if (length) HIP_TRY(hipMemcpyAsync(length, e->ep_length.p + lane0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (duration_reward) HIP_TRY(hipMemcpyAsync(duration_reward, e->ep_duration.p + lane0, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < n; ++k) {
    if (terminated) terminated[k] = fl[(size_t)k * 2];
    if (truncated) truncated[k] = fl[(size_t)k * 2 + 1];
  }
  return GPF_OK;
}

int gpf_get_episode_stats(gpf_handle e, int32_t lane0, int32_t n, double* return_running, double* return_last, int32_t* length_last,
                          int32_t* n_episodes) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_episode_stats: null");
  if (!e->ep_on) return fail(GPF_E_INVALID, "gpf_get_episode_stats: episode limits are off (gpf_set_episode_limit)");
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_get_episode_stats: bad lane range");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  const size_t w = gpf::EP_MAX_SLOTS;
  if (return_running) HIP_TRY(hipMemcpyAsync(return_running, e->ep_ret_run.p + (size_t)lane0 * w, (size_t)n * w * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (return_last) HIP_TRY(hipMemcpyAsync(return_last, e->ep_ret_last.p + (size_t)lane0 * w, (size_t)n * w * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (length_last) HIP_TRY(hipMemcpyAsync(length_last, e->ep_length_last.p + lane0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (n_episodes) HIP_TRY(hipMemcpyAsync(n_episodes, e->ep_n_episodes.p + lane0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_episode_device_pointers(gpf_handle e, void** out, int32_t n) {
  if (!e || !out || n != GPF_N_EPISODE_POINTERS) return fail(GPF_E_INVALID, "gpf_episode_device_pointers: null, or n is not GPF_N_EPISODE_POINTERS");
  if (!e->ep_on) return fail(GPF_E_INVALID, "gpf_episode_device_pointers: episode limits are off (gpf_set_episode_limit)");
  out[0] = e->ep_limit.p; out[1] = e->ep_flags.p; out[2] = e->ep_length.p; out[3] = e->ep_duration.p; out[4] = e->ep_ret_run.p;
  out[5] = e->ep_ret_last.p; out[6] = e->ep_length_last.p; out[7] = e->ep_n_episodes.p;
  return GPF_OK;
}

}  // extern "C"
