// gridpf_capi_alert.hip -- the alerts' entry points of the C ABI (include/gridpf.h: gpf_set_alerts, gpf_set_lane_alerts, gpf_alerts_on_device,
// gpf_alert_state_ints, gpf_get_alert_state, gpf_set_alert_state, gpf_get_alert_reward, gpf_alert_device_pointers) and the host side of
// alert_prestep_kernel / alert_poststep_kernel (gridpf_alert.hpp), on the engine of gridpf_engine.hpp.  Everything a descriptor, a mask
// or a state row can get wrong is refused here, before the device is touched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "gridpf_engine.hpp"
#include "gridpf_alert.hpp"

namespace {

gpf::AlertCfg alert_cfg(const gpf_engine* e) {
  const gpf_alert_desc& d = e->al_desc;
  return gpf::AlertCfg{e->al_A, d.time_window, d.reward_min_no_blackout, d.reward_min_blackout, d.reward_max_no_blackout, d.reward_max_blackout};
}

gpf::AlertDev alert_dev(const gpf_engine* e, bool with_act) {
  gpf::AlertDev d{};
  d.obs = e->al_obs.p; d.aux = e->al_aux.p; d.act = with_act ? e->al_act.p : nullptr; d.reward = e->al_reward.p;
  d.done = e->done.p; d.episode = e->episode.p;
  if (e->opp_n_area > 0) {
    d.info = e->opp_area_state.p + GPF_OPP_AS_INFO_LINE; d.info_lane = e->opp_n_area * GPF_OPP_AREA_STATE_INTS; d.info_area = GPF_OPP_AREA_STATE_INTS;
    d.lines = e->opp_area_lines.p;
  } else {
    d.info = e->opp_state.p + GPF_OPP_S_INFO_LINE; d.info_lane = GPF_OPP_STATE_INTS; d.info_area = 0;
    d.lines = e->opp_lines.p;
  }
  d.area_of = e->al_area_of.p;
  if (e->ep_on) { d.ep_limit = e->ep_limit.p; d.end_bonus = e->ep_alert_bonus; }
  return d;
}

size_t obs_ints(const gpf_engine* e) { return (size_t)gpf::alert_obs_ints(e->al_A); }
size_t aux_words(const gpf_engine* e) { return (size_t)gpf::alert_aux_words(e->al_desc.time_window); }
size_t state_ints(int A, int W) { return (size_t)8 * A + 3 + (size_t)2 * (W + 2) * A; }

// the reset rows of lanes [lane0, lane0 + n): BaseEnv._reset_alert + AlertReward.reset, reward 0 (queued on the engine's stream)
int alert_clear(gpf_engine* e, int lane0, int n) {
  if (n == 0) return GPF_OK;
  const int A = e->al_A;
  const size_t no = obs_ints(e);
  std::vector<int> ob((size_t)n * no, 0);
  for (int k = 0; k < n; ++k)
    for (int t = 0; t < A; ++t) { ob[k * no + gpf::AO_SINCE_ALERT * A + t] = -1; ob[k * no + gpf::AO_SINCE_ATTACK * A + t] = -1; }
  HIP_TRY(hipMemcpyAsync(e->al_obs.p + (size_t)lane0 * no, ob.data(), ob.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemsetAsync(e->al_aux.p + (size_t)lane0 * aux_words(e), 0, (size_t)n * aux_words(e) * sizeof(unsigned long long), e->stream));
  HIP_TRY(hipMemsetAsync(e->al_reward.p + lane0, 0, (size_t)n * sizeof(float), e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));      // (ob is read by the copy)
  return GPF_OK;
}

}  // namespace

void alerts_off(gpf_engine* e) {
  e->al_on = e->al_host = e->al_dev = false;
  e->al_A = e->al_host_A = 0;
  e->al_obs.release(); e->al_area_of.release(); e->al_aux.release(); e->al_act.release(); e->al_reward.release();
}

int alert_prestep(gpf_engine* e) {
  const bool with_act = e->al_host || e->al_dev;
  e->al_host = e->al_dev = false;             // consumed by this launch, whatever happens below
  const unsigned blocks = (unsigned)((e->n_lanes + gpf::ALERT_WPB - 1) / gpf::ALERT_WPB);
  hipLaunchKernelGGL(gpf::alert_prestep_kernel, dim3(blocks), dim3(64 * gpf::ALERT_WPB), 0, e->stream, alert_cfg(e), alert_dev(e, with_act), e->n_lanes);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

int alert_poststep(gpf_engine* e) {
  const unsigned blocks = (unsigned)((e->n_lanes + gpf::ALERT_WPB - 1) / gpf::ALERT_WPB);
  hipLaunchKernelGGL(gpf::alert_poststep_kernel, dim3(blocks), dim3(64 * gpf::ALERT_WPB), 0, e->stream, alert_cfg(e), alert_dev(e, false), e->n_lanes);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

hipError_t alert_copy_lanes(gpf_engine* e, int src, int dst, int n) {
  auto cp = [&](auto* p, size_t stride) {
    return hipMemcpyAsync(p + (size_t)dst * stride, p + (size_t)src * stride, (size_t)n * stride * sizeof(*p), hipMemcpyDeviceToDevice, e->stream);
  };
  hipError_t err = cp(e->al_obs.p, obs_ints(e));
  if (err == hipSuccess) err = cp(e->al_aux.p, aux_words(e));
  if (err == hipSuccess) err = cp(e->al_reward.p, 1);
  return err;
}

int alert_reset_lanes(gpf_engine* e, int lane0, int n) { return alert_clear(e, lane0, n); }

extern "C" {

int gpf_set_alerts(gpf_handle e, const gpf_alert_desc* d) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_alerts: null");
  if (!d) {
    if (e->al_on && !e->dry) { HIP_TRY(hipSetDevice(e->device)); HIP_TRY(hipStreamSynchronize(e->stream)); }
    alerts_off(e);
    return GPF_OK;
  }
  const std::string at = "gpf_set_alerts: ";
  if (!e->opp_host_kind || (!e->dry && !e->opp_kind))
    return fail(GPF_E_INVALID, at + "no opponent (gpf_set_opponent): the alertable lines are the opponent's attackable lines");
  const int A = (int)e->opp_host_lines.size();
  if (A > GPF_ALERT_MAX_LINES)
    return fail(GPF_E_INVALID, at + std::to_string(A) + " alertable lines: more than GPF_ALERT_MAX_LINES = " + std::to_string(GPF_ALERT_MAX_LINES));
  if (d->time_window < 1 || d->time_window > GPF_ALERT_MAX_WINDOW)
    return fail(GPF_E_INVALID, at + "time_window " + std::to_string(d->time_window) + " is outside [1, GPF_ALERT_MAX_WINDOW = " + std::to_string(GPF_ALERT_MAX_WINDOW) + "]");
  for (float v : {d->reward_min_no_blackout, d->reward_min_blackout, d->reward_max_no_blackout, d->reward_max_blackout})
    if (!std::isfinite(v)) return fail(GPF_E_INVALID, at + "a reward constant is not finite");
  if (e->dry) {
    e->al_host_A = A;
    return fail(GPF_E_DEVICE, "gpf_set_alerts: header-only handle: no HIP device");
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  alerts_off(e);
  e->al_desc = *d; e->al_A = A; e->al_host_A = A;
  std::vector<int> area_of(A, 0);
  for (int a = 0; a < e->opp_n_area; ++a)
    for (int i = e->opp_area_off[a]; i < e->opp_area_off[a + 1]; ++i) area_of[i] = a;
  const size_t cap = (size_t)e->cap_lanes;
  hipError_t err = e->al_area_of.upload(area_of.data(), area_of.size());
  if (err == hipSuccess) err = e->al_obs.alloc(cap * obs_ints(e));
  if (err == hipSuccess) err = e->al_aux.alloc(cap * aux_words(e));
  if (err == hipSuccess) err = e->al_act.alloc(cap);
  if (err == hipSuccess) err = e->al_reward.alloc(cap);
  if (err == hipSuccess) err = hipMemset(e->al_act.p, 0, cap * sizeof(unsigned long long));
  if (err != hipSuccess) { alerts_off(e); HIP_TRY(err); }
  int rc = alert_clear(e, 0, e->cap_lanes);
  if (rc != GPF_OK) { alerts_off(e); return rc; }
  e->al_on = true;
  return GPF_OK;
}

int gpf_set_lane_alerts(gpf_handle e, const uint64_t* mask) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_lane_alerts: null");
  if (!e->al_on && !(e->dry && e->al_host_A > 0)) return fail(GPF_E_INVALID, "gpf_set_lane_alerts: alerts are off (gpf_set_alerts)");
  const int A = e->al_host_A;
  if (mask)
    for (int k = 0; k < e->n_lanes; ++k)
      if (mask[k] & ~gpf::alert_valid_bits(A))
        return fail(GPF_E_INVALID, "gpf_set_lane_alerts: lane " + std::to_string(k) + ": an alert on a line at or above the " + std::to_string(A) + " alertable lines");
  if (e->dry) return fail(GPF_E_DEVICE, "gpf_set_lane_alerts: header-only handle: no HIP device");
  e->al_dev = false;
  if (!mask) { e->al_host = false; return GPF_OK; }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(e->al_act.p, mask, (size_t)e->n_lanes * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));      // (the caller's array is free on return)
  e->al_host = true;
  return GPF_OK;
}

int gpf_alerts_on_device(gpf_handle e, int32_t on) {
  if (!e) return fail(GPF_E_INVALID, "gpf_alerts_on_device: null");
  if (!e->al_on) return fail(GPF_E_INVALID, "gpf_alerts_on_device: alerts are off (gpf_set_alerts)");
  e->al_dev = on != 0;
  if (on) e->al_host = false;
  return GPF_OK;
}

int gpf_alert_state_ints(gpf_handle e, int32_t* n_ints) {
  if (!e || !n_ints) return fail(GPF_E_INVALID, "gpf_alert_state_ints: null");
  if (!e->al_on) return fail(GPF_E_INVALID, "gpf_alert_state_ints: alerts are off (gpf_set_alerts)");
  *n_ints = (int32_t)state_ints(e->al_A, e->al_desc.time_window);
  return GPF_OK;
}

int gpf_get_alert_state(gpf_handle e, int32_t lane0, int32_t n, int32_t* state) {
  if (!check_range(e, lane0, n) || !state) return fail(GPF_E_INVALID, "gpf_get_alert_state: bad lane range or null");
  if (!e->al_on) return fail(GPF_E_INVALID, "gpf_get_alert_state: alerts are off (gpf_set_alerts)");
  if (n == 0) return GPF_OK;
  const int A = e->al_A, R = e->al_desc.time_window + 2;
  const size_t no = obs_ints(e), na = aux_words(e), ns = state_ints(A, e->al_desc.time_window);
  std::vector<int> ob((size_t)n * no);
  std::vector<unsigned long long> ax((size_t)n * na);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(ob.data(), e->al_obs.p + (size_t)lane0 * no, ob.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(ax.data(), e->al_aux.p + (size_t)lane0 * na, ax.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < n; ++k) {
    const int* o = &ob[k * no];
    const unsigned long long* x = &ax[k * na];
    int32_t* s = state + k * ns;
    auto bits = [&](int32_t* dst, unsigned long long w) { for (int t = 0; t < A; ++t) dst[t] = (int32_t)((w >> t) & 1); };
    std::copy_n(o + gpf::AO_ACTIVE * A, A, s);
    bits(s + A, x[gpf::AX_ALREADY]);
    std::copy_n(o + gpf::AO_SINCE_ALERT * A, A, s + 2 * A);
    std::copy_n(o + gpf::AO_DURATION * A, A, s + 3 * A);
    std::copy_n(o + gpf::AO_SINCE_ATTACK * A, A, s + 4 * A);
    std::copy_n(o + gpf::AO_UNDER_ALERT * A, A, s + 5 * A);
    std::copy_n(o + gpf::AO_USED * A, A, s + 6 * A);
    s[7 * A] = o[gpf::AO_TOTAL * A];
    s[7 * A + 1] = (int32_t)(uint32_t)x[gpf::AX_ID];
    s[7 * A + 2] = (x[gpf::AX_ID] & gpf::AX_RAN) ? 1 : 0;
    bits(s + 7 * A + 3, x[gpf::AX_CURRENT]);
    for (int r = 0; r < 2 * R; ++r) bits(s + 8 * A + 3 + (size_t)r * A, x[gpf::AX_RINGS + r]);
  }
  return GPF_OK;
}

int gpf_set_alert_state(gpf_handle e, int32_t lane0, int32_t n, const int32_t* state) {
  if (!check_range(e, lane0, n) || !state) return fail(GPF_E_INVALID, "gpf_set_alert_state: bad lane range or null");
  if (!e->al_on) return fail(GPF_E_INVALID, "gpf_set_alert_state: alerts are off (gpf_set_alerts)");
  if (n == 0) return GPF_OK;
  const int A = e->al_A, R = e->al_desc.time_window + 2;
  const size_t no = obs_ints(e), na = aux_words(e), ns = state_ints(A, e->al_desc.time_window);
  std::vector<int> ob((size_t)n * no);
  std::vector<unsigned long long> ax((size_t)n * na);
  for (int k = 0; k < n; ++k) {
    const int32_t* s = state + k * ns;
    int* o = &ob[k * no];
    unsigned long long* x = &ax[k * na];
    const std::string at = "gpf_set_alert_state: lane " + std::to_string(lane0 + k) + ": ";
    bool ok = true;
    auto word = [&](const int32_t* src) { unsigned long long w = 0; for (int t = 0; t < A; ++t) { ok &= src[t] == 0 || src[t] == 1; w |= (unsigned long long)(src[t] & 1) << t; } return w; };
    (void)word(s);
    if (!ok) return fail(GPF_E_INVALID, at + "last_alert is not 0 / 1");
    std::copy_n(s, A, o + gpf::AO_ACTIVE * A);
    x[gpf::AX_ALREADY] = word(s + A);
    x[gpf::AX_CURRENT] = word(s + 7 * A + 3);
    for (int r = 0; r < 2 * R; ++r) x[gpf::AX_RINGS + r] = word(s + 8 * A + 3 + (size_t)r * A);
    if (!ok) return fail(GPF_E_INVALID, at + "a boolean entry (is_already_attacked, _lines_currently_attacked, the rings) is not 0 / 1");
    for (int t = 0; t < A; ++t) {
      if (s[2 * A + t] < -1 || s[4 * A + t] < -1) return fail(GPF_E_INVALID, at + "time_since_last_alert / time_since_last_attack below -1");
      if (s[3 * A + t] < 0) return fail(GPF_E_INVALID, at + "negative alert_duration");
      if (s[5 * A + t] < -1 || s[5 * A + t] > 1 || s[6 * A + t] < -1 || s[6 * A + t] > 1)
        return fail(GPF_E_INVALID, at + "attack_under_alert / was_alert_used_after_attack outside {-1, 0, 1}");
    }
    if (s[7 * A] < 0) return fail(GPF_E_INVALID, at + "negative total_number_of_alert");
    if (s[7 * A + 1] < 0 || s[7 * A + 1] >= R) return fail(GPF_E_INVALID, at + "_current_id is outside [0, time_window + 2)");
    if (s[7 * A + 2] != 0 && s[7 * A + 2] != 1) return fail(GPF_E_INVALID, at + "the ran flag is not 0 / 1");
    std::copy_n(s + 2 * A, A, o + gpf::AO_SINCE_ALERT * A);
    std::copy_n(s + 3 * A, A, o + gpf::AO_DURATION * A);
    std::copy_n(s + 4 * A, A, o + gpf::AO_SINCE_ATTACK * A);
    std::copy_n(s + 5 * A, A, o + gpf::AO_UNDER_ALERT * A);
    std::copy_n(s + 6 * A, A, o + gpf::AO_USED * A);
    o[gpf::AO_TOTAL * A] = s[7 * A];
    x[gpf::AX_ID] = (unsigned long long)(uint32_t)s[7 * A + 1] | (s[7 * A + 2] ? gpf::AX_RAN : 0);
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(e->al_obs.p + (size_t)lane0 * no, ob.data(), ob.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->al_aux.p + (size_t)lane0 * na, ax.data(), ax.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_alert_reward(gpf_handle e, int32_t lane0, int32_t n, float* reward) {
  if (!check_range(e, lane0, n) || !reward) return fail(GPF_E_INVALID, "gpf_get_alert_reward: bad lane range or null");
  if (!e->al_on) return fail(GPF_E_INVALID, "gpf_get_alert_reward: alerts are off (gpf_set_alerts)");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(reward, e->al_reward.p + lane0, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_alert_device_pointers(gpf_handle e, void** out, int32_t n) {
  if (!e || !out || n != GPF_N_ALERT_POINTERS) return fail(GPF_E_INVALID, "gpf_alert_device_pointers: null, or n is not GPF_N_ALERT_POINTERS");
  if (!e->al_on) return fail(GPF_E_INVALID, "gpf_alert_device_pointers: alerts are off (gpf_set_alerts)");
  out[0] = e->al_act.p; out[1] = e->al_reward.p; out[2] = e->al_obs.p;
  return GPF_OK;
}

}  // extern "C"
