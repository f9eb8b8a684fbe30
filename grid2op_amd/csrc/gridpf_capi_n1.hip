// gridpf_capi_n1.hip -- the N-1 screen's entry points of the C ABI (include/gridpf.h: gpf_set_n1_screen, gpf_get_n1_values,
// gpf_get_n1_summary, gpf_n1_device_pointers) and the host side of the kernels of gridpf_n1.hpp, on the engine of gridpf_engine.hpp.
// Everything a screen can get wrong is refused here, before the device is touched.  A launch in which no environment lane changed its
// topology class does no host work that grows with n_env x K: the plans of the two lane ranges are cached (fan_plans).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#define GPF_N1_KERNEL
#include "gridpf_engine.hpp"
#include "gridpf_n1.hpp"

static_assert(gpf::RW_N1 == GPF_RW_N1, "kinds");

namespace {

constexpr FanOwner N1 = FanOwner::n1_screen;

void n1_release(gpf_engine* e) {
  e->n1_slots = false;
  e->n1_lines.release(); e->n1_info.release(); e->n1_slot_idx.release(); e->n1_value.release(); e->n1_worst.release();
  e->fan.release();
}

// the screen that is set goes (the stream has drained): its contingency lanes are ordinary lanes again
int n1_off(gpf_engine* e) {
  if (e->fan.on(N1)) { int rc = fan_mark_lanes(e, e->h_lane_n1, 0); if (rc != GPF_OK) return rc; }
  n1_release(e);
  return GPF_OK;
}

gpf::N1Dev n1_dev(const gpf_engine* e) {
  const gpf::GridDev& g = e->g;
  gpf::N1Dev d{};
  d.lines = e->n1_lines.p; d.inj = e->inj.p; d.topo = e->topo.p; d.shunt_bus = e->shunt_bus.p;
  d.line_or_pos = e->line_or_pos.p; d.line_ex_pos = e->line_ex_pos.p;
  d.out = e->out.p; d.status = e->status.p; d.done = e->done.p; d.thermal = e->thermal_limit.p;
  if (e->ep_on) { d.ep_limit = e->ep_limit.p; d.episode = e->episode.p; }       // a step at the lane's limit is the reference's is_done
  d.value = e->n1_value.p; d.worst = e->n1_worst.p; d.info = e->n1_info.p;
  d.n_env = e->fan.n_env; d.K = e->fan.K; d.n_inj = g.n_inj; d.dim_topo = g.dim_topo; d.n_shunt = g.n_shunt; d.n_line = g.n_line;
  d.n_out = g.n_out; d.off_a_or = e->oo.a_or;
  return d;
}

// the index of a GPF_RW_N1 slot (p[0], a whole number), or -1
int slot_index(const gpf_reward_slot& s) {
  const double v = s.p[0];
  if (!std::isfinite(v) || v != std::floor(v) || v < 0.0 || v > (double)INT_MAX) return -1;
  return (int)v;
}

}  // namespace

int n1_plans(gpf_engine* e) {
  const LaneFan& f = e->fan;
  // a contingency lane carries its environment's planning entries (a single line outage never changes a lane's topology class); the
  // host's mirror of its sent topology is unknown
  if (!(e->plan_valid && f.plans_valid))
    for (int i = 0; i < f.n_env; ++i)
      for (int k = 0; k < f.K; ++k) lane_inherit(e, f.lane(i, k), i, false);
  return fan_plans(e);
}

int n1_screen(gpf_engine* e, int max_iter, double tol_mva) {
  int rc = n1_plans(e);                     // (the topology post-step's read-back may have re-keyed environment lanes)
  if (rc != GPF_OK) return rc;
  const gpf::N1Dev d = n1_dev(e);
  const int nc = d.n_env * d.K;
  hipLaunchKernelGGL(gpf::n1_fanout_kernel, dim3((unsigned)nc), dim3(64), 0, e->stream, d);
  HIP_TRY(hipGetLastError());
  rc = runpf_range(e, d.n_env, nc, 0, max_iter, tol_mva, &e->fan.sec.p, &e->fan.sec.pb);
  if (rc != GPF_OK) return rc;
  hipLaunchKernelGGL(gpf::n1_reduce_kernel, dim3((unsigned)((nc + gpf::N1_WPB - 1) / gpf::N1_WPB)), dim3(64 * gpf::N1_WPB), 0, e->stream, d);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(gpf::n1_summary_kernel, dim3((unsigned)((d.n_env + gpf::N1_WPB - 1) / gpf::N1_WPB)), dim3(64 * gpf::N1_WPB), 0, e->stream, d);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

int n1_fill_slots(gpf_engine* e, int lane0, int n, float* reward, long long row_stride) {
  const int total = n * e->rw_n_slot;
  if (total <= 0 || lane0 >= e->fan.n_env) return GPF_OK;
  hipLaunchKernelGGL(gpf::n1_slot_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, e->n1_value.p, e->n1_slot_idx.p,
                     e->rw_n_slot, e->fan.n_env, e->fan.K, lane0, n, reward, row_stride);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

int n1_check_slots(gpf_engine* e, int n_slot, const gpf_reward_slot* slots) {
  for (int s = 0; s < n_slot; ++s) {
    if (slots[s].kind != GPF_RW_N1) continue;
    const std::string sl = "gpf_set_rewards: slot " + std::to_string(s) + ": ";
    const int K = e->fan.owned_by(N1) ? e->fan.K : 0;
    if (K == 0) return fail(GPF_E_INVALID, sl + "GPF_RW_N1 needs the N-1 screen (gpf_set_n1_screen), which is off");
    const int idx = slot_index(slots[s]);
    if (idx < 0 || idx >= K)
      return fail(GPF_E_INVALID, sl + "GPF_RW_N1: p[0] must be an index into the " + std::to_string(K) + " watched lines of gpf_set_n1_screen");
  }
  return GPF_OK;
}

int n1_set_slots(gpf_engine* e, int n_slot, const gpf_reward_slot* slots) {
  int idx[GPF_REWARD_MAX_SLOTS];
  bool any = false;
  for (int s = 0; s < GPF_REWARD_MAX_SLOTS; ++s) {
    idx[s] = (s < n_slot && slots[s].kind == GPF_RW_N1) ? slot_index(slots[s]) : -1;
    any = any || idx[s] >= 0;
  }
  e->n1_slots = false;
  if (!any) return GPF_OK;
  HIP_TRY(e->n1_slot_idx.upload(idx, GPF_REWARD_MAX_SLOTS));
  e->n1_slots = true;
  return GPF_OK;
}

extern "C" {

int gpf_set_n1_screen(gpf_handle e, int32_t n_env, const int32_t* lines, int32_t n_lines) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_n1_screen: null");
  const std::string at = "gpf_set_n1_screen: ";
  if (e->n1_slots) return fail(GPF_E_INVALID, at + "a reward slot of kind GPF_RW_N1 reads the screen's table: set the rewards anew (gpf_set_rewards) first");
  if (n_lines == 0) {
    if (!e->fan.owned_by(N1)) return GPF_OK;
    if (e->fan.on(N1)) { HIP_TRY(hipSetDevice(e->device)); HIP_TRY(hipStreamSynchronize(e->stream)); }
    return n1_off(e);
  }
  if (e->fan.owned_by(FanOwner::lookahead))
    return fail(GPF_E_INVALID, at + "the look-ahead (gpf_set_lookahead) is set and claims the lanes behind the environments: switch it off first");
  if (n_lines < 0 || !lines) return fail(GPF_E_INVALID, at + "negative n_lines, or no lines");
  for (int k = 0; k < n_lines; ++k)
    if (lines[k] < 0 || lines[k] >= e->g.n_line)
      return fail(GPF_E_INVALID, at + "lines[" + std::to_string(k) + "] = " + std::to_string(lines[k]) + " is outside [0, n_line = " + std::to_string(e->g.n_line) + ")");
  if (n_env <= 0) return fail(GPF_E_INVALID, at + "n_env must be positive");
  if ((long long)n_env * (1 + (long long)n_lines) > (long long)e->n_lanes)
    return fail(GPF_E_CAPACITY, at + std::to_string(n_env) + " environments x (1 + " + std::to_string(n_lines) + " watched lines) need " +
                                std::to_string((long long)n_env * (1 + (long long)n_lines)) + " lanes, the engine has " + std::to_string(e->n_lanes));
  if (e->dry) {
    e->fan.claim(N1, n_env, n_lines, true);
    return fail(GPF_E_DEVICE, "gpf_set_n1_screen: header-only handle: no HIP device");
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = n1_off(e);
  if (rc != GPF_OK) return rc;
  const size_t ne = (size_t)n_env, K = (size_t)n_lines;
  hipError_t err = e->n1_lines.upload(lines, K);
  if (err == hipSuccess) err = e->n1_value.alloc(ne * K);
  if (err == hipSuccess) err = e->n1_worst.alloc(ne);
  if (err == hipSuccess) err = e->n1_info.alloc(ne * 3);
  if (err == hipSuccess) err = hipMemset(e->n1_value.p, 0, ne * K * sizeof(float));
  if (err == hipSuccess) err = hipMemset(e->n1_worst.p, 0, ne * sizeof(float));
  if (err == hipSuccess) err = hipMemset(e->n1_info.p, 0, ne * 3 * sizeof(int));
  if (err != hipSuccess) { n1_release(e); HIP_TRY(err); }
  e->fan.claim(N1, n_env, n_lines, false);
  rc = fan_mark_lanes(e, e->h_lane_n1, 1);
  if (rc == GPF_OK) HIP_TRY(hipStreamSynchronize(e->stream));
  if (rc != GPF_OK) n1_release(e);
  return rc;
}

int gpf_get_n1_values(gpf_handle e, int32_t lane0, int32_t n, float* value) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_n1_values: null");
  if (!e->fan.on(N1)) return fail(GPF_E_INVALID, "gpf_get_n1_values: the N-1 screen is off (gpf_set_n1_screen)");
  if (lane0 < 0 || n < 0 || lane0 + n > e->fan.n_env || (!value && n)) return fail(GPF_E_INVALID, "gpf_get_n1_values: bad environment range or null");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(value, e->n1_value.p + (size_t)lane0 * e->fan.K, (size_t)n * e->fan.K * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_n1_summary(gpf_handle e, int32_t lane0, int32_t n, float* worst, int32_t* arg_worst, int32_t* n_insecure, int32_t* n_diverged) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_n1_summary: null");
  if (!e->fan.on(N1)) return fail(GPF_E_INVALID, "gpf_get_n1_summary: the N-1 screen is off (gpf_set_n1_screen)");
  if (lane0 < 0 || n < 0 || lane0 + n > e->fan.n_env) return fail(GPF_E_INVALID, "gpf_get_n1_summary: bad environment range");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  std::vector<int> info((size_t)n * 3);
  if (worst) HIP_TRY(hipMemcpyAsync(worst, e->n1_worst.p + lane0, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(info.data(), e->n1_info.p + (size_t)lane0 * 3, info.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < n; ++k) {
    if (arg_worst) arg_worst[k] = info[(size_t)k * 3];
    if (n_insecure) n_insecure[k] = info[(size_t)k * 3 + 1];
    if (n_diverged) n_diverged[k] = info[(size_t)k * 3 + 2];
  }
  return GPF_OK;
}

int gpf_n1_device_pointers(gpf_handle e, void** out, int32_t n) {
  if (!e || !out || n != GPF_N_N1_POINTERS) return fail(GPF_E_INVALID, "gpf_n1_device_pointers: null, or n is not GPF_N_N1_POINTERS");
  if (!e->fan.on(N1)) return fail(GPF_E_INVALID, "gpf_n1_device_pointers: the N-1 screen is off (gpf_set_n1_screen)");
  out[0] = e->n1_value.p; out[1] = e->n1_worst.p; out[2] = e->n1_info.p; out[3] = e->n1_lines.p;
  return GPF_OK;
}

}  // extern "C"
