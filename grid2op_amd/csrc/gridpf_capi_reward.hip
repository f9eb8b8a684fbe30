// gridpf_capi_reward.hip -- the rewards' entry points of the C ABI (include/gridpf.h: gpf_set_rewards, gpf_get_rewards, gpf_rewards_eval,
// gpf_reward_device_pointers) and the host side of reward_kernel (gridpf_reward.hpp), on the engine of gridpf_engine.hpp.  Everything a
// slot or the cost table can get wrong is refused here, before the device is touched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>

#include "gridpf_engine.hpp"
#include "gridpf_reward.hpp"

static_assert(sizeof(gpf::RewardSlot) == sizeof(gpf_reward_slot) && offsetof(gpf::RewardSlot, p) == offsetof(gpf_reward_slot, p), "RewardSlot is gpf_reward_slot");
static_assert(gpf::RW_MAX_SLOTS == GPF_REWARD_MAX_SLOTS && gpf::RW_REDISP == GPF_RW_REDISP && gpf::RW_L2RPN == GPF_RW_L2RPN &&
              gpf::RW_LINES_CAPACITY == GPF_RW_LINES_CAPACITY && gpf::RW_ECONOMIC == GPF_RW_ECONOMIC && gpf::RW_GAMEPLAY == GPF_RW_GAMEPLAY, "kinds");

namespace {

// parameters of a kind that must be finite, and the index of its dts (-1: none)
void kind_params(int kind, int& n_p, int& i_dts) {
  switch (kind) {
    case GPF_RW_REDISP: n_p = 5; i_dts = 4; break;
    case GPF_RW_ECONOMIC: n_p = 4; i_dts = 3; break;
    case GPF_RW_GAMEPLAY: n_p = 2; i_dts = -1; break;
    default: n_p = 0; i_dts = -1; break;
  }
}

void rewards_off(gpf_engine* e) {
  e->n1_slots = false;
  e->rw_on = false; e->rw_n_slot = 0; e->rw_cost_on = false;
  e->rw_slots.release(); e->rw_cost.release(); e->rw_out.release(); e->rw_ill_snap.release();
}

// the lanes' state as reward_kernel reads it; the flag sources and the output are the caller's
gpf::RewardDev reward_dev(const gpf_engine* e) {
  const gpf::GridDev& g = e->g;
  gpf::RewardDev d{};
  d.out = e->out.p; d.inj = e->inj.p; d.rho = e->rho.p; d.line_status = e->line_status.p; d.thermal = e->thermal_limit.p;
  d.dispatch = e->env_on ? e->env_actual.p : (e->has_delta ? e->lane_gen_delta.p : nullptr);
  d.cost = e->rw_cost_on ? e->rw_cost.p : nullptr;
  d.done = e->done.p;
  d.n_out = g.n_out; d.n_inj = g.n_inj; d.off_gen_p = e->oo.gen_p; d.off_load_p = e->oo.load_p; d.off_a_or = e->oo.a_or; d.off_sto = e->oo.inj_sto_p;
  d.n_gen = g.n_gen; d.n_load = g.n_load; d.n_line = g.n_line; d.n_sto = g.n_sto;
  return d;
}

int reward_launch(gpf_engine* e, const gpf::RewardDev& d, int lane0, int n) {
  const unsigned blocks = (unsigned)((n + gpf::RW_WPB - 1) / gpf::RW_WPB);
  hipLaunchKernelGGL(gpf::reward_kernel, dim3(blocks), dim3(64 * gpf::RW_WPB), 0, e->stream, d,
                     reinterpret_cast<const gpf::RewardSlot*>(e->rw_slots.p), e->rw_n_slot, lane0, n);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

}  // namespace

int reward_prestep(gpf_engine* e) {
  HIP_TRY(hipMemcpyAsync(e->rw_ill_snap.p, e->env_illegal.p, (size_t)e->n_lanes * sizeof(int), hipMemcpyDeviceToDevice, e->stream));
  return GPF_OK;
}

int reward_poststep(gpf_engine* e, bool topo_flags, bool combined) {
  gpf::RewardDev d = reward_dev(e);
  d.topo_flags = (topo_flags && !combined) ? e->ta_flags.p : nullptr;
  d.step_flags = combined ? e->cb_flags.p : nullptr;        // combined mode: the flags of the whole step (gridpf_combined.hpp)
  if (e->env_on) { d.ill_now = e->env_illegal.p; d.ill_snap = e->rw_ill_snap.p; }
  if (e->ep_on) { d.ep_limit = e->ep_limit.p; d.episode = e->episode.p; }     // a step at the lane's limit is the reference's is_done
  d.reward = e->rw_out.p; d.row_stride = e->rw_n_slot;
  int rc = reward_launch(e, d, 0, e->n_lanes);
  if (rc == GPF_OK && e->n1_slots) rc = n1_fill_slots(e, 0, e->n_lanes, e->rw_out.p, e->rw_n_slot);     // GPF_RW_N1: the screen's table entries
  return rc;
}

int reward_reset_lanes(gpf_engine* e, int lane0, int n) {
  HIP_TRY(hipMemsetAsync(e->rw_out.p + (size_t)lane0 * e->rw_n_slot, 0, (size_t)n * e->rw_n_slot * sizeof(float), e->stream));
  return GPF_OK;
}

extern "C" {

int gpf_set_rewards(gpf_handle e, int32_t n_slot, const gpf_reward_slot* slots, const float* gen_cost_per_mw) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_rewards: null");
  if (n_slot == 0 || !slots) {
    if (e->rw_on) { HIP_TRY(hipSetDevice(e->device)); HIP_TRY(hipStreamSynchronize(e->stream)); }
    rewards_off(e);
    if (e->ep_on) return episode_rewards_changed(e);
    return GPF_OK;
  }
  const std::string at = "gpf_set_rewards: ";
  if (n_slot < 0 || n_slot > GPF_REWARD_MAX_SLOTS)
    return fail(GPF_E_INVALID, at + std::to_string(n_slot) + " slots: outside [0, GPF_REWARD_MAX_SLOTS = " + std::to_string(GPF_REWARD_MAX_SLOTS) + "]");
  bool need_cost = false;
  for (int s = 0; s < n_slot; ++s) {
    const int kind = slots[s].kind;
    const std::string sl = at + "slot " + std::to_string(s) + ": ";
    if (kind == GPF_RW_N1) continue;       // (checked below, against the screen)
    if (kind < GPF_RW_REDISP || kind > GPF_RW_GAMEPLAY) return fail(GPF_E_INVALID, sl + "unknown kind " + std::to_string(kind));
    int n_p, i_dts;
    kind_params(kind, n_p, i_dts);
    for (int i = 0; i < n_p; ++i)
      if (!std::isfinite(slots[s].p[i])) return fail(GPF_E_INVALID, sl + "parameter " + std::to_string(i) + " is not finite");
    if (i_dts >= 0 && !(slots[s].p[i_dts] > 0.0)) return fail(GPF_E_INVALID, sl + "dts must be positive");
    need_cost = need_cost || kind == GPF_RW_REDISP || kind == GPF_RW_ECONOMIC;
  }
  if (need_cost) {
    if (!gen_cost_per_mw) return fail(GPF_E_INVALID, at + "GPF_RW_REDISP / GPF_RW_ECONOMIC need gen_cost_per_mw");
    for (int i = 0; i < e->g.n_gen; ++i)
      if (!std::isfinite(gen_cost_per_mw[i]) || gen_cost_per_mw[i] < 0.f)
        return fail(GPF_E_INVALID, at + "gen_cost_per_mw[" + std::to_string(i) + "] is negative or not finite");
  }
  { int rc_n = n1_check_slots(e, n_slot, slots); if (rc_n != GPF_OK) return rc_n; }
  if (e->dry) return fail(GPF_E_DEVICE, "gpf_set_rewards: header-only handle: no HIP device");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  rewards_off(e);
  const size_t cap = (size_t)e->cap_lanes;
  hipError_t err = e->rw_slots.upload(reinterpret_cast<const unsigned char*>(slots), (size_t)n_slot * sizeof(gpf_reward_slot));
  if (err == hipSuccess && need_cost) err = e->rw_cost.upload(gen_cost_per_mw, (size_t)e->g.n_gen);
  if (err == hipSuccess) err = e->rw_out.alloc(cap * n_slot);
  if (err == hipSuccess) err = e->rw_ill_snap.alloc(cap);
  if (err == hipSuccess) err = hipMemset(e->rw_out.p, 0, cap * n_slot * sizeof(float));
  if (err == hipSuccess) err = hipMemset(e->rw_ill_snap.p, 0, cap * sizeof(int));
  if (err != hipSuccess) { rewards_off(e); HIP_TRY(err); }
  e->rw_n_slot = n_slot; e->rw_cost_on = need_cost; e->rw_on = true;
  { int rc_n = n1_set_slots(e, n_slot, slots); if (rc_n != GPF_OK) { rewards_off(e); return rc_n; } }
  if (e->ep_on) return episode_rewards_changed(e);    // the returns of another slot table mean nothing for this one
  return GPF_OK;
}

int gpf_get_rewards(gpf_handle e, int32_t lane0, int32_t n, float* reward) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_rewards: null");
  if (!e->rw_on) return fail(GPF_E_INVALID, "gpf_get_rewards: rewards are off (gpf_set_rewards)");
  if (!check_range(e, lane0, n) || !reward) return fail(GPF_E_INVALID, "gpf_get_rewards: bad lane range or null");
  if (e->last_n_steps != 1)
    return fail(GPF_E_INVALID, "gpf_get_rewards: the last gpf_step_n was a multi-step launch: it queues nothing for rewards (use n_steps = 1, or gpf_rewards_eval)");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(reward, e->rw_out.p + (size_t)lane0 * e->rw_n_slot, (size_t)n * e->rw_n_slot * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_rewards_eval(gpf_handle e, int32_t lane0, int32_t n, const uint8_t* flags_dev, float* out_dev, int64_t row_stride) {
  if (!e) return fail(GPF_E_INVALID, "gpf_rewards_eval: null");
  if (!e->rw_on) return fail(GPF_E_INVALID, "gpf_rewards_eval: rewards are off (gpf_set_rewards)");
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_rewards_eval: bad lane range");
  if (out_dev && row_stride < e->rw_n_slot) return fail(GPF_E_INVALID, "gpf_rewards_eval: row_stride is smaller than the number of slots");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  gpf::RewardDev d = reward_dev(e);
  d.status = e->status.p;
  d.eval_flags = flags_dev;
  d.reward = out_dev ? out_dev : e->rw_out.p + (size_t)lane0 * e->rw_n_slot;
  d.row_stride = out_dev ? (long long)row_stride : (long long)e->rw_n_slot;
  int rc = reward_launch(e, d, lane0, n);
  if (rc == GPF_OK && e->n1_slots) rc = n1_fill_slots(e, lane0, n, d.reward, d.row_stride);      // GPF_RW_N1: the last launch's table entries
  return rc;
}

int gpf_reward_device_pointers(gpf_handle e, void** out, int32_t n) {
  if (!e || !out || n != GPF_N_REWARD_POINTERS) return fail(GPF_E_INVALID, "gpf_reward_device_pointers: null, or n is not GPF_N_REWARD_POINTERS");
  if (!e->rw_on) return fail(GPF_E_INVALID, "gpf_reward_device_pointers: rewards are off (gpf_set_rewards)");
  out[0] = e->rw_out.p;
  return GPF_OK;
}

}  // extern "C"
