// gridpf_capi_combined.hip -- combined topology + injection actions: the entry points of the C ABI (include/gridpf.h:
// gpf_set_combined_actions, gpf_get_action_flags, gpf_combined_device_pointers) and the host side of the three side kernels
// (gridpf_combined.hpp), on the engine of gridpf_engine.hpp.  Everything a descriptor can get wrong is refused here, before the device is
// touched.
#include <hip/hip_runtime.h>

#include <cmath>

#define GPF_COMBINED_KERNEL
#include "gridpf_engine.hpp"
#include "gridpf_combined.hpp"

static_assert(gpf::CB_REDISP_FIXED_GEN == GPF_CB_REDISP_FIXED_GEN && gpf::CB_REDISP_RAMP_UP == GPF_CB_REDISP_RAMP_UP &&
              gpf::CB_REDISP_RAMP_DOWN == GPF_CB_REDISP_RAMP_DOWN && gpf::CB_STORAGE_POWER == GPF_CB_STORAGE_POWER &&
              gpf::CB_CURTAIL_RANGE == GPF_CB_CURTAIL_RANGE && gpf::CB_CURTAIL_FIXED_GEN == GPF_CB_CURTAIL_FIXED_GEN &&
              gpf::CB_DISCO_STORAGE == GPF_CB_DISCO_STORAGE && gpf::CB_TOPO_RULES == GPF_CB_TOPO_RULES &&
              gpf::CB_TOPO_AMBIGUOUS == GPF_CB_TOPO_AMBIGUOUS, "reasons");

namespace {

void combined_off(gpf_engine* e) {
  e->cb_on = false; e->cb_check = false;
  e->cb_flags.release(); e->cb_screen.release(); e->cb_ill_snap.release(); e->cb_max_prod.release(); e->cb_max_absorb.release();
}

// what the kernels of THIS launch read and write.  acts: it carries topology actions; a held storage action stays outside the screen
gpf::CombinedDev combined_dev(const gpf_engine* e, bool acts, bool screened, int rules_on) {
  const gpf::GridDev& g = e->g;
  gpf::CombinedDev d{};
  d.g.n_gen = g.n_gen; d.g.n_sto = g.n_sto;
  d.g.ramp_up = e->rd_ru.p; d.g.ramp_down = e->rd_rd.p; d.g.redispatchable = e->rd_redisp.p;
  d.g.renewable = e->env_has_ren ? e->env_renewable.p : nullptr;
  d.g.sto_max_prod = e->cb_max_prod.n ? e->cb_max_prod.p : nullptr; d.g.sto_max_absorb = e->cb_max_absorb.n ? e->cb_max_absorb.p : nullptr;
  d.g.sto_pos = e->sto_pos.p;
  d.dim_topo = g.dim_topo; d.n_line = g.n_line; d.n_sub = g.n_sub; d.n_slot = e->ta_n_slot; d.n_act = e->ta_n_act;
  d.check_values = e->cb_check ? 1 : 0; d.rules_on = rules_on;
  d.had_topo = acts ? 1 : 0; d.screened = screened ? 1 : 0;
  d.act_r = e->env_act_r ? e->env_act_redisp.p : nullptr;
  d.act_s = (e->env_act_s && !e->env_hold) ? e->env_act_storage : nullptr;
  d.act_c = e->env_act_c ? e->env_act_curtail.p : nullptr;
  d.topo = e->topo.p; d.slots = e->ta_act.p; d.tab_amb = e->ta_amb.p; d.tab_word = e->ta_sto_word.p;
  d.env_illegal = e->env_illegal.p; d.ill_snap = e->cb_ill_snap.p; d.screen = e->cb_screen.p;
  d.topo_flags = e->ta_flags.p; d.aff = e->ta_aff.p; d.flags = e->cb_flags.p;
  return d;
}

template <typename K>
int combined_launch(gpf_engine* e, K kernel, const gpf::CombinedDev& d) {
  const unsigned blocks = (unsigned)((e->n_lanes + gpf::CB_WPB - 1) / gpf::CB_WPB);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * gpf::CB_WPB), 0, e->stream, d, e->n_lanes);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

}  // namespace

int combined_screen(gpf_engine* e, bool acts, int rules_on) { return combined_launch(e, gpf::combined_screen_kernel, combined_dev(e, acts, true, rules_on)); }
int combined_cancel(gpf_engine* e, bool acts) { return combined_launch(e, gpf::combined_cancel_kernel, combined_dev(e, acts, true, 0)); }
int combined_settle(gpf_engine* e, bool acts, bool screened) { return combined_launch(e, gpf::combined_settle_kernel, combined_dev(e, acts, screened, 0)); }

int combined_reset_lanes(gpf_engine* e, int lane0, int n) {
  HIP_TRY(hipMemsetAsync(e->cb_flags.p + (size_t)lane0 * 4, 0, (size_t)n * 4, e->stream));
  HIP_TRY(hipMemsetAsync(e->cb_screen.p + lane0, 0, (size_t)n, e->stream));
  return GPF_OK;
}

hipError_t combined_copy_lanes(gpf_engine* e, int src, int dst, int n) {
  hipError_t err = hipMemcpyAsync(e->cb_flags.p + (size_t)dst * 4, e->cb_flags.p + (size_t)src * 4, (size_t)n * 4, hipMemcpyDeviceToDevice, e->stream);
  if (err == hipSuccess) err = hipMemcpyAsync(e->cb_screen.p + dst, e->cb_screen.p + src, (size_t)n, hipMemcpyDeviceToDevice, e->stream);
  return err;
}

extern "C" {

int gpf_set_combined_actions(gpf_handle e, const gpf_combined_desc* d) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_combined_actions: null");
  const std::string at = "gpf_set_combined_actions: ";
  if (!d || !d->on) {
    if (e->cb_on && !e->dry) { HIP_TRY(hipSetDevice(e->device)); HIP_TRY(hipStreamSynchronize(e->stream)); }
    combined_off(e);
    return GPF_OK;
  }
  if (!e->env_on) return fail(GPF_E_INVALID, at + "the environment dynamics are off (gpf_set_env_dynamics)");
  if (!e->ta_on) return fail(GPF_E_INVALID, at + "the acting path is off (gpf_set_topo_rules / gpf_upload_topo_actions)");
  const int ns = e->g.n_sto;
  const bool limits = d->check_values && ns > 0 && d->storage_max_p_prod && d->storage_max_p_absorb;
  if (d->check_values && ns > 0 && (d->storage_max_p_prod == nullptr) != (d->storage_max_p_absorb == nullptr))
    return fail(GPF_E_INVALID, at + "storage_max_p_prod and storage_max_p_absorb come together");
  if (limits)
    for (int i = 0; i < ns; ++i)
      if (!std::isfinite(d->storage_max_p_prod[i]) || !std::isfinite(d->storage_max_p_absorb[i]) || d->storage_max_p_prod[i] < 0.f || d->storage_max_p_absorb[i] < 0.f)
        return fail(GPF_E_INVALID, at + "storage unit " + std::to_string(i) + ": a limit is negative or not finite");
  if (e->dry) return fail(GPF_E_DEVICE, "gpf_set_combined_actions: header-only handle: no HIP device");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  combined_off(e);
  const size_t cap = (size_t)e->cap_lanes;
  hipError_t err = e->cb_flags.alloc(cap * 4);
  if (err == hipSuccess) err = e->cb_screen.alloc(cap);
  if (err == hipSuccess) err = e->cb_ill_snap.alloc(cap);
  if (err == hipSuccess) err = hipMemset(e->cb_flags.p, 0, cap * 4);
  if (err == hipSuccess) err = hipMemset(e->cb_screen.p, 0, cap);
  if (err == hipSuccess) err = hipMemset(e->cb_ill_snap.p, 0, cap * sizeof(int));
  if (err == hipSuccess && limits) err = e->cb_max_prod.upload(d->storage_max_p_prod, (size_t)ns);
  if (err == hipSuccess && limits) err = e->cb_max_absorb.upload(d->storage_max_p_absorb, (size_t)ns);
  if (err != hipSuccess) { combined_off(e); HIP_TRY(err); }
  e->cb_check = d->check_values != 0;
  e->cb_on = true;
  return GPF_OK;
}

int gpf_get_action_flags(gpf_handle e, int32_t lane0, int32_t n, uint8_t* flags) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_action_flags: null");
  if (!e->cb_on) return fail(GPF_E_INVALID, "gpf_get_action_flags: combined actions are off (gpf_set_combined_actions)");
  if (!check_range(e, lane0, n) || (n && !flags)) return fail(GPF_E_INVALID, "gpf_get_action_flags: bad lane range or null");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(flags, e->cb_flags.p + (size_t)lane0 * 4, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_combined_device_pointers(gpf_handle e, void** out, int32_t n) {
  if (!e || !out || n != GPF_N_COMBINED_POINTERS) return fail(GPF_E_INVALID, "gpf_combined_device_pointers: null, or n is not GPF_N_COMBINED_POINTERS");
  if (!e->cb_on) return fail(GPF_E_INVALID, "gpf_combined_device_pointers: combined actions are off (gpf_set_combined_actions)");
  out[0] = e->cb_flags.p;
  return GPF_OK;
}

}  // extern "C"
