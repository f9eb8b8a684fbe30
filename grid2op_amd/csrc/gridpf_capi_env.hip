// gridpf_capi_env.hip -- the environment's injection dynamics (gpf::EnvDyn: redispatch, storage, curtailment): the entry points of the C
// ABI (include/gridpf.h: gpf_set_storage_params ... gpf_set_env_illegal) and the lanes' state, on the engine of gridpf_engine.hpp.  The
// dynamics themselves run inside the step kernels (gridpf_sparse.hpp); the one kernel here copies their state between lanes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "gridpf_engine.hpp"

namespace gpf {
// the environment-dynamics state of the source lane -> the scratch lane (simulate: _ObsEnv starts from the environment's own
// _target_dispatch / _actual_dispatch / _gen_activeprod_t_redisp / storage charge / curtailment limits, Environment/_obsEnv.py) or the
// contingency lane (gpf_fanout_n1)
__global__ void simulate_env_copy_kernel(EnvDyn E, int n_gen, int n_sto, const int* __restrict__ src_lanes, int n_act, int n_dst, int dst0) {
  const int q = blockIdx.x;
  if (q >= n_dst) return;
  const int src = src_lanes[q / n_act], dst = dst0 + q, tid = threadIdx.x;
  for (int i = tid; i < n_gen; i += blockDim.x) {
    const size_t s_ = (size_t)src * n_gen + i, d_ = (size_t)dst * n_gen + i;
    E.target[d_] = E.target[s_]; E.actual[d_] = E.actual[s_]; E.prev_p[d_] = E.prev_p[s_]; E.already[d_] = E.already[s_]; E.limit[d_] = E.limit[s_];
  }
  for (int i = tid; i < n_sto; i += blockDim.x) E.charge[(size_t)dst * n_sto + i] = E.charge[(size_t)src * n_sto + i];
  if (tid == 0) { E.amount_prev[dst] = E.amount_prev[src]; E.curt_prev[dst] = E.curt_prev[src]; E.fresh[dst] = E.fresh[src]; E.illegal[dst] = E.illegal[src]; }
}
}  // namespace gpf

// the ONE statement of which engine buffer is which field (everything but the action pointers of a launch)
gpf::EnvDyn env_dyn(const gpf_engine* e) {
  gpf::EnvDyn E{};
  E.on = 1; E.hold_storage = e->env_hold ? 1 : 0; E.loss_on = e->env_loss_on; E.coeff = e->env_coeff; E.eps_poly = e->rd_eps; E.tol_poly = e->env_tol;
  E.target = e->env_target.p; E.actual = e->env_actual.p; E.prev_p = e->env_prev.p; E.already = e->env_already.p; E.charge = e->env_charge.p;
  E.amount_prev = e->env_amount_prev.p; E.fresh = e->env_fresh.p;
  E.limit = e->env_limit.p; E.curt_prev = e->env_curt_prev.p;
  E.illegal = e->env_illegal.p;
  E.renewable = e->env_has_ren ? e->env_renewable.p : nullptr;
  E.pmin = e->rd_pmin.p; E.pmax = e->rd_pmax.p; E.ramp_up = e->rd_ru.p; E.ramp_down = e->rd_rd.p; E.redispatchable = e->rd_redisp.p;
  E.Emax = e->sto_emax.p; E.Emin = e->sto_emin.p; E.loss = e->sto_loss.p; E.eff_c = e->sto_effc.p; E.eff_d = e->sto_effd.p; E.charge0 = e->sto_charge0.p;
  return E;
}

// env dynamics of lanes [lane0, lane0 + n) back to the state after env.reset(): no dispatch, initial state of charge
int env_reset_lanes(gpf_engine* e, int lane0, int n) {
  const size_t ng = e->g.n_gen, ns = e->g.n_sto;
  HIP_TRY(hipMemsetAsync(e->env_target.p + lane0 * ng, 0, n * ng * sizeof(float), e->stream));
  HIP_TRY(hipMemsetAsync(e->env_actual.p + lane0 * ng, 0, n * ng * sizeof(float), e->stream));
  HIP_TRY(hipMemsetAsync(e->env_prev.p + lane0 * ng, 0, n * ng * sizeof(float), e->stream));
  HIP_TRY(hipMemsetAsync(e->env_already.p + lane0 * ng, 0, n * ng, e->stream));
  HIP_TRY(hipMemsetAsync(e->env_amount_prev.p + lane0, 0, (size_t)n * sizeof(float), e->stream));
  HIP_TRY(hipMemsetAsync(e->env_curt_prev.p + lane0, 0, (size_t)n * sizeof(float), e->stream));
  HIP_TRY(hipMemsetAsync(e->env_illegal.p + lane0, 0, (size_t)n * sizeof(int), e->stream));
  {
    std::vector<float> ones((size_t)n * ng, 1.0f);
    HIP_TRY(hipMemcpyAsync(e->env_limit.p + lane0 * ng, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  HIP_TRY(hipMemsetAsync(e->env_fresh.p + lane0, 1, (size_t)n, e->stream));
  if (ns) {
    std::vector<float> c((size_t)n * ns);
    for (int k = 0; k < n; ++k) std::copy(e->h_charge0.begin(), e->h_charge0.end(), c.begin() + (size_t)k * ns);
    HIP_TRY(hipMemcpyAsync(e->env_charge.p + lane0 * ns, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return GPF_OK;
}

// the dynamics are part of the lane's state (Backend.copy / env.copy keep them)
hipError_t env_copy_lanes(gpf_engine* e, int src, int dst, int n) {
  const gpf::GridDev& g = e->g;
  hipError_t err = hipSuccess;
  auto cp = [&](const auto& arr, size_t stride) { if (err == hipSuccess) err = rows_copy(e, arr, stride, src, dst, n); };
  cp(e->env_target, g.n_gen); cp(e->env_actual, g.n_gen); cp(e->env_prev, g.n_gen); cp(e->env_already, g.n_gen); cp(e->env_limit, g.n_gen);
  cp(e->env_charge, g.n_sto); cp(e->env_amount_prev, 1); cp(e->env_curt_prev, 1); cp(e->env_fresh, 1); cp(e->env_illegal, 1);
  return err;
}

int env_copy_from(gpf_engine* e, const int* src_lanes_dev, int n_act, int n_dst, int dst0) {
  hipLaunchKernelGGL(gpf::simulate_env_copy_kernel, dim3((unsigned)n_dst), dim3(64), 0, e->stream, env_dyn(e), e->g.n_gen, e->g.n_sto, src_lanes_dev,
                     n_act, n_dst, dst0);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

namespace {
// The agents' per-launch actions go through a pinned block of the engine: the caller's (pageable) arrays are copied into it, the
// uploads are true asynchronous DMA behind whatever the stream is doing, and NOTHING is waited for -- a host agent that acts at every
// step paid a staged pageable copy plus a stream synchronisation per step before.  The block is rewritten by the next call, which
// first waits for the event recorded behind this call's uploads (reached long before: they sit in front of the step launch).
// Layout: redispatch [B][n_gen] | storage [B][n_sto] | curtailment [B][n_gen].
int act_pin_begin(gpf_engine* e) {
  const size_t B = e->cap_lanes, ng = e->g.n_gen, ns = std::max(e->g.n_sto, 1), need = B * (2 * ng + ns);     // (the device layout: padded lane count)
  if (e->act_up) HIP_TRY(hipEventSynchronize(e->act_up));
  if (e->act_pin.n < need) {
    HIP_TRY(e->act_pin.reserve(need));
    std::memset(e->act_pin.p, 0, need * sizeof(float));         // (the padding lanes' rows travel with the others)
  }
  if (!e->act_up) HIP_TRY(e->act_up.create(hipEventDisableTiming));
  return GPF_OK;
}
}  // namespace

extern "C" {

int gpf_set_storage_params(gpf_handle e, const double* emax, const double* emin, const double* loss, const double* eff_charge,
                           const double* eff_discharge, const float* charge0, double delta_time_seconds, int32_t activate_loss) {
  if (!e || delta_time_seconds <= 0.0) return fail(GPF_E_INVALID, "gpf_set_storage_params: bad arguments");
  const size_t ns = e->g.n_sto;
  if (ns && (!emax || !emin || !loss || !eff_charge || !eff_discharge || !charge0)) return fail(GPF_E_INVALID, "gpf_set_storage_params: null");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(e->sto_emax.upload(emax, ns)); HIP_TRY(e->sto_emin.upload(emin, ns)); HIP_TRY(e->sto_loss.upload(loss, ns));
  HIP_TRY(e->sto_effc.upload(eff_charge, ns)); HIP_TRY(e->sto_effd.upload(eff_discharge, ns)); HIP_TRY(e->sto_charge0.upload(charge0, ns));
  e->h_charge0.assign(charge0, charge0 + ns);
  e->env_coeff = delta_time_seconds / 3600.0;
  e->env_loss_on = activate_loss ? 1 : 0;
  e->sto_ready = true;
  e->params_s_valid = false;
  return GPF_OK;
}

int gpf_set_env_dynamics(gpf_handle e, int32_t on, double tol_poly) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_env_dynamics: null");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->plan_valid = false;
  if (!on) { e->env_on = false; e->params_s_valid = false; return GPF_OK; }
  if (!e->rd_ready) return fail(GPF_E_INVALID, "gpf_set_env_dynamics: call gpf_set_gen_limits first");
  if (e->g.n_sto && !e->sto_ready) return fail(GPF_E_INVALID, "gpf_set_env_dynamics: call gpf_set_storage_params first (the grid has storage units)");
  if (e->g.n_gen > 64 || e->g.n_sto > 64) return fail(GPF_E_CAPACITY, "gpf_set_env_dynamics: more than 64 generators or storage units");
  const size_t B = e->cap_lanes, ng = e->g.n_gen, ns = std::max(e->g.n_sto, 1);
  if (!e->env_target.p) {
    HIP_TRY(e->env_target.alloc(B * ng)); HIP_TRY(e->env_actual.alloc(B * ng)); HIP_TRY(e->env_prev.alloc(B * ng)); HIP_TRY(e->env_already.alloc(B * ng));
    HIP_TRY(e->env_charge.alloc(B * ns)); HIP_TRY(e->env_amount_prev.alloc(B)); HIP_TRY(e->env_fresh.alloc(B));
    // the redispatch and storage action rows of all lanes are ONE allocation ([B][n_gen] | [B][n_storage]): a host agent's two uploads per step are one DMA
    HIP_TRY(e->env_act_redisp.alloc(B * ng + B * ns)); e->env_act_storage = e->env_act_redisp.p + B * ng;
    HIP_TRY(e->env_limit.alloc(B * ng)); HIP_TRY(e->env_curt_prev.alloc(B)); HIP_TRY(e->env_act_curtail.alloc(B * ng)); HIP_TRY(e->env_illegal.alloc(B));
    HIP_TRY(hipMemset(e->env_act_redisp.p, 0, B * ng * sizeof(float))); HIP_TRY(hipMemset(e->env_act_storage, 0, B * ns * sizeof(float)));
    HIP_TRY(hipMemset(e->env_charge.p, 0, B * ns * sizeof(float)));
  }
  e->env_on = true;
  e->env_tol = tol_poly > 0.0 ? tol_poly : 1e-2;
  e->env_act_r = e->env_act_s = e->env_act_c = false; e->env_hold = false;
  e->params_s_valid = false;
  return env_reset_lanes(e, 0, e->cap_lanes);
}

int gpf_set_lane_actions(gpf_handle e, const float* redispatch, const float* storage_power, int32_t hold_storage) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_lane_actions: null");
  if (!e->env_on) return fail(GPF_E_INVALID, "gpf_set_lane_actions: the environment dynamics are off (gpf_set_env_dynamics)");
  HIP_TRY(hipSetDevice(e->device));
  const size_t B = e->n_lanes, ng = e->g.n_gen, ns = e->g.n_sto;
  if (redispatch || (storage_power && ns)) {
    const int rc = act_pin_begin(e);
    if (rc != GPF_OK) return rc;
  }
  const size_t Bc = e->cap_lanes, so = Bc * ng;                  // storage rows: behind the (padded) redispatch rows, on the host block as on the device
  if (redispatch) std::memcpy(e->act_pin.p, redispatch, B * ng * sizeof(float));
  if (storage_power && ns) std::memcpy(e->act_pin.p + so, storage_power, B * ns * sizeof(float));
  if (redispatch && storage_power && ns) {
    HIP_TRY(hipMemcpyAsync(e->env_act_redisp.p, e->act_pin.p, (so + B * ns) * sizeof(float), hipMemcpyHostToDevice, e->stream));     // one DMA for both
  } else if (redispatch) {
    HIP_TRY(hipMemcpyAsync(e->env_act_redisp.p, e->act_pin.p, B * ng * sizeof(float), hipMemcpyHostToDevice, e->stream));
  } else if (storage_power && ns) {
    HIP_TRY(hipMemcpyAsync(e->env_act_storage, e->act_pin.p + so, B * ns * sizeof(float), hipMemcpyHostToDevice, e->stream));
  }
  e->env_act_r = redispatch != nullptr;
  e->env_act_s = storage_power != nullptr && ns > 0;
  e->env_hold = hold_storage != 0;
  if (redispatch || (storage_power && ns)) HIP_TRY(hipEventRecord(e->act_up, e->stream));
  return GPF_OK;
}

int gpf_lane_actions_on_device(gpf_handle e, int32_t redispatch, int32_t storage_power, int32_t curtailment, int32_t hold_storage) {
  if (!e) return fail(GPF_E_INVALID, "gpf_lane_actions_on_device: null");
  if (!e->env_on) return fail(GPF_E_INVALID, "gpf_lane_actions_on_device: the environment dynamics are off (gpf_set_env_dynamics)");
  if (curtailment && !e->env_has_ren) return fail(GPF_E_INVALID, "gpf_lane_actions_on_device: curtailment needs gpf_set_gen_renewable");
  HIP_TRY(hipSetDevice(e->device));
  e->env_act_r = redispatch != 0;
  e->env_act_s = storage_power != 0 && e->g.n_sto > 0;
  e->env_act_c = curtailment != 0;
  e->env_hold = hold_storage != 0;
  return GPF_OK;
}

int gpf_set_gen_renewable(gpf_handle e, const uint8_t* renewable) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_gen_renewable: null");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->env_renewable.release();
  e->env_has_ren = false;
  if (renewable) { HIP_TRY(e->env_renewable.upload(renewable, (size_t)e->g.n_gen)); e->env_has_ren = true; }
  e->params_s_valid = false;
  return GPF_OK;
}

int gpf_set_lane_curtailment(gpf_handle e, const float* limit) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_lane_curtailment: null");
  if (!e->env_on || !e->env_has_ren) return fail(GPF_E_INVALID, "gpf_set_lane_curtailment: needs gpf_set_env_dynamics and gpf_set_gen_renewable");
  HIP_TRY(hipSetDevice(e->device));
  if (!limit) { e->env_act_c = false; return GPF_OK; }
  const size_t n = (size_t)e->n_lanes * e->g.n_gen;
  for (size_t i = 0; i < n; ++i) if (!(limit[i] == -1.0f || (limit[i] >= 0.0f && limit[i] <= 1.0f))) return fail(GPF_E_INVALID, "gpf_set_lane_curtailment: limits are ratios in [0, 1], -1 = no change");
  {
    const int rc = act_pin_begin(e);
    if (rc != GPF_OK) return rc;
  }
  float* stage = e->act_pin.p + (size_t)e->cap_lanes * (e->g.n_gen + std::max(e->g.n_sto, 1));       // (behind the redispatch | storage rows: act_pin_begin)
  std::memcpy(stage, limit, n * sizeof(float));
  HIP_TRY(hipMemcpyAsync(e->env_act_curtail.p, stage, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipEventRecord(e->act_up, e->stream));
  e->env_act_c = true;
  return GPF_OK;
}

int gpf_get_env_state(gpf_handle e, int32_t lane0, int32_t n, float* target, float* actual, float* prev_p, uint8_t* already_modified,
                      float* charge, float* amount_prev, float* curtail_limit, float* curtail_prev) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_get_env_state: bad range");
  if (!e->env_on) return fail(GPF_E_INVALID, "gpf_get_env_state: the environment dynamics are off");
  HIP_TRY(hipSetDevice(e->device));
  const size_t ng = e->g.n_gen, ns = e->g.n_sto;
  HIP_TRY(rows_to_host(e, target, e->env_target, ng, lane0, n)); HIP_TRY(rows_to_host(e, actual, e->env_actual, ng, lane0, n));
  HIP_TRY(rows_to_host(e, prev_p, e->env_prev, ng, lane0, n)); HIP_TRY(rows_to_host(e, already_modified, e->env_already, ng, lane0, n));
  HIP_TRY(rows_to_host(e, charge, e->env_charge, ns, lane0, n)); HIP_TRY(rows_to_host(e, amount_prev, e->env_amount_prev, 1, lane0, n));
  HIP_TRY(rows_to_host(e, curtail_limit, e->env_limit, ng, lane0, n)); HIP_TRY(rows_to_host(e, curtail_prev, e->env_curt_prev, 1, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_env_illegal(gpf_handle e, int32_t lane0, int32_t n, int32_t* count) {
  if (!check_range(e, lane0, n) || !count) return fail(GPF_E_INVALID, "gpf_get_env_illegal: bad range / null");
  if (!e->env_on) return fail(GPF_E_INVALID, "gpf_get_env_illegal: the environment dynamics are off");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(rows_to_host(e, count, e->env_illegal, 1, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_set_env_illegal(gpf_handle e, int32_t lane0, int32_t n, const int32_t* count) {
  if (!check_range(e, lane0, n) || !count) return fail(GPF_E_INVALID, "gpf_set_env_illegal: bad range / null");
  if (!e->env_on) return fail(GPF_E_INVALID, "gpf_set_env_illegal: the environment dynamics are off");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(rows_to_device(e, e->env_illegal, count, 1, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_set_env_state(gpf_handle e, int32_t lane0, int32_t n, const float* target, const float* actual, const float* prev_p,
                      const uint8_t* already_modified, const float* charge, const float* amount_prev, const float* curtail_limit,
                      const float* curtail_prev) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_set_env_state: bad range");
  if (!e->env_on) return fail(GPF_E_INVALID, "gpf_set_env_state: the environment dynamics are off");
  HIP_TRY(hipSetDevice(e->device));
  const size_t ng = e->g.n_gen, ns = e->g.n_sto;
  HIP_TRY(rows_to_device(e, e->env_target, target, ng, lane0, n)); HIP_TRY(rows_to_device(e, e->env_actual, actual, ng, lane0, n));
  HIP_TRY(rows_to_device(e, e->env_prev, prev_p, ng, lane0, n)); HIP_TRY(rows_to_device(e, e->env_already, already_modified, ng, lane0, n));
  HIP_TRY(rows_to_device(e, e->env_charge, charge, ns, lane0, n)); HIP_TRY(rows_to_device(e, e->env_amount_prev, amount_prev, 1, lane0, n));
  HIP_TRY(rows_to_device(e, e->env_limit, curtail_limit, ng, lane0, n)); HIP_TRY(rows_to_device(e, e->env_curt_prev, curtail_prev, 1, lane0, n));
  if (prev_p) HIP_TRY(hipMemsetAsync(e->env_fresh.p + lane0, 0, (size_t)n, e->stream));     // previous set-points given: not a fresh episode
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

}  // extern "C"
