// gridpf_capi_cursor.hip -- the chronics cursor's entry points of the C ABI (include/gridpf.h: gpf_set_chronics_cursor,
// gpf_upload_cursor_draws, gpf_get_cursor_state, gpf_set_cursor_state, gpf_cursor_device_pointers) and the host side of
// cursor_prestep_kernel (gridpf_cursor.hpp), on the engine of gridpf_engine.hpp.  Everything a descriptor can get wrong is refused here,
// before the device is touched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#define GPF_CURSOR_KERNEL
#include "gridpf_engine.hpp"
#include "gridpf_cursor.hpp"

static_assert(gpf::CUR_STATE_INTS == GPF_CURSOR_STATE_INTS && gpf::CUR_SEQUENTIAL == GPF_CURSOR_SEQUENTIAL && gpf::CUR_SAMPLED == GPF_CURSOR_SAMPLED &&
                  gpf::CUR_FLAG_DRAWS_EXHAUSTED == GPF_CURSOR_FLAG_DRAWS_EXHAUSTED && gpf::CUR_FLAG_NEXT_POS_WRAPPED == GPF_CURSOR_FLAG_NEXT_POS_WRAPPED &&
                  gpf::CUR_DRAWS_TABLE == GPF_OPP_DRAWS_TABLE && gpf::CUR_DRAWS_PHILOX == GPF_OPP_DRAWS_PHILOX,
              "gridpf_cursor.hpp and include/gridpf.h name the same values");

namespace {

void cursor_off(gpf_engine* e) {
  e->cur_on = e->cur_host_on = false;
  e->cur_n_draw = 0;
  e->cur_order.release(); e->cur_pos.release(); e->cur_next_pos.release(); e->cur_n_started.release(); e->cur_draws_used.release();
  e->cur_flags.release(); e->cur_first_row.release(); e->cur_skip.release(); e->cur_cdf.release(); e->cur_draws.release();
}

// the seven per-lane arrays in the column order of gpf_get_cursor_state
void cursor_columns(gpf_engine* e, int* col[gpf::CUR_STATE_INTS]) {
  col[0] = e->lane_table.p; col[1] = e->lane_offset.p; col[2] = e->cur_pos.p; col[3] = e->cur_next_pos.p; col[4] = e->cur_n_started.p;
  col[5] = e->cur_draws_used.p; col[6] = e->cur_flags.p;
}

}  // namespace

int cursor_prestep(gpf_engine* e, int t) {
  const gpf_cursor_desc& c = e->cur_desc;
  gpf::CursorCfg cfg{};
  cfg.n_order = c.n_order; cfg.order = e->cur_order.p; cfg.policy = c.policy; cfg.cdf = c.policy == GPF_CURSOR_SAMPLED ? e->cur_cdf.p : nullptr;
  cfg.source = c.draw_source; cfg.seed_lo = c.seed_lo; cfg.seed_hi = c.seed_hi; cfg.lane_base = c.lane_base; cfg.n_draw = e->cur_n_draw;
  cfg.T = e->chron_T;
  gpf::CursorDev d{};
  d.episode = e->episode.p; d.skip = e->cur_skip.p; d.table = e->lane_table.p; d.offset = e->lane_offset.p;
  d.pos = e->cur_pos.p; d.next_pos = e->cur_next_pos.p; d.n_started = e->cur_n_started.p; d.draws_used = e->cur_draws_used.p;
  d.flags = e->cur_flags.p; d.first_row = e->cur_first_row.p;
  d.draws = c.draw_source == GPF_OPP_DRAWS_TABLE && e->cur_n_draw > 0 ? e->cur_draws.p : nullptr;
  const unsigned blocks = (unsigned)((e->n_lanes + gpf::CUR_BLOCK - 1) / gpf::CUR_BLOCK);
  hipLaunchKernelGGL(gpf::cursor_prestep_kernel, dim3(blocks), dim3(gpf::CUR_BLOCK), 0, e->stream, cfg, d, t, e->n_lanes);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

hipError_t cursor_copy_lanes(gpf_engine* e, int src, int dst, int n) {
  auto cp = [&](auto* p) {
    return hipMemcpyAsync(p + dst, p + src, (size_t)n * sizeof(*p), hipMemcpyDeviceToDevice, e->stream);
  };
  int* col[gpf::CUR_STATE_INTS];
  cursor_columns(e, col);
  hipError_t err = hipSuccess;
  for (int k = 0; k < gpf::CUR_STATE_INTS && err == hipSuccess; ++k) err = cp(col[k]);
  if (err == hipSuccess) err = cp(e->cur_first_row.p);
  if (err == hipSuccess) err = cp(e->cur_skip.p);
  if (err == hipSuccess && e->cur_n_draw > 0)
    err = hipMemcpyAsync(e->cur_draws.p + (size_t)dst * e->cur_n_draw, e->cur_draws.p + (size_t)src * e->cur_n_draw,
                         (size_t)n * e->cur_n_draw * sizeof(double), hipMemcpyDeviceToDevice, e->stream);
  for (int k = 0; k < n; ++k) {          // the host's words about the lanes follow them
    e->h_lane_table[dst + k] = e->h_lane_table[src + k]; e->h_lane_offset[dst + k] = e->h_lane_offset[src + k];
    e->h_lane_forecast[dst + k] = e->h_lane_forecast[src + k]; e->h_lane_n1[dst + k] = e->h_lane_n1[src + k];
  }
  return err;
}

hipError_t cursor_mark_lanes(gpf_engine* e, int lane0, int n, int skip) {
  return hipMemsetAsync(e->cur_skip.p + lane0, skip ? 1 : 0, (size_t)n, e->stream);
}

hipError_t cursor_fetch_mirrors(gpf_engine* e) {
  hipError_t err = hipMemcpyAsync(e->h_lane_table.data(), e->lane_table.p, (size_t)e->n_lanes * sizeof(int), hipMemcpyDeviceToHost, e->stream);
  if (err == hipSuccess)
    err = hipMemcpyAsync(e->h_lane_offset.data(), e->lane_offset.p, (size_t)e->n_lanes * sizeof(int), hipMemcpyDeviceToHost, e->stream);
  return err;
}

extern "C" {

int gpf_set_chronics_cursor(gpf_handle e, const gpf_cursor_desc* d) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_chronics_cursor: null");
  if (!d) {
    if (e->cur_on && !e->dry) { HIP_TRY(hipSetDevice(e->device)); HIP_TRY(hipStreamSynchronize(e->stream)); }
    cursor_off(e);
    return GPF_OK;
  }
  const std::string at = "gpf_set_chronics_cursor: ";
  const int B = e->n_lanes;
  if (d->n_order <= 0 || !d->order) return fail(GPF_E_INVALID, at + "the order is empty");
  if (d->policy != GPF_CURSOR_SEQUENTIAL && d->policy != GPF_CURSOR_SAMPLED) return fail(GPF_E_INVALID, at + "unknown policy " + std::to_string(d->policy));
  if (d->draw_source != GPF_OPP_DRAWS_TABLE && d->draw_source != GPF_OPP_DRAWS_PHILOX)
    return fail(GPF_E_INVALID, at + "unknown draw source " + std::to_string(d->draw_source));
  if (d->lane_base < 0) return fail(GPF_E_INVALID, at + "lane_base must not be negative");
  int max_table = 0, max_first = 0;
  for (int i = 0; i < d->n_order; ++i) {
    if (d->order[i] < 0) return fail(GPF_E_INVALID, at + "order[" + std::to_string(i) + "] is negative");
    max_table = std::max(max_table, d->order[i]);
  }
  if (d->policy == GPF_CURSOR_SAMPLED) {
    if (!d->cdf) return fail(GPF_E_INVALID, at + "the sampled policy needs a cdf");
    double prev = 0.0;
    for (int i = 0; i < d->n_order; ++i) {
      if (!(d->cdf[i] >= prev) || !std::isfinite(d->cdf[i])) return fail(GPF_E_INVALID, at + "the cdf is not non-decreasing to 1 (entry " + std::to_string(i) + ")");
      prev = d->cdf[i];
    }
    if (prev != 1.0) return fail(GPF_E_INVALID, at + "the cdf is not non-decreasing to 1 (its last entry is not 1)");
  }
  for (int k = 0; k < (d->lane_first_row ? B : 1); ++k) {
    const int r = d->lane_first_row ? d->lane_first_row[k] : d->first_row;
    if (r < 0) return fail(GPF_E_INVALID, at + "first_row " + std::to_string(r) + " is outside [0, T)");
    max_first = std::max(max_first, r);
  }
  for (int k = 0; k < (d->lane_next_pos ? B : 1); ++k) {
    const int q = d->lane_next_pos ? d->lane_next_pos[k] : d->next_pos;
    if (q >= d->n_order) return fail(GPF_E_INVALID, at + "next_pos " + std::to_string(q) + " >= n_order = " + std::to_string(d->n_order));
  }
  if (e->dry) {                               // (no tables on a header-only handle: the checks against them need a device)
    cursor_off(e);
    e->cur_host_on = true;
    return fail(GPF_E_DEVICE, "gpf_set_chronics_cursor: header-only handle: no HIP device");
  }
  if (!e->chron.p || e->chron_T <= 0) return fail(GPF_E_INVALID, at + "no chronics uploaded (gpf_upload_chronics)");
  if (max_table >= e->chron_tables)
    return fail(GPF_E_INVALID, at + "an order entry is " + std::to_string(max_table) + ", the uploaded chronics have n_tables = " + std::to_string(e->chron_tables));
  if (max_first >= e->chron_T)
    return fail(GPF_E_INVALID, at + "first_row " + std::to_string(max_first) + " is outside [0, T = " + std::to_string(e->chron_T) + ")");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  cursor_off(e);
  const size_t cap = (size_t)e->cap_lanes;
  std::vector<int> first(cap, 0), next(cap, 0), minus(cap, -1);
  std::vector<unsigned char> skip(cap, 0);
  for (int k = 0; k < B; ++k) {
    first[k] = d->lane_first_row ? d->lane_first_row[k] : d->first_row;
    next[k] = d->lane_next_pos ? d->lane_next_pos[k] : d->next_pos;
    if (next[k] < 0) next[k] = -1;
    skip[k] = (e->h_lane_forecast[k] || e->h_lane_n1[k]) ? 1 : 0;
  }
  hipError_t err = e->cur_order.upload(d->order, (size_t)d->n_order);
  if (err == hipSuccess && d->policy == GPF_CURSOR_SAMPLED) err = e->cur_cdf.upload(d->cdf, (size_t)d->n_order);
  if (err == hipSuccess) err = e->cur_first_row.upload(first.data(), cap);
  if (err == hipSuccess) err = e->cur_next_pos.upload(next.data(), cap);
  if (err == hipSuccess) err = e->cur_pos.upload(minus.data(), cap);
  if (err == hipSuccess) err = e->cur_skip.upload(skip.data(), cap);
  for (DevArr<int>* a : {&e->cur_n_started, &e->cur_draws_used, &e->cur_flags}) {
    if (err == hipSuccess) err = a->alloc(cap);
    if (err == hipSuccess) err = hipMemset(a->p, 0, cap * sizeof(int));
  }
  if (err != hipSuccess) { cursor_off(e); HIP_TRY(err); }
  e->cur_desc = *d;
  e->cur_desc.order = nullptr; e->cur_desc.cdf = nullptr; e->cur_desc.lane_first_row = nullptr; e->cur_desc.lane_next_pos = nullptr;
  e->cur_max_table = max_table; e->cur_max_first_row = max_first;
  e->cur_on = true;
  return GPF_OK;
}

int gpf_upload_cursor_draws(gpf_handle e, int32_t n_draw, const double* draws) {
  if (!e) return fail(GPF_E_INVALID, "gpf_upload_cursor_draws: null");
  if (!e->cur_on) return fail(GPF_E_INVALID, "gpf_upload_cursor_draws: the chronics cursor is off (gpf_set_chronics_cursor)");
  if (e->cur_desc.draw_source != GPF_OPP_DRAWS_TABLE) return fail(GPF_E_INVALID, "gpf_upload_cursor_draws: the cursor's draw source is not GPF_OPP_DRAWS_TABLE");
  if (n_draw < 0 || (n_draw > 0 && !draws)) return fail(GPF_E_INVALID, "gpf_upload_cursor_draws: bad arguments");
  for (size_t i = 0; i < (size_t)e->n_lanes * n_draw; ++i)
    if (!(draws[i] >= 0.0 && draws[i] < 1.0)) return fail(GPF_E_INVALID, "gpf_upload_cursor_draws: draw " + std::to_string(i) + " is outside [0, 1)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->cur_n_draw = 0;
  HIP_TRY(e->cur_draws.alloc((size_t)e->cap_lanes * n_draw));
  if (n_draw) {
    HIP_TRY(hipMemset(e->cur_draws.p, 0, (size_t)e->cap_lanes * n_draw * sizeof(double)));
    HIP_TRY(hipMemcpy(e->cur_draws.p, draws, (size_t)e->n_lanes * n_draw * sizeof(double), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemset(e->cur_draws_used.p, 0, (size_t)e->cap_lanes * sizeof(int)));
  e->cur_n_draw = n_draw;
  return GPF_OK;
}

int gpf_get_cursor_state(gpf_handle e, int32_t lane0, int32_t n, int32_t* state) {
  if (!check_range(e, lane0, n) || !state) return fail(GPF_E_INVALID, "gpf_get_cursor_state: bad lane range or null");
  if (!e->cur_on) return fail(GPF_E_INVALID, "gpf_get_cursor_state: the chronics cursor is off (gpf_set_chronics_cursor)");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  int* col[gpf::CUR_STATE_INTS];
  cursor_columns(e, col);
  for (int k = 0; k < gpf::CUR_STATE_INTS; ++k)
    HIP_TRY(hipMemcpy2DAsync(state + k, gpf::CUR_STATE_INTS * sizeof(int), col[k] + lane0, sizeof(int), sizeof(int), (size_t)n, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_set_cursor_state(gpf_handle e, int32_t lane0, int32_t n, const int32_t* state) {
  if (!check_range(e, lane0, n) || !state) return fail(GPF_E_INVALID, "gpf_set_cursor_state: bad lane range or null");
  if (!e->cur_on) return fail(GPF_E_INVALID, "gpf_set_cursor_state: the chronics cursor is off (gpf_set_chronics_cursor)");
  for (int k = 0; k < n; ++k) {
    const int32_t* s = state + (size_t)k * gpf::CUR_STATE_INTS;
    const std::string at = "gpf_set_cursor_state: lane " + std::to_string(lane0 + k) + ": ";
    if (s[0] < 0 || s[0] >= e->chron_tables) return fail(GPF_E_INVALID, at + "the table is outside [0, n_tables)");
    if (s[2] < -1 || s[2] >= e->cur_desc.n_order) return fail(GPF_E_INVALID, at + "pos is outside [-1, n_order)");
    if (s[3] >= e->cur_desc.n_order) return fail(GPF_E_INVALID, at + "next_pos >= n_order");
    if (s[4] < 0 || s[5] < 0) return fail(GPF_E_INVALID, at + "negative episode or draw count");
  }
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int* col[gpf::CUR_STATE_INTS];
  cursor_columns(e, col);
  for (int k = 0; k < gpf::CUR_STATE_INTS; ++k)
    HIP_TRY(hipMemcpy2D(col[k] + lane0, sizeof(int), state + k, gpf::CUR_STATE_INTS * sizeof(int), sizeof(int), (size_t)n, hipMemcpyHostToDevice));
  for (int k = 0; k < n; ++k) {
    e->h_lane_table[lane0 + k] = state[(size_t)k * gpf::CUR_STATE_INTS]; e->h_lane_offset[lane0 + k] = state[(size_t)k * gpf::CUR_STATE_INTS + 1];
  }
  return GPF_OK;
}

int gpf_cursor_device_pointers(gpf_handle e, void** out, int32_t n) {
  if (!e || !out || n != GPF_N_CURSOR_POINTERS) return fail(GPF_E_INVALID, "gpf_cursor_device_pointers: null, or n is not GPF_N_CURSOR_POINTERS");
  if (!e->cur_on) return fail(GPF_E_INVALID, "gpf_cursor_device_pointers: the chronics cursor is off (gpf_set_chronics_cursor)");
  out[0] = e->cur_next_pos.p; out[1] = e->cur_pos.p; out[2] = e->cur_n_started.p;
  return GPF_OK;
}

}  // extern "C"
