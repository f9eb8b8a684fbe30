// gridpf_capi_graph.hip -- the bus-graph observation entry points of the C ABI (include/gridpf.h: gpf_set_graph_obs, gpf_graph_layout,
// gpf_graph_obs, gpf_graph_obs_host): the host side of the kernel of gridpf_graph.hpp, on the engine of gridpf_engine.hpp.  Everything a
// call can get wrong is refused here, before the device is touched.
#include <hip/hip_runtime.h>

#include <cstdlib>

#define GPF_GRAPH_KERNEL
#include "gridpf_engine.hpp"
#include "gridpf_graph.hpp"

static_assert(gpf::GR_MAX_BUS == GPF_GRAPH_MAX_BUS && gpf::GR_N_FEAT == GPF_GRAPH_N_FEATURES, "gridpf_graph.hpp and include/gridpf.h disagree");

namespace {

// the index row's sections in the order of GPF_GRAPH_*
void section_widths(const gpf_engine* e, int32_t w[GPF_GRAPH_N_SECTIONS]) {
  const gpf::GridDev& g = e->g;
  const int32_t v[GPF_GRAPH_N_SECTIONS] = {1, g.n_load, g.n_gen, g.n_sto, g.n_line, g.n_line, g.n_shunt, g.n_sub * g.n_busbar};
  std::copy(v, v + GPF_GRAPH_N_SECTIONS, w);
}

// the launch into device buffers (validated by check_call)
int launch_graph(gpf_engine* e, int lane0, int n, int* index, float* feat, float* dense) {
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  const gpf::GridDev& g = e->g;
  gpf::GraphDev d{};
  d.T = gpf::graph_tab_view(e->h_gr_tab.data(), e->gr_tab.p);
  d.topo = e->topo_out.p; d.shunt_bus = e->shunt_bus_out.p; d.out = e->out.p; d.sub_cd = e->ta_on ? e->ta_sub_cd.p : nullptr; d.done = e->done.p;
  d.index = index; d.feat = feat; d.dense = dense; d.n_out = g.n_out; d.game_over_fill = e->gr_gof ? 1 : 0;
  const size_t nb = (size_t)g.n_sub * g.n_busbar;
  // the planes' zero fill and the entries the kernel stores afterwards touch the same addresses: stream order puts the fill first
  if (dense) HIP_TRY(hipMemsetAsync(dense, 0, (size_t)n * 3 * nb * nb * sizeof(float), e->stream));
  const unsigned blocks = (unsigned)((n + gpf::GR_WPB - 1) / gpf::GR_WPB);
  // the lanes' rows are staged in LDS where a block's four fit what a launch may ask for; larger grids gather from global memory
  const bool stage = e->gr_stage && (size_t)gpf::GR_WPB * gpf::graph_lds_ints(d.T, g.n_out, true) * sizeof(int) <= gpf::GR_STAGE_MAX_BYTES;
  const size_t lds = (size_t)gpf::GR_WPB * gpf::graph_lds_ints(d.T, g.n_out, stage) * sizeof(int);
  hipLaunchKernelGGL(gpf::graph_obs_kernel, dim3(blocks), dim3(64 * gpf::GR_WPB), lds, e->stream, d, lane0, n, stage ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

int check_call(gpf_engine* e, int lane0, int n, const void* index, const void* feat, const char* who) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, std::string(who) + ": bad lane range");
  if (!e->gr_on) return fail(GPF_E_INVALID, std::string(who) + ": the graph observation is off (gpf_set_graph_obs)");
  if (!index || !feat) return fail(GPF_E_INVALID, std::string(who) + ": index_out and features_out must not be NULL");
  if (e->dry) return fail(GPF_E_DEVICE, std::string(who) + ": header-only handle");
  return GPF_OK;
}

}  // namespace

extern "C" {

int gpf_set_graph_obs(gpf_handle e, int32_t on, int32_t game_over_fill) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_graph_obs: null");
  if (!on) {
    if (!e->dry && e->gr_on) { HIP_TRY(hipSetDevice(e->device)); HIP_TRY(hipStreamSynchronize(e->stream)); }
    e->gr_on = false;
    e->h_gr_tab.clear(); e->gr_tab.release(); e->gr_index.release(); e->gr_feat.release(); e->gr_dense.release();
    return GPF_OK;
  }
  const gpf::GridDev& g = e->g;
  const long long nb = (long long)g.n_sub * g.n_busbar;
  if (nb > GPF_GRAPH_MAX_BUS)
    return fail(GPF_E_INVALID, "gpf_set_graph_obs: " + std::to_string(nb) + " buses (n_sub * n_busbar), more than GPF_GRAPH_MAX_BUS = " +
                                   std::to_string(GPF_GRAPH_MAX_BUS));
  gpf::GraphGrid gg{};
  gg.n_sub = g.n_sub; gg.n_busbar = g.n_busbar; gg.n_load = g.n_load; gg.n_gen = g.n_gen; gg.n_sto = g.n_sto; gg.n_line = g.n_line;
  gg.n_shunt = g.n_shunt; gg.dim_topo = g.dim_topo;
  gg.load_sub = e->h_load_sub.data(); gg.load_pos = e->h_load_pos.data(); gg.gen_sub = e->h_gen_sub.data(); gg.gen_pos = e->h_gen_pos.data();
  gg.sto_sub = e->h_sto_sub.data(); gg.sto_pos = e->h_sto_pos.data(); gg.lor_sub = e->h_line_or_sub.data(); gg.lor_pos = e->h_line_or_pos.data();
  gg.lex_sub = e->h_line_ex_sub.data(); gg.lex_pos = e->h_line_ex_pos.data(); gg.shunt_sub = e->h_shunt_sub.data();
  const gpf::OutOff& o = e->oo;
  gg.o_p_or = o.p_or; gg.o_q_or = o.q_or; gg.o_v_or = o.v_or; gg.o_p_ex = o.p_ex; gg.o_q_ex = o.q_ex; gg.o_v_ex = o.v_ex; gg.o_gen_p = o.gen_p;
  gg.o_gen_q = o.gen_q; gg.o_load_p = o.load_p; gg.o_load_q = o.load_q; gg.o_sto_p = o.sto_p; gg.o_sh_p = o.sh_p; gg.o_sh_q = o.sh_q;
  std::vector<int> blob = gpf::graph_build_tab(gg);
  if (!e->dry) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->gr_on = false;
    HIP_TRY(e->gr_tab.upload(blob.data(), blob.size()));
  }
  e->h_gr_tab = std::move(blob);
  e->gr_gof = game_over_fill != 0;
  const char* st = std::getenv("GRIDPF_GRAPH_STAGE");          // "0": never stage the lanes' rows in LDS (A/B timing and the tests)
  e->gr_stage = !(st && st[0] == '0');
  e->gr_on = true;
  return GPF_OK;
}

int gpf_graph_layout(gpf_handle e, int32_t* offsets, int32_t* widths, int32_t* index_width, int32_t* nb) {
  if (!e) return fail(GPF_E_INVALID, "gpf_graph_layout: null");
  int32_t w[GPF_GRAPH_N_SECTIONS];
  section_widths(e, w);
  int32_t at = 0;
  for (int s = 0; s < GPF_GRAPH_N_SECTIONS; ++s) {
    if (offsets) offsets[s] = at;
    if (widths) widths[s] = w[s];
    at += w[s];
  }
  if (index_width) *index_width = at;
  if (nb) *nb = w[GPF_GRAPH_BUS_GLOBAL];
  return GPF_OK;
}

int gpf_graph_obs(gpf_handle e, int32_t lane0, int32_t n, int32_t* index_out, float* features_out, float* dense_out) {
  int rc = check_call(e, lane0, n, index_out, features_out, "gpf_graph_obs");
  if (rc != GPF_OK) return rc;
  return launch_graph(e, lane0, n, index_out, features_out, dense_out);
}

int gpf_graph_obs_host(gpf_handle e, int32_t lane0, int32_t n, int32_t* index_out, float* features_out, float* dense_out) {
  int rc = check_call(e, lane0, n, index_out, features_out, "gpf_graph_obs_host");
  if (rc != GPF_OK) return rc;
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  const gpf::GridDev& g = e->g;
  const size_t nb = (size_t)g.n_sub * g.n_busbar, width = e->h_gr_tab.empty() ? 0 : (size_t)gpf::graph_index_width(gpf::graph_tab_view(e->h_gr_tab.data(), nullptr));
  HIP_TRY(hipStreamSynchronize(e->stream));          // (a grown staging buffer frees the old one: nothing queued may still read it)
  HIP_TRY(e->gr_index.ensure((size_t)n * width));
  HIP_TRY(e->gr_feat.ensure((size_t)n * nb * GPF_GRAPH_N_FEATURES));
  if (dense_out) HIP_TRY(e->gr_dense.ensure((size_t)n * 3 * nb * nb));
  rc = launch_graph(e, lane0, n, e->gr_index.p, e->gr_feat.p, dense_out ? e->gr_dense.p : nullptr);
  if (rc != GPF_OK) return rc;
  HIP_TRY(hipMemcpyAsync(index_out, e->gr_index.p, (size_t)n * width * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(features_out, e->gr_feat.p, (size_t)n * nb * GPF_GRAPH_N_FEATURES * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (dense_out) HIP_TRY(hipMemcpyAsync(dense_out, e->gr_dense.p, (size_t)n * 3 * nb * nb * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

}  // extern "C"
