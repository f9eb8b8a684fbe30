// gridpf_capi_ptdf.hip -- the DC sensitivity (PTDF / LODF) entry points of the C ABI (include/gridpf.h: gpf_ptdf_* and gpf_lodf_screen):
// the host side of the kernels of gridpf_ptdf.hpp, gridpf_ptdf_batch.hpp and gridpf_ptdf_group.hpp, on the engine of gridpf_engine.hpp.
#include <hip/hip_runtime.h>

#include <chrono>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>

#include "gridpf_engine.hpp"
#include "gridpf_ptdf.hpp"
#include "gridpf_ptdf_batch.hpp"
#include "gridpf_ptdf_group.hpp"

extern "C" {

/* ---- DC sensitivity (PTDF) path ------------------------------------------------------------------------------------ */
int gpf_ptdf_build(gpf_handle e, int32_t lane) {
  if (!check_range(e, lane, 1)) return fail(GPF_E_INVALID, "gpf_ptdf_build: bad lane");
  HIP_TRY(hipSetDevice(e->device));
  const gpf::GridDev& g = e->g;
  const gpf::OutOff& oo = e->oo;
  std::vector<int> topo(g.dim_topo), sb(std::max(g.n_shunt, 1));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(topo.data(), e->topo.p + (size_t)lane * g.dim_topo, (size_t)g.dim_topo * sizeof(int), hipMemcpyDeviceToHost));
  if (g.n_shunt) HIP_TRY(hipMemcpy(sb.data(), e->shunt_bus.p + (size_t)lane * g.n_shunt, (size_t)g.n_shunt * sizeof(int), hipMemcpyDeviceToHost));
  const int nbt = g.nb_tot;
  auto bus_of = [&](int sub, int local) -> int { return (local >= 1 && local <= g.n_busbar) ? sub + (local - 1) * g.n_sub : -1; };
  std::vector<char> act(nbt, 0), ref(nbt, 0);
  std::vector<int> lf(g.n_line, -1), lt(g.n_line, -1);
  for (int l = 0; l < g.n_line; ++l) {
    const int bo = topo[e->h_line_or_pos[l]], be = topo[e->h_line_ex_pos[l]];
    if (bo >= 1 && be >= 1) {
      lf[l] = bus_of(e->h_line_or_sub[l], bo); lt[l] = bus_of(e->h_line_ex_sub[l], be);
      if (lf[l] < 0 || lt[l] < 0) return fail(GPF_E_INVALID, "gpf_ptdf_build: bus id out of range");
      act[lf[l]] = act[lt[l]] = 1;
    }
  }
  std::vector<int> inj_bus(g.n_inj, -1);
  std::vector<double> inj_w(g.n_inj, 0.0);
  for (int i = 0; i < g.n_gen; ++i) {
    const int b = bus_of(e->h_gen_sub[i], topo[e->h_gen_pos[i]]);
    if (b < 0) continue;
    act[b] = 1;
    if (e->h_gen_slack[i]) ref[b] = 1; else { inj_bus[oo.inj_gen_p + i] = b; inj_w[oo.inj_gen_p + i] = 1.0; }
  }
  for (int i = 0; i < g.n_load; ++i) {
    const int b = bus_of(e->h_load_sub[i], topo[e->h_load_pos[i]]);
    if (b >= 0) { act[b] = 1; inj_bus[oo.inj_load_p + i] = b; inj_w[oo.inj_load_p + i] = -1.0; }
  }
  for (int i = 0; i < g.n_sto; ++i) {
    const int b = bus_of(e->h_sto_sub[i], topo[e->h_sto_pos[i]]);
    if (b >= 0) { act[b] = 1; inj_bus[oo.inj_sto_p + i] = b; inj_w[oo.inj_sto_p + i] = -1.0; }
  }
  for (int i = 0; i < g.n_shunt; ++i) {
    const int b = bus_of(e->h_shunt_sub[i], sb[i]);
    if (b >= 0) { act[b] = 1; inj_bus[oo.inj_sh_p + i] = b; inj_w[oo.inj_sh_p + i] = -e->h_shunt_fact[i]; }
  }
  // reduced B' over the active non-reference buses, inverted by Gauss-Jordan with partial pivoting (once per topology)
  std::vector<int> idx(nbt, -1), buses;
  bool any_ref = false;
  for (int b = 0; b < nbt; ++b) { any_ref |= (act[b] && ref[b]); if (act[b] && !ref[b]) { idx[b] = (int)buses.size(); buses.push_back(b); } }
  if (!any_ref) return fail(GPF_E_INVALID, "gpf_ptdf_build: no in-service slack generator in this topology");
  const int nr = (int)buses.size();
  std::vector<double> M((size_t)nr * 2 * nr, 0.0);
  for (int r = 0; r < nr; ++r) M[(size_t)r * 2 * nr + nr + r] = 1.0;
  for (int l = 0; l < g.n_line; ++l) {
    if (lf[l] < 0 || lf[l] == lt[l]) continue;
    const double bb = e->h_br_bdc[l];
    const int a = idx[lf[l]], c = idx[lt[l]];
    if (a >= 0) M[(size_t)a * 2 * nr + a] += bb;
    if (c >= 0) M[(size_t)c * 2 * nr + c] += bb;
    if (a >= 0 && c >= 0) { M[(size_t)a * 2 * nr + c] -= bb; M[(size_t)c * 2 * nr + a] -= bb; }
  }
  for (int k = 0; k < nr; ++k) {
    int p = k;
    for (int r = k + 1; r < nr; ++r) if (std::fabs(M[(size_t)r * 2 * nr + k]) > std::fabs(M[(size_t)p * 2 * nr + k])) p = r;
    const double pv = M[(size_t)p * 2 * nr + k];
    if (!(std::fabs(pv) > 1e-12)) return fail(GPF_E_INVALID, "gpf_ptdf_build: the topology is islanded (singular B')");
    if (p != k) for (int q = 0; q < 2 * nr; ++q) std::swap(M[(size_t)k * 2 * nr + q], M[(size_t)p * 2 * nr + q]);
    const double rp = 1.0 / pv;
    for (int q = 0; q < 2 * nr; ++q) M[(size_t)k * 2 * nr + q] *= rp;
    for (int r = 0; r < nr; ++r) {
      if (r == k) continue;
      const double mlt = M[(size_t)r * 2 * nr + k];
      if (mlt == 0.0) continue;
      for (int q = k; q < 2 * nr; ++q) M[(size_t)r * 2 * nr + q] -= mlt * M[(size_t)k * 2 * nr + q];
    }
  }
  auto X = [&](int bus_row, int bus_col) -> double {
    const int r = bus_row >= 0 ? idx[bus_row] : -1, c = idx[bus_col];
    return (r >= 0 && c >= 0) ? M[(size_t)r * 2 * nr + nr + c] : 0.0;
  };
  e->h_ptdf.assign((size_t)g.n_line * nbt, 0.0);
  // the device GEMM runs over the ACTIVE buses only (compact index: half of the n_sub * n_busbar ids are unused)
  std::vector<int> compact(nbt, -1);
  int n_act = 0;
  for (int b = 0; b < nbt; ++b) if (act[b]) compact[b] = n_act++;
  const int nb_pad = std::max(4, (n_act + 3) & ~3), line_pad = (g.n_line + 15) & ~15;
  const int kpad = (nb_pad + 31) & ~31;                      // (rows behind nb_pad stay zero: gpf_ptdf_flows_rows runs whole trips of 8 k-steps)
  std::vector<double> pt((size_t)kpad * line_pad, 0.0);
  for (int l = 0; l < g.n_line; ++l) {
    if (lf[l] < 0 || lf[l] == lt[l]) continue;
    for (int b = 0; b < nbt; ++b) {
      if (idx[b] < 0) continue;
      const double v = e->h_br_bdc[l] * (X(lf[l], b) - X(lt[l], b));
      e->h_ptdf[(size_t)l * nbt + b] = v;
      pt[(size_t)compact[b] * line_pad + l] = v;
    }
  }
  for (int i = 0; i < g.n_inj; ++i) if (inj_bus[i] >= 0) inj_bus[i] = compact[inj_bus[i]];
  e->ptdf_ready = false;
  HIP_TRY(e->ptdf_inj_bus.upload(inj_bus.data(), inj_bus.size()));
  HIP_TRY(e->ptdf_inj_w.upload(inj_w.data(), inj_w.size()));
  HIP_TRY(e->ptdf_t.upload(pt.data(), pt.size()));
  if (e->ptdf_nb_pad != nb_pad || e->ptdf_line_pad != line_pad || !e->ptdf_flow.p) {
    HIP_TRY(e->ptdf_flow.alloc((size_t)e->cap_lanes * line_pad));
  }
  {   // LODF[l][k] = H[l][k] / (1 - H[k][k]), H[l][k] = PTDF[l][from_k] - PTDF[l][to_k]; LODF[k][k] = -1
    std::vector<double> lo_((size_t)g.n_line * line_pad, 0.0);
    // elements on every bus: a line whose outage only removes a bus that carries nothing else (one line end, no injection) does not
    // island anything -- the reference's DC power flow of that contingency converges with every other flow unchanged: column of zeros
    std::vector<int> n_lines_at(nbt, 0), n_other_at(nbt, 0);
    for (int l = 0; l < g.n_line; ++l) if (lf[l] >= 0) { ++n_lines_at[lf[l]]; ++n_lines_at[lt[l]]; }
    for (int i = 0; i < g.n_gen; ++i) { const int b = bus_of(e->h_gen_sub[i], topo[e->h_gen_pos[i]]); if (b >= 0) ++n_other_at[b]; }
    for (int i = 0; i < g.n_load; ++i) { const int b = bus_of(e->h_load_sub[i], topo[e->h_load_pos[i]]); if (b >= 0) ++n_other_at[b]; }
    for (int i = 0; i < g.n_sto; ++i) { const int b = bus_of(e->h_sto_sub[i], topo[e->h_sto_pos[i]]); if (b >= 0) ++n_other_at[b]; }
    for (int i = 0; i < g.n_shunt; ++i) { const int b = bus_of(e->h_shunt_sub[i], sb[i]); if (b >= 0) ++n_other_at[b]; }
    for (int k = 0; k < g.n_line; ++k) {
      if (lf[k] < 0 || lf[k] == lt[k]) continue;                 // an open line: its outage changes nothing
      const double hkk = e->h_ptdf[(size_t)k * nbt + lf[k]] - e->h_ptdf[(size_t)k * nbt + lt[k]];
      const double den = 1.0 - hkk;
      const bool dangling = (n_lines_at[lf[k]] == 1 && n_other_at[lf[k]] == 0) || (n_lines_at[lt[k]] == 1 && n_other_at[lt[k]] == 0);
      for (int l = 0; l < g.n_line; ++l) {
        const double hlk = e->h_ptdf[(size_t)l * nbt + lf[k]] - e->h_ptdf[(size_t)l * nbt + lt[k]];
        lo_[(size_t)l * line_pad + k] = std::fabs(den) < 1e-8 ? (dangling ? 0.0 : std::nan("")) : (l == k ? -1.0 : hlk / den);   // (a dangling line: the whole column is zero, as in the batch builder)
      }
    }
    { std::vector<float> lof(lo_.begin(), lo_.end()); HIP_TRY(e->lodf.upload(lof.data(), lof.size())); }
    HIP_TRY(e->lodf_worst.alloc((size_t)e->cap_lanes * line_pad));
  }
  e->ptdf_nb_pad = nb_pad; e->ptdf_line_pad = line_pad;
  e->ptdf_ready = true;
  e->ptdf_batch = false;
  return GPF_OK;
}

// PtdfDev of the tables the flows / screening kernels run on: the single topology of gpf_ptdf_build or the class tables of gpf_ptdf_build_batch
static gpf::PtdfDev ptdf_dev(gpf_engine* e) {
  gpf::PtdfDev P{};
  P.n_inj = e->g.n_inj; P.nb_pad = e->ptdf_nb_pad; P.line_pad = e->ptdf_line_pad; P.n_line = e->g.n_line;
  if (e->ptdf_batch) {
    P.inj_bus = nullptr; P.inj_w = e->ptdfb_inj_w.p; P.ptdf_t = e->ptdfb_t.p;
    P.order = e->ptdfb_order.p; P.blk_class = e->ptdfb_blk_class.p; P.cls_desc = e->ptdfb_desc.p; P.cls_status = e->ptdfb_status.p;
    P.desc_stride = e->ptdfb_desc_stride; P.inj_bus_off = gpf::PTDFB_HDR + 2 * e->g.n_line;
    P.ptdf_stride = (long long)e->ptdfb_kpad * e->ptdf_line_pad;
  } else {
    P.inj_bus = e->ptdf_inj_bus.p; P.inj_w = e->ptdf_inj_w.p; P.ptdf_t = e->ptdf_t.p;
  }
  return P;
}

// A few PERSISTENT host threads for the table walks of gpf_ptdf_build_batch (row hashes / comparisons, descriptors of unseen classes): creating
// threads per call cost more than the work it spread (measured on the MI355X box: no gain from 4 fresh std::threads on 0.8 ms of work).
// Workers sleep on a condition variable between calls; they are detached at process exit (never joined: no ordering against the HIP runtime).
namespace {
class HostPool {
 public:
  static HostPool& get() { static HostPool* p = new HostPool(); return *p; }      // (intentionally leaked)
  int size() const { return n_workers_ + 1; }
  // body(part, n_parts) for part = 0 .. n_parts - 1, part 0 on the caller's thread; returns when all parts are done
  void run(int n_parts, const std::function<void(int, int)>& body) {
    n_parts = std::max(1, std::min(n_parts, size()));
    if (n_parts == 1) { body(0, 1); return; }
    std::lock_guard<std::mutex> call_lk(call_mu_);          // one parallel region at a time
    {
      std::lock_guard<std::mutex> lk(mu_);
      body_ = &body; parts_ = n_parts; next_ = 1; left_ = n_parts - 1; ++gen_;
    }
    cv_.notify_all();
    body(0, n_parts);
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return left_ == 0; });
    body_ = nullptr;
  }
 private:
  HostPool() {
    const char* v = getenv("GRIDPF_PTDFB_THREADS");
    int t = v ? atoi(v) : 4;
    const int hw = (int)std::thread::hardware_concurrency();
    if (hw > 0 && t > hw) t = hw;
    n_workers_ = std::max(0, t - 1);
    for (int w = 0; w < n_workers_; ++w) std::thread([this] { loop(); }).detach();
  }
  void loop() {
    unsigned long long seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return gen_ != seen && next_ < parts_; });
      const unsigned long long g = gen_;
      while (gen_ == g && next_ < parts_) {
        const int part = next_++;
        const std::function<void(int, int)>* b = body_;
        const int np = parts_;
        lk.unlock();
        (*b)(part, np);
        lk.lock();
        if (--left_ == 0) done_.notify_all();
      }
      seen = g;
    }
  }
  std::mutex mu_, call_mu_;
  std::condition_variable cv_, done_;
  const std::function<void(int, int)>* body_ = nullptr;
  int n_workers_ = 0, parts_ = 0, next_ = 0, left_ = 0;
  unsigned long long gen_ = 0;
};
}  // namespace

// completes the asynchronous tail of gpf_ptdf_build_batch: class status in h_ptdfb_status, kernel duration in ptdfb_kernel_ms
static int ptdfb_finish(gpf_engine* e) {
  if (!e->ptdfb_pending) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::copy(e->ptdfb_status_pin.p, e->ptdfb_status_pin.p + e->h_ptdfb_status.size(), e->h_ptdfb_status.begin());
  if (e->ptdfb_prefetched && e->ptdfb_host_stale) {            // (device path: the class map and the descriptor headers came back behind the status)
    const int n = e->ptdfb_n, nc = e->ptdfb_classes;
    e->h_ptdfb_lane_class.assign(e->ptdfg_back_pin.p, e->ptdfg_back_pin.p + n);
    e->h_ptdfb_hdr.assign(e->ptdfg_back_pin.p + n, e->ptdfg_back_pin.p + n + (size_t)nc * 4);
    e->ptdfb_host_stale = false;
  }
  e->ptdfb_prefetched = false;
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e->ptdfb_ev_a, e->ptdfb_ev_b);
  e->ptdfb_kernel_ms = ms;
  e->ptdfb_pending = false;
  return GPF_OK;
}

// lane -> class map and descriptor headers of a build whose integer half ran on the device: to the host mirrors, on demand (12 KB for 2 048
// lanes / 256 classes; the descriptors themselves stay on the device); with_bus: the compact -> bus maps too (gpf_ptdf_batch_get)
static int ptdfb_fetch_host(gpf_engine* e, bool with_bus = false) {
  if (!e->ptdfb_host_stale && !(with_bus && e->ptdfb_bus_stale)) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const int n = e->ptdfb_n, nc = e->ptdfb_classes, stride = e->ptdfb_desc_stride, nbt = e->g.nb_tot;
  if (e->ptdfb_host_stale) {
    e->h_ptdfb_lane_class.resize(n);
    HIP_TRY(hipMemcpy(e->h_ptdfb_lane_class.data(), e->ptdfg_lane_class.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    e->h_ptdfb_hdr.resize((size_t)nc * 4);
    HIP_TRY(hipMemcpy2D(e->h_ptdfb_hdr.data(), 4 * sizeof(int), e->ptdfb_desc.p, (size_t)stride * sizeof(int), 4 * sizeof(int), (size_t)nc, hipMemcpyDeviceToHost));
    e->ptdfb_host_stale = false;
  }
  if (with_bus && e->ptdfb_bus_stale) {
    std::vector<int> c2b((size_t)nc * nbt);
    HIP_TRY(hipMemcpy(c2b.data(), e->ptdfg_c2b.p, c2b.size() * sizeof(int), hipMemcpyDeviceToHost));
    e->h_ptdfb_bus.assign(nc, std::vector<int>());
    for (int c = 0; c < nc; ++c) {
      const int n_act = e->h_ptdfb_hdr[(size_t)c * 4 + 1];
      e->h_ptdfb_bus[c].assign(c2b.begin() + (size_t)c * nbt, c2b.begin() + (size_t)c * nbt + n_act);
    }
    e->ptdfb_bus_stale = false;
  }
  return GPF_OK;
}

// The integer half of gpf_ptdf_build_batch on the device.  out[0..3] = classes, slots, largest n_pad, largest n_act.  Returns GPF_OK with
// *done = false when the device path does not apply or flagged something (hash collision inside a class, bus id out of range, capacity):
// the caller then takes the host path, which reports the error properly.
static int ptdfb_group_on_device(gpf_engine* e, int lane0, int n, int stride, int out[4], bool* done) {
  *done = false;
  const gpf::GridDev& g = e->g;
  if (n > gpf::PTDFG_MAX_LANES || g.nb_tot > gpf::PTDFG_MAX_BUS || g.n_line > 256 || getenv("GRIDPF_PTDFB_HOST")) return GPF_OK;
  HIP_TRY(e->ptdfg_hash.ensure((size_t)n)); HIP_TRY(e->ptdfg_lane_class.ensure((size_t)n)); HIP_TRY(e->ptdfg_first.ensure((size_t)n));
  HIP_TRY(e->ptdfb_order.ensure((size_t)16 * n)); HIP_TRY(e->ptdfb_blk_class.ensure((size_t)n));
  HIP_TRY(e->ptdfb_desc.ensure((size_t)n * stride)); HIP_TRY(e->ptdfg_c2b.ensure((size_t)n * g.nb_tot)); HIP_TRY(e->ptdfg_info.ensure(8));
  HIP_TRY(e->ptdfg_info_pin.reserve(8));
  gpf::PtdfGroupDev D{};
  D.topo = e->topo.p; D.shunt_bus = e->shunt_bus.p;
  D.lane0 = lane0; D.n = n; D.dim_topo = g.dim_topo; D.n_shunt = g.n_shunt; D.n_sub = g.n_sub; D.n_busbar = g.n_busbar; D.n_line = g.n_line;
  D.n_gen = g.n_gen; D.n_load = g.n_load; D.n_sto = g.n_sto; D.n_inj = g.n_inj;
  D.inj_gen_p = e->oo.inj_gen_p; D.inj_load_p = e->oo.inj_load_p; D.inj_sto_p = e->oo.inj_sto_p; D.inj_sh_p = e->oo.inj_sh_p;
  D.line_or_pos = e->line_or_pos.p; D.line_ex_pos = e->line_ex_pos.p; D.line_or_sub = e->line_or_sub.p; D.line_ex_sub = e->line_ex_sub.p;
  D.gen_pos = e->gen_pos.p; D.gen_sub = e->gen_sub.p; D.load_pos = e->load_pos.p; D.load_sub = e->load_sub.p; D.sto_pos = e->sto_pos.p;
  D.sto_sub = e->sto_sub.p; D.shunt_sub = e->shunt_sub.p; D.gen_slack = e->gen_slack.p;
  D.desc_stride = stride;
  D.hash = e->ptdfg_hash.p; D.lane_class = e->ptdfg_lane_class.p; D.first_lane = e->ptdfg_first.p; D.order = e->ptdfb_order.p;
  D.blk_class = e->ptdfb_blk_class.p; D.desc = e->ptdfb_desc.p; D.c2b = e->ptdfg_c2b.p; D.info = e->ptdfg_info.p;
  hipLaunchKernelGGL(gpf::ptdfg_hash_kernel, dim3(n), dim3(64), 0, e->stream, D);
  int np2 = gpf::PTDFG_SORT_THREADS;                   // (ptdfg_group_kernel sorts a multiple of its workgroup)
  while (np2 < n) np2 <<= 1;
  const size_t lds_sort = (size_t)np2 * 20;
  static size_t lds_sort_set[64] = {0};
  if (lds_sort > lds_sort_set[e->device & 63]) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&gpf::ptdfg_group_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sort));
    lds_sort_set[e->device & 63] = lds_sort;
  }
  hipLaunchKernelGGL(gpf::ptdfg_group_kernel, dim3(1), dim3(gpf::PTDFG_SORT_THREADS), lds_sort, e->stream, D);
  hipLaunchKernelGGL(gpf::ptdfg_verify_kernel, dim3(n), dim3(64), 0, e->stream, D);
  hipLaunchKernelGGL(gpf::ptdfg_desc_kernel, dim3(n), dim3(gpf::PTDFG_DESC_THREADS), 0, e->stream, D);     // (blocks beyond the class count return at once)
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(e->ptdfg_info_pin.p, e->ptdfg_info.p, 8 * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const int* info = e->ptdfg_info_pin.p;
  if (info[4] || info[5] || info[0] <= 0) return GPF_OK;           // -> host path
  out[0] = info[0]; out[1] = info[1]; out[2] = std::max(16, info[2]); out[3] = std::max(1, info[3]);
  *done = true;
  return GPF_OK;
}

/* ---- PTDF / LODF of every distinct topology of a lane range, built on the device (gridpf_ptdf_batch.hpp) --------------------------- */
int gpf_ptdf_build_batch(gpf_handle e, int32_t lane0, int32_t n, int32_t with_lodf, int32_t* n_classes_out) {
  if (!check_range(e, lane0, n) || n <= 0) return fail(GPF_E_INVALID, "gpf_ptdf_build_batch: bad lane range");
  HIP_TRY(hipSetDevice(e->device));
  // a rebuild overwrites the lane -> class map and may regrow the device tables before it can fail: from here until it has succeeded there
  // are NO tables (gpf_ptdf_flows / gpf_ptdf_batch_get refuse), instead of new lane classes against old tables
  e->ptdf_ready = false; e->ptdf_batch = false;
  e->ptdfb_pending = false;                        // (a status nobody asked for: the stream orders the next build behind the last one)
  const gpf::GridDev& g = e->g;
  const gpf::OutOff& oo = e->oo;
  const int nl = g.n_line, nbt = g.nb_tot, nsh = g.n_shunt;
  static const bool stage_timing = getenv("GRIDPF_SIM_TIMING") != nullptr;      // developer: stage times of the call on stderr
  auto now_us = [] { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() * 1e-3; };
  double tm[6] = {0, 0, 0, 0, 0, 0};
  // ---- the integer half: on the device (gridpf_ptdf_group.hpp) when the range allows it, else -- and whenever the device flagged something -- on the host
  const int stride = (gpf::PTDFB_HDR + 3 * nl + g.n_inj + gpf::PTDFB_MAX_N + 1 + 2 * nl + 3) & ~3;
  int nc = 0, npad_max = 16, nact_max = 1;
  size_t n_slots = 0;
  std::vector<int> desc, order, blk_class;
  int grp[4] = {0, 0, 0, 0};
  bool dev = false;
  { const int rc_g = ptdfb_group_on_device(e, lane0, n, stride, grp, &dev); if (rc_g != GPF_OK) return rc_g; }
  auto host_group = [&]() -> int {
  // the lanes' topology rows as they are on the device (a cascade inside gpf_step_n may have tripped lines the host never saw)
  // (when no kernel can have rewritten them -- no cascade, no outage tables since the engine was created -- and the host sent every row of the
  //  range itself, the host mirrors ARE the device rows: no trip over PCIe, no synchronisation; 2 048 rows of 560 ints are 4.6 MB)
  std::vector<int> topo_own, sb_own;
  const int* topo_p = nullptr;
  const int* sb_p = nullptr;
  bool mirror_ok = !e->dev_topo_dirty && getenv("GRIDPF_PTDFB_NO_MIRROR") == nullptr;
  for (int k = lane0; k < lane0 + n && mirror_ok; ++k)
    mirror_ok = e->h_lane_topo[(size_t)k * g.dim_topo] != INT_MIN && (!nsh || e->h_lane_sb[(size_t)k * nsh] != INT_MIN);
  if (stage_timing) tm[0] = now_us();
  if (mirror_ok) {
    topo_p = e->h_lane_topo.data() + (size_t)lane0 * g.dim_topo;
    sb_p = e->h_lane_sb.data() + (size_t)lane0 * std::max(nsh, 1);
  } else {
    topo_own.resize((size_t)n * g.dim_topo); sb_own.resize((size_t)n * std::max(nsh, 1));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stage_timing) tm[0] = now_us();
    HIP_TRY(hipMemcpy(topo_own.data(), e->topo.p + (size_t)lane0 * g.dim_topo, topo_own.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (nsh) HIP_TRY(hipMemcpy(sb_own.data(), e->shunt_bus.p + (size_t)lane0 * nsh, (size_t)n * nsh * sizeof(int), hipMemcpyDeviceToHost));
    topo_p = topo_own.data(); sb_p = sb_own.data();
  }
  struct RowView { const int* p; const int* data() const { return p; } int operator[](size_t i) const { return p[i]; } } topo{topo_p}, sb{sb_p};
  if (stage_timing) tm[1] = now_us();
  // ---- classes: lanes with identical (topology row, shunt buses) ----------------------------------------------------------------------
  std::unordered_map<uint64_t, std::vector<int>> cls_of;     // row hash -> classes with that hash (rows compared on a hit)
  std::vector<int> first_lane;                       // representative lane (index in the range) of each class
  std::vector<uint64_t> first_hash;                  // its row hash (key of the descriptor cache)
  e->h_ptdfb_lane_class.assign(n, -1);
  auto same_rows = [&](int a, int b) {
    return std::memcmp(topo.data() + (size_t)a * g.dim_topo, topo.data() + (size_t)b * g.dim_topo, (size_t)g.dim_topo * sizeof(int)) == 0 &&
           (!nsh || std::memcmp(sb.data() + (size_t)a * nsh, sb.data() + (size_t)b * nsh, (size_t)nsh * sizeof(int)) == 0);
  };
  cls_of.reserve((size_t)n);
  // host threads for the two table walks of this call (row hashes, descriptors of unseen classes): a few hundred microseconds of one core each
  // for 2 048 lanes / 256 classes of a 118-substation grid, embarrassingly parallel
  HostPool& pool = HostPool::get();
  auto par_for = [&](int count, int min_per_thread, const std::function<void(int, int, int)>& body) {     // body(begin, end, part index)
    const int nt = std::max(1, std::min(pool.size(), count / std::max(1, min_per_thread)));
    pool.run(nt, [&](int part, int n_parts) { body((int)((long long)count * part / n_parts), (int)((long long)count * (part + 1) / n_parts), part); });
  };
  std::vector<uint64_t> row_hash((size_t)n);
  par_for(n, 256, [&](int k0, int k1, int) {
  for (int k = k0; k < k1; ++k) {
    // row hash: four independent multiply-xor chains over the row (one dependent multiply per int was 1 ms for 2 048 rows of 560 ints);
    // equal hashes are confirmed by comparing the rows, so the hash only has to spread
    const int* tp = topo.data() + (size_t)k * g.dim_topo;
    uint64_t h0 = 1469598103934665603ull, h1 = 0x9E3779B97F4A7C15ull, h2 = 0xC2B2AE3D27D4EB4Full, h3 = 0x165667B19E3779F9ull;
    int i = 0;
    for (; i + 8 <= g.dim_topo; i += 8) {
      h0 = (h0 ^ ((uint64_t)(uint32_t)tp[i] | ((uint64_t)(uint32_t)tp[i + 1] << 32))) * 0x9FB21C651E98DF25ull;
      h1 = (h1 ^ ((uint64_t)(uint32_t)tp[i + 2] | ((uint64_t)(uint32_t)tp[i + 3] << 32))) * 0xD6E8FEB86659FD93ull;
      h2 = (h2 ^ ((uint64_t)(uint32_t)tp[i + 4] | ((uint64_t)(uint32_t)tp[i + 5] << 32))) * 0xA0761D6478BD642Full;
      h3 = (h3 ^ ((uint64_t)(uint32_t)tp[i + 6] | ((uint64_t)(uint32_t)tp[i + 7] << 32))) * 0xE7037ED1A0B428DBull;
    }
    for (; i < g.dim_topo; ++i) h0 = (h0 ^ (uint32_t)tp[i]) * 1099511628211ull;
    for (int q = 0; q < nsh; ++q) h1 = (h1 ^ ((uint32_t)sb[(size_t)k * nsh + q] + 0x9E3779B9u)) * 1099511628211ull;
    uint64_t h = h0 ^ (h1 >> 29 | h1 << 35) ^ (h2 >> 17 | h2 << 47) ^ (h3 >> 41 | h3 << 23);
    h ^= h >> 32;
    row_hash[k] = h;
  }
  });
  // classes by hash first (no row is touched), then every lane's row is compared with its class representative's -- in parallel: the two
  // passes over the rows (hash, confirm) are what grouping costs (4.6 MB each for 2 048 lanes of a 118-substation grid, memory-bound on one core)
  for (int k = 0; k < n; ++k) {
    const uint64_t h = row_hash[k];
    std::vector<int>& cand = cls_of[h];
    if (cand.empty()) { cand.push_back((int)first_lane.size()); first_lane.push_back(k); first_hash.push_back(h); }
    e->h_ptdfb_lane_class[k] = cand[0];
  }
  std::vector<char> differs((size_t)n, 0);
  par_for(n, 256, [&](int k0, int k1, int) {
    for (int k = k0; k < k1; ++k) { const int rep = first_lane[e->h_ptdfb_lane_class[k]]; differs[k] = (rep != k && !same_rows(rep, k)) ? 1 : 0; }
  });
  for (int k = 0; k < n; ++k) {                     // (a 64-bit hash collision between different rows: never seen; handled the slow way)
    if (!differs[k]) continue;
    const uint64_t h = row_hash[k];
    std::vector<int>& cand = cls_of[h];
    int c = -1;
    for (size_t q = 1; q < cand.size(); ++q) if (same_rows(first_lane[cand[q]], k)) { c = cand[q]; break; }
    if (c < 0) { c = (int)first_lane.size(); first_lane.push_back(k); first_hash.push_back(h); cand.push_back(c); }
    e->h_ptdfb_lane_class[k] = c;
  }
  nc = (int)first_lane.size();
  if (stage_timing) tm[2] = now_us();
  // descriptor: header | lf | lt | inj_bus | lflag | row pointers of B' [PTDFB_MAX_N + 1] | row entries [2 n_line] (gridpf_ptdf_batch.hpp)
  if (nl > 65535) return fail(GPF_E_CAPACITY, "gpf_ptdf_build_batch: more than 65535 lines");
  desc.assign((size_t)nc * stride, -1);
  e->h_ptdfb_bus.assign(nc, std::vector<int>());
  auto bus_of = [&](int sub, int local) -> int { return (local >= 1 && local <= g.n_busbar) ? sub + (local - 1) * g.n_sub : -1; };
  // One descriptor per class: ~3 us of table walks each (800 us for 256 classes of a 118-substation grid on one core)
  struct ClsScratch { std::vector<char> act, ref, has_ref; std::vector<int> bf, bt, n_lines_at, n_other_at, ibus, compact, comp, cnt; int npad_max = 16, nact_max = 1; };
  auto build_class = [&](int c, ClsScratch& S_) -> int {
    std::vector<char>&act = S_.act, &ref = S_.ref, &has_ref = S_.has_ref;
    std::vector<int>&bf = S_.bf, &bt = S_.bt, &n_lines_at = S_.n_lines_at, &n_other_at = S_.n_other_at, &ibus = S_.ibus, &compact = S_.compact, &comp = S_.comp, &cnt = S_.cnt;
    const int* tp = topo.data() + (size_t)first_lane[c] * g.dim_topo;
    const int* sbp = sb.data() + (size_t)first_lane[c] * std::max(nsh, 1);
    int* d = desc.data() + (size_t)c * stride;
    int* lf = d + gpf::PTDFB_HDR;
    int* lt = lf + nl;
    int* ib = lt + nl;
    int* lflag = ib + g.n_inj;
    act.assign(nbt, 0); ref.assign(nbt, 0);
    bf.assign(nl, -1); bt.assign(nl, -1);
    n_lines_at.assign(nbt, 0); n_other_at.assign(nbt, 0);      // in-service line ends / other elements on each bus
    for (int l = 0; l < nl; ++l) {
      const int bo = tp[e->h_line_or_pos[l]], be = tp[e->h_line_ex_pos[l]];
      if (bo >= 1 && be >= 1) {
        bf[l] = bus_of(e->h_line_or_sub[l], bo); bt[l] = bus_of(e->h_line_ex_sub[l], be);
        if (bf[l] < 0 || bt[l] < 0) return 1;
        act[bf[l]] = act[bt[l]] = 1;
      }
    }
    ibus.assign(g.n_inj, -1);
    for (int i = 0; i < g.n_gen; ++i) {
      const int b = bus_of(e->h_gen_sub[i], tp[e->h_gen_pos[i]]);
      if (b < 0) continue;
      act[b] = 1;
      ++n_other_at[b];
      if (e->h_gen_slack[i]) ref[b] = 1; else ibus[oo.inj_gen_p + i] = b;
    }
    for (int i = 0; i < g.n_load; ++i) { const int b = bus_of(e->h_load_sub[i], tp[e->h_load_pos[i]]); if (b >= 0) { act[b] = 1; ++n_other_at[b]; ibus[oo.inj_load_p + i] = b; } }
    for (int i = 0; i < g.n_sto; ++i) { const int b = bus_of(e->h_sto_sub[i], tp[e->h_sto_pos[i]]); if (b >= 0) { act[b] = 1; ++n_other_at[b]; ibus[oo.inj_sto_p + i] = b; } }
    for (int i = 0; i < nsh; ++i) { const int b = bus_of(e->h_shunt_sub[i], sbp[i]); if (b >= 0) { act[b] = 1; ++n_other_at[b]; ibus[oo.inj_sh_p + i] = b; } }
    for (int l = 0; l < nl; ++l) if (bf[l] >= 0) { ++n_lines_at[bf[l]]; ++n_lines_at[bt[l]]; }
    // compact numbering: active non-reference buses first, then the active reference buses
    compact.assign(nbt, -1);
    std::vector<int>& c2b = e->h_ptdfb_bus[c];
    c2b.reserve(nbt);
    int nr = 0, n_act = 0;
    for (int b = 0; b < nbt; ++b) if (act[b] && !ref[b]) { compact[b] = nr++; c2b.push_back(b); }
    n_act = nr;
    bool any_ref = false;
    for (int b = 0; b < nbt; ++b) if (act[b] && ref[b]) { compact[b] = n_act++; c2b.push_back(b); any_ref = true; }
    // connectivity (rundcpp(check_connectivity=True), pandaPowerBackend.py:1090): every active bus must reach a reference bus
    int status = any_ref ? 0 : 3;
    if (any_ref) {
      comp.resize(nbt);
      for (int b = 0; b < nbt; ++b) comp[b] = b;
      auto find = [&](int x) { while (comp[x] != x) { comp[x] = comp[comp[x]]; x = comp[x]; } return x; };
      for (int l = 0; l < nl; ++l) if (bf[l] >= 0 && bf[l] != bt[l]) comp[find(bf[l])] = find(bt[l]);
      has_ref.assign(nbt, 0);
      for (int b = 0; b < nbt; ++b) if (act[b] && ref[b]) has_ref[find(b)] = 1;
      for (int b = 0; b < nbt; ++b) if (act[b] && !has_ref[find(b)]) { status = 2; break; }
    }
    const int n_pad = std::max(16, (nr + 15) & ~15);
    if (n_pad > gpf::PTDFB_MAX_N) return 2;
    d[0] = nr; d[1] = n_act; d[2] = n_pad; d[3] = status;
    for (int l = 0; l < nl; ++l) {
      const bool on = bf[l] >= 0 && bf[l] != bt[l];
      lf[l] = on ? compact[bf[l]] : -1; lt[l] = on ? compact[bt[l]] : -1;
      // a line end on a bus that carries nothing else: the outage of the line removes the bus (no islanding, the other flows stand)
      lflag[l] = (on && ((n_lines_at[bf[l]] == 1 && n_other_at[bf[l]] == 0) || (n_lines_at[bt[l]] == 1 && n_other_at[bt[l]] == 0))) ? 1 : 0;
    }
    {   // rows of the reduced B': for every non-reference bus r the lines at it, ascending, as line | other end << 16
      int* cptr = lflag + nl;
      int* cent = cptr + gpf::PTDFB_MAX_N + 1;
      cnt.assign(nr + 1, 0);
      for (int l = 0; l < nl; ++l) { if (lf[l] < 0) continue; if (lf[l] < nr) ++cnt[lf[l]]; if (lt[l] < nr) ++cnt[lt[l]]; }
      int acc = 0;
      for (int r = 0; r < nr; ++r) { cptr[r] = acc; acc += cnt[r]; cnt[r] = cptr[r]; }
      for (int r = nr; r <= gpf::PTDFB_MAX_N; ++r) cptr[r] = acc;
      for (int i = 0; i < 2 * nl; ++i) cent[i] = 0;
      for (int l = 0; l < nl; ++l) {
        if (lf[l] < 0) continue;
        if (lf[l] < nr) cent[cnt[lf[l]]++] = l | (lt[l] << 16);
        if (lt[l] < nr) cent[cnt[lt[l]]++] = l | (lf[l] << 16);
      }
    }
    for (int i = 0; i < g.n_inj; ++i) ib[i] = ibus[i] >= 0 ? compact[ibus[i]] : -1;
    S_.npad_max = std::max(S_.npad_max, n_pad);
    S_.nact_max = std::max(S_.nact_max, n_act);
    return 0;
  };
  {
    // Descriptors are cached by topology row (hash + the row itself, compared on a hit): a rebuild after some lanes changed their topology
    // -- or the next contingency scan over the same family of topologies -- only walks the tables for classes it has not seen.
    ClsScratch scr;
    const size_t row_ints = (size_t)g.dim_topo + (size_t)nsh;
    const bool no_cache = getenv("GRIDPF_PTDFB_NO_CACHE") != nullptr;      // developer / bench: every class counts as never seen (read at every call)
    if (no_cache || e->ptdfb_cache_stride != stride || e->ptdfb_cache_n > 8192) { e->ptdfb_cache.clear(); e->ptdfb_cache_n = 0; e->ptdfb_cache_stride = stride; }
    std::vector<int> miss;
    for (int c = 0; c < nc; ++c) {
      const int* tp = topo.data() + (size_t)first_lane[c] * g.dim_topo;
      const int* sbp = sb.data() + (size_t)first_lane[c] * std::max(nsh, 1);
      int* d = desc.data() + (size_t)c * stride;
      auto it_b = e->ptdfb_cache.find(first_hash[c]);
      const gpf_engine::PtdfbCached* hit = nullptr;
      if (it_b != e->ptdfb_cache.end())
        for (const auto& ce : it_b->second)
          if (std::memcmp(ce.row.data(), tp, (size_t)g.dim_topo * sizeof(int)) == 0 && (!nsh || std::memcmp(ce.row.data() + g.dim_topo, sbp, (size_t)nsh * sizeof(int)) == 0)) { hit = &ce; break; }
      if (hit) {
        std::memcpy(d, hit->desc.data(), (size_t)stride * sizeof(int));
        e->h_ptdfb_bus[c] = hit->c2b;
      } else miss.push_back(c);
    }
    // the classes never seen before: their descriptors are independent table walks -- spread over the host threads
    std::vector<int> miss_err(miss.size(), 0);
    std::vector<gpf_engine::PtdfbCached> miss_ce(miss.size());      // (the cache entries too: three allocations + 9 KB of copies per class)
    (void)scr;
    par_for((int)miss.size(), 16, [&](int q0, int q1, int) {
      ClsScratch scr_t;
      for (int q = q0; q < q1; ++q) {
        const int c = miss[q];
        miss_err[q] = build_class(c, scr_t);
        if (miss_err[q]) continue;
        gpf_engine::PtdfbCached& ce = miss_ce[q];
        ce.row.resize(row_ints);
        std::memcpy(ce.row.data(), topo.data() + (size_t)first_lane[c] * g.dim_topo, (size_t)g.dim_topo * sizeof(int));
        if (nsh) std::memcpy(ce.row.data() + g.dim_topo, sb.data() + (size_t)first_lane[c] * nsh, (size_t)nsh * sizeof(int));
        const int* d = desc.data() + (size_t)c * stride;
        ce.desc.assign(d, d + stride);
        ce.c2b = e->h_ptdfb_bus[c];
      }
    });
    for (size_t q = 0; q < miss.size(); ++q) {
      const int c = miss[q];
      const int err = miss_err[q];
      if (err == 1) return fail(GPF_E_INVALID, "gpf_ptdf_build_batch: bus id out of range");
      if (err == 2) return fail(GPF_E_CAPACITY, "gpf_ptdf_build_batch: more than 256 active non-reference buses in one topology");
      e->ptdfb_cache[first_hash[c]].push_back(std::move(miss_ce[q]));
      ++e->ptdfb_cache_n;
    }
    for (int c = 0; c < nc; ++c) {
      const int* d = desc.data() + (size_t)c * stride;
      npad_max = std::max(npad_max, d[2]);
      nact_max = std::max(nact_max, d[1]);
    }
  }
  if (stage_timing) tm[3] = now_us();
  // ---- slots: lanes grouped by class, every group padded to a multiple of 16 ------------------------------------------------------------
  std::vector<std::vector<int>> members(nc);
  for (int k = 0; k < n; ++k) members[e->h_ptdfb_lane_class[k]].push_back(lane0 + k);
  for (int c = 0; c < nc; ++c) {
    for (int ln : members[c]) order.push_back(ln);
    while (order.size() & 15) order.push_back(-1);
    while (blk_class.size() * 16 < order.size()) blk_class.push_back(c);
  }
  n_slots = order.size();
  return GPF_OK;
  };
  if (dev) { nc = grp[0]; n_slots = (size_t)grp[1]; npad_max = grp[2]; nact_max = grp[3]; }
  else { const int rc_h = host_group(); if (rc_h != GPF_OK) return rc_h; }
  const int line_pad = (nl + 15) & ~15;
  const int nb_pad = std::max(4, (nact_max + 3) & ~3), kpad = (nb_pad + 31) & ~31;
  e->ptdf_ready = false;
  // (grow-only buffers: a rebuild after a few topology changes allocates nothing; uploads ride the engine's stream in front of the kernel)
  if (!dev) {
    HIP_TRY(e->ptdfb_desc.put(desc.data(), desc.size(), e->stream));
    HIP_TRY(e->ptdfb_order.put(order.data(), order.size(), e->stream));
    HIP_TRY(e->ptdfb_blk_class.put(blk_class.data(), blk_class.size(), e->stream));
  }
  HIP_TRY(e->ptdfb_status.ensure(nc));
  HIP_TRY(e->ptdfb_work.ensure((size_t)nc * npad_max * npad_max));
  HIP_TRY(e->ptdfb_t.ensure((size_t)nc * kpad * line_pad));
  if (with_lodf) HIP_TRY(e->ptdfb_lodf.ensure((size_t)nc * nl * line_pad)); else e->ptdfb_lodf.release();
  if (!e->ptdfb_inj_w.p) {
    std::vector<double> w(g.n_inj, 0.0);
    for (int i = 0; i < g.n_gen; ++i) w[oo.inj_gen_p + i] = 1.0;
    for (int i = 0; i < g.n_load; ++i) w[oo.inj_load_p + i] = -1.0;
    for (int i = 0; i < g.n_sto; ++i) w[oo.inj_sto_p + i] = -1.0;
    for (int i = 0; i < nsh; ++i) w[oo.inj_sh_p + i] = -e->h_shunt_fact[i];
    HIP_TRY(e->ptdfb_inj_w.upload(w.data(), w.size()));
  }
  if (e->ptdf_line_pad != line_pad || !e->ptdf_flow.p) HIP_TRY(e->ptdf_flow.alloc((size_t)e->cap_lanes * line_pad));
  if (with_lodf && (e->ptdf_line_pad != line_pad || !e->lodf_worst.p)) HIP_TRY(e->lodf_worst.alloc((size_t)e->cap_lanes * line_pad));
  gpf::PtdfBuildDev D{};
  D.n_line = nl; D.line_pad = line_pad; D.n_inj = g.n_inj; D.kpad = kpad; D.desc_stride = stride;
  D.work_stride = (long long)npad_max * npad_max; D.ptdf_stride = (long long)kpad * line_pad; D.lodf_stride = (long long)nl * line_pad;
  D.desc = e->ptdfb_desc.p; D.br_bdc = e->br_bdc.p; D.work = e->ptdfb_work.p; D.ptdf_t = e->ptdfb_t.p; D.lodf = with_lodf ? e->ptdfb_lodf.p : nullptr;
  D.status = e->ptdfb_status.p;
  DevArr<long long> dbg;
  static const bool want_dbg = getenv("GRIDPF_PTDFB_DEBUG") != nullptr;     // developer: per-phase shader-clock stamps of class 0 on stderr
  if (want_dbg) { HIP_TRY(dbg.alloc((size_t)nc * 8)); HIP_TRY(hipMemset(dbg.p, 0, (size_t)nc * 8 * sizeof(long long))); D.dbg = dbg.p; }
  // reduced dimension <= 128 (118-substation grids): the matrix of a class lives in LDS (ptdf_build_lds_kernel), else in global memory
  const bool no_resident = getenv("GRIDPF_PTDFB_GLOBAL") != nullptr;   // developer / tests: force the global-memory kernel (read at every call)
  const bool resident = npad_max <= 128 && line_pad <= gpf::PTDFB_LDS_THREADS && !no_resident && gpf::ptdfb_lds_bytes_resident(npad_max, line_pad, nl) <= LDS_HARD_LIMIT;
  const size_t lds = resident ? gpf::ptdfb_lds_bytes_resident(npad_max, line_pad, nl) : gpf::ptdfb_lds_bytes(npad_max, line_pad);
  static size_t lds_set[64][2] = {{0}};
  if (lds > lds_set[e->device & 63][resident]) {
    HIP_TRY(hipFuncSetAttribute(resident ? reinterpret_cast<const void*>(&gpf::ptdf_build_lds_kernel) : reinterpret_cast<const void*>(&gpf::ptdf_build_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_set[e->device & 63][resident] = lds;
  }
  if (stage_timing) tm[4] = now_us();
  if (!e->ptdfb_ev_a) { HIP_TRY(e->ptdfb_ev_a.create()); HIP_TRY(e->ptdfb_ev_b.create()); }     // (the engine's: destroyed with it)
  HIP_TRY(e->ptdfb_status_pin.reserve(nc, nc / 4 + 64));
  struct { hipEvent_t a, b; } ev{e->ptdfb_ev_a, e->ptdfb_ev_b};
  HIP_TRY(hipEventRecord(ev.a, e->stream));
  if (resident) hipLaunchKernelGGL(gpf::ptdf_build_lds_kernel, dim3(nc), dim3(gpf::PTDFB_LDS_THREADS), lds, e->stream, D);
  else hipLaunchKernelGGL(gpf::ptdf_build_kernel, dim3(nc), dim3(gpf::PTDFB_THREADS), lds, e->stream, D);
  hipError_t le = hipGetLastError();
  HIP_TRY(hipEventRecord(ev.b, e->stream));
  if (le != hipSuccess) return fail(GPF_E_DEVICE, std::string("ptdf_build_kernel: ") + hipGetErrorString(le));
  // the class status comes back by DMA into a pinned block behind the kernel; nobody waits here -- the flows / screening calls queue on the
  // same stream, gpf_ptdf_batch_info (status, kernel time) synchronises when it is asked (ptdfb_finish)
  e->h_ptdfb_status.assign(nc, 0);
  HIP_TRY(hipMemcpyAsync(e->ptdfb_status_pin.p, e->ptdfb_status.p, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  e->ptdfb_n = n; e->ptdfb_classes = nc; e->ptdfb_desc_stride = stride;      // (what ptdfb_finish / ptdfb_fetch_host size their copies by)
  e->ptdfb_host_stale = dev; e->ptdfb_bus_stale = dev;
  e->ptdfb_prefetched = false;
  if (dev) {                                        // what gpf_ptdf_batch_info will be asked for rides the same stream: one wait gets it all
    const size_t need = (size_t)n + (size_t)nc * 4;
    HIP_TRY(e->ptdfg_back_pin.reserve(need, need / 4 + 256));
    HIP_TRY(hipMemcpyAsync(e->ptdfg_back_pin.p, e->ptdfg_lane_class.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpy2DAsync(e->ptdfg_back_pin.p + n, 4 * sizeof(int), e->ptdfb_desc.p, (size_t)stride * sizeof(int), 4 * sizeof(int), (size_t)nc, hipMemcpyDeviceToHost, e->stream));
    e->ptdfb_prefetched = true;
  }
  e->ptdfb_pending = true;
  float ms = 0.f;
  if (stage_timing || want_dbg) { int rc_f = ptdfb_finish(e); if (rc_f != GPF_OK) return rc_f; ms = (float)e->ptdfb_kernel_ms; }
  if (stage_timing)
    fprintf(stderr, "[gridpf] ptdf_build_batch %d lanes, %d classes: rows to the host %.0f us, grouping %.0f, descriptors %.0f, slots + uploads %.0f, kernel + status %.0f\n",
            n, nc, tm[1] - tm[0], tm[2] - tm[1], tm[3] - tm[2], tm[4] - tm[3], now_us() - tm[4]);
  if (want_dbg) {
    std::vector<long long> h((size_t)nc * 8);
    (void)hipMemcpy(h.data(), dbg.p, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
    int c_ok = 0;
    while (c_ok < nc - 1 && e->h_ptdfb_status[c_ok] != 0) ++c_ok;
    const long long* s_ = h.data() + (size_t)c_ok * 8;
    fprintf(stderr, "[gridpf] ptdf_build_kernel class %d (n_pad %d), shader clocks: assemble %lld, gauss-jordan %lld (panel loads %lld, tile inversions %lld, trailing "
                    "updates %lld), PTDF^T %lld, LODF %lld (row builds %lld); kernel %.1f us\n", c_ok, dev ? 0 : desc[(size_t)c_ok * stride + 2], s_[1] - s_[0], s_[3] - s_[1], s_[7], s_[2], s_[6],
            s_[4] - s_[3], s_[5] ? s_[5] - s_[4] : 0LL, s_[7], ms * 1e3);
    dbg.release();
  }
  if (e->window) { ++e->win_launches; e->win_marked = false; }
  if (!dev) { e->h_ptdfb_desc = std::move(desc); e->h_ptdfb_hdr.clear(); }
  e->ptdfb_host_stale = dev; e->ptdfb_bus_stale = dev;                       // (device path: lane -> class map, descriptors, compact -> bus maps are fetched when somebody asks)
  e->ptdfb_lane0 = lane0; e->ptdfb_n = n; e->ptdfb_classes = nc; e->ptdfb_slots = (int)n_slots; e->ptdfb_kpad = kpad;
  e->ptdfb_npad_max = npad_max; e->ptdfb_desc_stride = stride;
  e->ptdf_nb_pad = nb_pad; e->ptdf_line_pad = line_pad;
  e->ptdf_rows_valid = 0;
  e->ptdf_batch = true;
  e->ptdf_ready = true;
  if (n_classes_out) *n_classes_out = nc;
  return GPF_OK;
}

int gpf_ptdf_batch_info(gpf_handle e, int32_t* lane_class, int32_t* class_status, int32_t* class_n, double* kernel_ms) {
  if (!e) return fail(GPF_E_INVALID, "gpf_ptdf_batch_info: null");
  if (!e->ptdf_ready || !e->ptdf_batch) return fail(GPF_E_INVALID, "gpf_ptdf_batch_info: call gpf_ptdf_build_batch first");
  if (class_status || kernel_ms) { const int rc_f = ptdfb_finish(e); if (rc_f != GPF_OK) return rc_f; }
  if (lane_class || class_n) { const int rc_m = ptdfb_fetch_host(e); if (rc_m != GPF_OK) return rc_m; }
  if (lane_class) std::copy(e->h_ptdfb_lane_class.begin(), e->h_ptdfb_lane_class.end(), lane_class);
  if (class_status) std::copy(e->h_ptdfb_status.begin(), e->h_ptdfb_status.end(), class_status);
  if (class_n) for (int c = 0; c < e->ptdfb_classes; ++c) class_n[c] = e->h_ptdfb_hdr.empty() ? e->h_ptdfb_desc[(size_t)c * e->ptdfb_desc_stride] : e->h_ptdfb_hdr[(size_t)c * 4];
  if (kernel_ms) *kernel_ms = e->ptdfb_kernel_ms;
  return GPF_OK;
}

int gpf_ptdf_batch_get(gpf_handle e, int32_t cls, double* ptdf, double* lodf) {
  if (!e) return fail(GPF_E_INVALID, "gpf_ptdf_batch_get: null");
  if (!e->ptdf_ready || !e->ptdf_batch) return fail(GPF_E_INVALID, "gpf_ptdf_batch_get: call gpf_ptdf_build_batch first");
  if (cls < 0 || cls >= e->ptdfb_classes) return fail(GPF_E_INVALID, "gpf_ptdf_batch_get: bad class");
  { const int rc_m = ptdfb_fetch_host(e, true); if (rc_m != GPF_OK) return rc_m; }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const int nl = e->g.n_line, lp = e->ptdf_line_pad, nbt = e->g.nb_tot, kpad = e->ptdfb_kpad;
  if (ptdf) {
    std::vector<double> pt((size_t)kpad * lp);
    HIP_TRY(hipMemcpy(pt.data(), e->ptdfb_t.p + (size_t)cls * kpad * lp, pt.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::fill(ptdf, ptdf + (size_t)nl * nbt, 0.0);
    const std::vector<int>& c2b = e->h_ptdfb_bus[cls];
    for (size_t c = 0; c < c2b.size(); ++c)
      for (int l = 0; l < nl; ++l) ptdf[(size_t)l * nbt + c2b[c]] = pt[c * lp + l];
  }
  if (lodf) {
    if (!e->ptdfb_lodf.p) return fail(GPF_E_INVALID, "gpf_ptdf_batch_get: the batch was built without LODF tables");
    std::vector<float> lof((size_t)nl * lp);
    HIP_TRY(hipMemcpy(lof.data(), e->ptdfb_lodf.p + (size_t)cls * nl * lp, lof.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int m = 0; m < nl; ++m) for (int k = 0; k < nl; ++k) lodf[(size_t)m * nl + k] = (double)lof[(size_t)m * lp + k];
  }
  return GPF_OK;
}

int gpf_ptdf_get(gpf_handle e, double* ptdf) {
  if (!e || !ptdf) return fail(GPF_E_INVALID, "gpf_ptdf_get: null");
  if (!e->ptdf_ready || e->ptdf_batch) return fail(GPF_E_INVALID, "gpf_ptdf_get: call gpf_ptdf_build first (per-lane topologies: gpf_ptdf_batch_get)");
  std::copy(e->h_ptdf.begin(), e->h_ptdf.end(), ptdf);
  return GPF_OK;
}

int gpf_ptdf_flows(gpf_handle e, int32_t lane0, int32_t n) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_ptdf_flows: bad range");
  if (!e->ptdf_ready) return fail(GPF_E_INVALID, "gpf_ptdf_flows: call gpf_ptdf_build first");
  if (n == 0) return GPF_OK;
  if (e->ptdf_batch && (lane0 != e->ptdfb_lane0 || n != e->ptdfb_n))
    return fail(GPF_E_INVALID, "gpf_ptdf_flows: per-lane topologies (gpf_ptdf_build_batch): the call must cover exactly the lane range that was built");
  HIP_TRY(hipSetDevice(e->device));
  const gpf::PtdfDev P = ptdf_dev(e);
  const size_t lds_a = (size_t)16 * gpf::ptdf_a_stride(P.nb_pad) * sizeof(double);
  const int n_blk = e->ptdf_batch ? e->ptdfb_slots / 16 : (n + 15) / 16;
  hipLaunchKernelGGL(gpf::ptdf_flows_kernel, dim3(n_blk, (P.line_pad / 16 + 3) / 4), dim3(256), lds_a, e->stream, P, e->inj.p, lane0, n,
                     e->ptdf_flow.p);
  HIP_TRY(hipGetLastError());
  if (e->window) { ++e->win_launches; e->win_marked = false; }
  return GPF_OK;
}

int gpf_ptdf_flows_rows(gpf_handle e, int32_t t0, int32_t n_rows, double rebalance) {
  if (!e || n_rows <= 0) return fail(GPF_E_INVALID, "gpf_ptdf_flows_rows: bad arguments");
  if (!e->ptdf_ready) return fail(GPF_E_INVALID, "gpf_ptdf_flows_rows: call gpf_ptdf_build first");
  if (!e->chron.p || e->chron_T <= 0) return fail(GPF_E_INVALID, "gpf_ptdf_flows_rows: no chronics uploaded");
  HIP_TRY(hipSetDevice(e->device));
  const size_t need = (size_t)n_rows * e->cap_lanes * e->ptdf_line_pad;
  if (e->ptdf_flow_rows.n < need) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(e->ptdf_flow_rows.alloc(need));
  }
  if (e->ptdf_batch && (e->ptdfb_lane0 != 0 || e->ptdfb_n != e->n_lanes))
    return fail(GPF_E_INVALID, "gpf_ptdf_flows_rows: per-lane topologies (gpf_ptdf_build_batch) must have been built for ALL lanes");
  const gpf::PtdfDev P = ptdf_dev(e);
  gpf::PtdfRowsDev R{};
  R.chron = e->chron.p; R.lane_table = e->lane_table.p; R.lane_offset = e->lane_offset.p;
  R.lane_scale = e->has_scale ? e->lane_scale.p : nullptr; R.lane_gen_delta = e->has_delta ? e->lane_gen_delta.p : nullptr;
  R.gen_slack = e->gen_slack.p; R.T = e->chron_T; R.n_chron = e->g.n_chron; R.n_load = e->g.n_load; R.n_gen = e->g.n_gen;
  R.inj_gen_p = e->oo.inj_gen_p; R.inj_load_p = e->oo.inj_load_p; R.inj_sto_p = e->oo.inj_sto_p; R.n_inj_tail = e->g.n_inj - e->oo.inj_sto_p;
  R.rebalance = rebalance;
  R.kpad = (P.nb_pad + 31) & ~31;
  static const int mt_env = std::getenv("GRIDPF_PTDF_MT") ? std::atoi(std::getenv("GRIDPF_PTDF_MT")) : 0;      // developer override (1 | 2 | 4)
  const int mt = (mt_env == 1 || mt_env == 2 || mt_env == 4) ? mt_env : 2;
  const int NP = 16 * mt;
  const size_t lds_a = (size_t)NP * gpf::ptdf_rows_stride(R.kpad) * sizeof(double);
  const long long n_pairs = (long long)e->n_lanes * n_rows;
  // per-lane topologies: one block per (group of 16 slots, mt consecutive rows), see ptdf_rows_kernel
  const int n_units = e->ptdf_batch ? e->ptdfb_slots : e->n_lanes;
  const dim3 grid(e->ptdf_batch ? (unsigned)((size_t)(e->ptdfb_slots / 16) * ((n_rows + mt - 1) / mt)) : (unsigned)((n_pairs + NP - 1) / NP));
  static size_t lds_set[64][3] = {{0}};
#define GPF_PTDF_ROWS(MT_, SLOT_)                                                                                                      \
  do {                                                                                                                                 \
    if (lds_a > lds_set[e->device & 63][SLOT_]) {                                                                                      \
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&gpf::ptdf_rows_kernel<MT_>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a)); \
      lds_set[e->device & 63][SLOT_] = lds_a;                                                                                          \
    }                                                                                                                                  \
    hipLaunchKernelGGL(gpf::ptdf_rows_kernel<MT_>, grid, dim3(256), lds_a, e->stream, P, R, e->inj.p, n_units, (long long)e->cap_lanes, t0, \
                       n_rows, e->ptdf_flow_rows.p);                                                                                   \
  } while (0)
  if (mt == 4) GPF_PTDF_ROWS(4, 2); else if (mt == 2) GPF_PTDF_ROWS(2, 1); else GPF_PTDF_ROWS(1, 0);
#undef GPF_PTDF_ROWS
  HIP_TRY(hipGetLastError());
  e->ptdf_rows_valid = n_rows;
  if (e->window) { ++e->win_launches; e->win_marked = false; }
  return GPF_OK;
}

int gpf_get_ptdf_flows_rows(gpf_handle e, int32_t row0, int32_t n_rows, int32_t lane0, int32_t n, float* p_or) {
  if (!check_range(e, lane0, n) || !p_or || row0 < 0 || n_rows < 0 || row0 + n_rows > e->ptdf_rows_valid)
    return fail(GPF_E_INVALID, "gpf_get_ptdf_flows_rows: bad range (only the rows of the last gpf_ptdf_flows_rows are retrievable)");
  HIP_TRY(hipSetDevice(e->device));
  for (int r = 0; r < n_rows; ++r)
    HIP_TRY(hipMemcpy2DAsync(p_or + (size_t)r * n * e->g.n_line, (size_t)e->g.n_line * sizeof(float),
                             e->ptdf_flow_rows.p + ((size_t)(row0 + r) * e->cap_lanes + lane0) * e->ptdf_line_pad,
                             (size_t)e->ptdf_line_pad * sizeof(float), (size_t)e->g.n_line * sizeof(float), (size_t)n, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_ptdf_flows(gpf_handle e, int32_t lane0, int32_t n, float* p_or) {
  if (!check_range(e, lane0, n) || !p_or) return fail(GPF_E_INVALID, "gpf_get_ptdf_flows: bad arguments");
  if (!e->ptdf_ready) return fail(GPF_E_INVALID, "gpf_get_ptdf_flows: call gpf_ptdf_build first");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy2DAsync(p_or, (size_t)e->g.n_line * sizeof(float), e->ptdf_flow.p + (size_t)lane0 * e->ptdf_line_pad,
                           (size_t)e->ptdf_line_pad * sizeof(float), (size_t)e->g.n_line * sizeof(float), (size_t)n,
                           hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_lodf_screen(gpf_handle e, int32_t lane0, int32_t n, const float* cap_mw, float* worst) {
  if (!check_range(e, lane0, n) || !worst) return fail(GPF_E_INVALID, "gpf_lodf_screen: bad arguments");
  if (!e->ptdf_ready) return fail(GPF_E_INVALID, "gpf_lodf_screen: call gpf_ptdf_build and gpf_ptdf_flows first");
  if (n == 0) return GPF_OK;
  if (e->ptdf_batch && (lane0 != e->ptdfb_lane0 || n != e->ptdfb_n || !e->ptdfb_lodf.p))
    return fail(GPF_E_INVALID, "gpf_lodf_screen: per-lane topologies: build them with LODF tables and screen exactly the lane range that was built");
  HIP_TRY(hipSetDevice(e->device));
  const int nl = e->g.n_line, lp = e->ptdf_line_pad;
  const float* ic = nullptr;
  if (cap_mw) {
    std::vector<float> inv(nl);
    for (int l = 0; l < nl; ++l) inv[l] = cap_mw[l] > 0.f ? 1.0f / cap_mw[l] : 0.f;
    if (!e->lodf_inv_cap.p) HIP_TRY(e->lodf_inv_cap.alloc(nl));
    HIP_TRY(hipMemcpyAsync(e->lodf_inv_cap.p, inv.data(), (size_t)nl * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    ic = e->lodf_inv_cap.p;
  }
  const size_t lds = ((size_t)5 * gpf::LODF_LPW + 1) * lp * sizeof(float);
  if (e->ptdf_batch)
    hipLaunchKernelGGL(gpf::lodf_screen_kernel, dim3(e->ptdfb_slots / gpf::LODF_LPW), dim3(256), lds, e->stream, nl, lp, e->ptdfb_lodf.p, ic, e->ptdf_flow.p,
                       lane0, n, e->lodf_worst.p, e->ptdfb_order.p, e->ptdfb_blk_class.p, (long long)nl * lp, e->ptdfb_status.p);
  else
    hipLaunchKernelGGL(gpf::lodf_screen_kernel, dim3((n + gpf::LODF_LPW - 1) / gpf::LODF_LPW), dim3(256), lds, e->stream, nl, lp, e->lodf.p, ic,
                       e->ptdf_flow.p, lane0, n, e->lodf_worst.p, nullptr, nullptr, 0LL, nullptr);
  HIP_TRY(hipGetLastError());
  if (e->window) { ++e->win_launches; e->win_marked = false; }
  HIP_TRY(hipMemcpy2DAsync(worst, (size_t)nl * sizeof(float), e->lodf_worst.p + (size_t)lane0 * lp, (size_t)lp * sizeof(float),
                           (size_t)nl * sizeof(float), (size_t)n, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

}  // extern "C"
