// gridpf_capi.hip -- host side of libgridpf.so: the C ABI declared in include/gridpf.h on the engine of gridpf_engine.hpp: creation, the
// lanes' lifecycle, launch planning and the launches of the kernels of gridpf_sparse.hpp and gridpf_redispatch.hpp.  The DC sensitivity
// part and every feature of the acting step have units of their own (gridpf_capi_<feature>.hip), called here through the hooks declared
// in gridpf_engine.hpp.  gfx950 only; no fallback path: if HIP is unavailable every entry point fails with GPF_E_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <climits>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "gridpf_engine.hpp"
#include "gridpf_lookahead.hpp"             // (la_maintenance_ahead; its kernels exist in gridpf_capi_lookahead.hip only)
#include "gridpf_redispatch.hpp"
#include "gridpf_topo.hpp"

namespace gpf {
// device-side lane utilities ------------------------------------------------------------------------------------------
__global__ void fanout_kernel(GridDev g, Bufs b, int src, int dst0, int n_dst, const int* __restrict__ out_lines) {
  const int k = blockIdx.x;
  if (k >= n_dst) return;
  const int dst = dst0 + k;
  const int tid = threadIdx.x;
  const double* sinj = b.inj + (size_t)src * g.n_inj;
  double* dinj = b.inj + (size_t)dst * g.n_inj;
  for (int i = tid; i < g.n_inj; i += blockDim.x) dinj[i] = sinj[i];
  const int* st = b.topo + (size_t)src * g.dim_topo;
  int* dt = b.topo + (size_t)dst * g.dim_topo;
  const int ol = out_lines ? out_lines[k] : -1;
  const int po = (ol >= 0 && ol < g.n_line) ? g.line_or_pos[ol] : -1;
  const int pe = (ol >= 0 && ol < g.n_line) ? g.line_ex_pos[ol] : -1;
  int* d0 = const_cast<int*>(b.topo0) + (size_t)dst * g.dim_topo;
  for (int i = tid; i < g.dim_topo; i += blockDim.x) { const int v = (i == po || i == pe) ? -1 : st[i]; dt[i] = v; d0[i] = v; }
  const int* ss = b.shunt_bus + (size_t)src * g.n_shunt;
  int* ds = b.shunt_bus + (size_t)dst * g.n_shunt;
  for (int i = tid; i < g.n_shunt; i += blockDim.x) ds[i] = ss[i];
  // the contingency lane is the source's environment with one line out: its protection counters and line cooldowns are the source's
  // (as gpf_copy_lanes and simulate_prepare_kernel copy them; a step that tracks cooldowns would otherwise start from stale ones)
  if (b.overflow_count) for (int i = tid; i < g.n_line; i += blockDim.x) b.overflow_count[(size_t)dst * g.n_line + i] = b.overflow_count[(size_t)src * g.n_line + i];
  if (b.cooldown) for (int i = tid; i < g.n_line; i += blockDim.x) b.cooldown[(size_t)dst * g.n_line + i] = b.cooldown[(size_t)src * g.n_line + i];
}

// gpf_solve_lane: the lane's inputs straight from the pinned host block (device-mapped: one PCIe read per element, all in flight
// together) into the lane's rows, and its result rows straight back into it -- two dispatches instead of eleven staged copies
// (5.6 us each on the stream: 60 of the 73 us a one-lane runpf took).  Offsets in bytes, 16-byte aligned pieces.
struct LaneBlob { size_t o_inj, o_topo, o_sb, o_out, o_tv, o_sbo, o_ls, o_st, o_vm, o_va; };
__global__ void lane_scatter_kernel(GridDev g, Bufs b, int lane, const unsigned char* __restrict__ blob, LaneBlob o) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* inj = reinterpret_cast<const double*>(blob + o.o_inj);
  const int* topo = reinterpret_cast<const int*>(blob + o.o_topo);
  const int* sb = reinterpret_cast<const int*>(blob + o.o_sb);
  double* dinj = b.inj + (size_t)lane * g.n_inj;
  int* dt = b.topo + (size_t)lane * g.dim_topo;
  int* d0 = const_cast<int*>(b.topo0) + (size_t)lane * g.dim_topo;
  int* ds = b.shunt_bus + (size_t)lane * g.n_shunt;
  for (int i = tid; i < g.n_inj; i += nt) dinj[i] = inj[i];
  for (int i = tid; i < g.dim_topo; i += nt) { const int v = topo[i]; dt[i] = v; d0[i] = v; }
  for (int i = tid; i < g.n_shunt; i += nt) ds[i] = sb[i];
}
__global__ void lane_gather_kernel(GridDev g, Bufs b, int lane, unsigned char* __restrict__ blob, LaneBlob o) {
  const int tid = threadIdx.x, nt = blockDim.x;
  float* out = reinterpret_cast<float*>(blob + o.o_out);
  int* tv = reinterpret_cast<int*>(blob + o.o_tv);
  int* sbo = reinterpret_cast<int*>(blob + o.o_sbo);
  unsigned char* ls = blob + o.o_ls;
  int* st = reinterpret_cast<int*>(blob + o.o_st);
  double* vm = reinterpret_cast<double*>(blob + o.o_vm);
  double* va = reinterpret_cast<double*>(blob + o.o_va);
  for (int i = tid; i < g.n_out; i += nt) out[i] = b.out[(size_t)lane * g.n_out + i];
  for (int i = tid; i < g.dim_topo; i += nt) tv[i] = b.topo_out[(size_t)lane * g.dim_topo + i];
  for (int i = tid; i < g.n_shunt; i += nt) sbo[i] = b.shunt_bus_out[(size_t)lane * g.n_shunt + i];
  for (int i = tid; i < g.n_line; i += nt) ls[i] = b.line_status[(size_t)lane * g.n_line + i];
  if (tid < 4) st[tid] = b.status[(size_t)lane * 4 + tid];
  for (int i = tid; i < g.nb_tot; i += nt) { vm[i] = b.bus_vm[(size_t)lane * g.nb_tot + i]; va[i] = b.bus_va[(size_t)lane * g.nb_tot + i]; }
  __threadfence_system();
}

// gpf_simulate_batch: topology / shunt rows of the source lanes -> one dense staging buffer (a single device-to-host copy)
__global__ void gather_topo_kernel(GridDev g, Bufs b, const int* __restrict__ src_lanes, int n_src, int* __restrict__ dst) {
  const int k = blockIdx.x;
  if (k >= n_src) return;
  const int src = src_lanes[k];
  const int w = g.dim_topo + g.n_shunt;
  for (int i = threadIdx.x; i < g.dim_topo; i += blockDim.x) dst[(size_t)k * w + i] = b.topo[(size_t)src * g.dim_topo + i];
  for (int i = threadIdx.x; i < g.n_shunt; i += blockDim.x) dst[(size_t)k * w + g.dim_topo + i] = b.shunt_bus[(size_t)src * g.n_shunt + i];
}

// gpf_simulate_batch: destination lane d = dst0 + b * n_act + k takes over everything of source lane b that is not topology
// (injection row, protection counters, chronics table / jitter / redispatch delta) and gets the chronics-table row to step on:
// the source's current row idx = (t_obs + offset) mod T for time_step 0, else forecast row n_h * idx + time_step - 1.
__global__ void simulate_prepare_kernel(GridDev g, Bufs b, const int* __restrict__ src_lanes, int n_act, int n_dst, int dst0, int t_obs,
                                        int T, int n_h, int time_step, int* __restrict__ lane_table, int* __restrict__ lane_offset,
                                        float* __restrict__ lane_scale, float* __restrict__ lane_gen_delta) {
  const int q = blockIdx.x;
  if (q >= n_dst) return;
  const int src = src_lanes[q / n_act], dst = dst0 + q, tid = threadIdx.x;
  for (int i = tid; i < g.n_inj; i += blockDim.x) b.inj[(size_t)dst * g.n_inj + i] = b.inj[(size_t)src * g.n_inj + i];
  for (int i = tid; i < g.n_line; i += blockDim.x) b.overflow_count[(size_t)dst * g.n_line + i] = b.overflow_count[(size_t)src * g.n_line + i];
  for (int i = tid; i < g.n_line; i += blockDim.x) b.cooldown[(size_t)dst * g.n_line + i] = b.cooldown[(size_t)src * g.n_line + i];
  if (lane_scale) for (int i = tid; i < 2 * g.n_load; i += blockDim.x) lane_scale[(size_t)dst * 2 * g.n_load + i] = lane_scale[(size_t)src * 2 * g.n_load + i];
  if (lane_gen_delta) for (int i = tid; i < g.n_gen; i += blockDim.x) lane_gen_delta[(size_t)dst * g.n_gen + i] = lane_gen_delta[(size_t)src * g.n_gen + i];
  if (tid == 0) {
    lane_table[dst] = lane_table[src];
    int idx = (t_obs + lane_offset[src]) % T;
    if (idx < 0) idx += T;
    lane_offset[dst] = time_step == 0 ? idx : n_h * idx + (time_step - 1);
    b.done[dst] = 0;
  }
}

}  // namespace gpf

// the lanes' rows were sent by the host (their reset topology is their topology again)
void topo_unmoved(gpf_engine* e, int lane0, int n) {
  if (e->ta_n_moved == 0) return;
  for (int k = lane0; k < lane0 + n; ++k) if (e->ta_moved[k]) { e->ta_moved[k] = 0; --e->ta_n_moved; }
}

namespace {

// number of active buses and Newton unknowns of one lane (host mirror of K1's counting)
void count_lane(const gpf_engine* e, const int* topo, const int* shunt_bus, int& nb, int& nj, int& mb) {
  const gpf::GridDev& g = e->g;
  std::vector<unsigned char> act(g.nb_tot, 0), type(g.nb_tot, 0);
  auto mark = [&](int sub, int local) -> int {
    if (local < 1 || local > g.n_busbar) return -1;
    int gb = sub + (local - 1) * g.n_sub;
    act[gb] = 1;
    return gb;
  };
  for (int l = 0; l < g.n_line; ++l) {
    int bo = topo[e->h_line_or_pos[l]], be = topo[e->h_line_ex_pos[l]];
    if (bo >= 1 && be >= 1) { mark(e->h_line_or_sub[l], bo); mark(e->h_line_ex_sub[l], be); }
  }
  for (int i = 0; i < g.n_gen; ++i) {
    int gb = mark(e->h_gen_sub[i], topo[e->h_gen_pos[i]]);
    if (gb >= 0) type[gb] = std::max<unsigned char>(type[gb], e->h_gen_slack[i] ? 2 : 1);
  }
  for (int i = 0; i < g.n_load; ++i) mark(e->h_load_sub[i], topo[e->h_load_pos[i]]);
  for (int i = 0; i < g.n_sto; ++i) mark(e->h_sto_sub[i], topo[e->h_sto_pos[i]]);
  if (shunt_bus)
    for (int i = 0; i < g.n_shunt; ++i) mark(e->h_shunt_sub[i], shunt_bus[i]);
  nb = 0;
  nj = 0;
  for (int b = 0; b < g.nb_tot; ++b) {
    if (!act[b]) continue;
    ++nb;
    if (type[b] == 0) nj += 2;
    else if (type[b] == 1) nj += 1;
  }
  mb = 1;
  for (int s = 0; s < g.n_sub; ++s) {
    int c = 0;
    for (int k = 0; k < g.n_busbar; ++k) c += act[s + k * g.n_sub];
    mb = std::max(mb, c);
  }
}



// flat programs (gridpf_symbolic.hpp: FlatProg) of one graph for the four group widths, in one device buffer; false: upload
// failed.  A graph too large for the 16-bit byte-offset fields gets none (fl[k].n_words == 0: it would not fit the LDS either).
bool upload_flats(const gpf::Symbolic& S, DevArr<int>& buf, gpf::SymDev& D, int lane_opt = 0) {
  D.rslot0 = S.rslot0;
  for (int k = 0; k < 4; ++k) { D.flat[k] = nullptr; D.fl[k] = gpf::FlatDev{}; }
  if (!gpf::flat_fits(S)) return true;
  std::vector<int> all;
  size_t off[4];
  for (int k = 0; k < 4; ++k) {
    // (the lane assignment is a pure function of the graph: engines of the same grid -- every HipBackend copy pool, every test --
    //  share one build per process)
    static std::mutex cache_mu;                                // engines are created from several host threads (one per device)
    static std::unordered_map<std::string, gpf::FlatProg> cache;
    std::string key;
    if (lane_opt > 0) {
      key = std::to_string(S.slot_row.size()) + ":" + std::to_string(S.slot_col.size()) + ":" + std::to_string(S.prog.size()) + ":";
      key.append(reinterpret_cast<const char*>(S.slot_row.data()), S.slot_row.size() * sizeof(int));
      key.append(reinterpret_cast<const char*>(S.slot_col.data()), S.slot_col.size() * sizeof(int));
      key.append(reinterpret_cast<const char*>(S.prog.data()), S.prog.size() * sizeof(int));
      key += "/" + std::to_string(16 << k) + "/" + std::to_string(lane_opt) + "/" + std::to_string(S.gj_lv0) + "/" + std::to_string(S.nslot_lu);
    }
    gpf::FlatProg F;
    bool have = false;
    if (lane_opt > 0) {
      std::lock_guard<std::mutex> lk(cache_mu);
      auto hit = cache.find(key);
      if (hit != cache.end()) { F = hit->second; have = true; }
    }
    if (!have) {
      F = gpf::build_flat(S, 16 << k, lane_opt);               // (the search runs outside the lock: a second thread may repeat it)
      if (lane_opt > 0) {
        std::lock_guard<std::mutex> lk(cache_mu);
        if (cache.size() < 64) cache.emplace(key, F);
      }
    }
    off[k] = all.size();
    all.insert(all.end(), F.words.begin(), F.words.end());
    gpf::FlatDev& f = D.fl[k];
    f.n_fwd = F.n_fwd; f.n_scale = F.n_scale; f.n_scale_rhs = F.n_scale_rhs; f.n_back = F.n_back; f.scale_off = F.scale_off;
    f.back_off = F.back_off; f.rhs_field0 = F.rhs_field0; f.n_words = (int)F.words.size(); f.wave_closed = F.wave_closed ? 1 : 0;
    f.solo_fwd = (int)F.solo_fwd; f.solo_back = (int)F.solo_back;
  }
  if (buf.upload(all.data(), all.size()) != hipSuccess) return false;
  for (int k = 0; k < 4; ++k) D.flat[k] = buf.p + off[k];
  if (g_dry_create) {                           // header-only handle: no device copy; "has flat programs" is what the planner asks (never dereferenced on the host)
    static int dry_words;
    for (int k = 0; k < 4; ++k) D.flat[k] = &dry_words;
  }
  return true;
}

gpf::Symbolic build_symbolic_resident(const gpf::GridDev& g, int n_rows, int n_line, const int* lo, const int* le, bool yb_in_lds);

// Topology class of a lane whose substations are split (gridpf_sparse.hpp: TopoClassDev).  Key = busbar of every line end
// (an open end counts as busbar 1) + which busbars >= 2 carry any element; classes are built on first sight and cached.
// Returns the class id, or -1 (classes disabled / capacity) -> the lane falls back to the NB = n_busbar kernel.
int topo_class_of(gpf_engine* e, const int* topo, const int* shunt_bus) {
  const gpf::GridDev& g = e->g;
  if (e->no_classes || g.n_busbar < 2 || e->classes.size() >= 8192) return -1;
  const int nbb = g.n_busbar;
  std::string key((size_t)2 * g.n_line + (size_t)g.n_sub * nbb, '\0');
  auto bb = [&](int v) { return v >= 2 && v <= nbb ? v : 1; };
  for (int l = 0; l < g.n_line; ++l) {
    key[2 * l] = (char)bb(topo[e->h_line_or_pos[l]]);
    key[2 * l + 1] = (char)bb(topo[e->h_line_ex_pos[l]]);
  }
  char* used = &key[(size_t)2 * g.n_line];                  // [sub][busbar-1]: the busbar carries an element
  auto mark = [&](int sub, int v) { if (v >= 1 && v <= nbb) used[(size_t)sub * nbb + (v - 1)] = 1; };
  for (int l = 0; l < g.n_line; ++l) { mark(e->h_line_or_sub[l], key[2 * l]); mark(e->h_line_ex_sub[l], key[2 * l + 1]); }
  for (int i = 0; i < g.n_gen; ++i) mark(e->h_gen_sub[i], topo[e->h_gen_pos[i]]);
  for (int i = 0; i < g.n_load; ++i) mark(e->h_load_sub[i], topo[e->h_load_pos[i]]);
  for (int i = 0; i < g.n_sto; ++i) mark(e->h_sto_sub[i], topo[e->h_sto_pos[i]]);
  if (shunt_bus) for (int i = 0; i < g.n_shunt; ++i) mark(e->h_shunt_sub[i], shunt_bus[i]);
  std::string elem(used, (size_t)g.n_sub * nbb);                        // busbars that really carry an element
  for (int s_ = 0; s_ < g.n_sub; ++s_) used[(size_t)s_ * nbb] = 1;      // the busbar-1 node always exists
  auto it = e->class_of_key.find(key);
  if (it != e->class_of_key.end()) return it->second;
  // nodes: (sub, busbar 1) -> sub; used busbars >= 2 -> n_sub, n_sub + 1, ...
  std::vector<int> node_of((size_t)g.n_sub * nbb, -1);
  int n_nodes = g.n_sub;
  for (int s_ = 0; s_ < g.n_sub; ++s_) node_of[(size_t)s_ * nbb] = s_;
  for (int s_ = 0; s_ < g.n_sub; ++s_)
    for (int k = 1; k < nbb; ++k) if (used[(size_t)s_ * nbb + k]) node_of[(size_t)s_ * nbb + k] = n_nodes++;
  if (n_nodes > 32767) return -1;
  std::vector<int> lo(g.n_line), le(g.n_line);
  for (int l = 0; l < g.n_line; ++l) {
    lo[l] = node_of[(size_t)e->h_line_or_sub[l] * nbb + (key[2 * l] - 1)];
    le[l] = node_of[(size_t)e->h_line_ex_sub[l] * nbb + (key[2 * l + 1] - 1)];
  }
  gpf::Symbolic S = build_symbolic_resident(g, n_nodes, g.n_line, lo.data(), le.data(), true);
  if (S.nslot > 65535 || !gpf::flat_fits(S)) return -1;
  auto c = std::make_unique<gpf_engine::TopoClassHost>();
  std::vector<int> fi;
  auto puti = [&fi](const int* v, size_t n) { int off = (int)fi.size(); fi.insert(fi.end(), v, v + n); while (fi.size() & 3) fi.push_back(0); return off; };
  const int o_prog = puti(S.prog.data(), S.prog.size());
  std::vector<int> rc(S.nslot_y);
  for (int k = 0; k < S.nslot_y; ++k) rc[k] = S.slot_row[k] | (S.slot_col[k] << 16);
  const int o_rc = puti(rc.data(), rc.size());
  const std::vector<int> upv = gpf::build_upairs(S);
  const int o_up = puti(upv.data(), upv.size());
  const int o_br = puti(S.br_slot.data(), S.br_slot.size());
  const int o_no = puti(node_of.data(), node_of.size());
  if (c->tables.upload(fi.data(), fi.size()) != hipSuccess) return -1;
  c->n_nodes = n_nodes; c->nslot = S.nslot; c->nslot_y = S.nslot_y;
  gpf::SymDev& D = c->dev.sym;
  D = e->sym_dev;                                            // the grid's static blob pointers / offsets
  D.n = S.n; D.nslot = S.nslot; D.nslot_lu = S.nslot_lu; D.nslot_y = S.nslot_y; D.n_levels = S.n_levels; D.back_off = S.back_off; D.back_first = S.back_first;
  D.scale_off = S.scale_off; D.n_scale = S.n_scale; D.n_prog = (int)S.prog.size();
  {   // with every line in service the bus graph of a lane of this class is exactly this graph: connected <=> one component
      // over the nodes that carry an element (an element-only node without a line is an island)
    std::vector<int> comp(n_nodes);
    for (int i = 0; i < n_nodes; ++i) comp[i] = i;
    auto find = [&](int x) { while (comp[x] != x) { comp[x] = comp[comp[x]]; x = comp[x]; } return x; };
    for (int l = 0; l < g.n_line; ++l) comp[find(lo[l])] = find(le[l]);
    int root = -1;
    bool one = true;
    for (int s_ = 0; s_ < g.n_sub && one; ++s_)
      for (int k = 0; k < nbb && one; ++k)
        if (elem[(size_t)s_ * nbb + k]) {
          const int r = find(node_of[(size_t)s_ * nbb + k]);
          if (root < 0) root = r; else one = (r == root);
        }
    D.static_connected = one ? 1 : 0;
  }
  D.prog = c->tables.p + o_prog;
  if (!upload_flats(S, c->flat, D) || !D.fl[3].wave_closed) return -1;
  c->dev.pair_rc = c->tables.p + o_rc; c->dev.up = c->tables.p + o_up; c->dev.br_slot = c->tables.p + o_br; c->dev.node_of = c->tables.p + o_no;
  D.n_up = (int)upv.size() / 2;
  const int id = (int)e->classes.size();
  e->classes.push_back(std::move(c));
  e->class_of_key.emplace(std::move(key), id);
  return id;
}


// Symbolic analysis whose Gauss-Jordan tail (Symbolic::gj_lv0) does not cost a resident workgroup per CU.  The 2-wavefront kernels
// of the large grids live on 4 workgroups of ~39 KB per CU: the tail's fill blocks (40 bytes each with the kept DC factors) are
// taken only as far as the count of workgroups that fit stays the same (measured on 118 substations: 52 extra blocks = 3 instead of
// 4 workgroups per CU = -37 %; the allocation is granular and a 40 704-byte workgroup no longer fits four times).  Small grids
// (instance groups / one wavefront, a few hundred bytes of fill) keep the default budget.
size_t gj_workgroups_per_cu(size_t lds_bytes) { return (160 * 1024) / std::max<size_t>((lds_bytes + 512 + 1023) / 1024 * 1024, 1024); }
gpf::Symbolic build_symbolic_resident(const gpf::GridDev& g, int n_rows, int n_line, const int* lo, const int* le, bool yb_in_lds) {
  if (const char* ev = std::getenv("GRIDPF_GJ_BUDGET")) return gpf::build_symbolic(n_rows, n_line, lo, le, 1, std::atoi(ev));   // developer override
  gpf::Symbolic S = gpf::build_symbolic(n_rows, n_line, lo, le);
  if (n_rows < 64) return S;
  auto lds = [&](int nslot) { return gpf::lds_bytes_sparse<1>(g, nslot, yb_in_lds ? S.nslot_y : 0, 0, false, 1, n_rows, true); };
  while (S.nslot > S.nslot_lu && gj_workgroups_per_cu(lds(S.nslot)) < gj_workgroups_per_cu(lds(S.nslot_lu)))
    S = gpf::build_symbolic(n_rows, n_line, lo, le, 1, S.nslot - S.nslot_lu - 1);
  return S;
}

int plan_launch_uncached(gpf_engine* e, int lane0, int n, LaunchPlan& p, LaunchPlan& pb, bool list_tail = false);

// p: the plan of the range (or of its single-busbar lanes when the batch is mixed); pb.sparse_nb != 0: second launch for
// the lanes that have a split substation (both then run from device lane lists)
int plan_launch(gpf_engine* e, int lane0, int n, LaunchPlan& p, LaunchPlan& pb) {
  const bool whole = (lane0 == 0 && n == e->n_lanes);
  if (whole && e->plan_valid) { p = e->plan_cached; pb = e->plan_b_cached; return GPF_OK; }
  // whatever invalidated the batch's plan invalidated the fan's two (fan_plans makes them, calls this last and only then marks them valid)
  if (whole) e->fan.plans_valid = false;
  int rc = plan_launch_uncached(e, lane0, n, p, pb);
  if (!whole && (p.n_list || pb.n_list)) e->plan_valid = false;     // the device lane lists were overwritten
  if (rc == GPF_OK && whole) { e->plan_cached = p; e->plan_b_cached = pb; e->plan_valid = true; }
  return rc;
}

// list_tail: a range of unsplit lanes that does not end on an instance group runs from a lane list padded with ghost lanes, on the
// groups the whole batch runs on (a contiguous range would fall back to narrower groups: other bits and a slower kernel on small grids)
int plan_launch_uncached(gpf_engine* e, int lane0, int n, LaunchPlan& p, LaunchPlan& pb, bool list_tail) {
  pb = LaunchPlan{};
  p = LaunchPlan{};
  p.ipw = 1;
  p.wpi = 1;
  p.minw = 2;
  int mb = 1;
  for (int k = lane0; k < lane0 + n; ++k) mb = std::max(mb, e->lane_mb[k]);
  // kernel S plan of n lanes that all run with NBK busbars per substation block; listed: the lanes come from an index list
  auto plan_sparse = [&](int nbk, int n_l, int lane0_l, bool listed, LaunchPlan& q) -> bool {
    // small grids do not have 64-wide work: several instances share a wavefront (instance groups, gridpf_sparse.hpp).
    // Contiguous sub-ranges must be group-aligned (or end at the padded tail of the lane buffers); lists are padded.
    int ipw = 1;
    if (nbk == 1) {
      ipw = e->ipw_override ? e->ipw_override : (e->g.n_sub <= 8 ? 4 : e->g.n_sub <= 24 ? 2 : 1);
      while (!listed && ipw > 1 && !(lane0_l % ipw == 0 && (n_l % ipw == 0 || lane0_l + n_l == e->n_lanes))) ipw >>= 1;
    }
    auto need = [&](int tier) -> size_t {
      const int wpi_n = (nbk == 1 && ipw == 1) ? (e->wpi_override ? std::min(e->wpi_override, 2) : (e->g.n_sub >= 64 && e->sym_dev.fl[3].wave_closed ? 2 : 1)) : 1;
      // (instance-group kernels stream the flat program from global memory: gridpf_sparse.hpp lu_ac)
      const size_t static_bytes = gpf::stat_bytes(e->sym_dev.so, tier, nbk == 1, ipw > 1 ? 0 : e->sym_dev.fl[gpf::gw_index(64 / ipw * wpi_n)].n_words);
      const bool st = tier > 0;
      const bool dcf = e->dcf != 0;
      return nbk == 1 ? gpf::lds_bytes_sparse<1>(e->g, e->sym.nslot, e->sym.nslot_y, static_bytes, st, ipw, -1, dcf)
           : nbk == 2 ? gpf::lds_bytes_sparse<2>(e->g, e->sym.nslot_lu, e->sym.nslot_y, static_bytes, st, 1, -1, dcf)
                      : gpf::lds_bytes_sparse<3>(e->g, e->sym.nslot_lu, e->sym.nslot_y, static_bytes, st, 1, -1, dcf);
    };
    // stage the static tables + the injection row in LDS only when that does not cost residency: blocks per CU
    // (160 KiB / footprint) must still cover what the launch needs at once, or what the un-staged kernel would get
    const size_t l_gl = need(0);
    const size_t n_blocks = ((size_t)n_l + ipw - 1) / ipw;
    const size_t want = std::min<size_t>(std::min<size_t>((n_blocks + 255) / 256, LDS_HARD_LIMIT / std::max<size_t>(l_gl, 1)), 8);
    int stage = 0;
    const int top_tier = std::min(nbk == 1 ? 2 : 1, e->stage_max);
    for (int tier = top_tier; tier >= 1 && !stage; --tier)
      if (need(tier) <= LDS_HARD_LIMIT && LDS_HARD_LIMIT / need(tier) >= want) stage = tier;
    if (e->stage_force >= 0 && e->stage_force <= top_tier && need(e->stage_force) <= LDS_HARD_LIMIT) stage = e->stage_force;
    if (ipw > 1 && stage != 2) { ipw = 1; stage = 0; for (int tier = top_tier; tier >= 1 && !stage; --tier) if (need(tier) <= LDS_HARD_LIMIT && LDS_HARD_LIMIT / need(tier) >= want) stage = tier; }
    if (e->env_on && ipw == 1) stage = 0;                       // the ENV step kernels exist for tier 0 (and tier 2 with instance groups)
    const size_t l = need(stage);
    if (l > LDS_HARD_LIMIT) return false;
    if (nbk == 1 && !e->sym_dev.flat[0]) return false;           // no flat program: graph beyond the 16-bit slot fields
    q.sparse_nb = nbk;
    q.ipw = ipw;
    q.minw = 2;
    // large grids: phases loop over hundreds of items -> several wavefronts per instance (block-wide barriers)
    // (2 wavefronts per instance need a flat program whose passes keep every destination inside one wavefront -- bitwise
    //  reproducibility; the NB = n_busbar kernels use the level-header program, which is not packed that way: one wavefront
    //  unless GRIDPF_WPI=2 asks for the faster, not bit-reproducible variant)
    q.wpi = (nbk == 1 && ipw == 1) ? (e->wpi_override ? std::min(e->wpi_override, 2) : (e->g.n_sub >= 64 && e->sym_dev.fl[3].wave_closed ? 2 : 1))
          : (nbk == 2 && e->wpi_override == 2) ? 2 : 1;
    if (q.wpi > 1) q.minw = 2;
    q.sparse_stage = stage;
    q.lds = l;
    q.dcf = e->dcf;
    q.yreg = false;
    // Ybus blocks in registers (2 wavefronts per instance, tables in global memory, at most 4 pairs per lane): when the LDS they
    // free holds the factored DC matrix without costing a block per CU, every step of a launch skips the DC assembly + factorisation
    if (nbk == 1 && !listed && ipw == 1 && q.wpi == 2 && stage == 0 && !e->no_yreg && e->dcf_env != 0 && (e->sym.nslot_y - e->g.n_sub) / 2 <= 4 * 128 && e->g.n_sub <= 128) {
      const size_t ly = gpf::lds_bytes_sparse<1>(e->g, e->sym.nslot, 0, 0, false, 1, -1, true);
      if (ly <= LDS_HARD_LIMIT && LDS_HARD_LIMIT / ly >= std::min<size_t>(LDS_HARD_LIMIT / l, want)) { q.yreg = true; q.dcf = 1; q.lds = ly; }
    }
    return true;
  };
  // more than 3 busbars per substation: only through topology classes (the NB = n_busbar block kernels exist for 1..3)
  const bool blocks_ok = e->g.n_busbar <= GPF_MAX_BUSBAR_BLOCKS;
  if (e->g.n_sub * mb <= 32000) {
#ifdef GPF_TIMING
    if (e->work.n < (size_t)e->cap_lanes * gpf::GPF_WORK_ROW) HIP_TRY(e->work.alloc((size_t)e->cap_lanes * gpf::GPF_WORK_ROW));
#endif
    // lanes with split substations: (1) topology classes -- the single-busbar kernel on the lane's bus-level graph --, else
    // (2) the NB = n_busbar kernel; the lanes without a split keep the plain single-busbar kernel (mixed batch: two launches)
    if (mb > 1 && !e->no_partition) {
      std::vector<int> la, lb, lc;
      bool all_classed = true;
      // ONE topology-class launch serves the whole mixed batch when every lane has a class (the lanes without a split run
      // their own class at the same speed); on small grids the lanes are packed by class into instance groups
      bool everyone = true;
      for (int k = lane0; k < lane0 + n && everyone; ++k) everyone = e->lane_class[k] >= 0;
      const int tc_ipw = e->ipw_override ? e->ipw_override : (e->g.n_sub <= 8 ? 4 : e->g.n_sub <= 24 ? 2 : 1);
      if (everyone) {
        std::vector<int> order(n);
        for (int k = 0; k < n; ++k) order[k] = lane0 + k;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return e->lane_class[a] < e->lane_class[b]; });
        for (size_t i = 0; i < order.size();) {
          const int cid = e->lane_class[order[i]];
          size_t j = i;
          while (j < order.size() && e->lane_class[order[j]] == cid) { lb.push_back(order[j]); lc.push_back(cid); ++j; }
          while (lb.size() % tc_ipw) { lb.push_back(e->n_lanes); lc.push_back(cid); }      // ghost lanes complete the group
          i = j;
        }
      } else
      for (int k = lane0; k < lane0 + n; ++k) {
        if (e->lane_mb[k] == 1) la.push_back(k);
        else { lb.push_back(k); lc.push_back(e->lane_class[k]); all_classed &= (e->lane_class[k] >= 0); }
      }
      LaunchPlan qa = p, qb = p;
      bool ok_b;
      if (all_classed) {
        qb.tc = true; qb.sparse_nb = 1; qb.ipw = everyone ? tc_ipw : 1; qb.sparse_stage = 0; qb.minw = 2;
        qb.wpi = qb.ipw > 1 ? 1 : (e->wpi_override ? (e->wpi_override >= 2 ? 2 : 1) : (e->g.n_sub >= 64 ? 2 : 1));
        for (int cid : lc) {
          const auto& c = e->classes[cid];
          qb.tc_rows = std::max(qb.tc_rows, c->n_nodes); qb.tc_nslot = std::max(qb.tc_nslot, c->nslot); qb.tc_nslot_y = std::max(qb.tc_nslot_y, c->nslot_y);
        }
        // DC factors kept across the steps of a launch: alone (every lane has a class: ONE launch, its own parameter block) when
        // that does not cost residency; next to a launch of unsplit lanes the shared parameter block carries that plan's setting
        auto lds_tc = [&](bool dcf_) { return gpf::lds_bytes_sparse<1>(e->g, qb.tc_nslot, qb.tc_nslot_y, 0, false, qb.ipw, qb.tc_rows, dcf_); };
        qb.dcf = everyone ? 0 : e->dcf;
        qb.lds = lds_tc(qb.dcf != 0);
        if (everyone && e->dcf_env != 0) {
          const size_t nblk = (lb.size() + qb.ipw - 1) / qb.ipw, with = lds_tc(true);
          const size_t want_tc = std::min<size_t>(std::min<size_t>((nblk + 255) / 256, LDS_HARD_LIMIT / std::max<size_t>(qb.lds, 1)), 8);
          if (with <= LDS_HARD_LIMIT && LDS_HARD_LIMIT / with >= want_tc) { qb.dcf = 1; qb.lds = with; }
        }
        ok_b = qb.lds <= LDS_HARD_LIMIT;
        if (ok_b && e->d_classes_count != e->classes.size()) {
          std::vector<gpf::TopoClassDev> hc(e->classes.size());
          for (size_t i = 0; i < hc.size(); ++i) hc[i] = e->classes[i]->dev;
          HIP_TRY(e->d_classes.upload(hc.data(), hc.size()));
          e->d_classes_count = hc.size();
        }
      } else {
        ok_b = blocks_ok && plan_sparse(e->g.n_busbar, (int)lb.size(), 0, true, qb);
      }
      const bool ok_a = la.empty() || plan_sparse(1, (int)la.size(), 0, true, qa);
      if (ok_a && ok_b) {
        qa.n_list = (int)la.size(); qb.n_list = (int)lb.size();
        while (la.size() % 4) la.push_back(e->n_lanes);             // ghost lane (pristine state, never read back)
        while (lb.size() % 4) { lb.push_back(e->n_lanes); lc.push_back(lc.empty() ? 0 : lc.back()); }
        auto fit = [&](DevArr<int>& d, size_t need_n) -> hipError_t {
          if (d.n >= need_n) return hipSuccess;
          return d.alloc(std::max<size_t>(need_n, (size_t)e->cap_lanes + 8) * 2);
        };
        HIP_TRY(fit(e->list_a, la.size() + 4)); HIP_TRY(fit(e->list_b, lb.size() + 4)); HIP_TRY(fit(e->list_c, lc.size() + 4));
        if (!la.empty()) HIP_TRY(hipMemcpyAsync(e->list_a.p, la.data(), la.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->list_b.p, lb.data(), lb.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->list_c.p, lc.data(), lc.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));                    // the host vectors go out of scope
        qa.list = e->list_a.p; qb.list = e->list_b.p; qb.cls_list = e->list_c.p;
        if (qa.n_list == 0) { p = qb; }                              // every lane is split: one launch
        else { p = qa; pb = qb; }
        return GPF_OK;
      }
    }
    if (list_tail && mb == 1) {
      const int full = e->ipw_override ? e->ipw_override : (e->g.n_sub <= 8 ? 4 : e->g.n_sub <= 24 ? 2 : 1);
      LaunchPlan q = p;
      if (full > 1 && (lane0 % full || (n % full && lane0 + n != e->n_lanes)) && plan_sparse(1, n, 0, true, q) && q.ipw == full) {
        std::vector<int> la(n);
        for (int k = 0; k < n; ++k) la[k] = lane0 + k;
        while (la.size() % 4) la.push_back(e->n_lanes);               // ghost lane (pristine state, never read back)
        if (e->list_a.n < la.size() + 4) HIP_TRY(e->list_a.alloc(std::max<size_t>(la.size() + 4, (size_t)e->cap_lanes + 8) * 2));
        HIP_TRY(hipMemcpyAsync(e->list_a.p, la.data(), la.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));                     // the host vector goes out of scope
        q.n_list = n; q.list = e->list_a.p;
        p = q;
        return GPF_OK;
      }
    }
    if ((mb == 1 || blocks_ok) && plan_sparse(mb == 1 ? 1 : e->g.n_busbar, n, lane0, false, p)) return GPF_OK;
    if (mb > 1 && !blocks_ok)
      return fail(GPF_E_CAPACITY, "a lane with a split substation has no topology class (GRIDPF_NO_CLASSES / GRIDPF_NO_PARTITION set, or the class "
                                  "could not be built) and the grid has more than 3 busbars per substation: the block kernels cover 1..3");
  }
  return fail(GPF_E_CAPACITY, "grid too large: per-instance LDS footprint of the block-sparse kernel exceeds 160 KiB");
}

int upload_params_s(gpf_engine* e, const gpf::Bufs& b, const LaunchPlan* tc, int dcf) {
  gpf::DevParamsS hp{};
  hp.g = e->g;
  hp.b = b;
  hp.oo = e->oo;
  hp.sym = e->sym_dev;
  hp.classes = e->d_classes.p;
  hp.tc_rows = tc ? tc->tc_rows : 0; hp.tc_nslot = tc ? tc->tc_nslot : 0; hp.tc_nslot_y = tc ? tc->tc_nslot_y : 0;
  hp.dcf = dcf;
  if (e->env_on) {
    gpf::EnvDyn& E = hp.env;
    E = env_dyn(e);                          // ... and the actions this launch carries
    E.act_redisp = e->env_act_r ? e->env_act_redisp.p : nullptr; E.act_storage = e->env_act_s ? e->env_act_storage : nullptr;
    E.act_curtail = e->env_act_c ? e->env_act_curtail.p : nullptr;
  }
  if (!e->d_params_s.p) HIP_TRY(e->d_params_s.alloc(1));
  if (!e->params_s_valid || std::memcmp(&hp, &e->h_params_s, sizeof(hp)) != 0) {
    e->h_params_s = hp;
    HIP_TRY(hipMemcpyAsync(e->d_params_s.p, &e->h_params_s, sizeof(hp), hipMemcpyHostToDevice, e->stream));
    e->params_s_valid = true;
  }
  return GPF_OK;
}

// the engine's specialised kernels for the launch that follows upload_params_s (nullptr: ahead-of-time kernels).  The literals of the
// specialised kernels ARE this engine's grid: any change of the grid-level part of the parameter block switches them off.
GpfJit* jit_for_launch(gpf_engine* e) {
  if (!e->jit.on) return nullptr;
  const gpf::DevParamsS& hp = e->h_params_s;
  if (std::memcmp(&hp.g, &e->jit_g, sizeof(hp.g)) || std::memcmp(&hp.oo, &e->jit_oo, sizeof(hp.oo)) || std::memcmp(&hp.sym, &e->jit_sym, sizeof(hp.sym))) {
    e->jit.on = false;
    e->jit.message = "the grid-level parameter block changed after gpf_jit_enable: specialised kernels switched off";
    fprintf(stderr, "[gridpf] jit: %s\n", e->jit.message.c_str());
    return nullptr;
  }
  return &e->jit;
}

int prof_begin(gpf_engine* e, hipEvent_t& a, hipEvent_t& b) {
  if (e->ev_used == e->ev_pool.size()) {
    std::pair<Event, Event> ev;
    HIP_TRY(ev.first.create());
    HIP_TRY(ev.second.create());
    e->ev_pool.push_back(std::move(ev));
  }
  a = e->ev_pool[e->ev_used].first;
  b = e->ev_pool[e->ev_used].second;
  ++e->ev_used;
  HIP_TRY(hipEventRecord(a, e->stream));
  return GPF_OK;
}

int drain_events(gpf_engine* e) {
  for (size_t i = 0; i < e->ev_used; ++i) {
    HIP_TRY(hipEventSynchronize(e->ev_pool[i].second));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev_pool[i].first, e->ev_pool[i].second));
    e->acc_ms += ms;
    e->acc_launches += 1;
  }
  e->ev_used = 0;
  return GPF_OK;
}

int reset_lanes_unchecked(gpf_engine* e, int lane0, int n) {
  HIP_TRY(hipSetDevice(e->device));
  const gpf::GridDev& g = e->g;
  // replicate the pristine rows (host staging keeps this a plain strided copy)
  std::vector<double> inj((size_t)n * g.n_inj);
  std::vector<int> topo((size_t)n * g.dim_topo), sb((size_t)n * g.n_shunt);
  for (int k = 0; k < n; ++k) {
    std::copy(e->h_init_inj.begin(), e->h_init_inj.end(), inj.begin() + (size_t)k * g.n_inj);
    std::copy(e->h_init_topo.begin(), e->h_init_topo.end(), topo.begin() + (size_t)k * g.dim_topo);
    if (g.n_shunt) std::copy(e->h_init_shunt_bus.begin(), e->h_init_shunt_bus.end(), sb.begin() + (size_t)k * g.n_shunt);
  }
  HIP_TRY(hipMemcpyAsync(e->inj.p + (size_t)lane0 * g.n_inj, inj.data(), inj.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->topo.p + (size_t)lane0 * g.dim_topo, topo.data(), topo.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->topo0.p + (size_t)lane0 * g.dim_topo, topo.data(), topo.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  if (g.n_shunt)
    HIP_TRY(hipMemcpyAsync(e->shunt_bus.p + (size_t)lane0 * g.n_shunt, sb.data(), sb.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemsetAsync(e->overflow_count.p + (size_t)lane0 * g.n_line, 0, (size_t)n * g.n_line * sizeof(int), e->stream));
  HIP_TRY(hipMemsetAsync(e->cooldown.p + (size_t)lane0 * g.n_line, 0, (size_t)n * g.n_line * sizeof(int), e->stream));
  HIP_TRY(hipMemsetAsync(e->done.p + lane0, 0, (size_t)n, e->stream));
  HIP_TRY(hipMemsetAsync(e->episode.p + (size_t)lane0 * 2, 0, (size_t)n * 2 * sizeof(int), e->stream));
  HIP_TRY(hipMemsetAsync(e->status.p + (size_t)lane0 * 4, 0xFF, (size_t)n * 4 * sizeof(int), e->stream));
  if (e->env_on) { int rc_e = env_reset_lanes(e, lane0, n); if (rc_e != GPF_OK) return rc_e; }
  if (e->ta_on) { int rc_t = topo_reset_lanes(e, lane0, n); if (rc_t != GPF_OK) return rc_t; }
  if (e->al_on) { int rc_a = alert_reset_lanes(e, lane0, n); if (rc_a != GPF_OK) return rc_a; }
  if (e->rw_on) { int rc_r = reward_reset_lanes(e, lane0, n); if (rc_r != GPF_OK) return rc_r; }
  if (e->ep_on) { int rc_p = episode_reset_lanes(e, lane0, n); if (rc_p != GPF_OK) return rc_p; }
  if (e->cb_on) { int rc_c = combined_reset_lanes(e, lane0, n); if (rc_c != GPF_OK) return rc_c; }
  topo_unmoved(e, lane0, n);
  HIP_TRY(hipStreamSynchronize(e->stream));
  const int init_class = topo_class_of(e, e->h_init_topo.data(), g.n_shunt ? e->h_init_shunt_bus.data() : nullptr);
  for (int k = lane0; k < lane0 + n; ++k) {
    e->lane_nb[k] = e->init_nb; e->lane_nj[k] = e->init_nj; e->lane_mb[k] = e->init_mb; e->lane_class[k] = init_class;
    std::copy(e->h_init_topo.begin(), e->h_init_topo.end(), e->h_lane_topo.begin() + (size_t)k * g.dim_topo);
    if (g.n_shunt) std::copy(e->h_init_shunt_bus.begin(), e->h_init_shunt_bus.end(), e->h_lane_sb.begin() + (size_t)k * g.n_shunt);
  }
  e->plan_valid = false;
  return GPF_OK;
}

}  // namespace

// the plan of a lane range on device lane lists of the caller's: the planner fills list_a / list_b / list_c, which stand in for the
// caller's three for the duration of the call (the batch's cached plan and its lists are untouched)
int plan_launch_own(gpf_engine* e, int lane0, int n, LaunchPlan& p, LaunchPlan& pb, DevArr<int>* lists, bool list_tail) {
  DevArr<int>* mine[3] = {&e->list_a, &e->list_b, &e->list_c};
  auto swap_all = [&]() { for (int i = 0; i < 3; ++i) { std::swap(mine[i]->p, lists[i].p); std::swap(mine[i]->n, lists[i].n); std::swap(mine[i]->cap, lists[i].cap); } };
  swap_all();
  const int rc = plan_launch_uncached(e, lane0, n, p, pb, list_tail);
  swap_all();
  return rc;
}

int fan_plans(gpf_engine* e) {
  LaneFan& f = e->fan;
  if (e->plan_valid && f.plans_valid) return GPF_OK;
  f.plans_valid = false;
  ++f.plans_gen;
  // (the environment lanes run on the instance groups of a launch without the fan, whatever n_env is: their bits are that launch's)
  int rc = plan_launch_own(e, 0, f.n_env, f.env.p, f.env.pb, f.env.lists, true);
  if (rc == GPF_OK) rc = plan_launch_own(e, f.n_env, f.n_sec(), f.sec.p, f.sec.pb, f.sec.lists);
  // the batch's own plan, last: from here on plan_valid says "nothing that plans depend on has changed", for these two as well
  int32_t whole[8];
  if (rc == GPF_OK) rc = gpf_get_plan(e, whole);
  f.plans_valid = rc == GPF_OK;
  return rc;
}

int fan_mark_lanes(gpf_engine* e, std::vector<char>& flags, int mark) {
  std::fill_n(flags.begin() + e->fan.n_env, e->fan.n_sec(), (char)mark);
  if (e->cur_on) HIP_TRY(cursor_mark_lanes(e, e->fan.n_env, e->fan.n_sec(), mark));     // secondary lanes start no scenario of their own
  return GPF_OK;
}

gpf_engine::~gpf_engine() {
  if (dry) return;                      // (a header-only handle owns no device resource)
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  gpf_jit_release(jit);
}

extern "C" {

const char* gpf_last_error(void) { return g_err.c_str(); }
int gpf_version(void) { return GPF_ABI_VERSION; }

// ---- grid-specialised step kernels (gridpf_jit.hip) ----------------------------------------------------------------------------
namespace {
gpf::DevParamsS jit_block(gpf_engine* e) {
  gpf::DevParamsS hp{};
  hp.g = e->g; hp.oo = e->oo; hp.sym = e->sym_dev;
  return hp;
}
}  // namespace

int gpf_jit_enable(gpf_handle e, const char* src_dir, const char* cache_dir) {
  if (!e) return fail(GPF_E_INVALID, "gpf_jit_enable: null handle");
  (void)hipSetDevice(e->device);
  std::string err;
  if (gpf_jit_configure(e->jit, src_dir, cache_dir, err) != 0) { e->jit.on = false; e->jit.message = err; return fail(GPF_E_UNSUPPORTED, err); }
  const gpf::DevParamsS hp = jit_block(e);
  const std::string header = gpf_jit_header(hp);
  if (!e->jit.can_compile && !gpf_jit_has_aot(e->jit, header)) {       // nothing to load and nothing to compile with: say so now, not launch by launch
    e->jit.on = false;
    e->jit.message = "gpf_jit_enable: no ahead-of-time code objects for this grid (grid2op_amd/_aot) and no compiler at run time: " + e->jit.compile_why;
    return fail(GPF_E_UNSUPPORTED, e->jit.message);
  }
  if (header != e->jit.header) { gpf_jit_release(e->jit); e->jit.header = header; }
  e->jit_g = hp.g; e->jit_oo = hp.oo; e->jit_sym = hp.sym;
  e->jit.on = true;
  return GPF_OK;
}

int gpf_jit_disable(gpf_handle e) {
  if (!e) return fail(GPF_E_INVALID, "gpf_jit_disable: null handle");
  e->jit.on = false;
  return GPF_OK;
}

int gpf_jit_features(gpf_handle e, int32_t on) {
  if (!e) return fail(GPF_E_INVALID, "gpf_jit_features: null handle");
  e->jit.features = on != 0;
  return GPF_OK;
}

int gpf_jit_info(gpf_handle e, int64_t* counts, double* seconds, char* text, size_t cap) {
  if (!e) return fail(GPF_E_INVALID, "gpf_jit_info: null handle");
  if (counts) { counts[0] = e->jit.on ? 1 : 0; counts[1] = e->jit.n_compiled; counts[2] = e->jit.n_cached; counts[3] = e->jit.n_failed; counts[4] = e->jit.n_launches; counts[5] = e->jit.n_aot; }
  if (seconds) *seconds = e->jit.seconds;
  if (text && cap) {
    const std::string t = e->jit.variants + (e->jit.message.empty() ? "" : " | " + e->jit.message);
    snprintf(text, cap, "%s", t.c_str());
  }
  return GPF_OK;
}

int gpf_jit_source(gpf_handle e, char* text, size_t cap, size_t* need) {
  if (!e) return fail(GPF_E_INVALID, "gpf_jit_source: null handle");
  const std::string header = gpf_jit_header(jit_block(e));
  if (need) *need = header.size() + 1;
  if (text && cap) snprintf(text, cap, "%s", header.c_str());
  return GPF_OK;
}

int gpf_device_count(int32_t* n_devices) {
  if (!n_devices) return fail(GPF_E_INVALID, "gpf_device_count: null");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *n_devices = n;
  return GPF_OK;
}

int gpf_create(const gpf_grid_desc* d, int32_t n_lanes, int32_t device, gpf_handle* out_h) {
  if (!d || !out_h || n_lanes <= 0) return fail(GPF_E_INVALID, "gpf_create: bad arguments");
  if (d->n_sub <= 0 || d->n_busbar <= 0 || d->n_line < 0 || d->n_gen <= 0) return fail(GPF_E_INVALID, "gpf_create: bad sizes");
  if (d->n_line > 256) return fail(GPF_E_CAPACITY, "gpf_create: n_line > 256 not supported by the step kernel");
  if (d->n_busbar > GPF_MAX_BUSBAR)
    return fail(GPF_E_CAPACITY, "gpf_create: more than 64 busbars per substation (GPF_MAX_BUSBAR)");
  const bool dry = device == GPF_DEVICE_NONE;
  struct DryGuard { bool on; explicit DryGuard(bool d_) : on(d_) { if (on) g_dry_create = true; } ~DryGuard() { if (on) g_dry_create = false; } } dry_guard(dry);
  if (!dry) {
    int ndev = 0;
    hipError_t e0 = hipGetDeviceCount(&ndev);
    if (e0 != hipSuccess || ndev == 0)
      return fail(GPF_E_DEVICE, std::string("no HIP device available: ") + hipGetErrorString(e0));
    if (device < 0 || device >= ndev) return fail(GPF_E_INVALID, "gpf_create: bad device index");
    HIP_TRY(hipSetDevice(device));
  }
  std::unique_ptr<gpf_engine> own(new gpf_engine());   // frees what was allocated on every early return; the caller's on success
  gpf_engine* e = own.get();
  e->device = device;
  e->dry = dry;
  {
    const char* np_ = std::getenv("GRIDPF_NO_PARTITION");
    e->no_partition = np_ && np_[0] == '1';
    const char* nc_ = std::getenv("GRIDPF_NO_CLASSES");
    e->no_classes = nc_ && nc_[0] == '1';
    const char* iw = std::getenv("GRIDPF_IPW");
    e->ipw_override = (iw && (iw[0] == '1' || iw[0] == '2' || iw[0] == '4')) ? iw[0] - '0' : 0;
    const char* ww = std::getenv("GRIDPF_WPI");
    e->wpi_override = (ww && (ww[0] == '1' || ww[0] == '2')) ? ww[0] - '0' : 0;
    const char* det = std::getenv("GRIDPF_DETERMINISTIC");
    if (det && det[0] == '1') e->wpi_override = 1;
    e->wpi_env = e->wpi_override;
  }
  e->n_lanes = n_lanes;
  e->cap_lanes = (n_lanes + 7) & ~3;          // >= 4 ghost lanes (pristine state): padding of instance groups / lane lists
  gpf::GridDev& g = e->g;
  g.n_sub = d->n_sub; g.n_busbar = d->n_busbar; g.nb_tot = d->n_sub * d->n_busbar;
  g.n_line = d->n_line; g.n_gen = d->n_gen; g.n_load = d->n_load; g.n_sto = d->n_storage; g.n_shunt = d->n_shunt;
  g.dim_topo = d->dim_topo; g.sn_mva = d->sn_mva; g.inv_sn_mva = 1.0 / d->sn_mva;
  const int nl = g.n_line, ng = g.n_gen, nd = g.n_load, ns = g.n_sto, nsh = g.n_shunt;
  e->oo = gpf::make_offsets(nl, ng, nd, ns, nsh);
  g.n_inj = 2 * ng + 2 * nd + 2 * ns + 2 * nsh;
  g.n_out = 10 * nl + 4 * ng + 4 * nd + 4 * ns + 3 * nsh;
  g.n_chron = 2 * nd + 2 * ng;
  gpf_layout& L = e->layout;
  const gpf::OutOff& o = e->oo;
  L.n_inj = g.n_inj; L.inj_gen_p = o.inj_gen_p; L.inj_gen_vm = o.inj_gen_vm; L.inj_load_p = o.inj_load_p;
  L.inj_load_q = o.inj_load_q; L.inj_storage_p = o.inj_sto_p; L.inj_storage_q = o.inj_sto_q; L.inj_shunt_p = o.inj_sh_p;
  L.inj_shunt_q = o.inj_sh_q;
  L.n_out = g.n_out; L.out_p_or = o.p_or; L.out_q_or = o.q_or; L.out_v_or = o.v_or; L.out_a_or = o.a_or; L.out_theta_or = o.th_or;
  L.out_p_ex = o.p_ex; L.out_q_ex = o.q_ex; L.out_v_ex = o.v_ex; L.out_a_ex = o.a_ex; L.out_theta_ex = o.th_ex;
  L.out_gen_p = o.gen_p; L.out_gen_q = o.gen_q; L.out_gen_v = o.gen_v; L.out_gen_theta = o.gen_th;
  L.out_load_p = o.load_p; L.out_load_q = o.load_q; L.out_load_v = o.load_v; L.out_load_theta = o.load_th;
  L.out_storage_p = o.sto_p; L.out_storage_q = o.sto_q; L.out_storage_v = o.sto_v; L.out_storage_theta = o.sto_th;
  L.out_shunt_p = o.sh_p; L.out_shunt_q = o.sh_q; L.out_shunt_v = o.sh_v;
  L.n_chron = g.n_chron; L.chron_load_p = 0; L.chron_load_q = nd; L.chron_prod_p = 2 * nd; L.chron_prod_v = 2 * nd + ng;
  L.nb_total = g.nb_tot;

  auto cp = [](std::vector<int>& dst, const int32_t* src, int n) { dst.assign(src, src + n); };
  cp(e->h_line_or_sub, d->line_or_sub, nl); cp(e->h_line_ex_sub, d->line_ex_sub, nl);
  cp(e->h_line_or_pos, d->line_or_pos_topo_vect, nl); cp(e->h_line_ex_pos, d->line_ex_pos_topo_vect, nl);
  cp(e->h_gen_sub, d->gen_sub, ng); cp(e->h_gen_pos, d->gen_pos_topo_vect, ng);
  cp(e->h_load_sub, d->load_sub, nd); cp(e->h_load_pos, d->load_pos_topo_vect, nd);
  if (ns) { cp(e->h_sto_sub, d->storage_sub, ns); cp(e->h_sto_pos, d->storage_pos_topo_vect, ns); }
  if (nsh) cp(e->h_shunt_sub, d->shunt_sub, nsh);
  e->h_gen_slack.assign(d->gen_slack, d->gen_slack + ng);
  e->h_br_bdc.assign(d->br_bdc, d->br_bdc + nl);
  e->h_shunt_fact.assign(d->shunt_fact, d->shunt_fact + nsh);
  e->h_init_inj.assign(d->init_inj, d->init_inj + g.n_inj);
  e->h_init_topo.assign(d->init_topo, d->init_topo + g.dim_topo);
  if (nsh) e->h_init_shunt_bus.assign(d->init_shunt_bus, d->init_shunt_bus + nsh);
  // basic validation of the index tables (a wrong table would make the kernels read out of bounds)
  auto in_range = [](const std::vector<int>& v, int hi) { for (int x : v) if (x < 0 || x >= hi) return false; return true; };
  if (!in_range(e->h_line_or_sub, g.n_sub) || !in_range(e->h_line_ex_sub, g.n_sub) || !in_range(e->h_gen_sub, g.n_sub) ||
      !in_range(e->h_load_sub, g.n_sub) || !in_range(e->h_sto_sub, g.n_sub) || !in_range(e->h_shunt_sub, g.n_sub) ||
      !in_range(e->h_line_or_pos, g.dim_topo) || !in_range(e->h_line_ex_pos, g.dim_topo) || !in_range(e->h_gen_pos, g.dim_topo) ||
      !in_range(e->h_load_pos, g.dim_topo) || !in_range(e->h_sto_pos, g.dim_topo)) {
    return fail(GPF_E_INVALID, "gpf_create: index table out of range");
  }

  // (the first failure stops the uploads and names its buffer)
  hipError_t err = hipSuccess;
  std::string what;
  auto up = [&](const char* name, auto& arr, const auto* src, size_t count) {
    if (err == hipSuccess && (err = arr.upload(src, count)) != hipSuccess) what = std::string("upload ") + name;
  };
  auto al = [&](const char* name, auto& arr, size_t count) {
    if (err == hipSuccess && (err = arr.alloc(count)) != hipSuccess) what = std::string("alloc ") + name;
  };
  up("sub_vn_kv", e->sub_vn_kv, d->sub_vn_kv, g.n_sub); up("line_or_sub", e->line_or_sub, d->line_or_sub, nl);
  up("line_ex_sub", e->line_ex_sub, d->line_ex_sub, nl); up("line_or_pos", e->line_or_pos, d->line_or_pos_topo_vect, nl);
  up("line_ex_pos", e->line_ex_pos, d->line_ex_pos_topo_vect, nl); up("br_y", e->br_y, d->br_y, 8 * (size_t)nl);
  up("br_bdc", e->br_bdc, d->br_bdc, nl); up("gen_sub", e->gen_sub, d->gen_sub, ng); up("gen_pos", e->gen_pos, d->gen_pos_topo_vect, ng);
  up("gen_min_q", e->gen_min_q, d->gen_min_q, ng); up("gen_max_q", e->gen_max_q, d->gen_max_q, ng);
  up("gen_slack", e->gen_slack, d->gen_slack, ng); up("load_sub", e->load_sub, d->load_sub, nd);
  up("load_pos", e->load_pos, d->load_pos_topo_vect, nd); up("sto_sub", e->sto_sub, d->storage_sub, ns);
  up("sto_pos", e->sto_pos, d->storage_pos_topo_vect, ns); up("shunt_sub", e->shunt_sub, d->shunt_sub, nsh);
  up("shunt_fact", e->shunt_fact, d->shunt_fact, nsh); up("d_init_inj", e->d_init_inj, d->init_inj, g.n_inj);
  up("d_init_topo", e->d_init_topo, d->init_topo, g.dim_topo); up("d_init_shunt_bus", e->d_init_shunt_bus, d->init_shunt_bus, nsh);
  g.sub_vn_kv = e->sub_vn_kv.p; g.line_or_sub = e->line_or_sub.p; g.line_ex_sub = e->line_ex_sub.p;
  g.line_or_pos = e->line_or_pos.p; g.line_ex_pos = e->line_ex_pos.p; g.br_y = e->br_y.p; g.br_bdc = e->br_bdc.p;
  g.gen_sub = e->gen_sub.p; g.gen_pos = e->gen_pos.p; g.gen_min_q = e->gen_min_q.p; g.gen_max_q = e->gen_max_q.p;
  g.gen_slack = e->gen_slack.p; g.load_sub = e->load_sub.p; g.load_pos = e->load_pos.p; g.sto_sub = e->sto_sub.p;
  g.sto_pos = e->sto_pos.p; g.shunt_sub = e->shunt_sub.p; g.shunt_fact = e->shunt_fact.p;

  const size_t B = (size_t)e->cap_lanes;   // padded: ghost lanes hold the pristine state and are never read back
  al("inj", e->inj, B * g.n_inj); al("topo", e->topo, B * g.dim_topo); al("shunt_bus", e->shunt_bus, B * nsh);
  al("out", e->out, B * g.n_out); al("topo_out", e->topo_out, B * g.dim_topo); al("shunt_bus_out", e->shunt_bus_out, B * nsh);
  al("line_status", e->line_status, B * nl); al("status", e->status, B * 4); al("bus_vm", e->bus_vm, B * g.nb_tot);
  al("bus_va", e->bus_va, B * g.nb_tot); al("overflow_count", e->overflow_count, B * nl); al("disc_round", e->disc_round, B * nl);
  al("rho", e->rho, B * nl); al("cooldown", e->cooldown, B * nl); al("topo0", e->topo0, B * g.dim_topo); al("done", e->done, B);
  al("episode", e->episode, B * 2); al("lane_table", e->lane_table, B); al("lane_offset", e->lane_offset, B);
  al("thermal_limit", e->thermal_limit, nl); al("tmp_lines", e->tmp_lines, std::max<size_t>(B, 1));
  if (err != hipSuccess) return fail(GPF_E_DEVICE, what + ": " + hipGetErrorString(err));
  if (!dry) {
    hipError_t es = e->stream.create(hipStreamNonBlocking);
    if (es != hipSuccess) return fail(GPF_E_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(es));
  }
  count_lane(e, e->h_init_topo.data(), nsh ? e->h_init_shunt_bus.data() : nullptr, e->init_nb, e->init_nj, e->init_mb);
  e->lane_nb.assign(e->cap_lanes, e->init_nb);
  e->lane_nj.assign(e->cap_lanes, e->init_nj);
  e->lane_mb.assign(e->cap_lanes, e->init_mb);
  e->lane_class.assign(e->cap_lanes, -1);
  e->h_lane_table.assign(e->cap_lanes, 0);
  e->h_lane_offset.assign(e->cap_lanes, 0);
  e->h_lane_forecast.assign(e->cap_lanes, 0);
  e->h_lane_n1.assign(e->cap_lanes, 0);
  e->h_lane_topo.assign((size_t)e->cap_lanes * g.dim_topo, INT_MIN);
  e->h_lane_sb.assign((size_t)e->cap_lanes * std::max(g.n_shunt, 1), INT_MIN);
  {
    // symbolic analysis of the substation graph for the block-sparse kernels (once per grid)
    {
      // + slot layout search (gridpf_symbolic.hpp optimize_slot_layout; GRIDPF_SLOT_OPT=<iterations>, 0 = off); the result is a pure
      // function of the substation graph: one search per process and graph
      static std::mutex mu;
      static std::map<std::string, gpf::Symbolic> cache;
      const char* ev = std::getenv("GRIDPF_SLOT_OPT");
      // (default: grids of more than 24 substations -- one instance per wavefront or two wavefronts per instance, LDS-pipe-bound:
      //  N-1 fan-out on 36 substations +3.9 %, 118 substations +1.2 %; the instance-group kernels of the small grids lose 0.7 %)
      const int slot_opt = ev ? std::atoi(ev) : (g.n_sub > 24 ? 3000 : 0);
      std::string key(reinterpret_cast<const char*>(e->h_line_or_sub.data()), (size_t)nl * sizeof(int));
      key.append(reinterpret_cast<const char*>(e->h_line_ex_sub.data()), (size_t)nl * sizeof(int));
      const char* evb = std::getenv("GRIDPF_GJ_BUDGET");
      key += "/" + std::to_string(g.n_sub) + "/" + std::to_string(slot_opt) + "/" + (evb ? evb : "") + "/" + std::to_string(g.n_gen) + "/" +
             std::to_string(g.n_load) + "/" + std::to_string(g.n_sto) + "/" + std::to_string(g.n_shunt);
      std::lock_guard<std::mutex> lk(mu);
      auto it = cache.find(key);
      if (it == cache.end()) {
        gpf::Symbolic S0 = build_symbolic_resident(g, g.n_sub, nl, e->h_line_or_sub.data(), e->h_line_ex_sub.data(), false);
        it = cache.emplace(key, gpf::optimize_slot_layout(S0, slot_opt)).first;
      }
      e->sym = it->second;
    }
    const gpf::Symbolic& S = e->sym;
    if (S.nslot > 65535 || g.n_sub > 32767) return fail(GPF_E_CAPACITY, "grid too large for the 16-bit packed symbolic program");
    // the static blob of kernel S (layout: gpf::StatOff): doubles, then ints
    gpf::SymDev& D = e->sym_dev;
    gpf::StatOff& so = D.so;
    std::vector<double> fd;
    std::vector<int> fi;
    auto putd = [&fd](const double* v, size_t n) { int off = (int)fd.size(); fd.insert(fd.end(), v, v + n); if (fd.size() & 1) fd.push_back(0.0); return off; };
    auto puti = [&fi](const int* v, size_t n) { int off = (int)fi.size(); fi.insert(fi.end(), v, v + n); while (fi.size() & 3) fi.push_back(0); return off; };
    so.br_y = putd(d->br_y, (size_t)8 * nl); so.br_bdc = putd(d->br_bdc, nl); so.sub_vn_kv = putd(d->sub_vn_kv, g.n_sub);
    so.shunt_fact = putd(d->shunt_fact, nsh); so.gen_min_q = putd(d->gen_min_q, ng); so.gen_max_q = putd(d->gen_max_q, ng);
    {
      auto vn_of = [&](const int* sub, size_t n) { std::vector<double> v(n); for (size_t i = 0; i < n; ++i) v[i] = d->sub_vn_kv[sub[i]]; return v; };
      std::vector<double> lv((size_t)2 * nl);
      for (int l = 0; l < nl; ++l) { lv[2 * (size_t)l] = d->sub_vn_kv[d->line_or_sub[l]]; lv[2 * (size_t)l + 1] = d->sub_vn_kv[d->line_ex_sub[l]]; }
      so.line_vn = putd(lv.data(), lv.size());
      { std::vector<double> ka(lv.size()); for (size_t i = 0; i < lv.size(); ++i) ka[i] = 1000.0 / (1.7320508075688772935 * lv[i]); so.line_ka = putd(ka.data(), ka.size()); }
      { auto v = vn_of(d->load_sub, nd); so.load_vn = putd(v.data(), v.size()); }
      { auto v = vn_of(d->gen_sub, ng); so.gen_vn = putd(v.data(), v.size()); }
      { auto v = vn_of(d->storage_sub, ns); so.sto_vn = putd(v.data(), v.size()); }
      { auto v = vn_of(d->shunt_sub, nsh); so.shunt_vn = putd(v.data(), v.size()); }
    }
    {   // per-generator totals over the generators of its substation (pfsoln's reactive split when every generator is connected)
      std::vector<double> qmn(g.n_sub, 0.0), qmx(g.n_sub, 0.0), a(ng), b(ng);
      std::vector<int> cn(g.n_sub, 0), nsl(g.n_sub, 0), w(ng);
      for (int i = 0; i < ng; ++i) {
        const int sb = d->gen_sub[i];
        cn[sb] += 1; qmn[sb] += d->gen_min_q[i]; qmx[sb] += d->gen_max_q[i];
        if (d->gen_slack[i]) nsl[sb] += 1;
      }
      for (int i = 0; i < ng; ++i) { const int sb = d->gen_sub[i]; a[i] = qmn[sb]; b[i] = qmx[sb]; w[i] = cn[sb] | (nsl[sb] << 16); }
      so.gen_qmin_tot = putd(a.data(), a.size()); so.gen_qmax_tot = putd(b.data(), b.size());
      e->h_gen_cnt = w;
    }
    so.dc_inv = -1;
    D.dc_inv_g = nullptr;
    if (g.n_sub <= 512 && !std::getenv("GRIDPF_NO_DCINV")) {
      // inverse of the DC matrix of the reference topology (every line in service, reference buses = substations of the slack
      // generators), exactly as K3 assembles it: rows / columns of the reference buses are identity.  Column-major.
      const int n = g.n_sub;
      std::vector<char> is_ref(n, 0);
      for (int i = 0; i < ng; ++i) if (d->gen_slack[i]) is_ref[d->gen_sub[i]] = 1;
      std::vector<double> M((size_t)n * 2 * n, 0.0);
      std::vector<char> touched(n, 0);
      for (int l = 0; l < nl; ++l) {
        const int f = d->line_or_sub[l], t = d->line_ex_sub[l];
        touched[f] = touched[t] = 1;
        if (f == t) continue;
        const double bb = d->br_bdc[l];
        if (!is_ref[f]) M[(size_t)f * 2 * n + f] += bb;
        if (!is_ref[t]) M[(size_t)t * 2 * n + t] += bb;
        if (!is_ref[f] && !is_ref[t]) { M[(size_t)f * 2 * n + t] -= bb; M[(size_t)t * 2 * n + f] -= bb; }
      }
      bool ok = true;
      for (int i = 0; i < n; ++i) { if (is_ref[i]) M[(size_t)i * 2 * n + i] = 1.0; if (!touched[i]) ok = false; M[(size_t)i * 2 * n + n + i] = 1.0; }
      for (int k = 0; k < n && ok; ++k) {                          // Gauss-Jordan, partial pivoting
        int pv = k;
        for (int r = k + 1; r < n; ++r) if (std::fabs(M[(size_t)r * 2 * n + k]) > std::fabs(M[(size_t)pv * 2 * n + k])) pv = r;
        if (!(std::fabs(M[(size_t)pv * 2 * n + k]) > 1e-12)) { ok = false; break; }
        if (pv != k) for (int q = 0; q < 2 * n; ++q) std::swap(M[(size_t)k * 2 * n + q], M[(size_t)pv * 2 * n + q]);
        const double piv = M[(size_t)k * 2 * n + k];
        for (int q = 0; q < 2 * n; ++q) M[(size_t)k * 2 * n + q] /= piv;
        for (int r = 0; r < n; ++r) if (r != k) {
          const double m = M[(size_t)r * 2 * n + k];
          if (m != 0.0) for (int q = 0; q < 2 * n; ++q) M[(size_t)r * 2 * n + q] -= m * M[(size_t)k * 2 * n + q];
        }
      }
      if (ok) {
        // (the matrix is symmetric, its computed inverse only up to rounding: the table is made EXACTLY symmetric, so that the kernels may
        //  read it by rows or by columns, whichever their memory prefers, with identical results)
        std::vector<double> cm((size_t)n * n);
        for (int i = 0; i < n; ++i) for (int k = 0; k < n; ++k) cm[(size_t)k * n + i] = 0.5 * (M[(size_t)i * 2 * n + n + k] + M[(size_t)k * 2 * n + n + i]);
        // small grids: inside the static blob (staged in LDS with it); up to 63 substations (the single-wavefront kernels): a table of
        // its own in global memory, read through L2 (36 substations: 10 KB shared by every lane; +5.7 % at 4 096 lanes, +1.8 % on the
        // N-1 fan-out).  The two-wavefront kernels of the 118-substation grids keep their factored DC matrix in LDS instead: 118
        // dependent L2 reads per bus lane measured -6.8 % against 19 light passes over kept factors.  GRIDPF_DCINV_MAX moves the limit.
        const char* mx = std::getenv("GRIDPF_DCINV_MAX");
        if (n <= 24) so.dc_inv = putd(cm.data(), cm.size());
        else if (n <= (mx ? std::atoi(mx) : 63)) {
          if (e->dc_inv_g.upload(cm.data(), cm.size()) != hipSuccess) return fail(GPF_E_DEVICE, "upload dc_inv");
          so.dc_inv = -2;
          D.dc_inv_g = e->dc_inv_g.p;
        }
      }
    }
    so.prog = puti(S.prog.data(), S.prog.size());                // 16-byte aligned: level headers are read as int4
    { std::vector<int> rc(S.nslot_y); for (int k = 0; k < S.nslot_y; ++k) rc[k] = S.slot_row[k] | (S.slot_col[k] << 16); so.pair_rc = puti(rc.data(), rc.size()); }
    { const std::vector<int> upv = gpf::build_upairs(S); so.up = puti(upv.data(), upv.size()); D.n_up = (int)upv.size() / 2; }
    so.n_int_hot = (int)fi.size();
    so.line_or_pos = puti(d->line_or_pos_topo_vect, nl); so.line_ex_pos = puti(d->line_ex_pos_topo_vect, nl);
    so.line_or_sub = puti(d->line_or_sub, nl); so.line_ex_sub = puti(d->line_ex_sub, nl);
    so.br_slot = puti(S.br_slot.data(), S.br_slot.size());
    so.gen_pos = puti(d->gen_pos_topo_vect, ng); so.gen_sub = puti(d->gen_sub, ng);
    { std::vector<int> sl(ng); for (size_t i = 0; i < ng; ++i) sl[i] = d->gen_slack[i] ? 1 : 0; so.gen_slack = puti(sl.data(), ng); }
    so.load_pos = puti(d->load_pos_topo_vect, nd); so.load_sub = puti(d->load_sub, nd);
    so.sto_pos = puti(d->storage_pos_topo_vect, ns); so.sto_sub = puti(d->storage_sub, ns);
    so.shunt_sub = puti(d->shunt_sub, nsh);
    so.gen_cnt = puti(e->h_gen_cnt.data(), e->h_gen_cnt.size());
    {
      std::vector<int> pl(g.dim_topo, -1);
      for (int l = 0; l < nl; ++l) { pl[d->line_or_pos_topo_vect[l]] = l; pl[d->line_ex_pos_topo_vect[l]] = l; }
      so.pos_line = puti(pl.data(), pl.size());
    }
    so.n_dbl = (int)fd.size(); so.n_int = (int)fi.size();
    hipError_t eu = e->stat_dbl.upload(fd.data(), fd.size());
    if (eu == hipSuccess) eu = e->stat_int.upload(fi.data(), fi.size());
    if (eu != hipSuccess) return fail(GPF_E_DEVICE, std::string("upload static tables: ") + hipGetErrorString(eu));
    D.n = S.n; D.nslot = S.nslot; D.nslot_lu = S.nslot_lu; D.nslot_y = S.nslot_y; D.n_levels = S.n_levels; D.back_off = S.back_off; D.back_first = S.back_first;
      {   // connectivity of the static substation graph (all lines in service): lets the kernel skip the label propagation
      std::vector<int> comp(g.n_sub);
      for (int i = 0; i < g.n_sub; ++i) comp[i] = i;
      auto find = [&](int x) { while (comp[x] != x) { comp[x] = comp[comp[x]]; x = comp[x]; } return x; };
      for (int l = 0; l < nl; ++l) comp[find(e->h_line_or_sub[l])] = find(e->h_line_ex_sub[l]);
      int roots = 0;
      for (int i = 0; i < g.n_sub; ++i) roots += (find(i) == i);
      D.static_connected = roots == 1 ? 1 : 0;
    } D.scale_off = S.scale_off; D.n_scale = S.n_scale; D.n_prog = (int)S.prog.size();
    D.stat_dbl = e->stat_dbl.p; D.stat_int = e->stat_int.p; D.prog = e->stat_int.p + so.prog;
    // the grid's own programs get the bank-conflict-aware lane assignment (a local search per pass, ~0.1-1 s once per engine;
    // GRIDPF_LANE_OPT=<iterations> overrides, 0 = sequential assignment); topology classes are built inside a step and skip it
    int lane_opt = 3000;
    if (const char* lo_ = std::getenv("GRIDPF_LANE_OPT")) lane_opt = std::max(0, atoi(lo_));
    if (!upload_flats(S, e->flat_prog, D, lane_opt)) return fail(GPF_E_DEVICE, "upload flat programs");
  }
  {
    // keep the factored DC matrix in LDS across the steps of a launch when that does not cost residency: the blocks per CU
    // the whole batch needs at once must still fit (GRIDPF_DCF=0|1 overrides)
    const int ipw = e->ipw_override ? e->ipw_override : (g.n_sub <= 8 ? 4 : g.n_sub <= 24 ? 2 : 1);
    const int wpi0 = e->wpi_override ? std::min(e->wpi_override, 2) : (g.n_sub >= 64 ? 2 : 1);
    const size_t stat2 = gpf::stat_bytes(e->sym_dev.so, 2, true, ipw > 1 ? 0 : e->sym_dev.fl[gpf::gw_index(64 / ipw * (ipw == 1 ? wpi0 : 1))].n_words);
    const size_t with = gpf::lds_bytes_sparse<1>(g, e->sym.nslot, e->sym.nslot_y, stat2, true, ipw, -1, true);
    const size_t n_blocks = ((size_t)n_lanes + ipw - 1) / ipw;
    const size_t want = std::min<size_t>((n_blocks + 255) / 256, 8);
    e->dcf = (with <= LDS_HARD_LIMIT && LDS_HARD_LIMIT / with >= want) ? 1 : 0;
    const char* dv = std::getenv("GRIDPF_DCF");
    if (dv && (dv[0] == '0' || dv[0] == '1')) { e->dcf = dv[0] - '0'; e->dcf_env = e->dcf; }
    const char* yv = std::getenv("GRIDPF_YREG");
    e->no_yreg = yv && yv[0] == '0';
    const char* sv_ = std::getenv("GRIDPF_STAGE");
    if (sv_ && sv_[0] >= '0' && sv_[0] <= '2') e->stage_max = sv_[0] - '0';
    const char* kp_ = std::getenv("GRIDPF_KEEP");
    e->keep_enabled = !(kp_ && kp_[0] == '0');
    const char* fs_ = std::getenv("GRIDPF_FORCE_STAGE");
    if (fs_ && fs_[0] >= '0' && fs_[0] <= '2') e->stage_force = fs_[0] - '0';
  }
  if (dry) { *out_h = own.release(); return GPF_OK; }      // header-only handle: gpf_jit_source / gpf_get_plan / gpf_get_layout / gpf_destroy
  HIP_TRY(hipMemsetAsync(e->status.p, 0xFF, B * 4 * sizeof(int), e->stream));
  HIP_TRY(hipMemsetAsync(e->overflow_count.p, 0, B * nl * sizeof(int), e->stream));
  HIP_TRY(hipMemsetAsync(e->cooldown.p, 0, B * nl * sizeof(int), e->stream));
  HIP_TRY(hipMemsetAsync(e->done.p, 0, B, e->stream));
  HIP_TRY(hipMemsetAsync(e->episode.p, 0, B * 2 * sizeof(int), e->stream));
  HIP_TRY(hipMemsetAsync(e->lane_table.p, 0, B * sizeof(int), e->stream));
  HIP_TRY(hipMemsetAsync(e->lane_offset.p, 0, B * sizeof(int), e->stream));
  {
    std::vector<float> lim(nl, 1e30f);
    HIP_TRY(hipMemcpyAsync(e->thermal_limit.p, lim.data(), nl * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  if (const char* j = getenv("GRIDPF_JIT")) {
    if (atoi(j) > 0 && gpf_jit_enable(e, nullptr, nullptr) != GPF_OK) fprintf(stderr, "[gridpf] GRIDPF_JIT: %s\n", g_err.c_str());
  }
  int rc = reset_lanes_unchecked(e, 0, e->cap_lanes);
  if (rc != GPF_OK) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  *out_h = own.release();
  return GPF_OK;
}

int gpf_destroy(gpf_handle e) {
  if (!e) return GPF_OK;
  delete e;
  return GPF_OK;
}

int gpf_get_layout(gpf_handle e, gpf_layout* out) {
  if (!e || !out) return fail(GPF_E_INVALID, "gpf_get_layout: null");
  *out = e->layout;
  return GPF_OK;
}

int gpf_set_deterministic(gpf_handle e, int32_t flag) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_deterministic: null");
  e->wpi_override = flag ? 1 : e->wpi_env;
  e->plan_valid = false;
  return GPF_OK;
}

int gpf_n_lanes(gpf_handle e) { return e ? e->n_lanes : GPF_E_INVALID; }
int gpf_lane_capacity(gpf_handle e) { return e ? e->cap_lanes : GPF_E_INVALID; }

int gpf_set_injections(gpf_handle e, int32_t lane0, int32_t n, const double* inj) {
  if (!check_range(e, lane0, n) || !inj) return fail(GPF_E_INVALID, "gpf_set_injections: bad range");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(rows_to_device(e, e->inj, inj, e->g.n_inj, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));   // the host buffer may be reused by the caller right away
  return GPF_OK;
}

}  // extern "C"
// the host's bookkeeping of one lane whose topology row is now `t` / `sb` (busbar / unknown counts, topology class, mirror of the
// sent rows); true: it changed.  gpf_set_topology and the read-back of the device-side topology actions (gpf_step_n) both use it.
bool note_lane_row(gpf_engine* e, int lane, const int* t, const int* sb) {
  const gpf::GridDev& g = e->g;
  if (!e->ta_may_split)                                    // (a row on a busbar >= 2: line-status actions may move lanes between classes)
    for (int i = 0; i < g.dim_topo && !e->ta_may_split; ++i) e->ta_may_split = t[i] >= 2;
  int* mt = e->h_lane_topo.data() + (size_t)lane * g.dim_topo;
  int* ms = e->h_lane_sb.data() + (size_t)lane * std::max(g.n_shunt, 1);
  if (std::memcmp(mt, t, (size_t)g.dim_topo * sizeof(int)) == 0 && (!g.n_shunt || std::memcmp(ms, sb, (size_t)g.n_shunt * sizeof(int)) == 0))
    return false;                                          // re-sent unchanged: counts and topology class stay
  std::memcpy(mt, t, (size_t)g.dim_topo * sizeof(int));
  if (g.n_shunt) std::memcpy(ms, sb, (size_t)g.n_shunt * sizeof(int));
  count_lane(e, t, sb, e->lane_nb[lane], e->lane_nj[lane], e->lane_mb[lane]);
  e->lane_class[lane] = topo_class_of(e, t, sb);
  return true;
}

void lane_inherit(gpf_engine* e, int dst, int src, bool copy_mirror) {
  const gpf::GridDev& g = e->g;
  e->lane_nb[dst] = e->lane_nb[src]; e->lane_nj[dst] = e->lane_nj[src]; e->lane_mb[dst] = e->lane_mb[src]; e->lane_class[dst] = e->lane_class[src];
  if (!copy_mirror) { e->h_lane_topo[(size_t)dst * g.dim_topo] = INT_MIN; return; }
  std::copy_n(e->h_lane_topo.begin() + (size_t)src * g.dim_topo, g.dim_topo, e->h_lane_topo.begin() + (size_t)dst * g.dim_topo);
  if (g.n_shunt) std::copy_n(e->h_lane_sb.begin() + (size_t)src * g.n_shunt, g.n_shunt, e->h_lane_sb.begin() + (size_t)dst * g.n_shunt);
}

int moved_list_readback(gpf_engine* e, MovedList& ml, int lane_lo, int lane_hi, const char* who, const std::function<void(int)>& per_lane) {
  const gpf::GridDev& g = e->g;
  const size_t w = (size_t)g.dim_topo + g.n_shunt, cap = (size_t)(lane_hi - lane_lo), need = 1 + cap + cap * w;
  if (ml.pin.n < need) { HIP_TRY(hipStreamSynchronize(e->stream)); HIP_TRY(ml.pin.reserve(need)); }
  int* const block = ml.pin.p;
  HIP_TRY(hipMemcpyAsync(block, ml.list.p, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const int cnt = block[0];
  if (cnt <= 0) return GPF_OK;
  if (!moved_list_count_ok(cnt, lane_lo, lane_hi)) return fail(GPF_E_DEVICE, std::string(who) + " count)");
  HIP_TRY(hipMemcpyAsync(block + 1, ml.list.p + 1, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(block + 1 + cap, ml.rows.p, (size_t)cnt * w * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  bool changed = false;
  const int bad = moved_list_visit(block, w, lane_lo, lane_hi, [&](int lane, const int* t) {
    changed |= note_lane_row(e, lane, t, g.n_shunt ? t + g.dim_topo : nullptr);
    if (per_lane) per_lane(lane);
  });
  if (bad) return fail(GPF_E_DEVICE, std::string(who) + " lane)");
  if (changed) e->plan_valid = false;
  return GPF_OK;
}

int check_action_items(gpf_engine* e, const char* who, int n_items, const int32_t* items, bool* bus_items) {
  const gpf::GridDev& g = e->g;
  bool bus = false;
  for (int q = 0; q < n_items; ++q) {
    const int kind = items[3 * q], id = items[3 * q + 1], v = items[3 * q + 2];
    const bool pos_kind = kind == GPF_ACT_SET_BUS || kind == GPF_ACT_CHANGE_BUS, line_kind = kind == GPF_ACT_SET_LINE_STATUS || kind == GPF_ACT_CHANGE_LINE_STATUS;
    if (!(pos_kind || line_kind || kind == GPF_ACT_SET_SHUNT_BUS) || id < 0 || (pos_kind && id >= g.dim_topo) || (line_kind && id >= g.n_line) ||
        (kind == GPF_ACT_SET_SHUNT_BUS && id >= g.n_shunt) || ((kind == GPF_ACT_SET_BUS || kind == GPF_ACT_SET_SHUNT_BUS) && (v < -1 || v > g.n_busbar)) ||
        (kind == GPF_ACT_CHANGE_BUS && g.n_busbar != 2))
      return fail(GPF_E_INVALID, std::string(who) + ": bad action item (kind, id or bus; change_bus needs exactly 2 busbars per substation)");
    bus |= kind == GPF_ACT_CHANGE_BUS || kind == GPF_ACT_SET_SHUNT_BUS || (kind == GPF_ACT_SET_BUS && v != 0);
  }
  if (bus_items) *bus_items = bus;
  return GPF_OK;
}

namespace {
// gpf_set_topology.  `engine_rows`: the rows were built by the library itself in its own PINNED block (gpf_simulate_batch: validated
// action items applied to rows that came from the device) -- no validation pass, the uploads are true asynchronous DMA and nothing is
// waited for (the block stays untouched until the stream has drained: the next user of it synchronises first).
int set_topology_rows(gpf_engine* e, int32_t lane0, int32_t n, const int32_t* topo, const int32_t* shunt_bus, bool engine_rows) {
  const gpf::GridDev& g = e->g;
  if (!engine_rows) {
    // validate BOTH arrays before anything is queued: a rejected call leaves the device state and the host mirror untouched
    auto bad_bus = [&g](int v) { return v == 0 || v < -1 || v > g.n_busbar; };
    for (size_t i = 0; i < (size_t)n * g.dim_topo; ++i)
      if (bad_bus(topo[i])) return fail(GPF_E_INVALID, "gpf_set_topology: local bus ids must be -1 or 1..n_busbar");
    if (shunt_bus && g.n_shunt)
      for (size_t i = 0; i < (size_t)n * g.n_shunt; ++i)
        if (bad_bus(shunt_bus[i])) return fail(GPF_E_INVALID, "gpf_set_topology: shunt bus ids must be -1 or 1..n_busbar");
  }
  HIP_TRY(hipMemcpyAsync(e->topo.p + (size_t)lane0 * g.dim_topo, topo, (size_t)n * g.dim_topo * sizeof(int),
                         hipMemcpyHostToDevice, e->stream));
  // the rows an auto-reset restores: copied on the device from the rows just uploaded (not a second trip over PCIe)
  HIP_TRY(hipMemcpyAsync(e->topo0.p + (size_t)lane0 * g.dim_topo, e->topo.p + (size_t)lane0 * g.dim_topo, (size_t)n * g.dim_topo * sizeof(int),
                         hipMemcpyDeviceToDevice, e->stream));
  std::vector<int> sb_host;
  if (shunt_bus && g.n_shunt) {
    HIP_TRY(hipMemcpyAsync(e->shunt_bus.p + (size_t)lane0 * g.n_shunt, shunt_bus, (size_t)n * g.n_shunt * sizeof(int),
                           hipMemcpyHostToDevice, e->stream));
  } else if (g.n_shunt) {
    sb_host.resize((size_t)n * g.n_shunt);
    HIP_TRY(hipMemcpyAsync(sb_host.data(), e->shunt_bus.p + (size_t)lane0 * g.n_shunt, sb_host.size() * sizeof(int),
                           hipMemcpyDeviceToHost, e->stream));
  }
  if (!engine_rows || !sb_host.empty()) HIP_TRY(hipStreamSynchronize(e->stream));
  topo_unmoved(e, lane0, n);                               // (the rows sent are the lanes' reset topology too: topo0 above)
  bool changed = false;
  for (int k = 0; k < n; ++k) {
    const int* sb = nullptr;
    if (g.n_shunt) sb = shunt_bus ? shunt_bus + (size_t)k * g.n_shunt : sb_host.data() + (size_t)k * g.n_shunt;
    changed |= note_lane_row(e, lane0 + k, topo + (size_t)k * g.dim_topo, sb);
  }
  if (changed) e->plan_valid = false;
  return GPF_OK;
}
}  // namespace
extern "C" {

int gpf_set_topology(gpf_handle e, int32_t lane0, int32_t n, const int32_t* topo, const int32_t* shunt_bus) {
  if (!check_range(e, lane0, n) || !topo) return fail(GPF_E_INVALID, "gpf_set_topology: bad range");
  HIP_TRY(hipSetDevice(e->device));
  return set_topology_rows(e, lane0, n, topo, shunt_bus, false);
}

int gpf_get_injections(gpf_handle e, int32_t lane0, int32_t n, double* inj) {
  if (!check_range(e, lane0, n) || !inj) return fail(GPF_E_INVALID, "gpf_get_injections: bad range");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(rows_to_host(e, inj, e->inj, e->g.n_inj, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_topology(gpf_handle e, int32_t lane0, int32_t n, int32_t* topo, int32_t* shunt_bus) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_get_topology: bad range");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(rows_to_host(e, topo, e->topo, e->g.dim_topo, lane0, n));
  HIP_TRY(rows_to_host(e, shunt_bus, e->shunt_bus, e->g.n_shunt, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_disconnect_line(gpf_handle e, int32_t lane, int32_t line_id) {
  if (!check_range(e, lane, 1) || line_id < 0 || line_id >= e->g.n_line) return fail(GPF_E_INVALID, "gpf_disconnect_line: bad ids");
  HIP_TRY(hipSetDevice(e->device));
  const int m1 = -1;
  int* row = e->topo.p + (size_t)lane * e->g.dim_topo;
  int* row0 = e->topo0.p + (size_t)lane * e->g.dim_topo;
  HIP_TRY(hipMemcpyAsync(row + e->h_line_or_pos[line_id], &m1, sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(row + e->h_line_ex_pos[line_id], &m1, sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(row0 + e->h_line_or_pos[line_id], &m1, sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(row0 + e->h_line_ex_pos[line_id], &m1, sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->h_lane_topo[(size_t)lane * e->g.dim_topo] = INT_MIN;          // host mirror of the sent topology: unknown from now on
  return GPF_OK;   // removing a branch never increases the bus / unknown counts: capacity bookkeeping unchanged
}

int gpf_reset_lanes(gpf_handle e, int32_t lane0, int32_t n) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_reset_lanes: bad range");
  return reset_lanes_unchecked(e, lane0, n);
}

int gpf_copy_lanes(gpf_handle e, int32_t src, int32_t dst, int32_t n) {
  if (!check_range(e, src, n) || !check_range(e, dst, n)) return fail(GPF_E_INVALID, "gpf_copy_lanes: bad range");
  if (src == dst || n == 0) return GPF_OK;
  if (std::abs(src - dst) < n) return fail(GPF_E_INVALID, "gpf_copy_lanes: overlapping ranges");
  HIP_TRY(hipSetDevice(e->device));
  const gpf::GridDev& g = e->g;
  hipError_t err = hipSuccess;
  auto cp = [&](const auto& arr, size_t stride) { if (err == hipSuccess) err = rows_copy(e, arr, stride, src, dst, n); };
  cp(e->inj, g.n_inj); cp(e->topo, g.dim_topo); cp(e->shunt_bus, g.n_shunt); cp(e->out, g.n_out); cp(e->topo_out, g.dim_topo);
  cp(e->shunt_bus_out, g.n_shunt); cp(e->line_status, g.n_line); cp(e->status, 4); cp(e->bus_vm, g.nb_tot); cp(e->bus_va, g.nb_tot);
  cp(e->overflow_count, g.n_line); cp(e->cooldown, g.n_line); cp(e->disc_round, g.n_line); cp(e->rho, g.n_line); cp(e->topo0, g.dim_topo);
  cp(e->done, 1); cp(e->episode, 2);
  if (e->env_on && err == hipSuccess) err = env_copy_lanes(e, src, dst, n);
  if (e->ta_on && err == hipSuccess) err = topo_copy_lanes(e, src, dst, n);
  if (e->opp_kind && err == hipSuccess) err = opponent_copy_lanes(e, src, dst, n);
  if (e->al_on && err == hipSuccess) err = alert_copy_lanes(e, src, dst, n);
  if (e->ep_on && err == hipSuccess) err = episode_copy_lanes(e, src, dst, n);
  if (e->cur_on && err == hipSuccess) err = cursor_copy_lanes(e, src, dst, n);
  if (e->cb_on && err == hipSuccess) err = combined_copy_lanes(e, src, dst, n);
  HIP_TRY(err);
  for (int k = 0; k < n; ++k) lane_inherit(e, dst + k, src + k, true);
  e->plan_valid = false;
  return GPF_OK;
}

int gpf_fanout_n1(gpf_handle e, int32_t src, int32_t dst0, int32_t n_out, const int32_t* out_lines) {
  if (!check_range(e, src, 1) || !check_range(e, dst0, n_out) || !out_lines) return fail(GPF_E_INVALID, "gpf_fanout_n1: bad range");
  if (src >= dst0 && src < dst0 + n_out) return fail(GPF_E_INVALID, "gpf_fanout_n1: source inside destination range");
  if (n_out == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  if (e->tmp_lines.n < (size_t)n_out) HIP_TRY(e->tmp_lines.alloc(n_out));
  HIP_TRY(hipMemcpyAsync(e->tmp_lines.p, out_lines, (size_t)n_out * sizeof(int), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(gpf::fanout_kernel, dim3(n_out), dim3(64), 0, e->stream, e->g, e->bufs(), src, dst0, n_out, e->tmp_lines.p);
  HIP_TRY(hipGetLastError());
  if (e->env_on) {                          // the contingency lanes start from the source's injection dynamics
    if (e->sim_src.n < 1) HIP_TRY(e->sim_src.alloc(1));
    HIP_TRY(hipMemcpyAsync(e->sim_src.p, &src, sizeof(int), hipMemcpyHostToDevice, e->stream));
    int rc_e = env_copy_from(e, e->sim_src.p, n_out, n_out, dst0); if (rc_e != GPF_OK) return rc_e;
  }
  if (e->ta_on) { int rc_t = topo_fanout_lanes(e, src, dst0, n_out); if (rc_t != GPF_OK) return rc_t; }   // ... and its acting-path state
  if (e->cur_on) HIP_TRY(cursor_mark_lanes(e, dst0, n_out, 1));     // contingency lanes start no scenario of their own
  std::fill_n(e->h_lane_n1.begin() + dst0, n_out, 1);
  HIP_TRY(hipStreamSynchronize(e->stream));   // out_lines may be reused by the caller
  for (int k = 0; k < n_out; ++k) lane_inherit(e, dst0 + k, src, false);     // a line was forced off on the device: mirror unknown
  topo_unmoved(e, dst0, n_out);                 // (fanout_kernel writes the contingency row as the lanes' reset topology too)
  e->plan_valid = false;
  return GPF_OK;
}

int gpf_runpf(gpf_handle e, int32_t lane0, int32_t n, int32_t is_dc, int32_t max_iter, double tol_mva) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_runpf: bad range");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  return runpf_range(e, lane0, n, is_dc, max_iter, tol_mva, nullptr, nullptr);
}

}  // extern "C"
// gpf_runpf on a checked range; pre_p / pre_pb: the range's plan, made by the caller (else it is planned here)
int runpf_range(gpf_engine* e, int lane0, int n, int is_dc, int max_iter, double tol_mva, const LaunchPlan* pre_p, const LaunchPlan* pre_pb) {
  LaunchPlan p, pb;
  int rc = GPF_OK;
  if (pre_p) { p = *pre_p; pb = *pre_pb; }
  else rc = plan_launch(e, lane0, n, p, pb);
  if (rc != GPF_OK) return rc;
  gpf::Bufs b = e->bufs();
  const double tol_pu = tol_mva / e->g.sn_mva;
  hipEvent_t ea = nullptr, eb = nullptr;
  rc = upload_params_s(e, b, p.tc ? &p : (pb.tc ? &pb : nullptr), p.dcf);
  if (rc != GPF_OK) return rc;
  if (e->profiling) { rc = prof_begin(e, ea, eb); if (rc != GPF_OK) return rc; }
  // (measured: forking the second launch onto its own stream costs more in cross-stream events than the overlap gains)
  p.jit = pb.jit = jit_for_launch(e);
  HIP_TRY(gpf_launch_runpf_sparse(p, e->device, e->d_params_s.p, e->stream, lane0, n, is_dc, max_iter, tol_pu));
  if (pb.sparse_nb) HIP_TRY(gpf_launch_runpf_sparse(pb, e->device, e->d_params_s.p, e->stream, lane0, n, is_dc, max_iter, tol_pu));
  HIP_TRY(hipGetLastError());
  if (e->profiling) HIP_TRY(hipEventRecord(eb, e->stream));
  if (e->window) { ++e->win_launches; e->win_marked = false; }
  return GPF_OK;
}
extern "C" {

// A blocking hipStreamSynchronize wakes up 10-15 us after the stream drained (interrupt + scheduler): a consumer of short launches
// (one 20-step launch of 14 substations is 0.4 ms, a one-lane runpf 30 us) pays that on every synchronisation.  Poll the stream for up
// to ~0.5 ms first (GRIDPF_SYNC_SPIN_US, 0: never), then block: long waits do not burn a host core.
static hipError_t sync_stream_spin(hipStream_t st) {
  static const long spin_us = getenv("GRIDPF_SYNC_SPIN_US") ? atol(getenv("GRIDPF_SYNC_SPIN_US")) : 500;
  if (spin_us > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t q = hipStreamQuery(st);
      if (q == hipSuccess) return hipSuccess;
      if (q != hipErrorNotReady) break;
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
    }
    (void)hipGetLastError();
  }
  return hipStreamSynchronize(st);
}

// The whole of HipBackend.runpf for ONE lane in a single call: push the lane's injections and topology (apply_action's
// scatter, pandaPowerBackend.py:920-975), solve (runpf -> pp.runpp / rundcpp, :1078-1120), read every result buffer back
// (the getters, :1566-1619) -- everything queued on the stream through one pinned staging block, ONE synchronisation.
int gpf_solve_lane(gpf_handle e, int32_t lane, const double* inj, const int32_t* topo, const int32_t* shunt_bus, int32_t is_dc,
                   int32_t max_iter, double tol_mva, float* out, int32_t* topo_vect, int32_t* shunt_bus_out, uint8_t* line_status,
                   int32_t* status, double* bus_vm, double* bus_va) {
  if (!check_range(e, lane, 1) || !inj || !topo) return fail(GPF_E_INVALID, "gpf_solve_lane: bad arguments");
  const gpf::GridDev& g = e->g;
  if (g.n_shunt && !shunt_bus) return fail(GPF_E_INVALID, "gpf_solve_lane: shunt_bus is required on a grid with shunts");
  auto bad_bus = [&g](int v) { return v == 0 || v < -1 || v > g.n_busbar; };
  for (int i = 0; i < g.dim_topo; ++i) if (bad_bus(topo[i])) return fail(GPF_E_INVALID, "gpf_solve_lane: local bus ids must be -1 or 1..n_busbar");
  for (int i = 0; i < g.n_shunt; ++i) if (bad_bus(shunt_bus[i])) return fail(GPF_E_INVALID, "gpf_solve_lane: shunt bus ids must be -1 or 1..n_busbar");
  HIP_TRY(hipSetDevice(e->device));
  // staging layout (16-byte aligned pieces): in: inj | topo | shunt_bus    out: out | topo_vect | shunt_bus_out | line_status | status | bus_vm | bus_va
  auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t o_inj = 0, o_topo = o_inj + al((size_t)g.n_inj * 8), o_sb = o_topo + al((size_t)g.dim_topo * 4);
  const size_t o_out = o_sb + al((size_t)g.n_shunt * 4), o_tv = o_out + al((size_t)g.n_out * 4), o_sbo = o_tv + al((size_t)g.dim_topo * 4);
  const size_t o_ls = o_sbo + al((size_t)g.n_shunt * 4), o_st = o_ls + al((size_t)g.n_line), o_vm = o_st + 16, o_va = o_vm + al((size_t)g.nb_tot * 8);
  const size_t total = o_va + al((size_t)g.nb_tot * 8);
  HIP_TRY(e->pin.reserve(total));
  unsigned char* P = e->pin.p;
  std::memcpy(P + o_inj, inj, (size_t)g.n_inj * 8);
  std::memcpy(P + o_topo, topo, (size_t)g.dim_topo * 4);
  if (g.n_shunt) std::memcpy(P + o_sb, shunt_bus, (size_t)g.n_shunt * 4);
  hipStream_t st = e->stream;
  // Host bookkeeping of the lane's topology (as gpf_set_topology) and launch planning come FIRST: both can fail (capacity), and a
  // rejected call must leave the device rows and the host mirror untouched -- the old bookkeeping is restored on failure.
  LaunchPlan p, pb;
  {
    int* mt = e->h_lane_topo.data() + (size_t)lane * g.dim_topo;
    int* ms = e->h_lane_sb.data() + (size_t)lane * std::max(g.n_shunt, 1);
    const bool same = std::memcmp(mt, topo, (size_t)g.dim_topo * sizeof(int)) == 0 &&
                      (!g.n_shunt || std::memcmp(ms, shunt_bus, (size_t)g.n_shunt * sizeof(int)) == 0);
    const int o_nb = e->lane_nb[lane], o_nj = e->lane_nj[lane], o_mb = e->lane_mb[lane], o_cls = e->lane_class[lane];
    topo_unmoved(e, lane, 1);                                // (lane_scatter_kernel writes the row as the lane's reset topology too)
    if (!same) {
      for (int i = 0; i < g.dim_topo && !e->ta_may_split; ++i) e->ta_may_split = topo[i] >= 2;
      count_lane(e, topo, g.n_shunt ? shunt_bus : nullptr, e->lane_nb[lane], e->lane_nj[lane], e->lane_mb[lane]);
      e->lane_class[lane] = topo_class_of(e, topo, g.n_shunt ? shunt_bus : nullptr);
      e->plan_valid = false;
    }
    int rc = plan_launch(e, lane, 1, p, pb);
    if (rc == GPF_OK) rc = upload_params_s(e, e->bufs(), p.tc ? &p : (pb.tc ? &pb : nullptr), p.dcf);
    if (rc != GPF_OK) {
      e->lane_nb[lane] = o_nb; e->lane_nj[lane] = o_nj; e->lane_mb[lane] = o_mb; e->lane_class[lane] = o_cls;
      e->plan_valid = false;
      return rc;
    }
    if (!same) {
      std::memcpy(mt, topo, (size_t)g.dim_topo * sizeof(int));
      if (g.n_shunt) std::memcpy(ms, shunt_bus, (size_t)g.n_shunt * sizeof(int));
    }
  }
  // GRIDPF_LANE_STAGED=1 (developer A/B): the eleven staged copies of rounds 1 - 4 instead of the two zero-copy dispatches
  static const bool staged = [] { const char* v = std::getenv("GRIDPF_LANE_STAGED"); return v && std::atoi(v) > 0; }();
  const gpf::LaneBlob lb{o_inj, o_topo, o_sb, o_out, o_tv, o_sbo, o_ls, o_st, o_vm, o_va};
  const gpf::Bufs bufs = e->bufs();
  if (staged) {
  HIP_TRY(hipMemcpyAsync(e->inj.p + (size_t)lane * g.n_inj, P + o_inj, (size_t)g.n_inj * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(e->topo.p + (size_t)lane * g.dim_topo, P + o_topo, (size_t)g.dim_topo * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(e->topo0.p + (size_t)lane * g.dim_topo, P + o_topo, (size_t)g.dim_topo * 4, hipMemcpyHostToDevice, st));
  if (g.n_shunt) HIP_TRY(hipMemcpyAsync(e->shunt_bus.p + (size_t)lane * g.n_shunt, P + o_sb, (size_t)g.n_shunt * 4, hipMemcpyHostToDevice, st));
  } else {
    hipLaunchKernelGGL(gpf::lane_scatter_kernel, dim3(1), dim3(256), 0, st, g, bufs, (int)lane, (const unsigned char*)e->pin.dev, lb);
    HIP_TRY(hipGetLastError());
  }
  const double tol_pu = tol_mva / g.sn_mva;
  p.jit = pb.jit = jit_for_launch(e);
  HIP_TRY(gpf_launch_runpf_sparse(p, e->device, e->d_params_s.p, st, lane, 1, is_dc, max_iter, tol_pu));
  if (pb.sparse_nb) HIP_TRY(gpf_launch_runpf_sparse(pb, e->device, e->d_params_s.p, st, lane, 1, is_dc, max_iter, tol_pu));
  if (e->window) { ++e->win_launches; e->win_marked = false; }
#define DL1(off, arr, stride, bytes_per) \
  if ((stride) > 0) HIP_TRY(hipMemcpyAsync(P + (off), e->arr.p + (size_t)lane * (stride), (size_t)(stride) * (bytes_per), hipMemcpyDeviceToHost, st))
  if (staged) {
  DL1(o_out, out, g.n_out, 4); DL1(o_tv, topo_out, g.dim_topo, 4); DL1(o_sbo, shunt_bus_out, g.n_shunt, 4); DL1(o_ls, line_status, g.n_line, 1);
  DL1(o_st, status, 4, 4); DL1(o_vm, bus_vm, g.nb_tot, 8); DL1(o_va, bus_va, g.nb_tot, 8);
  } else {
    hipLaunchKernelGGL(gpf::lane_gather_kernel, dim3(1), dim3(256), 0, st, g, bufs, (int)lane, e->pin.dev, lb);
    HIP_TRY(hipGetLastError());
  }
#undef DL1
  HIP_TRY(hipStreamSynchronize(st));          // (a wait this short: the runtime's own active wait beats polling hipStreamQuery by 3 - 5 us)
  if (out) std::memcpy(out, P + o_out, (size_t)g.n_out * 4);
  if (topo_vect) std::memcpy(topo_vect, P + o_tv, (size_t)g.dim_topo * 4);
  if (shunt_bus_out && g.n_shunt) std::memcpy(shunt_bus_out, P + o_sbo, (size_t)g.n_shunt * 4);
  if (line_status) std::memcpy(line_status, P + o_ls, (size_t)g.n_line);
  if (status) std::memcpy(status, P + o_st, 16);
  if (bus_vm) std::memcpy(bus_vm, P + o_vm, (size_t)g.nb_tot * 8);
  if (bus_va) std::memcpy(bus_va, P + o_va, (size_t)g.nb_tot * 8);
  return GPF_OK;
}

int gpf_get_results(gpf_handle e, int32_t lane0, int32_t n, float* out, int32_t* topo_vect, int32_t* shunt_bus,
                    uint8_t* line_status, int32_t* status, double* bus_vm, double* bus_va) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_get_results: bad range");
  HIP_TRY(hipSetDevice(e->device));
  const gpf::GridDev& g = e->g;
  HIP_TRY(rows_to_host(e, out, e->out, g.n_out, lane0, n)); HIP_TRY(rows_to_host(e, topo_vect, e->topo_out, g.dim_topo, lane0, n));
  HIP_TRY(rows_to_host(e, shunt_bus, e->shunt_bus_out, g.n_shunt, lane0, n)); HIP_TRY(rows_to_host(e, line_status, e->line_status, g.n_line, lane0, n));
  HIP_TRY(rows_to_host(e, status, e->status, 4, lane0, n)); HIP_TRY(rows_to_host(e, bus_vm, e->bus_vm, g.nb_tot, lane0, n));
  HIP_TRY(rows_to_host(e, bus_va, e->bus_va, g.nb_tot, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

// gpf_get_results into the engine's own PINNED block: the copies are true DMA (a pageable destination is staged through the runtime's
// bounce buffers at a fraction of the PCIe rate), one synchronisation, and the caller reads the rows where they landed -- no second
// host copy.  ptrs[k] = address of piece k inside the block (NULL when not asked for); valid until the next call of this function.
int gpf_get_results_pinned(gpf_handle e, int32_t lane0, int32_t n, int32_t what, void** ptrs) {
  if (!check_range(e, lane0, n) || !ptrs) return fail(GPF_E_INVALID, "gpf_get_results_pinned: bad range");
  HIP_TRY(hipSetDevice(e->device));
  const gpf::GridDev& g = e->g;
  const size_t N = (size_t)n;
  auto al = [](size_t v) { return (v + 63) & ~(size_t)63; };
  const size_t bytes[8] = {N * g.n_out * 4, N * g.dim_topo * 4, N * g.n_shunt * 4, N * g.n_line, N * 16, N * g.nb_tot * 8, N * g.nb_tot * 8, N * g.n_line * 4};
  size_t off[8], total = 0;
  for (int k = 0; k < 8; ++k) { off[k] = total; if ((what >> k) & 1) total += al(bytes[k]); }
  HIP_TRY(e->res_pin.reserve(total));
  const void* src[8] = {e->out.p + (size_t)lane0 * g.n_out, e->topo_out.p + (size_t)lane0 * g.dim_topo, e->shunt_bus_out.p + (size_t)lane0 * g.n_shunt,
                        e->line_status.p + (size_t)lane0 * g.n_line, e->status.p + (size_t)lane0 * 4, e->bus_vm.p + (size_t)lane0 * g.nb_tot,
                        e->bus_va.p + (size_t)lane0 * g.nb_tot, e->rho.p + (size_t)lane0 * g.n_line};
  for (int k = 0; k < 8; ++k) {
    ptrs[k] = nullptr;
    if (!((what >> k) & 1) || bytes[k] == 0) continue;
    HIP_TRY(hipMemcpyAsync(e->res_pin.p + off[k], src[k], bytes[k], hipMemcpyDeviceToHost, e->stream));
    ptrs[k] = e->res_pin.p + off[k];
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_upload_chronics(gpf_handle e, int32_t n_tables, int32_t T, const float* data) {
  if (!e || n_tables <= 0 || T <= 0 || !data) return fail(GPF_E_INVALID, "gpf_upload_chronics: bad arguments");
  if (e->cur_on && (n_tables <= e->cur_max_table || T <= e->cur_max_first_row))
    return fail(GPF_E_INVALID, "gpf_upload_chronics: the chronics cursor is on (gpf_set_chronics_cursor) and its order names table " +
                               std::to_string(e->cur_max_table) + ", its first_row row " + std::to_string(e->cur_max_first_row) +
                               ": upload at least that many tables and rows, or turn the cursor off first");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->maint.release();                       // belongs to the previous tables
  e->h_maint.clear(); e->h_hazard.clear();
  ++e->maint_gen;
  e->forecast.release(); e->fc_h = 0;
  HIP_TRY(e->chron.upload(data, (size_t)n_tables * T * e->g.n_chron));
  e->chron_T = T;
  if (n_tables < e->chron_tables) {
    // fewer tables than before: lanes that pointed past the new end fall back to table 0 (the kernel indexes the buffer
    // with lane_table unchecked)
    std::vector<int> lt(e->cap_lanes);
    HIP_TRY(hipMemcpy(lt.data(), e->lane_table.p, lt.size() * sizeof(int), hipMemcpyDeviceToHost));
    bool fix = false;
    for (int& v : lt) if (v < 0 || v >= n_tables) { v = 0; fix = true; }
    if (fix) HIP_TRY(hipMemcpy(e->lane_table.p, lt.data(), lt.size() * sizeof(int), hipMemcpyHostToDevice));
    e->h_lane_table = lt;
  }
  e->chron_tables = n_tables;
  return GPF_OK;
}

}  // extern "C"
namespace {
// maintenance.csv and hazards.csv both force a line out of service while flagged (the environment's "maintenance" / "hazards"
// modifications, Environment/baseEnv.py:2516-2563): the device holds the union of the two tables
int upload_outage_tables(gpf_engine* e) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->maint.release();
  e->maint_dur.release();
  ++e->maint_gen;
  if (e->h_maint.empty() && e->h_hazard.empty()) return GPF_OK;
  std::vector<unsigned char> u = e->h_maint.empty() ? e->h_hazard : e->h_maint;
  if (!e->h_maint.empty() && !e->h_hazard.empty()) for (size_t i = 0; i < u.size(); ++i) u[i] = (u[i] || e->h_hazard[i]) ? 1 : 0;
  HIP_TRY(e->maint.upload(u.data(), u.size()));
  // remaining duration of the maintenance / hazard under way at every row (GridValue.get_maintenance_duration_1d / get_hazard_duration_1d
  // while the outage lasts: 3, 2, 1 over a 3-step outage): what BaseEnv._update_time_reconnection_hazards_maintenance raises the line
  // cooldown to (baseEnv.py:2590-2597: the maximum of the two)
  const size_t nl = e->g.n_line, T = (size_t)e->chron_T, nt = (size_t)e->chron_tables;
  std::vector<unsigned short> dur(nt * T * nl, 0);
  auto scan = [&](const std::vector<unsigned char>& tab) {
    if (tab.empty()) return;
    for (size_t k = 0; k < nt; ++k)
      for (size_t l = 0; l < nl; ++l) {
        unsigned run = 0;
        for (size_t t = T; t-- > 0;) {
          run = tab[(k * T + t) * nl + l] ? std::min(run + 1u, 65535u) : 0u;
          unsigned short& d = dur[(k * T + t) * nl + l];
          if (run > d) d = (unsigned short)run;
        }
      }
  };
  scan(e->h_maint); scan(e->h_hazard);
  // (durations given by the caller win: tables that are a WINDOW of longer chronics cannot know how long an outage at their end lasts)
  if (e->h_outage_dur.size() == dur.size()) for (size_t i = 0; i < dur.size(); ++i) if (u[i]) dur[i] = e->h_outage_dur[i];
  HIP_TRY(e->maint_dur.upload(dur.data(), dur.size()));
  return GPF_OK;
}
int set_outage_table(gpf_engine* e, std::vector<unsigned char>& dst, int n_tables, int T, const uint8_t* data, const char* who) {
  if (!data) { dst.clear(); return upload_outage_tables(e); }
  if (n_tables != e->chron_tables || T != e->chron_T)
    return fail(GPF_E_INVALID, std::string(who) + ": shape must match the uploaded chronics tables (n_tables, T)");
  dst.assign(data, data + (size_t)n_tables * T * e->g.n_line);
  return upload_outage_tables(e);
}
}  // namespace
extern "C" {

int gpf_upload_maintenance(gpf_handle e, int32_t n_tables, int32_t T, const uint8_t* data) {
  if (!e) return fail(GPF_E_INVALID, "gpf_upload_maintenance: null");
  return set_outage_table(e, e->h_maint, n_tables, T, data, "gpf_upload_maintenance");
}

int gpf_upload_outage_durations(gpf_handle e, int32_t n_tables, int32_t T, const uint16_t* data) {
  if (!e) return fail(GPF_E_INVALID, "gpf_upload_outage_durations: null");
  if (!data) { e->h_outage_dur.clear(); return upload_outage_tables(e); }
  if (n_tables != e->chron_tables || T != e->chron_T)
    return fail(GPF_E_INVALID, "gpf_upload_outage_durations: shape must match the uploaded chronics tables (n_tables, T)");
  e->h_outage_dur.assign(data, data + (size_t)n_tables * T * e->g.n_line);
  return upload_outage_tables(e);
}

int gpf_upload_hazards(gpf_handle e, int32_t n_tables, int32_t T, const uint8_t* data) {
  if (!e) return fail(GPF_E_INVALID, "gpf_upload_hazards: null");
  return set_outage_table(e, e->h_hazard, n_tables, T, data, "gpf_upload_hazards");
}

int gpf_set_lane_chronics(gpf_handle e, const int32_t* lane_table, const int32_t* lane_offset, const float* lane_scale) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_lane_chronics: null");
  HIP_TRY(hipSetDevice(e->device));
  const size_t B = e->n_lanes;
  if (lane_table) {
    for (size_t k = 0; k < B; ++k)
      if (lane_table[k] < 0 || (e->chron_tables && lane_table[k] >= e->chron_tables)) return fail(GPF_E_INVALID, "lane_table out of range");
    HIP_TRY(hipMemcpyAsync(e->lane_table.p, lane_table, B * sizeof(int), hipMemcpyHostToDevice, e->stream));
    std::copy(lane_table, lane_table + B, e->h_lane_table.begin());
  }
  if (lane_offset) {
    HIP_TRY(hipMemcpyAsync(e->lane_offset.p, lane_offset, B * sizeof(int), hipMemcpyHostToDevice, e->stream));
    std::copy(lane_offset, lane_offset + B, e->h_lane_offset.begin());
    std::fill(e->h_lane_forecast.begin(), e->h_lane_forecast.end(), 0);       // every lane is back on the chronics tables
    std::fill(e->h_lane_n1.begin(), e->h_lane_n1.end(), 0);
    if (e->cur_on) HIP_TRY(cursor_mark_lanes(e, 0, e->cap_lanes, 0));
    if (e->fan.on(FanOwner::n1_screen)) { int rc_n = fan_mark_lanes(e, e->h_lane_n1, 1); if (rc_n != GPF_OK) return rc_n; }   // (the screen's contingency lanes stay what they are)
    if (e->fan.on(FanOwner::lookahead)) { int rc_l = la_mark_lanes(e); if (rc_l != GPF_OK) return rc_l; }   // (... and the look-ahead's scratch lanes)
  }
  if (lane_scale) {
    if (!e->lane_scale.p) {
      HIP_TRY(e->lane_scale.alloc((size_t)e->cap_lanes * 2 * e->g.n_load));
      HIP_TRY(hipMemsetAsync(e->lane_scale.p, 0, (size_t)e->cap_lanes * 2 * e->g.n_load * sizeof(float), e->stream));
    }
    HIP_TRY(hipMemcpyAsync(e->lane_scale.p, lane_scale, B * 2 * e->g.n_load * sizeof(float), hipMemcpyHostToDevice, e->stream));
    e->has_scale = true;
  } else {
    e->has_scale = false;
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_set_thermal_limits(gpf_handle e, const float* limit_a) {
  if (!e || !limit_a) return fail(GPF_E_INVALID, "gpf_set_thermal_limits: null");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(e->thermal_limit.p, limit_a, e->g.n_line * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

}  // extern "C"
namespace {
// the kernel's launch arguments of a step launch with these options (kept state: filled in by step_range)
gpf::StepArgs make_step_args(const gpf_step_opts* o, int lane0, int t0, int T, int n_steps) {
  gpf::StepArgs sa{};
  sa.t = t0; sa.T = T; sa.rebalance_on = o->rebalance > 0.0 ? 1 : 0; sa.rebalance = o->rebalance; sa.cascade = o->cascade;
  sa.is_dc = o->is_dc ? 1 : 0; sa.n_steps = n_steps; sa.auto_reset = o->auto_reset ? 1 : 0; sa.warm_start = o->warm_start ? 1 : 0;
  sa.nb_ts_allowed = o->nb_ts_allowed; sa.max_rounds = o->max_rounds; sa.hard_overflow = o->hard_overflow; sa.soft_overflow = o->soft_overflow;
  sa.nb_ts_reco = o->track_cooldown ? std::max(o->nb_ts_reco, 0) : -1;      // (kernel side: < 0 = the counters are not maintained)
  sa.lane0 = lane0;
  return sa;
}

// n_steps env steps of lanes [lane0, lane0 + n) from time index t0 (T rows per chronics table in `b.chron`)
int step_range(gpf_engine* e, const gpf::Bufs& b_in, int lane0, int n, int t0, int T, int n_steps, const gpf_step_opts* o, const char* who,
               bool keep_state = false, const LaunchPlan* pre_p = nullptr, const LaunchPlan* pre_pb = nullptr) {
  LaunchPlan p, pb;
  int rc = GPF_OK;
  if (pre_p) { p = *pre_p; pb = *pre_pb; }                // (the N-1 screen's plan of the environment lanes, lane lists of its own)
  else rc = plan_launch(e, lane0, n, p, pb);
  if (rc != GPF_OK) return rc;
  if (e->env_on) {
    const int lanes = p.wpi > 1 ? 64 : 64 / std::max(p.ipw, 1);
    if (e->g.n_gen > lanes || e->g.n_sto > lanes || pb.sparse_nb || p.sparse_nb != 1)
      return fail(GPF_E_CAPACITY, std::string(who) + ": the environment dynamics need n_gen and n_storage <= the lanes of an instance (16 / 32 / 64) "
                                  "and a batch that runs as one launch");
  }
  gpf::Bufs b = b_in;
  b.work = e->work.p;                 // (developer timing build: the stamp buffer is allocated by the planner)
  if (n_steps > 1 && pb.sparse_nb)
    return fail(GPF_E_INVALID, std::string(who) + ": multi-step launches need a batch that runs as ONE launch (mixed split / unsplit lanes "
                               "without topology classes run as two): use n_steps = 1");
  if (o->cascade != 0 || b.maint != nullptr) e->dev_topo_dirty = true;     // (lines tripped / taken out by the kernel: see gpf_ptdf_build_batch)
  gpf::StepArgs sa = make_step_args(o, lane0, t0, T, n_steps);
  // one-step launches of the engine's own lanes share the topology-derived state of the reference topology (gpf::KeepArgs): single-busbar
  // kernels only (the split lanes of a mixed batch -- topology classes, NB = 2 -- rebuild theirs).  The key is the pristine (ghost) lane's rows.
  if (keep_state && e->keep_enabled && n_steps == 1 && p.sparse_nb == 1 && !p.tc && !o->is_dc) {        // (a DC step builds no Ybus blocks)
    if (!e->keep.p) {
      gpf::KeepArgs k{};
      gpf::keep_layout(k, e->g, e->sym.nslot, e->sym.nslot_y, e->sym_dev.n_up);
      const size_t bytes = 2 * (size_t)k.stride;
      const gpf::OutOff& oo = e->oo;
      if (e->cap_lanes > e->n_lanes && e->keep.alloc(bytes) == hipSuccess) {
        HIP_TRY(hipMemsetAsync(e->keep.p, 0, bytes, e->stream));
        const size_t gl = (size_t)e->n_lanes;                   // first ghost lane: the state every lane is reset to, never mutated
        const int keyed = gpf::KEEP_KEYED;
        for (int v = 0; v < 2; ++v) {
          unsigned char* kb = e->keep.p + (size_t)v * (size_t)k.stride;
          int* kt = reinterpret_cast<int*>(kb) + gpf::KEEP_HDR_INTS;
          HIP_TRY(hipMemcpyAsync(kt, e->topo.p + gl * e->g.dim_topo, (size_t)e->g.dim_topo * sizeof(int), hipMemcpyDeviceToDevice, e->stream));
          if (e->g.n_shunt) {
            HIP_TRY(hipMemcpyAsync(kt + e->g.dim_topo, e->shunt_bus.p + gl * e->g.n_shunt, (size_t)e->g.n_shunt * sizeof(int), hipMemcpyDeviceToDevice, e->stream));
            HIP_TRY(hipMemcpyAsync(kb + k.off_kd, e->inj.p + gl * e->g.n_inj + oo.inj_sh_p, 2 * (size_t)e->g.n_shunt * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
          }
          HIP_TRY(hipMemcpyAsync(kb, &keyed, sizeof(int), hipMemcpyHostToDevice, e->stream));
        }
        HIP_TRY(hipStreamSynchronize(e->stream));               // (`keyed` is on this frame)
        k.p = e->keep.p;
        e->keep_args = k;
      } else { (void)hipGetLastError(); e->keep.release(); e->keep_enabled = false; }
    }
    if (e->keep.p) { sa.keep = e->keep_args; sa.keep.launch = ++e->keep_launch; }
  }
  const double tol_pu = o->tol_mva / e->g.sn_mva;
  hipEvent_t ea = nullptr, eb = nullptr;
  rc = upload_params_s(e, b, p.tc ? &p : (pb.tc ? &pb : nullptr), p.dcf);
  if (rc != GPF_OK) return rc;
  if (e->profiling) { rc = prof_begin(e, ea, eb); if (rc != GPF_OK) return rc; }
  p.env = pb.env = e->env_on;
  p.jit = pb.jit = jit_for_launch(e);
  int n_disp = 0;
  HIP_TRY(gpf_launch_step_sparse(p, e->device, e->d_params_s.p, e->h_params_s, e->stream, n, o->max_iter, tol_pu, sa, &n_disp));
  if (pb.sparse_nb) HIP_TRY(gpf_launch_step_sparse(pb, e->device, e->d_params_s.p, e->h_params_s, e->stream, n, o->max_iter, tol_pu, sa, &n_disp));
  e->n_step_calls += 1; e->n_step_dispatches += n_disp;
  HIP_TRY(hipGetLastError());
  if (e->profiling) HIP_TRY(hipEventRecord(eb, e->stream));
  if (e->window) { ++e->win_launches; e->win_marked = false; }
  return GPF_OK;
}

// _BackendAction.__iadd__ restricted to topology on one topology row (gridpf_topo.hpp: the implementation the device path shares)
void apply_topo_action(const gpf_engine* e, int* row, int* sb, const int* last, const int32_t* items, int n_items) {
  static thread_local std::vector<int> or_before, ex_before;
  or_before.resize(std::max(e->g.n_line, 1)); ex_before.resize(std::max(e->g.n_line, 1));
  const gpf::TopoMaps m{e->h_line_or_pos.data(), e->h_line_ex_pos.data(), e->g.n_line};
  gpf::apply_topo_action(m, row, sb, last, items, n_items, or_before.data(), ex_before.data(), 0, 1, gpf::NoSync{});
}
}  // namespace

// gpf_simulate_batch stage 3 and the look-ahead: simulate_prepare_kernel on the engine's stream
int simulate_prepare(gpf_engine* e, const int* src_lanes_dev, int n_act, int n_dst, int dst0, int t_obs, int time_step) {
  const bool fc = time_step > 0;
  if (e->has_scale && !e->lane_scale.p) return fail(GPF_E_INVALID, "gpf_simulate_batch: internal (lane_scale)");
  hipLaunchKernelGGL(gpf::simulate_prepare_kernel, dim3((unsigned)n_dst), dim3(64), 0, e->stream, e->g, e->bufs(), src_lanes_dev, n_act, n_dst,
                     dst0, t_obs, e->chron_T, fc ? e->fc_h : 1, time_step, e->lane_table.p, e->lane_offset.p,
                     e->has_scale ? e->lane_scale.p : nullptr, e->has_delta ? e->lane_gen_delta.p : nullptr);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

// gpf_simulate_batch stage 4 and the look-ahead: ONE step of scratch lanes [lane0, lane0 + n) on the chronics (time_step 0) or forecast
// tables (no trajectory rows: these are scratch lanes).  With the injection dynamics on it is ONE do-nothing step of the dynamics (the
// candidates are topology actions: no redispatch / storage part): pending injection actions are set aside for the duration of the call.
int simulate_step(gpf_engine* e, int lane0, int n, int time_step, const gpf_step_opts* o, const char* who, const LaunchPlan* pre_p, const LaunchPlan* pre_pb) {
  struct ActGuard {
    gpf_engine* e; bool r, s, c;
    explicit ActGuard(gpf_engine* e_) : e(e_), r(e_->env_act_r), s(e_->env_act_s), c(e_->env_act_c) { e->env_act_r = e->env_act_s = e->env_act_c = false; }
    ~ActGuard() { e->env_act_r = r; e->env_act_s = s; e->env_act_c = c; }
  } act_guard(e);
  const bool fc = time_step > 0;
  gpf::Bufs b = e->bufs();
  if (fc) b.chron = e->forecast.p;
  b.maint = nullptr;
  b.maint_dur = nullptr;               // (the cursor of a scratch lane is a row of the FORECAST tables: the outage tables have no such rows)
  b.traj_rho = nullptr; b.traj_status = nullptr; b.traj_out = nullptr; b.traj_topo = nullptr; b.traj_shb = nullptr; b.traj_lstat = nullptr; b.traj_cap = 0;
  gpf_step_opts oo = *o;
  oo.auto_reset = 0; oo.warm_start = 0;
  oo.track_cooldown = 0;               // one look-ahead step: the cooldowns copied from the source lanes stand
  return step_range(e, b, lane0, n, 0, fc ? e->chron_T * e->fc_h : e->chron_T, 1, &oo, who, false, pre_p, pre_pb);
}
extern "C" {

// The launch-feature word (gridpf_host.hpp: gpf_step_features) of a DESCRIBED gpf_step_n launch over all lanes of the engine: the engine's
// own state, plus the optional inputs `have` says the launch will have (a header-only handle has none of its own).  No device needed.
int gpf_jit_feature_word(gpf_handle e, int32_t n_steps, const gpf_step_opts* o, uint32_t have, uint32_t* word) {
  if (!e || !o || !word || n_steps <= 0) return fail(GPF_E_INVALID, "gpf_jit_feature_word: null / n_steps must be positive");
  LaunchPlan p, pb;
  int rc = plan_launch(e, 0, e->n_lanes, p, pb);
  if (rc != GPF_OK) return rc;
  gpf::DevParamsS hp{};
  hp.b = e->bufs();
  hp.dcf = p.dcf;
  gpf::Bufs& b = hp.b;
  auto some = [](auto*& q) { if (!q) q = reinterpret_cast<std::remove_reference_t<decltype(q)>>(uintptr_t(64)); };   // (never dereferenced: only null or not)
  if (have & GPF_HAVE_LANE_SCALE) some(b.lane_scale);
  if (have & GPF_HAVE_OUTAGES) { some(b.maint); some(b.maint_dur); }
  if (have & GPF_HAVE_GEN_DELTA) some(b.lane_gen_delta);
  if (have & GPF_HAVE_TRAJ_OBS) {
    some(b.traj_out); some(b.traj_topo); some(b.traj_shb); some(b.traj_lstat); some(b.traj_rho); some(b.traj_status);
    b.traj_cap = std::max(b.traj_cap, (int)n_steps);
  }
  gpf::StepArgs sa = make_step_args(o, 0, 0, std::max(e->chron_T, 1), n_steps);
  // (the kept state of the reference topology: what step_range decides for gpf_step_n)
  if (e->keep_enabled && n_steps == 1 && p.sparse_nb == 1 && !p.tc && !o->is_dc && e->cap_lanes > e->n_lanes) some(sa.keep.p);
  *word = gpf_step_features(sa, hp, p.n_list ? p.list : nullptr, p.n_list ? p.n_list : e->n_lanes, std::max(p.ipw, 1));
  return GPF_OK;
}

int gpf_step_n(gpf_handle e, int32_t t0, int32_t n_steps, const gpf_step_opts* o) {
  if (!e || !o) return fail(GPF_E_INVALID, "gpf_step_n: null");
  if (n_steps <= 0) return fail(GPF_E_INVALID, "gpf_step_n: n_steps must be positive");
  if ((e->ep_on || e->ep_host_on) && n_steps != 1)
    return fail(GPF_E_INVALID, "gpf_step_n: with an episode limit set (gpf_set_episode_limit) a launch must be a one-step launch (an episode "
                               "ends, and a truncated lane restarts, between two steps): use n_steps = 1");
  if ((e->cur_on || e->cur_host_on) && n_steps != 1)
    return fail(GPF_E_INVALID, "gpf_step_n: with the chronics cursor on (gpf_set_chronics_cursor) a launch must be a one-step launch (a lane "
                               "that restarts inside a launch would start a scenario there): use n_steps = 1");
  if (e->fan.owned_by(FanOwner::n1_screen) && n_steps != 1)
    return fail(GPF_E_INVALID, "gpf_step_n: with the N-1 screen on (gpf_set_n1_screen) a launch must be a one-step launch (the contingencies "
                               "are those of the state one step leaves): use n_steps = 1");
  if (e->fan.owned_by(FanOwner::lookahead) && n_steps != 1)
    return fail(GPF_E_INVALID, "gpf_step_n: with the look-ahead set (gpf_set_lookahead) a launch must be a one-step launch (the scratch lanes "
                               "behind the environments are not stepped): use n_steps = 1");
  if (!e->chron.p || e->chron_T <= 0) return fail(GPF_E_INVALID, "gpf_step_n: no chronics uploaded");
  if (e->traj_cap && n_steps > e->traj_cap)
    return fail(GPF_E_INVALID, "gpf_step_n: n_steps exceeds the trajectory buffer (gpf_set_trajectory sizes it; 0 releases it)");
  const bool acts = e->ta_on && (e->ta_host || e->ta_dev);
  if (acts && n_steps != 1)
    return fail(GPF_E_INVALID, "gpf_step_n: a launch that carries topology actions must be a one-step launch (the line-cooldown rule needs the "
                               "action step's trips and outages): use n_steps = 1");
  if (acts && e->ta_rules.cd_line > 0 && !o->track_cooldown)
    return fail(GPF_E_INVALID, "gpf_step_n: topology actions with cooldown_line > 0 need gpf_step_opts::track_cooldown (the agents' line "
                               "cooldowns are only counted down by a launch that maintains the line cooldowns)");
  if (e->ta_on && e->ta_n_moved > 0 && o->auto_reset && n_steps != 1)
    return fail(GPF_E_INVALID, "gpf_step_n: auto-reset in a multi-step launch while topology actions keep lanes on another topology class than "
                               "their reset topology (the launch plan cannot follow a reset inside the launch): use n_steps = 1, or send the "
                               "lanes' rows with gpf_set_topology / gpf_reset_lanes");
  const bool inj = e->env_on && (e->env_act_r || e->env_act_s || e->env_act_c);
  const bool comb = e->cb_on && e->env_on && e->ta_on && n_steps == 1;      // combined mode (gpf_set_combined_actions): gridpf_combined.hpp
  if (acts && inj && !e->cb_on)
    return fail(GPF_E_INVALID, "gpf_step_n: topology actions and injection actions (redispatch / storage / curtailment) are pending for the same "
                               "launch: combined actions are not supported (in the reference the illegality of either part cancels both) unless "
                               "gpf_set_combined_actions turned them on");
  if (acts && inj && e->env_hold && e->env_act_s)
    return fail(GPF_E_INVALID, "gpf_step_n: a held storage action (hold_storage) and topology actions are pending for the same launch: a combined "
                               "action cannot suppress one step of a held action; send the storage power at every step");
  if (e->cb_on && inj && n_steps != 1)
    return fail(GPF_E_INVALID, "gpf_step_n: in combined mode (gpf_set_combined_actions) a launch that carries injection actions must be a one-step "
                               "launch (the actions are screened once, in front of the step): use n_steps = 1");
  if (e->opp_kind && n_steps != 1)
    return fail(GPF_E_INVALID, "gpf_step_n: with an opponent set (gpf_set_opponent) a launch must be a one-step launch (the opponent's choice "
                               "needs the previous step's rho and line status): use n_steps = 1");
  if (e->opp_kind && !o->track_cooldown)
    return fail(GPF_E_INVALID, "gpf_step_n: an opponent (gpf_set_opponent) needs gpf_step_opts::track_cooldown (the attacked line's cooldown is "
                               "only counted down by a launch that maintains the line cooldowns)");
  HIP_TRY(hipSetDevice(e->device));
  int rc = GPF_OK;
  const bool n1 = e->fan.on(FanOwner::n1_screen);
  if (e->cur_on) {                          // first: every kernel behind it reads the scenario of a lane that starts an episode
    rc = cursor_prestep(e, t0);
    if (rc != GPF_OK) return rc;
  }
  if (comb && inj) {                        // in front of the pre-step: the storage units' busbars before the action
    rc = combined_screen(e, acts, e->ta_rules.on);
    if (rc != GPF_OK) return rc;
  }
  if (e->ta_on) {
    if (acts) { e->ta_host = e->ta_dev = false; e->dev_topo_dirty = true; }   // consumed by this launch, whatever happens below
    rc = topo_prestep(e, acts);
    if (rc != GPF_OK) return rc;
  }
  if (comb && inj && acts) {                // a verdict of either part leaves no injection action (without topology actions the screen did it)
    rc = combined_cancel(e, acts);
    if (rc != GPF_OK) return rc;
  }
  if (e->opp_kind) {                        // after the agent's action, before the step: the attack wins
    rc = opponent_prestep(e);
    if (rc != GPF_OK) return rc;
  }
  if (e->al_on) {                           // after the opponent, before the power flow (baseEnv.py:3295)
    rc = alert_prestep(e);
    if (rc != GPF_OK) return rc;
  }
  if (e->rw_on && e->env_on && n_steps == 1) {   // the cancelled-redispatch counters before the step: their change is the step's flag
    rc = reward_prestep(e);
    if (rc != GPF_OK) return rc;
  }
  if (e->fan.on()) {                        // only the environment lanes are stepped, on the fan's cached plan (the secondary lanes are their owner's)
    rc = n1 ? n1_plans(e) : fan_plans(e);
    if (rc != GPF_OK) return rc;
    rc = step_range(e, e->bufs(), 0, e->fan.n_env, t0, e->chron_T, n_steps, o, "gpf_step_n", true, &e->fan.env.p, &e->fan.env.pb);
  } else {
    rc = step_range(e, e->bufs(), 0, e->n_lanes, t0, e->chron_T, n_steps, o, "gpf_step_n", true);
  }
  if (rc != GPF_OK) return rc;
  // lanes an action moved to another class than their reset topology's: an auto-reset puts them back, the host re-keys them (with an
  // episode limit set the truncated lanes join the list, and it is read back once, behind episode_kernel)
  const bool list_resets = e->ta_on && o->auto_reset && e->ta_n_moved > 0;
  if (comb) {                               // a redispatch the step cancelled books nothing for the action; the step's flags
    rc = combined_settle(e, acts, inj);
    if (rc != GPF_OK) return rc;
  }
  if (e->ta_on) {                           // the cooldowns and last known busbars the step leaves
    rc = topo_poststep(e, acts, n_steps, list_resets);
    if (rc != GPF_OK) return rc;
    // (the screen plans its contingency lanes on the classes of the rows the step left: the lanes that auto-reset are re-keyed in front
    //  of it; behind episode_kernel the list is read again, with the truncated lanes -- a lane noted twice has not changed the second time)
    if (list_resets && (!e->ep_on || n1)) { rc = topo_readback(e, false); if (rc != GPF_OK) return rc; }
  }
  if (n1) {                                 // N1Reward's copies: behind the step and what the topology post-step leaves, in front of the
    rc = n1_screen(e, o->max_iter, o->tol_mva);   // rewards (GPF_RW_N1 reads the table) and of episode_kernel (it resets truncated lanes)
    if (rc != GPF_OK) return rc;
  }
  if (e->al_on) {                           // the reward of the step, on its done flag
    rc = alert_poststep(e);
    if (rc != GPF_OK) return rc;
  }
  if (e->rw_on && n_steps == 1) {           // the rewards of the step, last: on its results, done flag and flags
    rc = reward_poststep(e, acts, comb);
    if (rc != GPF_OK) return rc;
  }
  if (e->ep_on) {                           // the episode's end, behind everything that reads the final step's state
    rc = episode_poststep(e, o->auto_reset != 0, o->track_cooldown != 0, list_resets);
    if (rc != GPF_OK) return rc;
    if (list_resets) { rc = topo_readback(e, false); if (rc != GPF_OK) return rc; }
  }
  e->traj_valid = e->traj_cap ? n_steps : 0;
  e->last_t0 = t0; e->last_n_steps = n_steps; e->last_track_cooldown = o->track_cooldown != 0;
  if (e->env_on) {                          // the actions were consumed by this launch (a held storage action stays)
    // (the kernels only read an action buffer whose flag is set -- EnvDyn::act_* is NULL otherwise --, so "consumed" is the flag: no
    //  clearing dispatch behind every launch of an agent that acts at every step)
    e->env_act_r = false;
    if (!e->env_hold) e->env_act_s = false;
    e->env_act_c = false;                   // (the curtailment limits live on in the lanes' state)
  }
  return GPF_OK;
}

int gpf_upload_forecasts(gpf_handle e, int32_t n_tables, int32_t T, int32_t n_horizons, const float* data) {
  if (!e) return fail(GPF_E_INVALID, "gpf_upload_forecasts: null");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->forecast.release(); e->fc_h = 0;
  if (!data) return GPF_OK;
  if (n_horizons <= 0 || n_tables != e->chron_tables || T != e->chron_T)
    return fail(GPF_E_INVALID, "gpf_upload_forecasts: shape must match the uploaded chronics tables (n_tables, T), n_horizons >= 1");
  HIP_TRY(e->forecast.upload(data, (size_t)n_tables * T * n_horizons * e->g.n_chron));
  e->fc_h = n_horizons;
  return GPF_OK;
}

int gpf_simulate_batch(gpf_handle e, int32_t t_obs, int32_t time_step, int32_t n_src, const int32_t* src_lanes, int32_t n_act,
                       const int32_t* act_off, const int32_t* act_items, const int32_t* last_bus, int32_t dst_lane0,
                       const gpf_step_opts* o) {
  if (!e || !o || !src_lanes || !act_off || n_src <= 0 || n_act <= 0) return fail(GPF_E_INVALID, "gpf_simulate_batch: bad arguments");
  if (!e->chron.p || e->chron_T <= 0) return fail(GPF_E_INVALID, "gpf_simulate_batch: no chronics uploaded");
  if (time_step < 0 || (time_step > 0 && (!e->forecast.p || time_step > e->fc_h)))
    return fail(GPF_E_INVALID, "gpf_simulate_batch: no forecast for that horizon (gpf_upload_forecasts; NoForecastAvailable in the reference)");
  const gpf::GridDev& g = e->g;
  const long long n_dst = (long long)n_src * n_act;
  if (n_dst > e->n_lanes || !check_range(e, dst_lane0, (int)n_dst)) return fail(GPF_E_INVALID, "gpf_simulate_batch: destination range out of bounds");
  for (int b = 0; b < n_src; ++b)
    if (src_lanes[b] < 0 || src_lanes[b] >= e->n_lanes || (src_lanes[b] >= dst_lane0 && src_lanes[b] < dst_lane0 + n_dst))
      return fail(GPF_E_INVALID, "gpf_simulate_batch: source lane out of range or inside the destination range");
  for (int b = 0; b < n_src; ++b)
    if (e->h_lane_forecast[src_lanes[b]])
      return fail(GPF_E_INVALID, "gpf_simulate_batch: a source lane is itself a scratch lane of an earlier gpf_simulate_batch (its chronics cursor is an "
                                 "absolute row, of the forecast tables when it simulated a forecast): chained simulate is not supported -- simulate from "
                                 "the environment's lane, or send gpf_set_lane_chronics again");
  const int n_items_total = act_off[n_act];
  if (act_off[0] != 0 || (n_items_total > 0 && !act_items)) return fail(GPF_E_INVALID, "gpf_simulate_batch: bad action offsets");
  for (int k = 0; k < n_act; ++k) if (act_off[k + 1] < act_off[k]) return fail(GPF_E_INVALID, "gpf_simulate_batch: bad action offsets");
  if (int rc_i = check_action_items(e, "gpf_simulate_batch", n_items_total, act_items, nullptr)) return rc_i;
  HIP_TRY(hipSetDevice(e->device));
  static const bool sim_timing = getenv("GRIDPF_SIM_TIMING") != nullptr;        // developer: stage times of the call on stderr
  auto now_us = [] { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() * 1e-3; };
  const double tm0 = sim_timing ? now_us() : 0.0;
  // 1. the source lanes' topology / shunt rows as they are on the device NOW (trips and maintenance included) -> host
  const int w = g.dim_topo + g.n_shunt;
  if (e->sim_src.n < (size_t)n_src) HIP_TRY(e->sim_src.alloc((size_t)n_src));
  if (e->sim_rows.n < (size_t)n_src * w) HIP_TRY(e->sim_rows.alloc((size_t)n_src * w));
  HIP_TRY(hipMemcpyAsync(e->sim_src.p, src_lanes, (size_t)n_src * sizeof(int), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(gpf::gather_topo_kernel, dim3(n_src), dim3(64), 0, e->stream, e->g, e->bufs(), e->sim_src.p, n_src, e->sim_rows.p);
  HIP_TRY(hipGetLastError());
  // one pinned host block for the rows that cross PCIe in this call (true DMA both ways, no zero-filled vectors): the gathered source
  // rows, then the candidate topology / shunt rows.  It is only rewritten after the synchronisation below, i.e. when the uploads of
  // the previous call have long been consumed.
  const size_t n_rows = (size_t)n_src * w, n_topo = (size_t)n_dst * g.dim_topo, n_sb = (size_t)n_dst * std::max(g.n_shunt, 1);
  if (e->sim_pin.n < n_rows + n_topo + n_sb) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(e->sim_pin.reserve(n_rows + n_topo + n_sb));
  }
  int* const rows = e->sim_pin.p;
  HIP_TRY(hipMemcpyAsync(rows, e->sim_rows.p, n_rows * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (e->cur_on) HIP_TRY(cursor_fetch_mirrors(e));     // the device moved the lanes' cursors: the mirrors below are read back, not remembered
  HIP_TRY(hipStreamSynchronize(e->stream));
  const double tm1 = sim_timing ? now_us() : 0.0;
  // 2. candidate topologies on the host (the launch planner needs them anyway: busbars per substation, topology classes)
  int* const topo = e->sim_pin.p + n_rows;
  int* const sb = topo + n_topo;
  // Scheduled maintenance ahead of the observation (_ObsEnv.init, Environment/_obsEnv.py:361-385 with
  // BaseEnv._update_vector_with_timestep, baseEnv.py:4768-4825): a forecast `time_step` >= 1 steps ahead has the lines out whose
  // NEXT maintenance (the one obs.time_next_maintenance / duration_next_maintenance describe: the first flagged row from the
  // observation's row on) covers row idx + time_step -- it begins there (first_ts_maintenance) or is under way
  // (still_in_maintenance): la_maintenance_ahead, gridpf_lookahead.hpp.  Hazards are not forecast by the reference.  The line goes out
  // BEFORE the candidate action is applied.
  std::vector<std::vector<int>> maint_out(n_src);
  if (time_step >= 1 && !e->h_maint.empty()) {
    const int T = e->chron_T;
    for (int b = 0; b < n_src; ++b) {
      const int src = src_lanes[b];
      int idx = (t_obs + e->h_lane_offset[src]) % T;
      if (idx < 0) idx += T;
      const unsigned char* M = e->h_maint.data() + (size_t)e->h_lane_table[src] * T * g.n_line;
      for (int l = 0; l < g.n_line; ++l)
        if (gpf::la_maintenance_ahead(M, T, g.n_line, idx, time_step, l)) maint_out[b].push_back(l);
    }
  }
  for (int b = 0; b < n_src; ++b)
    for (int k = 0; k < n_act; ++k) {
      int* row = topo + ((size_t)b * n_act + k) * g.dim_topo;
      int* srow = sb + ((size_t)b * n_act + k) * std::max(g.n_shunt, 1);
      std::memcpy(row, rows + (size_t)b * w, (size_t)g.dim_topo * sizeof(int));
      if (g.n_shunt) std::memcpy(srow, rows + (size_t)b * w + g.dim_topo, (size_t)g.n_shunt * sizeof(int));
      for (int l : maint_out[b]) { row[e->h_line_or_pos[l]] = -1; row[e->h_line_ex_pos[l]] = -1; }
      apply_topo_action(e, row, g.n_shunt ? srow : nullptr, last_bus ? last_bus + (size_t)b * g.dim_topo : nullptr,
                        act_items + 3 * (size_t)act_off[k], act_off[k + 1] - act_off[k]);
    }
  const double tm2 = sim_timing ? now_us() : 0.0;
  int rc = set_topology_rows(e, dst_lane0, (int)n_dst, topo, g.n_shunt ? sb : nullptr, true);
  if (rc != GPF_OK) return rc;
  const double tm3 = sim_timing ? now_us() : 0.0;
  // 3. everything else of the source lanes + the chronics / forecast row to step on, on the device
  const bool fc = time_step > 0;
  rc = simulate_prepare(e, e->sim_src.p, n_act, (int)n_dst, dst_lane0, t_obs, time_step);
  if (rc != GPF_OK) return rc;
  for (long long q = 0; q < n_dst; ++q) {                     // host mirror of what the kernel writes
    const int src = src_lanes[q / n_act];
    int idx = (t_obs + e->h_lane_offset[src]) % e->chron_T;
    if (idx < 0) idx += e->chron_T;
    e->h_lane_table[dst_lane0 + q] = e->h_lane_table[src];
    e->h_lane_offset[dst_lane0 + q] = time_step == 0 ? idx : (fc ? e->fc_h : 1) * idx + (time_step - 1);
    e->h_lane_forecast[dst_lane0 + q] = 1;          // its cursor is an ABSOLUTE row (of the forecast tables when time_step > 0), not an offset to t
  }
  if (e->cur_on) HIP_TRY(cursor_mark_lanes(e, dst_lane0, (int)n_dst, 1));
  if (e->env_on) { rc = env_copy_from(e, e->sim_src.p, n_act, (int)n_dst, dst_lane0); if (rc != GPF_OK) return rc; }
  // 4. ONE step of the destination range on the forecast tables
  const double tm4 = sim_timing ? now_us() : 0.0;
  rc = simulate_step(e, dst_lane0, (int)n_dst, time_step, o, "gpf_simulate_batch", nullptr, nullptr);
  if (sim_timing)
    fprintf(stderr, "[gridpf] simulate_batch %lld lanes: gather + sync %.0f us, candidate rows %.0f, gpf_set_topology %.0f, prepare + mirror %.0f, plan + launch %.0f\n",
            n_dst, tm1 - tm0, tm2 - tm1, tm3 - tm2, tm4 - tm3, now_us() - tm4);
  return rc;
}

int gpf_step(gpf_handle e, int32_t t, int32_t max_iter, double tol_mva, double rebalance, int32_t cascade, float hard_overflow,
             float soft_overflow, int32_t nb_ts_allowed, int32_t max_rounds, int32_t is_dc) {
  gpf_step_opts o{};
  o.max_iter = max_iter; o.tol_mva = tol_mva; o.rebalance = rebalance; o.cascade = cascade; o.hard_overflow = hard_overflow;
  o.soft_overflow = soft_overflow; o.nb_ts_allowed = nb_ts_allowed; o.max_rounds = max_rounds; o.is_dc = is_dc; o.auto_reset = 0; o.warm_start = 0; o.track_cooldown = 0; o.nb_ts_reco = 0;
  return gpf_step_n(e, t, 1, &o);
}

int gpf_set_lane_redispatch(gpf_handle e, const float* delta_mw) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_lane_redispatch: null");
  HIP_TRY(hipSetDevice(e->device));
  if (!delta_mw) { e->has_delta = false; return GPF_OK; }
  const size_t n = (size_t)e->cap_lanes * e->g.n_gen;
  if (!e->lane_gen_delta.p) { HIP_TRY(e->lane_gen_delta.alloc(n)); HIP_TRY(hipMemsetAsync(e->lane_gen_delta.p, 0, n * sizeof(float), e->stream)); }
  HIP_TRY(hipMemcpyAsync(e->lane_gen_delta.p, delta_mw, (size_t)e->n_lanes * e->g.n_gen * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->has_delta = true;
  return GPF_OK;
}

int gpf_set_gen_limits(gpf_handle e, const double* pmin, const double* pmax, const double* ramp_up, const double* ramp_down,
                       const uint8_t* redispatchable, double eps_poly) {
  if (!e || !pmin || !pmax || !ramp_up || !ramp_down || !redispatchable) return fail(GPF_E_INVALID, "gpf_set_gen_limits: null");
  if (e->g.n_gen > gpf::RD_PER_LANE * gpf::WAVE) return fail(GPF_E_CAPACITY, "gpf_set_gen_limits: more than 256 generators");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t ng = e->g.n_gen;
  HIP_TRY(e->rd_pmin.upload(pmin, ng)); HIP_TRY(e->rd_pmax.upload(pmax, ng)); HIP_TRY(e->rd_ru.upload(ramp_up, ng));
  HIP_TRY(e->rd_rd.upload(ramp_down, ng)); HIP_TRY(e->rd_redisp.upload(redispatchable, ng));
  e->rd_eps = eps_poly;
  e->rd_ready = true;
  return GPF_OK;
}

int gpf_redispatch(gpf_handle e, int32_t lane0, int32_t n, const double* new_p, const double* prev_p, const double* actual,
                   const double* target, const uint8_t* modified, const double* rhs, int32_t apply, uint8_t* ok, float* actual_after) {
  if (!check_range(e, lane0, n) || !new_p || !prev_p || !actual || !target || !modified || !rhs)
    return fail(GPF_E_INVALID, "gpf_redispatch: bad arguments");
  if (!e->rd_ready) return fail(GPF_E_INVALID, "gpf_redispatch: call gpf_set_gen_limits first");
  if (n == 0) return GPF_OK;
  HIP_TRY(hipSetDevice(e->device));
  const size_t ng = e->g.n_gen, row = (size_t)n * ng;
  if (e->rd_in.n < 4 * row + (size_t)n) HIP_TRY(e->rd_in.alloc(4 * row + n));
  if (e->rd_u8.n < row + (size_t)n) HIP_TRY(e->rd_u8.alloc(row + n));
  if (e->rd_after.n < row) HIP_TRY(e->rd_after.alloc(row));
  double* d = e->rd_in.p;
  HIP_TRY(hipMemcpyAsync(d, new_p, row * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(d + row, prev_p, row * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(d + 2 * row, actual, row * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(d + 3 * row, target, row * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(d + 4 * row, rhs, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->rd_u8.p, modified, row, hipMemcpyHostToDevice, e->stream));
  float* delta = nullptr;
  if (apply) {
    const size_t nd = (size_t)e->cap_lanes * ng;
    if (!e->lane_gen_delta.p) { HIP_TRY(e->lane_gen_delta.alloc(nd)); HIP_TRY(hipMemsetAsync(e->lane_gen_delta.p, 0, nd * sizeof(float), e->stream)); }
    delta = e->lane_gen_delta.p + (size_t)lane0 * ng;
    e->has_delta = true;
  }
  gpf::RedispDev R{};
  R.n_gen = (int)ng; R.eps_poly = e->rd_eps; R.pmin = e->rd_pmin.p; R.pmax = e->rd_pmax.p; R.ramp_up = e->rd_ru.p; R.ramp_down = e->rd_rd.p;
  R.redispatchable = e->rd_redisp.p;
  hipLaunchKernelGGL(gpf::redispatch_kernel, dim3(n), dim3(gpf::WAVE), 0, e->stream, R, n, d, d + row, d + 2 * row, d + 3 * row, e->rd_u8.p,
                     d + 4 * row, e->rd_u8.p + row, e->rd_after.p, delta);
  HIP_TRY(hipGetLastError());
  if (ok) HIP_TRY(hipMemcpyAsync(ok, e->rd_u8.p + row, (size_t)n, hipMemcpyDeviceToHost, e->stream));
  if (actual_after) HIP_TRY(hipMemcpyAsync(actual_after, e->rd_after.p, row * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_set_trajectory(gpf_handle e, int32_t n_steps_cap, int32_t what) {
  if (!e || n_steps_cap < 0 || (what & ~(GPF_TRAJ_RHO | GPF_TRAJ_OBS))) return fail(GPF_E_INVALID, "gpf_set_trajectory: bad arguments");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->traj_rho.release(); e->traj_status.release(); e->traj_cool.release();
  e->traj_out.release(); e->traj_topo.release(); e->traj_shb.release(); e->traj_lstat.release();
  e->traj_cap = 0; e->traj_what = 0; e->traj_valid = 0;
  if (n_steps_cap > 0 && what) {
    const size_t rows = (size_t)n_steps_cap * e->cap_lanes;
    const gpf::GridDev& g = e->g;
    HIP_TRY(e->traj_rho.alloc(rows * g.n_line));
    HIP_TRY(e->traj_status.alloc(rows));
    HIP_TRY(hipMemset(e->traj_status.p, 0xFF, rows));
    HIP_TRY(e->traj_cool.alloc(rows * g.n_line));                 // line cooldowns of every step (written when the step tracks them)
    HIP_TRY(hipMemset(e->traj_cool.p, 0, rows * g.n_line * sizeof(short)));
    if (what & GPF_TRAJ_OBS) {
      HIP_TRY(e->traj_out.alloc(rows * g.n_out)); HIP_TRY(e->traj_topo.alloc(rows * g.dim_topo));
      HIP_TRY(e->traj_shb.alloc(rows * std::max(g.n_shunt, 1))); HIP_TRY(e->traj_lstat.alloc(rows * g.n_line));
    }
    e->traj_cap = n_steps_cap;
    e->traj_what = what | GPF_TRAJ_RHO;
  }
  return GPF_OK;
}

}  // extern "C"
namespace {
// rows [step0, step0 + n_steps) x lanes [lane0, lane0 + n) of a [cap][cap_lanes][stride] device buffer -> dense host array
template <class T>
int traj_copy(gpf_engine* e, T* dst, const T* src, size_t stride, int step0, int n_steps, int lane0, int n) {
  if (!dst || stride == 0 || n == 0 || n_steps == 0) return GPF_OK;
  const size_t B = e->cap_lanes;
  HIP_TRY(hipMemcpy2DAsync(dst, (size_t)n * stride * sizeof(T), src + ((size_t)step0 * B + lane0) * stride, B * stride * sizeof(T),
                           (size_t)n * stride * sizeof(T), (size_t)n_steps, hipMemcpyDeviceToHost, e->stream));
  return GPF_OK;
}
}  // namespace
extern "C" {

int gpf_get_trajectory(gpf_handle e, int32_t step0, int32_t n_steps, int32_t lane0, int32_t n, float* rho, int8_t* status) {
  if (!check_range(e, lane0, n) || step0 < 0 || n_steps < 0 || step0 + n_steps > e->traj_valid)
    return fail(GPF_E_INVALID, "gpf_get_trajectory: bad range (only the steps of the last gpf_step_n are retrievable)");
  HIP_TRY(hipSetDevice(e->device));
  int rc = traj_copy(e, rho, e->traj_rho.p, (size_t)e->g.n_line, step0, n_steps, lane0, n);
  if (rc == GPF_OK) rc = traj_copy(e, reinterpret_cast<signed char*>(status), e->traj_status.p, 1, step0, n_steps, lane0, n);
  if (rc != GPF_OK) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_trajectory_cooldown(gpf_handle e, int32_t step0, int32_t n_steps, int32_t lane0, int32_t n, int16_t* line_cooldown) {
  if (!check_range(e, lane0, n) || !line_cooldown || step0 < 0 || n_steps < 0 || step0 + n_steps > e->traj_valid || !e->traj_cool.p)
    return fail(GPF_E_INVALID, "gpf_get_trajectory_cooldown: bad range (only the steps of the last gpf_step_n are retrievable)");
  HIP_TRY(hipSetDevice(e->device));
  int rc = traj_copy(e, line_cooldown, e->traj_cool.p, (size_t)e->g.n_line, step0, n_steps, lane0, n);
  if (rc != GPF_OK) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_cooldown(gpf_handle e, int32_t lane0, int32_t n, int32_t* line_cooldown) {
  if (!check_range(e, lane0, n) || !line_cooldown) return fail(GPF_E_INVALID, "gpf_get_cooldown: bad arguments");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(rows_to_host(e, line_cooldown, e->cooldown, e->g.n_line, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_set_cooldown(gpf_handle e, int32_t lane0, int32_t n, const int32_t* line_cooldown) {
  if (!check_range(e, lane0, n) || !line_cooldown) return fail(GPF_E_INVALID, "gpf_set_cooldown: bad arguments");
  for (size_t i = 0; i < (size_t)n * e->g.n_line; ++i) if (line_cooldown[i] < 0) return fail(GPF_E_INVALID, "gpf_set_cooldown: negative counter");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(rows_to_device(e, e->cooldown, line_cooldown, e->g.n_line, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_trajectory_obs(gpf_handle e, int32_t step0, int32_t n_steps, int32_t lane0, int32_t n, float* out, int32_t* topo_vect,
                           int32_t* shunt_bus, uint8_t* line_status) {
  if (!check_range(e, lane0, n) || step0 < 0 || n_steps < 0 || step0 + n_steps > e->traj_valid)
    return fail(GPF_E_INVALID, "gpf_get_trajectory_obs: bad range (only the steps of the last gpf_step_n are retrievable)");
  if (!(e->traj_what & GPF_TRAJ_OBS))
    return fail(GPF_E_INVALID, "gpf_get_trajectory_obs: no observation trajectory (gpf_set_trajectory(.., GPF_TRAJ_OBS))");
  HIP_TRY(hipSetDevice(e->device));
  const gpf::GridDev& g = e->g;
  int rc = traj_copy(e, out, e->traj_out.p, (size_t)g.n_out, step0, n_steps, lane0, n);
  if (rc == GPF_OK) rc = traj_copy(e, topo_vect, e->traj_topo.p, (size_t)g.dim_topo, step0, n_steps, lane0, n);
  if (rc == GPF_OK) rc = traj_copy(e, shunt_bus, e->traj_shb.p, (size_t)g.n_shunt, step0, n_steps, lane0, n);
  if (rc == GPF_OK) rc = traj_copy(e, line_status, e->traj_lstat.p, (size_t)g.n_line, step0, n_steps, lane0, n);
  if (rc != GPF_OK) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_episode(gpf_handle e, int32_t lane0, int32_t n, uint8_t* done, int32_t* steps_and_resets) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_get_episode: bad range");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(rows_to_host(e, done, e->done, 1, lane0, n));
  HIP_TRY(rows_to_host(e, steps_and_resets, e->episode, 2, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_set_overflow_count(gpf_handle e, int32_t lane0, int32_t n, const int32_t* overflow_count) {
  if (!check_range(e, lane0, n) || !overflow_count) return fail(GPF_E_INVALID, "gpf_set_overflow_count: bad arguments");
  for (size_t i = 0; i < (size_t)n * e->g.n_line; ++i) if (overflow_count[i] < 0) return fail(GPF_E_INVALID, "gpf_set_overflow_count: negative counter");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(rows_to_device(e, e->overflow_count, overflow_count, e->g.n_line, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_get_step_outputs(gpf_handle e, int32_t lane0, int32_t n, float* rho, int32_t* overflow_count, int32_t* disc_round) {
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_get_step_outputs: bad range");
  HIP_TRY(hipSetDevice(e->device));
  const size_t nl = e->g.n_line;
  HIP_TRY(rows_to_host(e, rho, e->rho, nl, lane0, n));
  HIP_TRY(rows_to_host(e, overflow_count, e->overflow_count, nl, lane0, n));
  HIP_TRY(rows_to_host(e, disc_round, e->disc_round, nl, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

int gpf_sync(gpf_handle e) {
  if (!e) return fail(GPF_E_INVALID, "gpf_sync: null");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(sync_stream_spin(e->stream));           // (polls for up to GRIDPF_SYNC_SPIN_US before blocking, see sync_stream_spin)
  return GPF_OK;
}

static int close_window(gpf_engine* e) {
  if (!e->window) return GPF_OK;
  if (e->win_launches > 0) {
    if (!e->win_marked) HIP_TRY(hipEventRecord(e->win_b, e->stream));     // (mode 3 already recorded it behind the last launch)
    HIP_TRY(hipEventSynchronize(e->win_b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->win_a, e->win_b));
    e->acc_ms += ms;
    e->acc_launches += e->win_launches;
  }
  e->win_launches = 0;
  e->window = false;
  e->win_marked = false;
  return GPF_OK;
}

static int open_window(gpf_engine* e) {
  if (!e->win_a) { HIP_TRY(e->win_a.create()); HIP_TRY(e->win_b.create()); }
  HIP_TRY(hipEventRecord(e->win_a, e->stream));
  e->win_launches = 0;
  e->window = true;
  e->win_marked = false;
  return GPF_OK;
}

int gpf_set_profiling(gpf_handle e, int32_t mode) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_profiling: null");
  HIP_TRY(hipSetDevice(e->device));
  if (mode == 3) {                      // end of the running window = this point of the stream (asynchronous; read by the next call)
    if (e->window && e->win_launches > 0) { HIP_TRY(hipEventRecord(e->win_b, e->stream)); e->win_marked = true; }
    return GPF_OK;
  }
  int rc = close_window(e);
  if (rc != GPF_OK) return rc;
  e->profiling = mode == 2;
  if (mode == 1) return open_window(e);
  return GPF_OK;
}

int gpf_get_kernel_time(gpf_handle e, double* total_ms, int64_t* n_launches) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_kernel_time: null");
  HIP_TRY(hipSetDevice(e->device));
  int rc = drain_events(e);
  if (rc != GPF_OK) return rc;
  if (e->window) {                      // close the running window and open the next one
    rc = close_window(e);
    if (rc == GPF_OK) rc = open_window(e);
    if (rc != GPF_OK) return rc;
  }
  if (total_ms) *total_ms = e->acc_ms;
  if (n_launches) *n_launches = e->acc_launches;
  e->acc_ms = 0.0;
  e->acc_launches = 0;
  return GPF_OK;
}


#ifdef GPF_TIMING
int gpf_debug_read_work(gpf_handle e, double* out, int64_t n) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, e->work.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return GPF_OK;
}
#endif

int gpf_get_counters(gpf_handle e, int64_t out[2]) {
  if (!e || !out) return fail(GPF_E_INVALID, "gpf_get_counters: null");
  out[0] = e->n_step_calls; out[1] = e->n_step_dispatches;
  return GPF_OK;
}

int gpf_get_plan(gpf_handle e, int32_t out[8]) {
  if (!e || !out) return fail(GPF_E_INVALID, "gpf_get_plan: null");
  LaunchPlan p, pb;
  int rc = plan_launch(e, 0, e->n_lanes, p, pb);
  if (rc != GPF_OK) return rc;
  out[0] = p.sparse_nb; out[1] = p.ipw; out[2] = p.wpi; out[3] = p.sparse_stage; out[4] = p.yreg ? 1 : 0; out[5] = p.dcf;
  out[6] = (int32_t)p.lds; out[7] = p.tc ? 1 : 0;
  return GPF_OK;
}

int gpf_device_pointers(gpf_handle e, void** ptrs, void** stream) { return gpf_device_pointers_n(e, ptrs, GPF_N_DEVICE_POINTERS, stream); }

int gpf_device_pointers_n(gpf_handle e, void** out, int32_t n_ptrs, void** stream) {
  if (!e || !out || n_ptrs < 0) return fail(GPF_E_INVALID, "gpf_device_pointers: null");
  void* ptrs[GPF_N_DEVICE_POINTERS];
  ptrs[32] = e->obs_spec_on ? e->obs_vec.p : nullptr;
  ptrs[33] = e->ta_on && e->ta_n_act ? e->ta_mask.p : nullptr;
  ptrs[0] = e->inj.p; ptrs[1] = e->topo.p; ptrs[2] = e->shunt_bus.p; ptrs[3] = e->out.p; ptrs[4] = e->topo_out.p;
  ptrs[5] = e->line_status.p; ptrs[6] = e->status.p; ptrs[7] = e->chron.p;
  ptrs[8] = e->rho.p; ptrs[9] = e->overflow_count.p; ptrs[10] = e->done.p; ptrs[11] = e->episode.p; ptrs[12] = e->bus_vm.p;
  ptrs[13] = e->bus_va.p; ptrs[14] = e->shunt_bus_out.p; ptrs[15] = e->disc_round.p;
  ptrs[16] = e->traj_cap ? e->traj_rho.p : nullptr; ptrs[17] = e->traj_cap ? e->traj_status.p : nullptr;
  const bool obs = e->traj_cap && (e->traj_what & GPF_TRAJ_OBS);
  ptrs[18] = obs ? e->traj_out.p : nullptr; ptrs[19] = obs ? e->traj_topo.p : nullptr; ptrs[20] = obs ? e->traj_shb.p : nullptr;
  ptrs[21] = obs ? e->traj_lstat.p : nullptr;
  ptrs[22] = e->env_on ? e->env_act_redisp.p : nullptr; ptrs[23] = e->env_on ? e->env_act_storage : nullptr;
  ptrs[24] = e->env_on ? e->env_act_curtail.p : nullptr; ptrs[25] = e->env_on ? e->env_target.p : nullptr;
  ptrs[26] = e->env_on ? e->env_actual.p : nullptr; ptrs[27] = e->env_on ? e->env_charge.p : nullptr;
  ptrs[28] = e->ta_on ? e->ta_act.p : nullptr; ptrs[29] = e->ta_on ? e->ta_sub_cd.p : nullptr;
  ptrs[30] = e->ta_on ? e->ta_flags.p : nullptr; ptrs[31] = e->ta_on ? e->ta_last_bus.p : nullptr;
  for (int i = 0; i < n_ptrs; ++i) out[i] = i < GPF_N_DEVICE_POINTERS ? ptrs[i] : nullptr;     // never writes beyond the caller's array
  if (stream) *stream = e->stream;
  return GPF_OK;
}

}  // extern "C"
