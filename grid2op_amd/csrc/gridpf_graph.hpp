// gridpf_graph.hpp -- the observation as a bus graph, assembled on the device (gpf_set_graph_obs / gpf_graph_obs, include/gridpf.h, where
// the contract is stated).  Paths relative to the reference checkout:
//   live buses, compact ids      BaseObservation._aux_fun_get_bus / _get_bus_id (Observation/baseObservation.py:2081-2118, 2229-2243)
//   index row, dense plane 0     bus_connectivity_matrix(return_lines_index=True) (:2163-2227)
//   node p / q, dense planes 1-2 flow_bus_matrix(active_flow) (:2320-2445)
//   node v                       the overwrite order of get_energy_graph's bus_v (:2690-2695)
// Three parts.  The rule core (plain C++, the ONE statement of every rule: graph_node, graph_elem_bus, graph_pair_flows,
// graph_lane_elements) works on one lane's rows and the static tables; the table builder (graph_build_tab, host) makes those from the
// grid; the executors rank the live buses (a rank among the live buses in ascending global id) and hold the global -> compact map.  The
// kernel ranks with __ballot + popcount over chunks of 64 global ids and keeps the map (and, where they fit, copies of the lane's rows)
// in LDS; graph_lane_serial, the executor of the host emulator of tests/native/, does both with loops.  Every float is a float64 sum in
// a stated order rounded once, stored by the one thread that owns its address: the same bits in every run and at every place in the
// batch.  Without hipcc the kernel does not exist: the header then needs no HIP header.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GPF_GR_HD __host__ __device__
#else
#define GPF_GR_HD
#endif

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

namespace gpf {

constexpr int GR_MAX_BUS = 1024;     // (= GPF_GRAPH_MAX_BUS) NB the kernel's per-wavefront map has room for
constexpr int GR_N_FEAT = 4;         // (= GPF_GRAPH_N_FEATURES) p, q, v, cooldown
constexpr int GR_GEN = 0, GR_LOAD = 1, GR_STO = 2, GR_SHUNT = 3, GR_LOR = 4, GR_LEX = 5;   // element classes, in the order the node sums take them
constexpr int GR_CODE_SHIFT = 24;    // a substation's element: class << 24 | index

// The static tables: one int blob (`t`, on the host or on the device) and the offsets of its arrays.  Everything after `t` is an int:
// the blob starts with a copy of them (graph_tab_view reads it back).
struct GraphTab {
  const int* t;
  int n_sub, n_busbar, n_load, n_gen, n_sto, n_line, n_shunt, dim_topo;
  // substation -> its elements, sorted by class (GR_GEN .. GR_LEX) and index: el_code, el_pos = the element's topo_vect position (a
  // shunt: its index in the shunt row) and, for a line end, el_other = the position of the line's other end (else -1).  One pass over
  // a substation's list therefore meets the terms of a node sum in the stated order, with one round of table reads per element
  int sub_off, el_code, el_pos, el_other;
  int load_pos, load_sub, gen_pos, gen_sub, sto_pos, sto_sub, lor_pos, lor_sub, lex_pos, lex_sub, sh_sub;
  // lines on the same unordered substation pair: line l's group is grp_lines[grp_at[l] .. + grp_n[l]), ascending
  int grp_at, grp_n, grp_lines;
  // columns of the float32 results row
  int o_p_or, o_q_or, o_v_or, o_p_ex, o_q_ex, o_v_ex, o_gen_p, o_gen_q, o_load_p, o_load_q, o_sto_p, o_sh_p, o_sh_q;
  int total;                         // ints in the blob
};
constexpr int GR_HDR_INTS = (int)((sizeof(GraphTab) - offsetof(GraphTab, n_sub)) / sizeof(int));

// one lane's rows; sub_cd null: the engine does not track substation cooldowns
struct GraphRow {
  const int* topo;                   // [dim_topo]
  const int* shunt_bus;              // [n_shunt]
  const float* out;                  // [n_out] results row
  const int* sub_cd;                 // [n_sub] or null
};

GPF_GR_HD inline int graph_nb(const GraphTab& T) { return T.n_sub * T.n_busbar; }
// index row: n_bus | load | gen | storage | line_or | line_ex | shunt | bus_global
GPF_GR_HD inline int graph_index_width(const GraphTab& T) { return 1 + T.n_load + T.n_gen + T.n_sto + 2 * T.n_line + T.n_shunt + graph_nb(T); }

GPF_GR_HD inline bool graph_line_on(const GraphTab& T, const GraphRow& r, int l) {
  return r.topo[T.t[T.lor_pos + l]] > 0 && r.topo[T.t[T.lex_pos + l]] > 0;
}

struct GraphNode { bool live; float f[GR_N_FEAT]; };

// Global bus g = sub + (busbar - 1) * n_sub: whether it is live (it holds an end of a connected line) and its four features.  A gather
// over the elements of the bus's substation.
GPF_GR_HD inline GraphNode graph_node(const GraphTab& T, const GraphRow& r, int g) {
  const int s = g % T.n_sub, b = g / T.n_sub + 1;
  double p = 0.0, q = 0.0;
  int lor = -1, lex = -1;            // highest-index connected line with its origin / extremity here
  for (int e = T.t[T.sub_off + s]; e < T.t[T.sub_off + s + 1]; ++e) {
    const int code = T.t[T.el_code + e], kind = code >> GR_CODE_SHIFT, i = code & ((1 << GR_CODE_SHIFT) - 1), pos = T.t[T.el_pos + e];
    const int other = T.t[T.el_other + e];
    if ((kind == GR_SHUNT ? r.shunt_bus[pos] : r.topo[pos]) != b) continue;
    switch (kind) {
      case GR_GEN: p += (double)r.out[T.o_gen_p + i]; q += (double)r.out[T.o_gen_q + i]; break;
      case GR_LOAD: p -= (double)r.out[T.o_load_p + i]; q -= (double)r.out[T.o_load_q + i]; break;
      case GR_STO: p -= (double)r.out[T.o_sto_p + i]; break;
      case GR_SHUNT: p -= (double)r.out[T.o_sh_p + i]; q -= (double)r.out[T.o_sh_q + i]; break;
      case GR_LOR: if (i > lor && r.topo[other] > 0) lor = i; break;       // (this end is on busbar b > 0: the line is connected)
      default: if (i > lex && r.topo[other] > 0) lex = i; break;
    }
  }
  GraphNode nd;
  nd.live = lor >= 0 || lex >= 0;
  nd.f[0] = (float)p;
  nd.f[1] = (float)q;
  nd.f[2] = !nd.live ? 0.f : lex >= 0 ? r.out[T.o_v_ex + lex] : r.out[T.o_v_or + lor];
  nd.f[3] = r.sub_cd ? (float)r.sub_cd[s] : 0.f;
  return nd;
}

// compact id of the bus an element of substation `sub` on `busbar` sits on, through the executor's map (global id -> compact id, -1: the
// bus is not live); -1 for a disconnected element
template <typename Map>
GPF_GR_HD inline int graph_elem_bus(const GraphTab& T, int sub, int busbar, const Map& map) {
  if (busbar <= 0 || busbar > T.n_busbar) return -1;
  return map(sub + (busbar - 1) * T.n_sub);
}

template <typename Map>
GPF_GR_HD inline int graph_line_end(const GraphTab& T, const GraphRow& r, int l, bool ex, const Map& map) {
  if (!graph_line_on(T, r, l)) return -1;
  return ex ? graph_elem_bus(T, T.t[T.lex_sub + l], r.topo[T.t[T.lex_pos + l]], map) : graph_elem_bus(T, T.t[T.lor_sub + l], r.topo[T.t[T.lor_pos + l]], map);
}

// The two off-diagonal entries a connected line l (origin on compact bus a, extremity on b, a != b) takes part in, active and reactive:
// f = {P[a][b], P[b][a], Q[a][b], Q[b][a]}.  Entry [i][j] is minus the sum over the connected lines between the two buses, in index
// order, of p_or of a line from i to j and p_ex of a line from j to i.  Only the lines of l's substation pair can join the same two buses.
// false: a line with a lower index joins them too and owns the entries.
template <typename Map>
GPF_GR_HD inline bool graph_pair_flows(const GraphTab& T, const GraphRow& r, int l, int a, int b, const Map& map, float f[4]) {
  double pab = 0.0, pba = 0.0, qab = 0.0, qba = 0.0;
  const int e0 = T.t[T.grp_at + l], e1 = e0 + T.t[T.grp_n + l];
  for (int e = e0; e < e1; ++e) {
    const int m = T.t[T.grp_lines + e];
    if (!graph_line_on(T, r, m)) continue;
    const int ma = graph_line_end(T, r, m, false, map), mb = graph_line_end(T, r, m, true, map);
    const bool same = ma == a && mb == b, flip = ma == b && mb == a;
    if (!same && !flip) continue;
    if (m < l) return false;
    const double por = (double)r.out[T.o_p_or + m], pex = (double)r.out[T.o_p_ex + m], qor = (double)r.out[T.o_q_or + m], qex = (double)r.out[T.o_q_ex + m];
    if (same) { pab += por; pba += pex; qab += qor; qba += qex; }
    else { pba += por; pab += pex; qba += qor; qab += qex; }
  }
  f[0] = (float)-pab; f[1] = (float)-pba; f[2] = (float)-qab; f[3] = (float)-qba;
  return true;
}

// ---- the table builder (host): the grid's arrays -> the blob ------------------------------------------------------------------------
struct GraphGrid {
  int n_sub, n_busbar, n_load, n_gen, n_sto, n_line, n_shunt, dim_topo;
  const int *load_sub, *load_pos, *gen_sub, *gen_pos, *sto_sub, *sto_pos, *lor_sub, *lor_pos, *lex_sub, *lex_pos, *shunt_sub;
  int o_p_or, o_q_or, o_v_or, o_p_ex, o_q_ex, o_v_ex, o_gen_p, o_gen_q, o_load_p, o_load_q, o_sto_p, o_sh_p, o_sh_q;
};

inline GraphTab graph_tab_view(const int* host_blob, const int* t) {
  GraphTab T;
  memcpy(&T.n_sub, host_blob, GR_HDR_INTS * sizeof(int));
  T.t = t;
  return T;
}

inline std::vector<int> graph_build_tab(const GraphGrid& g) {
  GraphTab T{};
  T.n_sub = g.n_sub; T.n_busbar = g.n_busbar; T.n_load = g.n_load; T.n_gen = g.n_gen; T.n_sto = g.n_sto; T.n_line = g.n_line;
  T.n_shunt = g.n_shunt; T.dim_topo = g.dim_topo;
  T.o_p_or = g.o_p_or; T.o_q_or = g.o_q_or; T.o_v_or = g.o_v_or; T.o_p_ex = g.o_p_ex; T.o_q_ex = g.o_q_ex; T.o_v_ex = g.o_v_ex;
  T.o_gen_p = g.o_gen_p; T.o_gen_q = g.o_gen_q; T.o_load_p = g.o_load_p; T.o_load_q = g.o_load_q; T.o_sto_p = g.o_sto_p;
  T.o_sh_p = g.o_sh_p; T.o_sh_q = g.o_sh_q;
  std::vector<int> blob(GR_HDR_INTS, 0);
  auto put = [&](const std::vector<int>& a) { const int at = (int)blob.size(); blob.insert(blob.end(), a.begin(), a.end()); return at; };
  auto arr = [&](const int* p, int n) { return put(std::vector<int>(p, p + n)); };
  std::vector<std::vector<std::pair<int, std::pair<int, int>>>> per(g.n_sub);   // (code, (position, other end)) of every element of a substation
  auto add = [&](int kind, int n, const int* sub, const int* pos, const int* other) {
    for (int i = 0; i < n; ++i) per[sub[i]].push_back({(kind << GR_CODE_SHIFT) | i, {pos ? pos[i] : i, other ? other[i] : -1}});
  };
  add(GR_GEN, g.n_gen, g.gen_sub, g.gen_pos, nullptr); add(GR_LOAD, g.n_load, g.load_sub, g.load_pos, nullptr);
  add(GR_STO, g.n_sto, g.sto_sub, g.sto_pos, nullptr); add(GR_SHUNT, g.n_shunt, g.shunt_sub, nullptr, nullptr);
  add(GR_LOR, g.n_line, g.lor_sub, g.lor_pos, g.lex_pos); add(GR_LEX, g.n_line, g.lex_sub, g.lex_pos, g.lor_pos);
  std::vector<int> off(g.n_sub + 1, 0), code, pos, other;
  for (int s = 0; s < g.n_sub; ++s) {
    std::sort(per[s].begin(), per[s].end());
    for (auto& e : per[s]) { code.push_back(e.first); pos.push_back(e.second.first); other.push_back(e.second.second); }
    off[s + 1] = (int)code.size();
  }
  T.sub_off = put(off); T.el_code = put(code); T.el_pos = put(pos); T.el_other = put(other);
  T.load_pos = arr(g.load_pos, g.n_load); T.load_sub = arr(g.load_sub, g.n_load); T.gen_pos = arr(g.gen_pos, g.n_gen); T.gen_sub = arr(g.gen_sub, g.n_gen);
  T.sto_pos = arr(g.sto_pos, g.n_sto); T.sto_sub = arr(g.sto_sub, g.n_sto); T.lor_pos = arr(g.lor_pos, g.n_line); T.lor_sub = arr(g.lor_sub, g.n_line);
  T.lex_pos = arr(g.lex_pos, g.n_line); T.lex_sub = arr(g.lex_sub, g.n_line); T.sh_sub = arr(g.shunt_sub, g.n_shunt);
  std::map<std::pair<int, int>, std::vector<int>> groups;
  for (int l = 0; l < g.n_line; ++l) groups[{std::min(g.lor_sub[l], g.lex_sub[l]), std::max(g.lor_sub[l], g.lex_sub[l])}].push_back(l);
  std::vector<int> at(g.n_line), cnt(g.n_line), lines;
  for (auto& kv : groups) {
    for (int l : kv.second) { at[l] = (int)lines.size(); cnt[l] = (int)kv.second.size(); }
    lines.insert(lines.end(), kv.second.begin(), kv.second.end());
  }
  T.grp_at = put(at); T.grp_n = put(cnt); T.grp_lines = put(lines);
  T.total = (int)blob.size();
  memcpy(blob.data(), &T.n_sub, GR_HDR_INTS * sizeof(int));
  return blob;
}

// ---- one lane's rows: index [graph_index_width], feat [NB][4], dense [3][NB][NB] (null: none; zero on entry) -------------------------
// The game-over rows of the reference (baseObservation.py:2163-2177, 2321-2330): one bus, every element on it, nothing else.
GPF_GR_HD inline int graph_game_over_index(const GraphTab& T, int i) {
  return i == 0 ? 1 : i <= graph_index_width(T) - graph_nb(T) ? 0 : -1;
}

// The element sections of the index row and the off-diagonal entries of the dense planes, once the map stands: share t of `stride`
// takes elements t, t + stride, ... of every section (the kernel: thread t of 64; the emulator: one share).
template <typename Map>
GPF_GR_HD inline void graph_lane_elements(const GraphTab& T, const GraphRow& r, const Map& look, int* idx, float* dense, int t, int stride) {
  const int nb = graph_nb(T);
  int* o = idx + 1;
  for (int i = t; i < T.n_load; i += stride) o[i] = graph_elem_bus(T, T.t[T.load_sub + i], r.topo[T.t[T.load_pos + i]], look);
  o += T.n_load;
  for (int i = t; i < T.n_gen; i += stride) o[i] = graph_elem_bus(T, T.t[T.gen_sub + i], r.topo[T.t[T.gen_pos + i]], look);
  o += T.n_gen;
  for (int i = t; i < T.n_sto; i += stride) o[i] = graph_elem_bus(T, T.t[T.sto_sub + i], r.topo[T.t[T.sto_pos + i]], look);
  o += T.n_sto;
  for (int l = t; l < T.n_line; l += stride) {
    const int a = graph_line_end(T, r, l, false, look), b = graph_line_end(T, r, l, true, look);
    o[l] = a; o[T.n_line + l] = b;
    if (dense && a >= 0 && b >= 0 && a != b) {
      const size_t ab = (size_t)a * nb + b, ba = (size_t)b * nb + a, pl = (size_t)nb * nb;
      float f[4];
      if (graph_pair_flows(T, r, l, a, b, look, f)) {
        dense[ab] = 1.f; dense[ba] = 1.f;
        dense[pl + ab] = f[0]; dense[pl + ba] = f[1]; dense[2 * pl + ab] = f[2]; dense[2 * pl + ba] = f[3];
      }
    }
  }
  o += 2 * T.n_line;
  for (int i = t; i < T.n_shunt; i += stride) o[i] = graph_elem_bus(T, T.t[T.sh_sub + i], r.shunt_bus[i], look);
}

// a live bus with compact id cid stores what it owns: its feature row, its bus_global entry, its diagonal
GPF_GR_HD inline void graph_store_node(const GraphTab& T, const GraphNode& nd, int g, int cid, int* idx, float* feat, float* dense) {
  const int nb = graph_nb(T);
  for (int j = 0; j < GR_N_FEAT; ++j) feat[(size_t)cid * GR_N_FEAT + j] = nd.f[j];
  idx[graph_index_width(T) - nb + cid] = g;
  if (dense) {
    const size_t dg = (size_t)cid * nb + cid, pl = (size_t)nb * nb;
    dense[dg] = 1.f; dense[pl + dg] = nd.f[0]; dense[2 * pl + dg] = nd.f[1];
  }
}

// the executor of the host emulator: the buses one after the other, the map in a vector
inline void graph_lane_serial(const GraphTab& T, const GraphRow& r, bool over, int* idx, float* feat, float* dense) {
  const int nb = graph_nb(T), width = graph_index_width(T);
  if (dense) std::fill(dense, dense + (size_t)3 * nb * nb, 0.f);
  std::fill(feat, feat + (size_t)nb * GR_N_FEAT, 0.f);
  if (over) {
    for (int i = 0; i < width; ++i) idx[i] = graph_game_over_index(T, i);
    return;
  }
  std::vector<int> map(nb, -1);
  int base = 0;
  for (int g = 0; g < nb; ++g) {
    const GraphNode nd = graph_node(T, r, g);
    if (!nd.live) continue;
    map[g] = base;
    graph_store_node(T, nd, g, base++, idx, feat, dense);
  }
  idx[0] = base;
  for (int i = base; i < nb; ++i) idx[width - nb + i] = -1;
  graph_lane_elements(T, r, [&](int g) { return map[g]; }, idx, dense, 0, 1);
}

#if defined(__HIPCC__) && defined(GPF_GRAPH_KERNEL)
struct GraphDev {
  GraphTab T;
  const int* topo;                   // [lanes][dim_topo] topo_vect as the last solve left it
  const int* shunt_bus;              // [lanes][n_shunt]
  const float* out;                  // [lanes][n_out]
  const int* sub_cd;                 // [lanes][n_sub] or null
  const unsigned char* done;         // [lanes]
  int* index;                        // [n][graph_index_width]  rows of the range's first lane
  float* feat;                       // [n][NB][4]
  float* dense;                      // [n][3][NB][NB] or null; zeroed by a memset queued ahead of the kernel
  int n_out, game_over_fill;
};

constexpr int GR_WPB = 4;            // lanes (wavefronts) per block
constexpr size_t GR_STAGE_MAX_BYTES = 64 * 1024;   // dynamic LDS a block may ask for without an attribute of its own

// ints of dynamic LDS per wavefront: the global -> compact map and, staged, the lane's topo_vect, shunt buses and results row (each
// part a multiple of 4 ints)
__host__ __device__ inline int graph_lds_part(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int graph_lds_ints(const GraphTab& T, int n_out, bool stage) {
  return graph_lds_part(graph_nb(T)) + (stage ? graph_lds_part(T.dim_topo) + graph_lds_part(T.n_shunt) + graph_lds_part(n_out) : 0);
}

// One wavefront per lane, GR_WPB lanes per block; the lane's rows are wave-uniform addresses.  Phase 0 (stage != 0, uniform: the host
// sets it when GR_WPB lanes fit GR_STAGE_MAX_BYTES): the lane's topo_vect, shunt buses and results row are copied into LDS with coalesced
// loads, and the gathers below read the copies -- a gather is a chain of dependent loads (table entry, topo_vect entry, result), and at
// one or two wavefronts per SIMD nothing else hides their latency.  Phase 1: thread t owns global bus c * 64 + t of chunk c, gathers its
// node, and the chunk's live buses get the next compact ids by __ballot + popcount; the bus writes its features, its bus_global entry
// and its diagonal, and the map entry of its global id in the wavefront's LDS array.  Phase 2 (behind a barrier: the map is read by
// other threads than wrote it): the elements look their buses up, the lines store their off-diagonal entries (graph_pair_flows: one
// owner per pair of buses).  Dynamic LDS: GR_WPB * graph_lds_ints ints.  No scratch, no atomics.  Read-only on the lanes' state.
__global__ __launch_bounds__(64 * GR_WPB) void graph_obs_kernel(GraphDev d, int lane0, int n, int stage) {
  extern __shared__ int gr_lds[];
  const int tid = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int k = blockIdx.x * GR_WPB + w;
  const GraphTab& T = d.T;
  const int nb = graph_nb(T), width = graph_index_width(T), first_bus = width - nb;
  const size_t lane = (size_t)lane0 + (k < n ? k : 0);
  const bool act = k < n;
  const bool over = act && d.game_over_fill && d.done[lane] != 0;
  GraphRow r;
  r.topo = d.topo + lane * T.dim_topo; r.shunt_bus = d.shunt_bus + lane * T.n_shunt; r.out = d.out + lane * d.n_out;
  r.sub_cd = d.sub_cd ? d.sub_cd + lane * T.n_sub : nullptr;
  int* idx = d.index + (size_t)(act ? k : 0) * width;
  float* feat = d.feat + (size_t)(act ? k : 0) * nb * GR_N_FEAT;
  float* dense = d.dense ? d.dense + (size_t)(act ? k : 0) * 3 * nb * nb : nullptr;
  int* map = gr_lds + (size_t)w * graph_lds_ints(T, d.n_out, stage != 0);
  if (stage && act && !over) {
    int* s_topo = map + graph_lds_part(nb);
    int* s_shb = s_topo + graph_lds_part(T.dim_topo);
    float* s_out = (float*)(s_shb + graph_lds_part(T.n_shunt));
    for (int i = tid; i < T.dim_topo; i += 64) s_topo[i] = r.topo[i];
    for (int i = tid; i < T.n_shunt; i += 64) s_shb[i] = r.shunt_bus[i];
    for (int i = tid; i < d.n_out; i += 64) s_out[i] = r.out[i];
    r.topo = s_topo; r.shunt_bus = s_shb; r.out = s_out;
  }
  __syncthreads();
  if (over) {
    for (int i = tid; i < width; i += 64) idx[i] = graph_game_over_index(T, i);
    for (int i = tid; i < nb * GR_N_FEAT; i += 64) feat[i] = 0.f;
  } else if (act) {
    int base = 0;
    for (int c = 0; c * 64 < nb; ++c) {
      const int g = c * 64 + tid;
      GraphNode nd{};
      if (g < nb) nd = graph_node(T, r, g);
      const unsigned long long live = __ballot(nd.live);
      const int cid = base + __popcll(live & ((1ull << tid) - 1ull));
      if (g < nb) map[g] = nd.live ? cid : -1;
      if (nd.live) graph_store_node(T, nd, g, cid, idx, feat, dense);
      base += __popcll(live);
    }
    if (tid == 0) idx[0] = base;
    for (int i = base + tid; i < nb; i += 64) {
      idx[first_bus + i] = -1;
      for (int j = 0; j < GR_N_FEAT; ++j) feat[(size_t)i * GR_N_FEAT + j] = 0.f;
    }
  }
  __syncthreads();
  if (!act || over) return;
  graph_lane_elements(T, r, [&](int g) { return map[g]; }, idx, dense, tid, 64);
}
#endif  // __HIPCC__ && GPF_GRAPH_KERNEL

}  // namespace gpf
