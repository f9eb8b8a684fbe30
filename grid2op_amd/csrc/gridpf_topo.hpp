// gridpf_topo.hpp -- topology actions of the batched acting path (gpf_upload_topo_actions / gpf_set_lane_topo_actions, include/gridpf.h).
//
// What BaseEnv.step does between the agent and the backend for the topology part of an action (paths relative to the reference
// checkout), for every lane of a launch:
//   1. ambiguity (BaseAction._check_for_ambiguity, Action/baseAction.py:3498-3760): static per table entry, computed on the host
//      when the table is uploaded; an index outside the table counts as ambiguous;
//   2. impact (BaseAction.get_topological_impact, Action/baseAction.py:1782-2020) with the lane's line status before the step;
//   3. legality (Rules/LookParam.py:28-53 + Rules/PreventReconnection.py:23-60); an illegal or ambiguous action becomes do-nothing
//      (Environment/baseEnv.py:3700-3770);
//   4. application (_BackendAction.__iadd__, Action/_backendAction.py:836-919): apply_topo_action below -- the ONE implementation,
//      called by gpf_simulate_batch on the host and by topo_prestep_kernel on the device;
//   5. bookkeeping after the step (Environment/baseEnv.py:3346-3395, _BackendAction.update_state :1533-1555): topo_poststep_kernel.
//
// Composite actions (gpf_set_topo_slots) and rules by area (gpf_set_topo_areas; Rules/rulesByArea.py:120-140): a lane plays the
// concatenation, in slot order, of the item lists of its non-empty slots as ONE action -- dense arrays, run-time ambiguity
// (topo_dense_ambiguity, gridpf_topo_mask.hpp), impact, legality with the limits held per area, ONE call of apply_topo_action.  That is the
// GEN instantiation of topo_prestep_kernel; with one slot and no areas the engine launches the other one, which is the kernel as it was.
//
// Two parts: what the host shares (apply_topo_action, the argument blocks, the LDS size of the pre-step: gridpf_capi.hip's
// gpf_simulate_batch and the engine of gridpf_engine.hpp include the header for these) and, for the one unit that defines GPF_TOPO_KERNEL
// (gridpf_capi_topo.hip), the kernels.  Steps 1-4 on the device are topo_play_lane, a __device__ function: the unit that defines
// GPF_LA_KERNEL (gridpf_capi_lookahead.hip) gets it too, for the play kernel of gridpf_lookahead.hpp, and none of the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <limits.h>

#include "gridpf_episode.hpp"
#include "gridpf_topo_mask.hpp"

namespace gpf {

// action item kinds (= GPF_ACT_* of include/gridpf.h)
constexpr int TA_SET_BUS = 0, TA_SET_LINE_STATUS = 1, TA_CHANGE_BUS = 2, TA_CHANGE_LINE_STATUS = 3, TA_SET_SHUNT_BUS = 4;

struct TopoMaps { const int* or_pos; const int* ex_pos; int n_line; };
struct NoSync { __host__ __device__ void operator()() const {} };

// _BackendAction.__iadd__ restricted to topology (Action/_backendAction.py:836-919; ValueStore.set_status / change_status / set_val /
// change_val :140-234, _aux_iadd_reconcile_disco_reco :738-765) on one topology row; items = {kind, id, value} triples.  `last`: last
// known busbar per topo_vect position (NULL or < 1: busbar 1).  or_b / ex_b: scratch [n_line].  The item passes run on thread 0, the
// per-line passes on threads tid, tid + nth, ...; `sync` orders them (host: one thread, no-op).
template <class Sync>
__host__ __device__ inline void apply_topo_action(const TopoMaps& m, int* row, int* sb, const int* last, const int* items, int n_items,
                                                  int* or_b, int* ex_b, int tid, int nth, Sync sync) {
  auto old = [&](int pos) { return (last && last[pos] >= 1) ? last[pos] : 1; };
  auto reco = [&](int l) { const int po = m.or_pos[l], pe = m.ex_pos[l]; if (row[po] < 0) row[po] = old(po); if (row[pe] < 0) row[pe] = old(pe); };
  auto disco = [&](int l) { row[m.or_pos[l]] = -1; row[m.ex_pos[l]] = -1; };
  if (tid == 0) {
    // III line status: change_status, then set_status (a reconnected end goes back to its last known busbar)
    for (int k = 0; k < n_items; ++k) if (items[3 * k] == TA_CHANGE_LINE_STATUS) {
      const int l = items[3 * k + 1];
      if (row[m.or_pos[l]] > 0 || row[m.ex_pos[l]] > 0) disco(l); else reco(l);
    }
    for (int k = 0; k < n_items; ++k) if (items[3 * k] == TA_SET_LINE_STATUS) {
      const int l = items[3 * k + 1], v = items[3 * k + 2];
      if (v < 0) disco(l); else if (v > 0) reco(l);
    }
  }
  bool any_bus = false;                                         // (the line ends "before" are only needed by rule V)
  for (int k = 0; k < n_items && !any_bus; ++k) any_bus = items[3 * k] == TA_CHANGE_BUS || (items[3 * k] == TA_SET_BUS && items[3 * k + 2] != 0);
  sync();
  if (any_bus)
    for (int l = tid; l < m.n_line; l += nth) { or_b[l] = row[m.or_pos[l]]; ex_b[l] = row[m.ex_pos[l]]; }
  sync();
  // IV change_bus, then set_bus
  if (tid == 0) {
    for (int k = 0; k < n_items; ++k) if (items[3 * k] == TA_CHANGE_BUS) { int& v = row[items[3 * k + 1]]; if (v > 0) v = (1 - v) + 2; }
    for (int k = 0; k < n_items; ++k) if (items[3 * k] == TA_SET_BUS && items[3 * k + 2] != 0) row[items[3 * k + 1]] = items[3 * k + 2];
  }
  sync();
  // V a line with an open end is open; a line that was open and got a bus on one end is reconnected (other end: last known busbar)
  if (any_bus)
    for (int l = tid; l < m.n_line; l += nth) {
      const int o_ = row[m.or_pos[l]], x_ = row[m.ex_pos[l]];
      const bool d_now = or_b[l] == -1 || o_ == -1 || ex_b[l] == -1 || x_ == -1;
      const bool r_now = or_b[l] == -1 && (o_ >= 1 || x_ >= 1);
      if (r_now) reco(l); else if (d_now) disco(l);
    }
  if (tid == 0)
    for (int k = 0; k < n_items; ++k) if (items[3 * k] == TA_SET_SHUNT_BUS && sb && items[3 * k + 2] != 0) sb[items[3 * k + 1]] = items[3 * k + 2];
  sync();
}

// the uploaded action table (gpf_upload_topo_actions): offsets [n_act + 1] into items [][3], static ambiguity flags [n_act]
struct TopoTab { const int* off; const int* items; const unsigned char* amb; int n_act; };
// per-lane state of the acting path (rows padded to the engine's lane capacity)
struct TopoLanes {
  int* act;               // [lanes][n_slot] action indices of the next launch, -1 = empty slot
  int* sub_cd;            // [lanes][n_sub] times_before_topology_actionable
  int* last_bus;          // [lanes][dim_topo] last known busbar (_BackendAction.last_topo_registered)
  unsigned char* flags;   // [lanes][2] {is_illegal, is_ambiguous} of the last action launch
  unsigned char* aff;     // [lanes][n_line + n_sub] aff_lines | aff_subs of the legal action of the last action launch
  int* ep_snap;           // [lanes] auto-reset count before the launch (a lane that auto-reset is cleared afterwards)
  int* list;              // [1 + lanes]: count, then the lanes whose topology class key / busbar count changed
  int* list_rows;         // [lanes][dim_topo + n_shunt] their new rows (slot order of `list`)
  const int* pos_sub;     // [dim_topo] substation of every topo_vect position
  const int* pos_other;   // [dim_topo] the other end's position for a line end, else -1
  int n_slot;             // table entries per lane and step (gpf_set_topo_slots)
};
// composite actions and areas: sub_area [n_sub] (NULL: the whole grid is one area), max_items: n_slot x the items of the longest table entry
struct TopoComp { const int* sub_area; int n_area, max_items; };
// the grid maps and lane rows the three kernels touch (a small argument block: GridDev + Bufs by value cost SGPR spills)
struct TopoDev {
  int dim_topo, n_line, n_sub, n_shunt, n_busbar;
  const int* line_or_pos; const int* line_ex_pos; const int* shunt_sub;
  int* topo; int* shunt_bus; int* cooldown; const int* topo0; const int* episode; const unsigned char* done;
};
// rules (Parameters MAX_SUB_CHANGED / MAX_LINE_STATUS_CHANGED / NB_TIMESTEP_COOLDOWN_SUB / NB_TIMESTEP_COOLDOWN_LINE); on = 0: AlwaysLegal
struct TopoRules { int on, max_sub, max_line, cd_sub, cd_line; };

// LDS ints of topo_prestep_kernel.  max_items < 0: the instantiation for one slot and no areas; else the GEN one, with the gathered item
// list [max_items][3], change_bus kept apart from eff [dim_topo], the two line-status arrays of the ambiguity rules [2][n_line] and the
// per-area counters [2][TM_MAX_AREAS].
__host__ __device__ inline size_t topo_prestep_lds_ints(int dim_topo, int n_line, int n_sub, int n_shunt, int n_busbar, int max_items = -1) {
  const size_t base = 4 * (size_t)dim_topo + 3 * (size_t)n_line + (size_t)n_sub + 2 * (size_t)n_shunt + 4 * (size_t)n_sub * n_busbar + 8;
  return max_items < 0 ? base : base + 3 * (size_t)max_items + (size_t)dim_topo + 2 * (size_t)n_line + 2 * TM_MAX_AREAS;
}

#if defined(__HIPCC__) && (defined(GPF_TOPO_KERNEL) || defined(GPF_LA_KERNEL))
// Where the look-ahead's play kernel (gridpf_lookahead.hpp) departs from the pre-step: the table index comes from the candidate buffer,
// the planner's question is asked against the row the host last NOTED for the lane (noted[0] == INT_MIN: none), which is rewritten when
// the lane is listed, and the list is the look-ahead's own.
struct TopoLook { int act; int* noted; int* list; int* list_rows; };

// Steps 1-4 for one lane by one 64-thread block (one wavefront), its rows staged in LDS: the ONE statement of them on the device, for
// topo_prestep_kernel and la_play_kernel.  GEN: composite actions of s.n_slot entries and limits per area (`c`); else one entry per
// lane, whole-grid limits, `c` unused.  LOOK: the lane is a scratch lane that already holds its environment's rows, cooldowns and last
// known busbars; an ambiguous or illegal entry leaves them (the do-nothing row) and the lane still goes through the planner's
// question.  Returns the verdict, uniform over the block: 1 illegal, 2 ambiguous, 0 neither.
template <bool GEN, bool LOOK>
__device__ __forceinline__ int topo_play_lane(const TopoDev& g, const TopoTab& tab, const TopoLanes& s, const TopoRules& r, const TopoComp& c,
                                              int* lds, int lane, const TopoLook& k, int tid, int nth) {
  static_assert(!(GEN && LOOK), "the look-ahead plays single table entries");
  const int D = g.dim_topo, L = g.n_line, S = g.n_sub, NS = g.n_shunt, NBB = g.n_busbar;
  unsigned char* aff = s.aff + (size_t)lane * (L + S);
  for (int i = tid; i < L + S; i += nth) aff[i] = 0;
  int a = -1, n_items = 0;
  bool amb = false;
  if constexpr (GEN) {                                         // an index outside the table in any slot: ambiguous; all slots empty: nothing
    for (int k = 0; k < s.n_slot; ++k) {
      const int ak = s.act[(size_t)lane * s.n_slot + k];
      amb = amb || ak < -1 || ak >= tab.n_act;
      if (ak >= 0 && ak < tab.n_act) { a = ak; n_items += tab.off[ak + 1] - tab.off[ak]; }
    }
    amb = amb || n_items > c.max_items;                        // (the bound of `gath`; the engine sizes it n_slot x the longest entry, so an
                                                               //  index repeated over slots fits too and this never fires on a table it uploaded)
    // tab.amb is not consulted, even with one slot (areas only), where it would answer: the run-time pass below is the one rule for
    // every GEN launch, an ambiguous single entry costs one gather and one pass over the dense arrays before the lane stops
  } else {
    a = LOOK ? k.act : s.act[lane];
    amb = a < -1 || a >= tab.n_act || (a >= 0 && tab.amb[a]);
  }
  bool play = !(a == -1 || amb);                               // (uniform over the block)
  if (!play) {
    if (tid == 0) { s.flags[(size_t)lane * 2] = 0; s.flags[(size_t)lane * 2 + 1] = amb ? 1 : 0; }
    if constexpr (!LOOK) return amb ? 2 : 0;
  }
  int* row = lds;                 // [D] the row being acted on
  int* prev = row + D;            // [D] the row before the action
  int* setv = prev + D;           // [D] set_bus value (0: none)
  int* eff = setv + D;            // [D] change_bus, then "effective change"
  int* or_b = eff + D;            // [L]
  int* ex_b = or_b + L;           // [L]
  int* imp = ex_b + L;            // [L] aff_lines
  int* subf = imp + L;            // [S] aff_subs
  int* sbr = subf + S;            // [NS]
  int* sbp = sbr + NS;            // [NS]
  int* used0 = sbp + NS;          // [S][NBB] busbars >= 2 in the class key, before / after; busbars live as count_lane counts them
  int* used1 = used0 + S * NBB;
  int* act0 = used1 + S * NBB;
  int* act1 = act0 + S * NBB;
  int* cnt = act1 + S * NBB;      // [8] aff lines, aff subs, cooldown hit, key changed, busbar count before / after, list slot, ambiguous
  int* chg = cnt + 8;             // GEN: [D] change_bus
  int* setl = chg + D;            //      [L] set_line_status value
  int* swl = setl + L;            //      [L] change_line_status
  int* acnt = swl + L;            //      [2][TM_MAX_AREAS] aff lines / aff subs per area
  int* gath = acnt + 2 * TM_MAX_AREAS;   // [max_items][3] the concatenated item list
  const int* items = play ? tab.items + 3 * (size_t)tab.off[a] : nullptr;
  if constexpr (GEN) {
    int at = 0;
    for (int k = 0; k < s.n_slot; ++k) {                       // (uniform) slot after slot, every thread a stride of the slot's ints
      const int ak = s.act[(size_t)lane * s.n_slot + k];
      if (ak < 0) continue;
      const int o0 = tab.off[ak], n3 = 3 * (tab.off[ak + 1] - o0);
      for (int i = tid; i < n3; i += nth) gath[at + i] = tab.items[3 * (size_t)o0 + i];
      at += n3;
    }
    for (int i = tid; i < D; i += nth) chg[i] = 0;
    for (int i = tid; i < L; i += nth) { setl[i] = 0; swl[i] = 0; }
    if (tid < 2 * TM_MAX_AREAS) acnt[tid] = 0;
    items = gath;
  } else {
    n_items = play ? tab.off[a + 1] - tab.off[a] : 0;
  }
  const int* trow = g.topo + (size_t)lane * D;
  for (int i = tid; i < D; i += nth) { const int v = trow[i]; row[i] = v; prev[i] = v; setv[i] = 0; eff[i] = 0; }
  for (int i = tid; i < NS; i += nth) { const int v = g.shunt_bus[(size_t)lane * NS + i]; sbr[i] = v; sbp[i] = v; }
  for (int i = tid; i < L; i += nth) imp[i] = 0;
  for (int i = tid; i < S; i += nth) subf[i] = 0;
  for (int i = tid; i < 4 * S * NBB; i += nth) used0[i] = 0;
  if (tid < 8) cnt[tid] = 0;
  __syncthreads();
  // 2. impact (get_topological_impact with the lane's line status before the step)
  if (tid == 0)
    for (int k = 0; k < n_items; ++k) {
      const int kind = items[3 * k], id = items[3 * k + 1], v = items[3 * k + 2];
      if (kind == TA_SET_BUS) setv[id] = v;
      else if (kind == TA_CHANGE_BUS) eff[id] = 1;
      else if (kind == TA_CHANGE_LINE_STATUS || (kind == TA_SET_LINE_STATUS && v != 0)) imp[id] = 1;
      if constexpr (GEN) {
        if (kind == TA_CHANGE_BUS) chg[id] = 1;
        else if (kind == TA_SET_LINE_STATUS) setl[id] = v;
        else if (kind == TA_CHANGE_LINE_STATUS) swl[id] = 1;
      }
    }
  __syncthreads();
  if constexpr (GEN) {                                         // 1. ambiguity of the composite, on its dense arrays
    if (topo_dense_ambiguity(D, L, g.line_or_pos, g.line_ex_pos, setv, chg, setl, swl, tid, nth)) cnt[7] = 1;
    __syncthreads();
    if (cnt[7]) {
      if (tid == 0) { s.flags[(size_t)lane * 2] = 0; s.flags[(size_t)lane * 2 + 1] = 1; }
      return 2;
    }
  }
  for (int i = tid; i < D; i += nth) eff[i] = (eff[i] || setv[i] != 0) ? 1 : 0;
  __syncthreads();
  for (int l = tid; l < L; l += nth) {
    const int po = g.line_or_pos[l], pe = g.line_ex_pos[l];
    const bool st = prev[po] > 0 && prev[pe] > 0, notc = !st;
    bool im = imp[l] != 0, clr = im && notc;
    const bool hit = (setv[po] > 0 && notc) || (setv[pe] > 0 && notc) || (setv[po] < 0 && st) || (setv[pe] < 0 && st);
    im = im || hit; clr = clr || hit;
    if (clr) { eff[po] = 0; eff[pe] = 0; }
    imp[l] = im ? 1 : 0;
  }
  __syncthreads();
  for (int i = tid; i < D; i += nth) if (eff[i]) subf[s.pos_sub[i]] = 1;
  __syncthreads();
  // 3. legality (LookParam + PreventReconnection)
  bool illegal;
  if constexpr (GEN) {                                         // the limits per area; a line counts in the area of its origin substation
    for (int l = tid; l < L; l += nth) if (imp[l]) {
      atomicAdd(&acnt[c.sub_area ? c.sub_area[s.pos_sub[g.line_or_pos[l]]] : 0], 1);
      if (g.cooldown[(size_t)lane * L + l] > 0) cnt[2] = 1;
    }
    for (int i = tid; i < S; i += nth) if (subf[i]) {
      atomicAdd(&acnt[TM_MAX_AREAS + (c.sub_area ? c.sub_area[i] : 0)], 1);
      if (s.sub_cd[(size_t)lane * S + i] > 0) cnt[2] = 1;
    }
    __syncthreads();
    bool over = false;
    for (int k = 0; k < TM_MAX_AREAS; ++k) over = over || acnt[k] > r.max_line || acnt[TM_MAX_AREAS + k] > r.max_sub;
    illegal = r.on && (over || cnt[2] != 0);
  } else {
    for (int l = tid; l < L; l += nth) if (imp[l]) { atomicAdd(&cnt[0], 1); if (g.cooldown[(size_t)lane * L + l] > 0) cnt[2] = 1; }
    for (int i = tid; i < S; i += nth) if (subf[i]) { atomicAdd(&cnt[1], 1); if (s.sub_cd[(size_t)lane * S + i] > 0) cnt[2] = 1; }
    __syncthreads();
    illegal = r.on && (cnt[0] > r.max_line || cnt[1] > r.max_sub || cnt[2] != 0);
  }
  if (tid == 0 && play) { s.flags[(size_t)lane * 2] = illegal ? 1 : 0; s.flags[(size_t)lane * 2 + 1] = 0; }   // (LOOK, not played: no items, never illegal)
  if (illegal) { if constexpr (!LOOK) return 1; }
  if (!illegal) {                                              // (LOOK: an illegal entry leaves the do-nothing row)
    for (int l = tid; l < L; l += nth) aff[l] = (unsigned char)imp[l];
    for (int i = tid; i < S; i += nth) aff[L + i] = (unsigned char)subf[i];
    // 4. application
    struct BlockSync { __device__ void operator()() const { __syncthreads(); } };
    const TopoMaps m{g.line_or_pos, g.line_ex_pos, L};
    apply_topo_action(m, row, NS ? sbr : nullptr, s.last_bus + (size_t)lane * D, items, n_items, or_b, ex_b, tid, nth, BlockSync{});
  }
  const int verdict = (illegal ? 1 : 0) | (amb ? 2 : 0);
  // planning: the lane's topology class key (gridpf_capi.hip topo_class_of: busbar of every line end, an open end counting as
  // busbar 1, + the busbars >= 2 that carry an element) or its live busbars per substation (count_lane) changed -> host bookkeeping
  // (LOOK: changed against the row the host last noted for this scratch lane, not against the row before the action)
  const int* was = LOOK ? k.noted : prev;
  const int* sb_was = LOOK ? k.noted + D : sbp;
  auto bb = [NBB](int v) { return v >= 2 && v <= NBB ? v : 1; };
  for (int p = tid; p < D; p += nth) {
    const int v0 = was[p], v1 = row[p], sub = s.pos_sub[p], o = s.pos_other[p];
    if (o >= 0 && bb(v0) != bb(v1)) cnt[3] = 1;
    if (bb(v0) >= 2) used0[sub * NBB + v0 - 1] = 1;
    if (bb(v1) >= 2) used1[sub * NBB + v1 - 1] = 1;
    if (v0 >= 1 && v0 <= NBB && (o < 0 || was[o] >= 1)) act0[sub * NBB + v0 - 1] = 1;
    if (v1 >= 1 && v1 <= NBB && (o < 0 || row[o] >= 1)) act1[sub * NBB + v1 - 1] = 1;
  }
  for (int i = tid; i < NS; i += nth) {
    const int sub = g.shunt_sub[i], v0 = sb_was[i], v1 = sbr[i];
    if (bb(v0) >= 2) used0[sub * NBB + v0 - 1] = 1;
    if (bb(v1) >= 2) used1[sub * NBB + v1 - 1] = 1;
    if (v0 >= 1 && v0 <= NBB) act0[sub * NBB + v0 - 1] = 1;
    if (v1 >= 1 && v1 <= NBB) act1[sub * NBB + v1 - 1] = 1;
  }
  __syncthreads();
  for (int i = tid; i < S; i += nth) {
    int c0 = 0, c1 = 0;
    for (int k = 0; k < NBB; ++k) { c0 += act0[i * NBB + k]; c1 += act1[i * NBB + k]; if (used0[i * NBB + k] != used1[i * NBB + k]) cnt[3] = 1; }
    atomicMax(&cnt[4], c0); atomicMax(&cnt[5], c1);
  }
  __syncthreads();
  bool moved = cnt[3] != 0 || (cnt[4] > 1 ? cnt[4] : 1) != (cnt[5] > 1 ? cnt[5] : 1);
  if constexpr (LOOK) moved = moved || k.noted[0] == INT_MIN;
  int* orow = g.topo + (size_t)lane * D;
  for (int i = tid; i < D; i += nth) orow[i] = row[i];
  for (int i = tid; i < NS; i += nth) g.shunt_bus[(size_t)lane * NS + i] = sbr[i];
  if (!moved) return verdict;
  int* list = LOOK ? k.list : s.list;
  if (tid == 0) { const int slot = atomicAdd(&list[0], 1); list[1 + slot] = lane; cnt[6] = slot; }
  __syncthreads();                                             // (behind the last read of `was`, too)
  int* dst = (LOOK ? k.list_rows : s.list_rows) + (size_t)cnt[6] * (D + NS);
  for (int i = tid; i < D; i += nth) dst[i] = row[i];
  for (int i = tid; i < NS; i += nth) dst[D + i] = sbr[i];
  if constexpr (LOOK) {
    for (int i = tid; i < D; i += nth) k.noted[i] = row[i];
    for (int i = tid; i < NS; i += nth) k.noted[D + i] = sbr[i];
  }
  return verdict;
}

#ifdef GPF_TOPO_KERNEL
// Steps 1-4 for one lane per 64-thread block (topo_play_lane).  act_on = 0: only the auto-reset snapshot.
template <bool GEN>
__global__ __launch_bounds__(64) void topo_prestep_kernel(TopoDev g, TopoTab tab, TopoLanes s, TopoRules r, TopoComp c, int n_lanes, int act_on) {
  extern __shared__ int lds[];
  const int lane = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  if (lane >= n_lanes) return;
  if (tid == 0) s.ep_snap[lane] = g.episode[(size_t)lane * 2 + 1];
  if (!act_on) return;
  topo_play_lane<GEN, false>(g, tab, s, r, c, lds, lane, TopoLook{}, tid, nth);
}

// Step 5 for one lane per 64-thread block.  had_act: the launch (one step) carried topology actions; else n_steps do-nothing steps.
// list_resets: append every lane that auto-reset in this launch, with its reset rows, to s.list / s.list_rows (zeroed by the host): a
// lane an action moved to another topology class is back on the class of its reset topology, which the launch planner must learn.
__global__ __launch_bounds__(64) void topo_poststep_kernel(TopoDev g, TopoLanes s, TopoRules r, int n_lanes, int had_act, int n_steps,
                                                           int list_resets) {
  const int lane = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  if (lane >= n_lanes) return;
  const int D = g.dim_topo, L = g.n_line, S = g.n_sub;
  int* scd = s.sub_cd + (size_t)lane * S;
  int* lb = s.last_bus + (size_t)lane * D;
  const int* topo = g.topo + (size_t)lane * D;
  if (g.episode[(size_t)lane * 2 + 1] != s.ep_snap[lane]) {     // auto-reset in this launch: env.reset() starts from scratch
    topo_reset_acting(scd, lb, g.topo0 + (size_t)lane * D, S, D, tid, nth);
    if (list_resets) {
      __shared__ int slot;
      if (tid == 0) { slot = atomicAdd(&s.list[0], 1); s.list[1 + slot] = lane; }
      __syncthreads();
      const int NS = g.n_shunt;
      int* dst = s.list_rows + (size_t)slot * (D + NS);
      for (int i = tid; i < D; i += nth) dst[i] = topo[i];                 // (= topo0: the step kernel restored it)
      for (int i = tid; i < NS; i += nth) dst[D + i] = g.shunt_bus[(size_t)lane * NS + i];
    }
    return;
  }
  if (g.done[lane]) return;                                    // the step failed: the episode is over, nothing is booked
  if (had_act) {
    const unsigned char* aff = s.aff + (size_t)lane * (L + S);
    if (r.cd_line > 0)
      for (int l = tid; l < L; l += nth) { int* cd = g.cooldown + (size_t)lane * L + l; if (aff[l] && *cd < r.cd_line) *cd = r.cd_line; }
    if (r.cd_sub > 0)
      for (int i = tid; i < S; i += nth) { int v = scd[i] > 0 ? scd[i] - 1 : 0; if (aff[L + i]) v = r.cd_sub; scd[i] = v; }
  } else if (r.cd_sub > 0) {
    for (int i = tid; i < S; i += nth) { const int v = scd[i] - n_steps; scd[i] = v > 0 ? v : 0; }
  }
  for (int i = tid; i < D; i += nth) { const int v = topo[i]; if (v >= 1) lb[i] = v; }   // _BackendAction.update_state: update_connected
}

// gpf_fanout_n1: the contingency lanes take the source's acting-path state
__global__ void topo_fanout_kernel(TopoDev g, TopoLanes s, int src, int dst0, int n_dst) {
  const int k = blockIdx.x;
  if (k >= n_dst) return;
  const int dst = dst0 + k, D = g.dim_topo, S = g.n_sub;
  for (int i = threadIdx.x; i < S; i += blockDim.x) s.sub_cd[(size_t)dst * S + i] = s.sub_cd[(size_t)src * S + i];
  for (int i = threadIdx.x; i < D; i += blockDim.x) s.last_bus[(size_t)dst * D + i] = s.last_bus[(size_t)src * D + i];
  if (threadIdx.x < 2) s.flags[(size_t)dst * 2 + threadIdx.x] = s.flags[(size_t)src * 2 + threadIdx.x];
  if (threadIdx.x < s.n_slot) s.act[(size_t)dst * s.n_slot + threadIdx.x] = s.act[(size_t)src * s.n_slot + threadIdx.x];
}
#endif  // GPF_TOPO_KERNEL
#endif  // __HIPCC__ && (GPF_TOPO_KERNEL || GPF_LA_KERNEL)

}  // namespace gpf
