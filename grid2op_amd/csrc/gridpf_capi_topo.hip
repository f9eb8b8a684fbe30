// gridpf_capi_topo.hip -- topology actions of the batched acting path: the entry points of the C ABI (include/gridpf.h: gpf_set_topo_rules ...
// gpf_get_topo_action_mask) and the host side of the kernels of gridpf_topo.hpp and gridpf_topo_mask.hpp, on the engine of
// gridpf_engine.hpp.  The planner's bookkeeping the read-back feeds (note_lane_row, topo_unmoved) stays in gridpf_capi.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#define GPF_TOPO_KERNEL
#include "gridpf_engine.hpp"
#include "gridpf_combined.hpp"

// the argument blocks of the acting path's kernels (the look-ahead's play kernel takes the same two)
gpf::TopoDev topo_dev(const gpf_engine* e) {
  const gpf::GridDev& g = e->g;
  gpf::TopoDev d{};
  d.dim_topo = g.dim_topo; d.n_line = g.n_line; d.n_sub = g.n_sub; d.n_shunt = g.n_shunt; d.n_busbar = g.n_busbar;
  d.line_or_pos = g.line_or_pos; d.line_ex_pos = g.line_ex_pos; d.shunt_sub = g.shunt_sub;
  d.topo = e->topo.p; d.shunt_bus = e->shunt_bus.p; d.cooldown = e->cooldown.p; d.topo0 = e->topo0.p; d.episode = e->episode.p; d.done = e->done.p;
  return d;
}

gpf::TopoLanes topo_lanes(const gpf_engine* e) {
  gpf::TopoLanes t{};
  t.act = e->ta_act.p; t.sub_cd = e->ta_sub_cd.p; t.last_bus = e->ta_last_bus.p; t.flags = e->ta_flags.p; t.aff = e->ta_aff.p;
  t.ep_snap = e->ta_ep_snap.p; t.list = e->ta_moved_list.list.p; t.list_rows = e->ta_moved_list.rows.p; t.pos_sub = e->ta_pos_sub.p; t.pos_other = e->ta_pos_other.p;
  t.n_slot = e->ta_n_slot;
  return t;
}

namespace {
constexpr size_t TOPO_LDS_LIMIT = 64 * 1024;      // LDS of one workgroup

// composite actions (more than one slot) or limits per area: the pre-step runs its GEN instantiation
bool topo_general(const gpf_engine* e) { return e->ta_n_slot > 1 || e->ta_n_area > 0; }

// dynamic LDS of the pre-step kernel for a setting of slots / areas / gathered items
size_t topo_prestep_lds_bytes(const gpf_engine* e, int n_slot, int n_area, int max_items) {
  const gpf::GridDev& g = e->g;
  return gpf::topo_prestep_lds_ints(g.dim_topo, g.n_line, g.n_sub, g.n_shunt, g.n_busbar, (n_slot > 1 || n_area > 0) ? max_items : -1) * sizeof(int);
}

// items of the longest composite of a table: n_slot times its longest entry (one index may sit in several slots of a lane)
int topo_max_items(int n_act, const int* act_off, int n_slot) {
  int longest = 0;
  for (int k = 0; k < n_act; ++k) longest = std::max(longest, act_off[k + 1] - act_off[k]);
  return n_slot * longest;
}

// substation of every topo_vect position (host; a header-only handle needs no more)
void topo_host_maps(gpf_engine* e) {
  const gpf::GridDev& g = e->g;
  if (!e->h_ta_pos_sub.empty()) return;
  std::vector<int> pos_sub(g.dim_topo, 0);
  for (int l = 0; l < g.n_line; ++l) { pos_sub[e->h_line_or_pos[l]] = e->h_line_or_sub[l]; pos_sub[e->h_line_ex_pos[l]] = e->h_line_ex_sub[l]; }
  for (int i = 0; i < g.n_gen; ++i) pos_sub[e->h_gen_pos[i]] = e->h_gen_sub[i];
  for (int i = 0; i < g.n_load; ++i) pos_sub[e->h_load_pos[i]] = e->h_load_sub[i];
  for (int i = 0; i < g.n_sto; ++i) pos_sub[e->h_sto_pos[i]] = e->h_sto_sub[i];
  e->h_ta_pos_sub = pos_sub;
}

gpf::TopoMaskGrid topo_mask_grid(const gpf_engine* e) {
  return gpf::TopoMaskGrid{e->g.dim_topo, e->g.n_line, e->g.n_sub, e->h_line_or_pos.data(), e->h_line_ex_pos.data(), e->h_ta_pos_sub.data()};
}

// the acting path's buffers + static maps, once per engine (lanes start as after gpf_reset_lanes)
int topo_enable(gpf_engine* e) {
  if (e->ta_on) return GPF_OK;
  const gpf::GridDev& g = e->g;
  const size_t lds = gpf::topo_prestep_lds_ints(g.dim_topo, g.n_line, g.n_sub, g.n_shunt, g.n_busbar) * sizeof(int);
  if (lds > TOPO_LDS_LIMIT) return fail(GPF_E_CAPACITY, "topology actions: the grid's rows do not fit the 64 KiB of LDS of the pre-step kernel");
  HIP_TRY(hipSetDevice(e->device));
  const size_t cap = (size_t)e->cap_lanes;
  std::vector<int> pos_other(g.dim_topo, -1);
  for (int l = 0; l < g.n_line; ++l) { pos_other[e->h_line_or_pos[l]] = e->h_line_ex_pos[l]; pos_other[e->h_line_ex_pos[l]] = e->h_line_or_pos[l]; }
  topo_host_maps(e);
  HIP_TRY(e->ta_pos_sub.upload(e->h_ta_pos_sub.data(), e->h_ta_pos_sub.size()));
  HIP_TRY(e->ta_pos_other.upload(pos_other.data(), pos_other.size()));
  if (e->ta_n_area) HIP_TRY(e->ta_sub_area.upload(e->h_ta_sub_area.data(), e->h_ta_sub_area.size()));
  HIP_TRY(e->ta_act.alloc(cap * e->ta_n_slot)); HIP_TRY(e->ta_sub_cd.alloc(cap * g.n_sub)); HIP_TRY(e->ta_last_bus.alloc(cap * g.dim_topo));
  HIP_TRY(e->ta_ep_snap.alloc(cap)); HIP_TRY(e->ta_moved_list.alloc(cap, (size_t)g.dim_topo + g.n_shunt));
  HIP_TRY(e->ta_flags.alloc(cap * 2)); HIP_TRY(e->ta_aff.alloc(cap * ((size_t)g.n_line + g.n_sub)));
  HIP_TRY(hipMemsetAsync(e->ta_aff.p, 0, cap * ((size_t)g.n_line + g.n_sub), e->stream));
  e->ta_moved.assign(cap, 0);
  e->ta_n_moved = 0;
  e->ta_on = true;
  for (int v : e->h_init_topo) e->ta_may_split |= v >= 2;
  return topo_reset_lanes(e, 0, (int)cap);
}

// the acting path's row accessors below: argument checks (the first call allocates the acting path's buffers), one row range, a
// synchronisation (the caller may reuse its array at once)
template <typename T>
int topo_rows(gpf_engine* e, DevArr<T>& arr, size_t stride, int lane0, int n, T* get, const T* set, const char* who) {
  if (!check_range(e, lane0, n) || (!get && !set && n)) return fail(GPF_E_INVALID, std::string(who) + ": bad range");
  int rc = topo_enable(e);
  if (rc != GPF_OK || n == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(rows_to_host(e, get, arr, stride, lane0, n));
  HIP_TRY(rows_to_device(e, arr, set, stride, lane0, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}
}  // namespace

// Steps 1-4 of the acting path on the device (topo_prestep_kernel), then the host's planning bookkeeping of the lanes it moved to another
// topology class or busbar count: ONE compact read-back (count, lane ids, rows), skipped when the table cannot move a lane.
int topo_prestep(gpf_engine* e, bool acts) {
  const gpf::GridDev& g = e->g;
  const bool readback = acts && g.n_busbar >= 2 && (e->ta_bus_items || e->ta_may_split);
  if (acts) HIP_TRY(hipMemsetAsync(e->ta_moved_list.list.p, 0, sizeof(int), e->stream));
  const gpf::TopoTab tab{e->ta_off.p, e->ta_items.p, e->ta_amb.p, e->ta_n_act};
  const bool gen = topo_general(e);          // composite actions or areas: the GEN instantiation; else the kernel of one entry per lane
  const gpf::TopoComp comp{e->ta_n_area ? e->ta_sub_area.p : nullptr, e->ta_n_area, e->ta_max_items};
  const size_t lds = acts ? topo_prestep_lds_bytes(e, e->ta_n_slot, e->ta_n_area, e->ta_max_items) : 0;
  hipLaunchKernelGGL(gen ? gpf::topo_prestep_kernel<true> : gpf::topo_prestep_kernel<false>, dim3((unsigned)e->n_lanes), dim3(64), lds, e->stream,
                     topo_dev(e), tab, topo_lanes(e), e->ta_rules, comp, e->n_lanes, acts ? 1 : 0);
  HIP_TRY(hipGetLastError());
  if (!readback) return GPF_OK;
  return topo_readback(e, true);
}

// Step 5 (topo_poststep_kernel).  list_resets: the lanes that auto-reset in this launch are listed for topo_readback
int topo_poststep(gpf_engine* e, bool acts, int n_steps, bool list_resets) {
  if (list_resets) HIP_TRY(hipMemsetAsync(e->ta_moved_list.list.p, 0, sizeof(int), e->stream));
  hipLaunchKernelGGL(gpf::topo_poststep_kernel, dim3((unsigned)e->n_lanes), dim3(64), 0, e->stream, topo_dev(e), topo_lanes(e), e->ta_rules,
                     e->n_lanes, acts ? 1 : 0, n_steps, list_resets ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

// The compact list the topology kernels left in ta_moved_list -> the host's per-lane planning bookkeeping (note_lane_row: what
// gpf_set_topology does).  moved: the rows are action results (the lane's class may differ from its reset topology's); else they are
// reset topologies (the lane is back on the class of the rows last sent).
int topo_readback(gpf_engine* e, bool moved) {
  return moved_list_readback(e, e->ta_moved_list, 0, e->n_lanes, "gpf_step_n: internal (topology read-back", [e, moved](int lane) {
    if (moved && !e->ta_moved[lane]) { e->ta_moved[lane] = 1; ++e->ta_n_moved; }
    if (!moved && e->ta_moved[lane]) { e->ta_moved[lane] = 0; --e->ta_n_moved; }
  });
}

// acting-path state of lanes [lane0, lane0 + n) back to env.reset(): no cooldown, no pending action, last known busbar = the lanes'
// reset topology (busbar 1 where it has an open end)
int topo_reset_lanes(gpf_engine* e, int lane0, int n) {
  const gpf::GridDev& g = e->g;
  std::vector<int> lb((size_t)n * g.dim_topo), act((size_t)n * e->ta_n_slot, -1);
  for (int k = 0; k < n; ++k)
    for (int i = 0; i < g.dim_topo; ++i) lb[(size_t)k * g.dim_topo + i] = std::max(e->h_init_topo[i], 1);
  HIP_TRY(hipMemcpyAsync(e->ta_last_bus.p + (size_t)lane0 * g.dim_topo, lb.data(), lb.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->ta_act.p + (size_t)lane0 * e->ta_n_slot, act.data(), act.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemsetAsync(e->ta_sub_cd.p + (size_t)lane0 * g.n_sub, 0, (size_t)n * g.n_sub * sizeof(int), e->stream));
  HIP_TRY(hipMemsetAsync(e->ta_flags.p + (size_t)lane0 * 2, 0, (size_t)n * 2, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));                 // (the host vectors go out of scope)
  return GPF_OK;
}

// gpf_copy_lanes: the acting path's state, and whether an action has the lane on another topology class than its reset topology's
hipError_t topo_copy_lanes(gpf_engine* e, int src, int dst, int n) {
  const gpf::GridDev& g = e->g;
  hipError_t err = rows_copy(e, e->ta_sub_cd, g.n_sub, src, dst, n);
  if (err == hipSuccess) err = rows_copy(e, e->ta_last_bus, g.dim_topo, src, dst, n);
  if (err == hipSuccess) err = rows_copy(e, e->ta_flags, 2, src, dst, n);
  if (err == hipSuccess) err = rows_copy(e, e->ta_act, e->ta_n_slot, src, dst, n);
  if (err != hipSuccess) return err;
  for (int k = 0; k < n; ++k) { e->ta_n_moved += e->ta_moved[src + k] - e->ta_moved[dst + k]; e->ta_moved[dst + k] = e->ta_moved[src + k]; }
  return hipSuccess;
}

// gpf_fanout_n1: the contingency lanes take the source's acting-path state (cooldowns, last known busbars)
int topo_fanout_lanes(gpf_engine* e, int src, int dst0, int n_out) {
  hipLaunchKernelGGL(gpf::topo_fanout_kernel, dim3((unsigned)n_out), dim3(64), 0, e->stream, topo_dev(e), topo_lanes(e), src, dst0, n_out);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

extern "C" {

int gpf_set_topo_rules(gpf_handle e, int32_t on, int32_t max_sub_changed, int32_t max_line_status_changed, int32_t cooldown_sub,
                       int32_t cooldown_line) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_topo_rules: null");
  if (max_sub_changed < 0 || max_line_status_changed < 0 || cooldown_sub < 0 || cooldown_line < 0)
    return fail(GPF_E_INVALID, "gpf_set_topo_rules: negative parameter");
  if (e->ta_n_area && on && (max_sub_changed > gpf::TM_AREA_MAX_LIMIT || max_line_status_changed > gpf::TM_AREA_MAX_LIMIT))
    return fail(GPF_E_INVALID, "gpf_set_topo_rules: with areas set (gpf_set_topo_areas) the two limits must not exceed 254 (8-bit per-area counters)");
  int rc = topo_enable(e);
  if (rc != GPF_OK) return rc;
  e->ta_rules = gpf::TopoRules{on ? 1 : 0, max_sub_changed, max_line_status_changed, cooldown_sub, cooldown_line};
  return GPF_OK;
}

int gpf_upload_topo_actions(gpf_handle e, int32_t n_act, const int32_t* act_off, const int32_t* act_items, uint8_t* ambiguous) {
  if (!e || n_act < 0 || (n_act > 0 && !act_off)) return fail(GPF_E_INVALID, "gpf_upload_topo_actions: bad arguments");
  const gpf::GridDev& g = e->g;
  const int n_items_total = n_act ? act_off[n_act] : 0;
  if (n_act && (act_off[0] != 0 || (n_items_total > 0 && !act_items))) return fail(GPF_E_INVALID, "gpf_upload_topo_actions: bad action offsets");
  for (int k = 0; k < n_act; ++k) if (act_off[k + 1] < act_off[k]) return fail(GPF_E_INVALID, "gpf_upload_topo_actions: bad action offsets");
  bool bus_items = false;
  if (int rc_i = check_action_items(e, "gpf_upload_topo_actions", n_items_total, act_items, &bus_items)) return rc_i;
  const int max_items = topo_max_items(n_act, act_off, e->ta_n_slot);
  if (topo_prestep_lds_bytes(e, e->ta_n_slot, e->ta_n_area, max_items) > TOPO_LDS_LIMIT)
    return fail(GPF_E_INVALID, "gpf_upload_topo_actions: the gathered item list (gpf_set_topo_slots times the table's longest entry) does not fit "
                               "the 64 KiB of LDS of the pre-step kernel");
  topo_host_maps(e);
  // static ambiguity of every entry and the static summary the legality masks are evaluated from (gridpf_topo_mask.hpp)
  std::vector<unsigned char> amb((size_t)n_act, 0);
  const gpf::TopoMaskGrid mg = topo_mask_grid(e);
  gpf::topo_static_ambiguity(mg, n_act, act_off, act_items, amb.data());
  gpf::TopoMaskSummary ms;
  if (!gpf::build_topo_mask_summary(mg, n_act, act_off, act_items, amb.data(), ms, e->ta_n_area ? e->h_ta_sub_area.data() : nullptr))
    return fail(GPF_E_CAPACITY, "gpf_upload_topo_actions: more than 2^20 - 1 lines or substations (the summary words of the legality masks)");
  if (e->dry) {                                             // header-only handle: the table on the host (gpf_get_topo_action_areas)
    e->h_ta_off.assign(act_off, act_off + (n_act ? n_act + 1 : 0)); e->h_ta_items.assign(act_items, act_items + 3 * (size_t)n_items_total);
    e->h_ta_amb = amb; e->ta_n_act = n_act; e->ta_max_items = max_items;
    if (ambiguous) std::memcpy(ambiguous, amb.data(), amb.size());
    return GPF_OK;
  }
  int rc = topo_enable(e);
  if (rc != GPF_OK) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));                 // (a launch in flight may read the old table)
  e->ta_off.release(); e->ta_items.release(); e->ta_amb.release(); e->ta_sto_word.release();
  e->ta_m_off.release(); e->ta_m_line.release(); e->ta_m_sub.release(); e->ta_m_end.release(); e->ta_mask.release();
  e->ta_n_act = 0;
  if (n_act) {
    HIP_TRY(e->ta_off.upload(act_off, (size_t)n_act + 1));
    if (n_items_total) HIP_TRY(e->ta_items.upload(act_items, 3 * (size_t)n_items_total));
    HIP_TRY(e->ta_amb.upload(amb.data(), amb.size()));
    std::vector<unsigned long long> sto_word((size_t)n_act, 0);      // the storage units every entry reconnects or moves (gridpf_combined.hpp)
    gpf::combined_entry_words(n_act, act_off, act_items, g.n_sto, e->h_sto_pos.data(), sto_word.data());
    HIP_TRY(e->ta_sto_word.upload(sto_word.data(), sto_word.size()));
    HIP_TRY(e->ta_m_off.upload(ms.off.data(), ms.off.size())); HIP_TRY(e->ta_m_line.upload(ms.line.data(), ms.line.size()));
    HIP_TRY(e->ta_m_sub.upload(ms.sub.data(), ms.sub.size())); HIP_TRY(e->ta_m_end.upload(ms.end.data(), ms.end.size()));
    HIP_TRY(e->ta_mask.alloc((size_t)e->cap_lanes * n_act));
    HIP_TRY(hipMemset(e->ta_mask.p, 0, (size_t)e->cap_lanes * n_act));
    e->ta_n_act = n_act;
  }
  e->h_ta_off.assign(act_off, act_off + (n_act ? n_act + 1 : 0)); e->h_ta_items.assign(act_items, act_items + 3 * (size_t)n_items_total);
  e->h_ta_amb = amb; e->ta_max_items = max_items;
  e->ta_bus_items = bus_items;
  for (int q = 0; q < n_items_total; ++q)
    e->ta_may_split |= (act_items[3 * q] == GPF_ACT_SET_BUS && act_items[3 * q + 2] >= 2) || act_items[3 * q] == GPF_ACT_CHANGE_BUS;
  if (ambiguous) std::memcpy(ambiguous, amb.data(), amb.size());
  return GPF_OK;
}

int gpf_set_lane_topo_actions(gpf_handle e, const int32_t* index) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_lane_topo_actions: null");
  if (!index) { e->ta_host = false; return GPF_OK; }
  int rc = topo_enable(e);
  if (rc != GPF_OK) return rc;
  HIP_TRY(hipMemcpyAsync(e->ta_act.p, index, (size_t)e->n_lanes * e->ta_n_slot * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));                 // (the caller may reuse `index`)
  e->ta_host = true;
  return GPF_OK;
}

int gpf_topo_actions_on_device(gpf_handle e, int32_t on) {
  if (!e) return fail(GPF_E_INVALID, "gpf_topo_actions_on_device: null");
  int rc = topo_enable(e);
  if (rc != GPF_OK) return rc;
  e->ta_dev = on != 0;
  return GPF_OK;
}

int gpf_set_topo_areas(gpf_handle e, int32_t n_area, const int32_t* sub_area) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_topo_areas: null");
  const gpf::GridDev& g = e->g;
  if (n_area < 0) return fail(GPF_E_INVALID, "gpf_set_topo_areas: negative number of areas");
  if (n_area == 0 || !sub_area) n_area = 0;
  if (n_area > gpf::TM_MAX_AREAS) return fail(GPF_E_INVALID, "gpf_set_topo_areas: at most 16 areas");
  std::vector<int> area, seen((size_t)n_area, 0);
  if (n_area) {
    area.assign(sub_area, sub_area + g.n_sub);
    for (int v : area) {
      if (v < 0 || v >= n_area) return fail(GPF_E_INVALID, "gpf_set_topo_areas: a substation's area is outside [0, n_area)");
      seen[v] = 1;
    }
    for (int k = 0; k < n_area; ++k) if (!seen[k]) return fail(GPF_E_INVALID, "gpf_set_topo_areas: an area holds no substation");
    if (e->ta_rules.on && (e->ta_rules.max_sub > gpf::TM_AREA_MAX_LIMIT || e->ta_rules.max_line > gpf::TM_AREA_MAX_LIMIT))
      return fail(GPF_E_INVALID, "gpf_set_topo_areas: the limits of gpf_set_topo_rules exceed 254 (8-bit per-area counters)");
    if (topo_prestep_lds_bytes(e, e->ta_n_slot, n_area, e->ta_max_items) > TOPO_LDS_LIMIT)
      return fail(GPF_E_INVALID, "gpf_set_topo_areas: the pre-step kernel's rows do not fit the 64 KiB of LDS of a workgroup");
  }
  topo_host_maps(e);
  // the static areas in the summary of an uploaded table are re-derived
  gpf::TopoMaskSummary ms;
  const bool table = e->ta_n_act > 0;
  if (table && !gpf::build_topo_mask_summary(topo_mask_grid(e), e->ta_n_act, e->h_ta_off.data(), e->h_ta_items.data(), e->h_ta_amb.data(), ms,
                                             n_area ? area.data() : nullptr))
    return fail(GPF_E_CAPACITY, "gpf_set_topo_areas: internal (summary)");
  if (!e->dry) {
    int rc = topo_enable(e);
    if (rc != GPF_OK) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));               // (a launch in flight may read the old areas)
    if (n_area) HIP_TRY(e->ta_sub_area.upload(area.data(), area.size())); else e->ta_sub_area.release();
    if (table) { HIP_TRY(e->ta_m_line.upload(ms.line.data(), ms.line.size())); HIP_TRY(e->ta_m_sub.upload(ms.sub.data(), ms.sub.size())); }
  }
  e->h_ta_sub_area = area;
  e->ta_n_area = n_area;
  return GPF_OK;
}

int gpf_set_topo_slots(gpf_handle e, int32_t n_slot) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_topo_slots: null");
  if (n_slot < 1 || n_slot > 8) return fail(GPF_E_INVALID, "gpf_set_topo_slots: n_slot must be 1..8");
  const int max_items = e->ta_n_act ? topo_max_items(e->ta_n_act, e->h_ta_off.data(), n_slot) : 0;
  if (topo_prestep_lds_bytes(e, n_slot, e->ta_n_area, max_items) > TOPO_LDS_LIMIT)
    return fail(GPF_E_INVALID, "gpf_set_topo_slots: the gathered item list (n_slot times the table's longest entry) does not fit the 64 KiB of LDS "
                               "of the pre-step kernel");
  if (!e->dry) {
    int rc = topo_enable(e);
    if (rc != GPF_OK) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (n_slot != e->ta_n_slot) {                           // a buffer of the new shape, all slots empty: pending indices are dropped
      std::vector<int> none((size_t)e->cap_lanes * n_slot, -1);
      HIP_TRY(e->ta_act.upload(none.data(), none.size()));
      e->ta_host = e->ta_dev = false;
    }
  }
  e->ta_n_slot = n_slot;
  e->ta_max_items = max_items;
  return GPF_OK;
}

int gpf_get_topo_action_areas(gpf_handle e, uint32_t* areas) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_topo_action_areas: null");
  if (e->ta_n_act == 0) return fail(GPF_E_INVALID, "gpf_get_topo_action_areas: no action table (gpf_upload_topo_actions)");
  if (!areas) return fail(GPF_E_INVALID, "gpf_get_topo_action_areas: null output");
  gpf::topo_action_areas(topo_mask_grid(e), e->ta_n_act, e->h_ta_off.data(), e->h_ta_items.data(), e->ta_n_area ? e->h_ta_sub_area.data() : nullptr,
                         e->g.n_shunt ? e->h_shunt_sub.data() : nullptr, areas);
  return GPF_OK;
}

int gpf_get_sub_cooldown(gpf_handle e, int32_t lane0, int32_t n, int32_t* sub_cooldown) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_sub_cooldown: null");
  return topo_rows<int>(e, e->ta_sub_cd, e->g.n_sub, lane0, n, sub_cooldown, nullptr, "gpf_get_sub_cooldown");
}
int gpf_set_sub_cooldown(gpf_handle e, int32_t lane0, int32_t n, const int32_t* sub_cooldown) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_sub_cooldown: null");
  if (sub_cooldown) for (size_t i = 0; i < (size_t)std::max(n, 0) * e->g.n_sub; ++i)
    if (sub_cooldown[i] < 0) return fail(GPF_E_INVALID, "gpf_set_sub_cooldown: negative cooldown");
  return topo_rows<int>(e, e->ta_sub_cd, e->g.n_sub, lane0, n, nullptr, sub_cooldown, "gpf_set_sub_cooldown");
}
int gpf_get_last_bus(gpf_handle e, int32_t lane0, int32_t n, int32_t* last_bus) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_last_bus: null");
  return topo_rows<int>(e, e->ta_last_bus, e->g.dim_topo, lane0, n, last_bus, nullptr, "gpf_get_last_bus");
}
int gpf_set_last_bus(gpf_handle e, int32_t lane0, int32_t n, const int32_t* last_bus) {
  if (!e) return fail(GPF_E_INVALID, "gpf_set_last_bus: null");
  if (last_bus) for (size_t i = 0; i < (size_t)std::max(n, 0) * e->g.dim_topo; ++i) {
    if (last_bus[i] < 1 || last_bus[i] > e->g.n_busbar) return fail(GPF_E_INVALID, "gpf_set_last_bus: busbars must be 1..n_busbar");
    e->ta_may_split |= last_bus[i] >= 2;
  }
  return topo_rows<int>(e, e->ta_last_bus, e->g.dim_topo, lane0, n, nullptr, last_bus, "gpf_set_last_bus");
}
int gpf_get_topo_flags(gpf_handle e, int32_t lane0, int32_t n, uint8_t* flags) {
  if (!e) return fail(GPF_E_INVALID, "gpf_get_topo_flags: null");
  return topo_rows<unsigned char>(e, e->ta_flags, 2, lane0, n, flags, nullptr, "gpf_get_topo_flags");
}

int gpf_topo_action_mask(gpf_handle e, int32_t lane0, int32_t n, uint8_t* out_dev, int64_t row_stride) {
  if (!e) return fail(GPF_E_INVALID, "gpf_topo_action_mask: null");
  if (e->dry) return fail(GPF_E_INVALID, "gpf_topo_action_mask: header-only handle");
  if (!check_range(e, lane0, n)) return fail(GPF_E_INVALID, "gpf_topo_action_mask: bad lane range");
  if (!e->ta_on || e->ta_n_act == 0) return fail(GPF_E_INVALID, "gpf_topo_action_mask: no action table (gpf_upload_topo_actions)");
  if (out_dev && row_stride < e->ta_n_act) return fail(GPF_E_INVALID, "gpf_topo_action_mask: row_stride is smaller than the table's number of entries");
  if (n == 0) return GPF_OK;
  const gpf::GridDev& g = e->g;
  const size_t lds = (2 * (size_t)gpf::tm_words(g.n_line) + gpf::tm_words(g.n_sub)) * sizeof(unsigned long long);
  if (lds > 64 * 1024) return fail(GPF_E_CAPACITY, "gpf_topo_action_mask: the grid's line and substation bit sets do not fit 64 KiB of LDS");
  HIP_TRY(hipSetDevice(e->device));
  const gpf::TopoMaskTab tab{e->ta_m_off.p, e->ta_m_line.p, e->ta_m_sub.p, e->ta_m_end.p, e->ta_amb.p, e->ta_n_act};
  const gpf::TopoMaskLanes s{e->topo.p, e->cooldown.p, e->ta_sub_cd.p, e->line_or_pos.p, e->line_ex_pos.p, g.dim_topo, g.n_line, g.n_sub};
  const gpf::TopoRules& r = e->ta_rules;
  unsigned char* dst = out_dev ? out_dev : e->ta_mask.p + (size_t)lane0 * e->ta_n_act;
  const unsigned chunks = (unsigned)std::min((e->ta_n_act + gpf::TM_CHUNK - 1) / gpf::TM_CHUNK, 65535);
  hipLaunchKernelGGL(gpf::topo_mask_kernel, dim3((unsigned)n, chunks), dim3(64), lds, e->stream, tab, s, r.on, r.max_line, r.max_sub, lane0, n, dst,
                     out_dev ? (long long)row_stride : (long long)e->ta_n_act, (r.on && e->ta_n_area) ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return GPF_OK;
}

int gpf_get_topo_action_mask(gpf_handle e, int32_t lane0, int32_t n, uint8_t* host_out) {
  int rc = gpf_topo_action_mask(e, lane0, n, nullptr, 0);      // (its refusals first: they say what is missing)
  if (rc != GPF_OK) return rc;
  if (n > 0 && !host_out) return fail(GPF_E_INVALID, "gpf_get_topo_action_mask: null output");
  if (n > 0)
    HIP_TRY(hipMemcpyAsync(host_out, e->ta_mask.p + (size_t)lane0 * e->ta_n_act, (size_t)n * e->ta_n_act, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GPF_OK;
}

}  // extern "C"
