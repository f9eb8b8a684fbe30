// gridpf_engine.hpp -- what the C ABI units (gridpf_capi*.hip) share: the engine behind a gpf_handle, the owners of its device memory, pinned
// blocks, stream and events, the error plumbing, the row copies of lane-major arrays and the hooks each feature's unit offers the shared
// lifecycle code of gridpf_capi.hip.  Host-only: no header that defines a non-template kernel outside its unit's guard (each has one unit).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/gridpf.h"
#include "gridpf_common.hpp"
#include "gridpf_host.hpp"
#include "gridpf_lane_fan.hpp"
#include "gridpf_symbolic.hpp"
#include "gridpf_topo.hpp"                  // (TopoRules; its kernels exist in gridpf_capi_topo.hip only)

#pragma GCC visibility push(hidden)         // internal to libgridpf.so: only the gpf_* entry points are its interface

inline thread_local std::string g_err;      // gpf_last_error

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return fail(GPF_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));         \
  } while (0)

// gpf_create(device = GPF_DEVICE_NONE): a HEADER-ONLY handle is being built -- every host-side step of gpf_create runs (symbolic analysis, static
// tables, launch planning), nothing is allocated on or copied to a device (there may be none).  Thread-local: set for the duration of that call.
inline thread_local bool g_dry_create = false;

constexpr size_t LDS_HARD_LIMIT = 160 * 1024 - 256;   // dynamic LDS budget (a few static bytes: block-wide reductions)

// `n` elements of T in device memory, freed with the owner (move-only)
template <typename T>
struct DevArr {
  T* p = nullptr;
  size_t n = 0;
  size_t cap = 0;                          // elements allocated (ensure / put: grow-only buffers reused across calls)
  DevArr() = default;
  DevArr(const DevArr&) = delete; DevArr& operator=(const DevArr&) = delete;
  DevArr(DevArr&& o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
  ~DevArr() { release(); }
  hipError_t alloc(size_t count) {         // a new block (the old one is freed first)
    release();
    n = count;
    if (count == 0 || g_dry_create) return hipSuccess;
    return hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
  }
  hipError_t upload(const T* src, size_t count) {
    hipError_t e = alloc(count);
    if (e != hipSuccess || count == 0 || g_dry_create) return e;
    return hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    cap = 0;
  }
  hipError_t ensure(size_t count) {        // room for `count` elements; contents undefined afterwards when it had to grow
    if (count <= cap && p) { n = count; return hipSuccess; }
    release();
    const size_t want = count + count / 4;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(want, 1) * sizeof(T));
    cap = e == hipSuccess ? std::max<size_t>(want, 1) : 0;
    n = e == hipSuccess ? count : 0;
    return e;
  }
  hipError_t put(const T* src, size_t count, hipStream_t stream) {   // ensure + asynchronous upload on `stream` (src must stay alive until it ran)
    hipError_t e = ensure(count);
    if (e != hipSuccess || count == 0) return e;
    return hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, stream);
  }
};

// grow-only pinned host block of `n` elements of T (hipHostMalloc with `flags`), freed with the owner.  Mapped blocks also hold their
// device-side address (`dev`).
template <typename T>
struct HostPin {
  T* p = nullptr;
  T* dev = nullptr;
  size_t n = 0;
  const unsigned flags;
  explicit HostPin(unsigned flags_ = hipHostMallocDefault) : flags(flags_) {}
  HostPin(const HostPin&) = delete; HostPin& operator=(const HostPin&) = delete;
  ~HostPin() { if (p) (void)hipHostFree(p); }
  // room for `need` elements: a block of need + slack when it has to grow (contents undefined afterwards)
  hipError_t reserve(size_t need, size_t slack = 0) {
    if (need <= n) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = dev = nullptr; n = 0;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), (need + slack) * sizeof(T), flags);
    if (e != hipSuccess) return e;
    n = need + slack;
    if (flags & hipHostMallocMapped) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), p, 0);
    return e;
  }
};

// a HIP stream / event destroyed with the owner; both convert to the raw handle
struct Stream {
  hipStream_t h = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
  ~Stream() { if (h) (void)hipStreamDestroy(h); }
  hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&h, flags); }
  operator hipStream_t() const { return h; }
};

struct Event {
  hipEvent_t h = nullptr;
  Event() = default;
  Event(const Event&) = delete; Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : h(o.h) { o.h = nullptr; }
  ~Event() { if (h) (void)hipEventDestroy(h); }
  hipError_t create() { return hipEventCreate(&h); }
  hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&h, flags); }
  operator hipEvent_t() const { return h; }
};

// A moved-lane list: the lanes whose topology row a kernel moved off the one the host noted (device: count | lane ids, and their rows),
// with the pinned block the host reads it back into (moved_list_readback)
struct MovedList {
  DevArr<int> list, rows;
  HostPin<int> pin;
  hipError_t alloc(size_t cap, size_t w) { hipError_t err = list.alloc(cap + 1); return err == hipSuccess ? rows.alloc(cap * w) : err; }
  void release() { list.release(); rows.release(); }
};
using LaneFan = LaneFanT<LaunchPlan, DevArr<int>>;

struct gpf_engine {
  ~gpf_engine();                        // (gridpf_capi.hip: waits for the stream; the members free themselves)
  int device = 0;
  bool dry = false;                     // header-only handle (gpf_create with GPF_DEVICE_NONE): no device resources, no launches
  int n_lanes = 0;
  Stream stream;
  gpf::GridDev g{};
  gpf::OutOff oo{};
  gpf_layout layout{};
  // static tables (device)
  DevArr<double> sub_vn_kv, br_y, br_bdc, gen_min_q, gen_max_q, shunt_fact;
  DevArr<int> line_or_sub, line_ex_sub, line_or_pos, line_ex_pos, gen_sub, gen_pos, load_sub, load_pos, sto_sub, sto_pos,
      shunt_sub;
  DevArr<unsigned char> gen_slack;
  // host copies needed to size launches
  std::vector<int> h_line_or_sub, h_line_ex_sub, h_line_or_pos, h_line_ex_pos, h_gen_sub, h_gen_pos, h_load_sub, h_load_pos,
      h_sto_sub, h_sto_pos, h_shunt_sub;
  std::vector<unsigned char> h_gen_slack;
  std::vector<double> h_init_inj;
  std::vector<int> h_init_topo, h_init_shunt_bus;
  // per-lane state (device)
  DevArr<double> inj, bus_vm, bus_va, work;
  DevArr<int> topo, shunt_bus, topo_out, shunt_bus_out, status, overflow_count, disc_round, lane_table, lane_offset, tmp_lines;
  DevArr<int> cooldown;                 // [B][n_line] line cooldowns of the environment (gpf::Bufs::cooldown)
  // topology actions of the batched acting path (gridpf_topo.hpp, gridpf_capi_topo.hip): allocated by the first gpf_set_topo_rules /
  // gpf_upload_topo_actions
  bool ta_on = false;
  gpf::TopoRules ta_rules{};            // (on = 0 until gpf_set_topo_rules)
  DevArr<int> ta_act, ta_sub_cd, ta_last_bus, ta_ep_snap, ta_off, ta_items, ta_pos_sub, ta_pos_other;
  DevArr<unsigned char> ta_flags, ta_aff, ta_amb;
  int ta_n_act = 0;
  // legality masks of the table (gridpf_topo_mask.hpp): its static summary, uploaded with it, and the engine-owned masks [cap_lanes][ta_n_act]
  DevArr<int> ta_m_off, ta_m_line, ta_m_sub, ta_m_end;
  DevArr<unsigned char> ta_mask;
  std::vector<int> h_ta_pos_sub;        // substation of every topo_vect position (host copy of ta_pos_sub)
  // composite actions and rules by area (gpf_set_topo_slots / gpf_set_topo_areas): areas belong to the rules, not to lanes
  int ta_n_slot = 1;                    // table entries per lane and step: ta_act is [cap_lanes][ta_n_slot]
  int ta_max_items = 0;                 // ta_n_slot x the items of the table's longest entry (the gathered item list of the pre-step)
  int ta_n_area = 0;                    // 0: whole-grid limits
  std::vector<int> h_ta_sub_area;       // [n_sub] area of every substation (empty without areas)
  DevArr<int> ta_sub_area;
  std::vector<int> h_ta_off, h_ta_items;        // host copy of the table (a header-only handle has nothing else; areas set later re-derive the summary)
  std::vector<unsigned char> h_ta_amb;
  bool ta_bus_items = false;           // an entry of the table sets / changes a bus: the read-back of class changes is needed
  bool ta_may_split = false;            // some row or last-bus entry was on a busbar >= 2 (then line-status actions can change a class key too)
  bool ta_host = false, ta_dev = false; // the next launch carries indices set by the host / written on the device
  std::vector<char> ta_moved;           // per lane: an action moved it to another topology class than its reset topology's (auto-reset re-keys it)
  int ta_n_moved = 0;
  MovedList ta_moved_list;              // the lanes the pre-step moved, the lanes that auto-reset or were truncated
  // topology-derived state of the reference topology shared by the lanes of one-step launches (gpf::KeepArgs): two blobs (Ybus in LDS /
  // in registers), allocated and keyed by the first gpf_step_n with n_steps = 1; GRIDPF_KEEP=0 at gpf_create turns it off
  DevArr<unsigned char> keep;
  gpf::KeepArgs keep_args{};
  int keep_launch = 0;
  bool keep_enabled = true;
  DevArr<unsigned short> maint_dur;     // [chron_tables][chron_T][n_line] remaining duration of the maintenance / hazard under way, or empty
  DevArr<short> traj_cool;              // [traj_cap][cap_lanes][n_line]
  DevArr<float> out, chron, lane_scale, thermal_limit, rho;
  DevArr<unsigned char> line_status, done;
  DevArr<int> topo0, episode;           // topology last sent by the host (auto-reset target); {steps survived, resets} per lane
  DevArr<float> lane_gen_delta, traj_rho;
  DevArr<unsigned char> maint;          // [chron_tables][chron_T][n_line] scheduled maintenance OR hazards (forced outages), or empty
  std::vector<unsigned char> h_maint, h_hazard;   // host copies of the two tables (the device holds their union)
  std::vector<unsigned short> h_outage_dur;       // gpf_upload_outage_durations: remaining durations given by the caller (else derived from the tables)
  std::vector<int> h_lane_table, h_lane_offset;   // host mirror of lane_table / lane_offset (gpf_simulate_batch: maintenance ahead of a source lane)
  std::vector<char> h_lane_forecast;              // 1: the lane is a scratch lane of gpf_simulate_batch (its offset is an absolute row, of the forecast tables for time_step > 0)
  // injection dynamics of the environment (gpf::EnvDyn, gridpf_capi_env.hip)
  bool env_on = false, env_hold = false, env_act_r = false, env_act_s = false, sto_ready = false;
  int env_loss_on = 1;
  double env_coeff = 300.0 / 3600.0, env_tol = 1e-2;
  DevArr<float> env_target, env_actual, env_prev, env_charge, env_amount_prev, env_act_redisp, sto_charge0;
  float* env_act_storage = nullptr;     // [B][n_storage]: the tail of env_act_redisp (one allocation, one DMA for both action rows)
  DevArr<float> env_limit, env_curt_prev, env_act_curtail;
  DevArr<int> env_illegal;              // [B] cancelled (illegal) actions since the reset
  DevArr<unsigned char> env_already, env_fresh, env_renewable;
  bool env_act_c = false, env_has_ren = false;
  DevArr<double> sto_emax, sto_emin, sto_loss, sto_effc, sto_effd;
  std::vector<float> h_charge0;
  DevArr<float> forecast;               // [chron_tables][chron_T][fc_h][n_chron] *_forecasted tables (gpf_upload_forecasts), or empty
  int fc_h = 0;
  DevArr<int> sim_src, sim_rows;        // gpf_simulate_batch staging: source lane list, gathered topology rows
  struct PtdfbCached { std::vector<int> row, desc, c2b; };      // gpf_ptdf_build_batch: descriptor of a topology row seen before
  std::unordered_map<uint64_t, std::vector<PtdfbCached>> ptdfb_cache;
  size_t ptdfb_cache_n = 0;
  int ptdfb_cache_stride = 0;
  HostPin<unsigned char> res_pin;       // pinned block of gpf_get_results_pinned
  HostPin<float> act_pin;               // pinned staging of gpf_set_lane_actions / gpf_set_lane_curtailment (redispatch | storage | curtailment)
  Event act_up;                         // recorded behind the uploads that read it: the next call waits for it before rewriting the block
  HostPin<int> sim_pin;                 // its pinned host block (grow-only): gathered source rows | candidate topology rows | candidate shunt rows
  DevArr<signed char> traj_status;
  DevArr<float> traj_out;               // per-step observation trajectory (GPF_TRAJ_OBS): [traj_cap][cap_lanes][n_out] ...
  DevArr<int> traj_topo, traj_shb;
  DevArr<unsigned char> traj_lstat;
  int traj_cap = 0;
  int traj_what = 0;                    // GPF_TRAJ_* bits of the current buffers
  int traj_valid = 0;                   // steps of the trajectory written by the last gpf_step_n
  // observation vectors assembled on the device (gridpf_obs.hpp, gridpf_capi_obs.hip): the spec's segment table, the per-element affine map,
  // the calendar of the chronics tables and the maintenance look-ahead derived from the uploaded maintenance table
  bool obs_spec_on = false, obs_clock_on = false, obs_gof = true;
  int obs_dim = 0, obs_n_seg = 0;
  std::vector<int> h_obs_seg;           // [n_seg][5] {kind, source offset, length, destination offset, flags}
  DevArr<int> obs_seg;
  DevArr<float> obs_sub, obs_div, obs_vec;   // [dim], [dim], engine-owned output [cap_lanes][dim]
  DevArr<long long> obs_clock;          // [chron_tables] minutes since 1970-01-01 00:00 of row 0 of each table
  int obs_clock_tables = 0, obs_step_minutes = 5, obs_max_step = 0;
  DevArr<int> obs_maint_next, obs_maint_durn;   // [chron_tables][chron_T][n_line] time_next_maintenance / duration_next_maintenance at every row
  long long obs_maint_gen = -1, maint_gen = 0;  // generation of the outage tables the look-ahead was derived from / current generation
  // the observation as a bus graph (gridpf_graph.hpp, gridpf_capi_graph.hip): the static tables as one int blob, on the host and on the
  // device, the staging buffers of gpf_graph_obs_host (grow-only), and whether the kernel may copy a lane's rows into LDS (GRIDPF_GRAPH_STAGE)
  bool gr_on = false, gr_gof = true, gr_stage = true;
  std::vector<int> h_gr_tab;
  DevArr<int> gr_tab, gr_index;
  DevArr<float> gr_feat, gr_dense;
  // the opponent of the batched acting path (gridpf_opponent.hpp, gridpf_capi_opp.hip): its configuration (host), the attackable lines and
  // their normalisation, the per-lane state, the draws table and the Geometric schedules
  int opp_kind = 0;                     // GPF_OPP_*; 0: off -- gpf_step_n launches nothing for it
  gpf_opponent_desc opp_desc{};         // as validated (its pointers are not kept)
  int opp_n_draw = 0;
  DevArr<int> opp_lines, opp_state, opp_sched;
  DevArr<double> opp_norm, opp_budget, opp_draws;
  // ... and its areas (gpf_set_opponent_areas): the last validated descriptor's kind and lines on the host (kept on a header-only handle
  // too, so that everything about areas can be refused there), the lines grouped by area with each area's offset, and the per-(lane, area)
  // state and schedules.  opp_n_area 0: the single-area opponent.
  int opp_host_kind = 0, opp_n_area = 0;
  std::vector<int> opp_host_lines, opp_area_lines_host, opp_area_off;   // opp_area_off: [n_area + 1]
  DevArr<int> opp_area_lines, opp_area_tab, opp_area_state, opp_area_sched;   // opp_area_tab: [2][n_area] offsets, counts
  // alerts and AlertReward (gridpf_alert.hpp, gridpf_capi_alert.hip): the descriptor, the number of alertable lines (= the opponent's list
  // when gpf_set_alerts was called; al_host_A is kept on a header-only handle too, so that the masks can be refused there), the lanes'
  // observation block [cap_lanes][6 A + 1], words [cap_lanes][3 + 2 R], alert masks of the next launch and rewards of the last one
  bool al_on = false, al_host = false, al_dev = false;   // al_host / al_dev: the next launch carries masks set by the host / written on the device
  int al_A = 0, al_host_A = 0;
  gpf_alert_desc al_desc{};
  DevArr<int> al_obs, al_area_of;
  DevArr<unsigned long long> al_aux, al_act;
  DevArr<float> al_reward;
  // the environment's rewards (gridpf_reward.hpp, gridpf_capi_reward.hip): the slot table and the cost table on the device, the
  // engine-owned rewards [cap_lanes][rw_n_slot] of the last one-step launch and the snapshot of env_illegal queued before its step
  bool rw_on = false;
  int rw_n_slot = 0;
  bool rw_cost_on = false;              // a slot reads the cost table
  DevArr<unsigned char> rw_slots;       // [rw_n_slot] gpf_reward_slot
  DevArr<float> rw_cost, rw_out;
  DevArr<int> rw_ill_snap;              // [cap_lanes]
  // episode time limits (gridpf_episode.hpp, gridpf_capi_episode.hip): the lanes' limits, the flags / length / duration reward of the last
  // one-step launch, episode[lane][0] as that launch left it, and the statistics across launches (returns: [cap_lanes][8] float64).
  // ep_host_on: a header-only handle was given a valid limit (gpf_step_n refuses multi-step launches there too)
  bool ep_on = false, ep_host_on = false;
  float ep_per_timestep = 1.f, ep_alert_bonus = 0.f;
  DevArr<int> ep_limit, ep_length, ep_steps_prev, ep_length_last, ep_n_episodes;
  DevArr<unsigned char> ep_flags;
  DevArr<float> ep_duration;
  DevArr<double> ep_ret_run, ep_ret_last;
  // the chronics cursor (gridpf_cursor.hpp, gridpf_capi_cursor.hip): the validated configuration (host), the order and the cdf on the
  // device, the lanes' words, the byte that keeps the kernel off scratch and contingency lanes and the draws table.  cur_host_on: a
  // header-only handle was given a valid descriptor (gpf_step_n refuses multi-step launches there too)
  bool cur_on = false, cur_host_on = false;
  gpf_cursor_desc cur_desc{};           // as validated (its pointers are not kept)
  int cur_n_draw = 0, cur_max_table = 0, cur_max_first_row = 0;
  DevArr<int> cur_order, cur_pos, cur_next_pos, cur_n_started, cur_draws_used, cur_flags, cur_first_row;
  DevArr<unsigned char> cur_skip;
  DevArr<double> cur_cdf, cur_draws;
  // combined topology + injection actions (gridpf_combined.hpp, gridpf_capi_combined.hip): the step's flags [cap_lanes][4] of the last
  // one-step launch, the screen's verdict byte and the snapshot of env_illegal between its kernels, the storage units' power limits (empty:
  // not checked) and, uploaded with every action table, one word per entry: the storage units it reconnects or moves
  bool cb_on = false, cb_check = false;
  DevArr<unsigned char> cb_flags, cb_screen;
  DevArr<int> cb_ill_snap;
  DevArr<float> cb_max_prod, cb_max_absorb;
  DevArr<unsigned long long> ta_sto_word;
  LaneFan fan;                          // the lanes behind the environments: who owns them, the split, the cached plans of its two ranges
  // the N-1 screen (gridpf_n1.hpp, gridpf_capi_n1.hip; the fan's secondary lanes are its contingency lanes): the watched lines, the values
  // [n_env][K] and the summary of the last one-step launch and the table index of every reward slot (-1: not a GPF_RW_N1 slot)
  bool n1_slots = false;
  DevArr<int> n1_lines, n1_info, n1_slot_idx;
  DevArr<float> n1_value, n1_worst;
  // the look-ahead screen (gridpf_lookahead.hpp, gridpf_capi_lookahead.hip; the fan's secondary lanes are its scratch lanes): the
  // candidates, the outputs of the last call, the play kernel's moved list, the rows the host last noted for the scratch lanes (la_noted:
  // the host's mirrors while la_noted_gen is the fan's plans_gen) and the scheduled maintenance alone (the device holds its union with the hazards)
  long long la_noted_gen = -1, la_maint_gen = -1;       // la_maint_gen: generation of the outage tables la_maint was uploaded from
  DevArr<int> la_cand, la_best, la_info, la_noted, la_src;
  DevArr<float> la_value, la_best_value;
  DevArr<unsigned char> la_flags, la_maint;
  MovedList la_moved_list;
  // the look-ahead chain (gpf_set_lookahead_chain): the sticky record of every scratch lane over up to lc_max steps and the fall-back slot
  // of every environment.  lc_host_on: a header-only handle was given a valid chain
  bool lc_on = false, lc_host_on = false;
  int lc_max = 0;
  DevArr<int> lc_survived, lc_fallback, lc_fallback_steps;
  DevArr<float> lc_peak, lc_value_h;
  std::vector<char> h_lane_n1;          // 1: the lane is a contingency lane of gpf_fanout_n1 or of the screen (until gpf_set_lane_chronics)
  bool last_track_cooldown = false;     // whether the last gpf_step_n maintained the line cooldowns (and so wrote traj_cool)
  int last_t0 = 0, last_n_steps = 1;    // time index and step count of the last gpf_step_n (the chronics row each lane's last step read)
  bool has_delta = false;
  DevArr<double> rd_pmin, rd_pmax, rd_ru, rd_rd, rd_in;      // generator limits + staging of gpf_redispatch
  DevArr<unsigned char> rd_redisp, rd_u8;
  DevArr<float> rd_after;
  double rd_eps = 1e-4;
  bool rd_ready = false;
  // pinned host block of gpf_solve_lane (one lane in, one lane out), mapped into the device (coherent: the device reads / writes it
  // uncached, what the gather kernel wrote is in host memory when the stream has drained)
  HostPin<unsigned char> pin{hipHostMallocMapped | hipHostMallocCoherent};
  GpfJit jit;                           // grid-specialised step kernels (gpf_jit_enable; gridpf_jit.hip)
  gpf::GridDev jit_g;                   // the grid-level part of the parameter block the specialisation was generated from
  gpf::OutOff jit_oo;
  gpf::SymDev jit_sym;
  int dcf = 0;                          // the NB == 1 LDS layout has room for the factored DC matrix (decided once at gpf_create)
  DevArr<double> d_init_inj;
  DevArr<int> d_init_topo, d_init_shunt_bus;
  int chron_T = 0, chron_tables = 0;
  bool has_scale = false;
  // per-lane capacity bookkeeping (host): number of active buses / NR unknowns of each lane
  std::vector<int> lane_nb, lane_nj;
  int init_nb = 0, init_nj = 0;
  // block-sparse path (kernel S)
  gpf::Symbolic sym;
  // DC sensitivity path (gridpf_ptdf.hpp, gridpf_capi_ptdf.hip)
  DevArr<int> ptdf_inj_bus;
  DevArr<double> ptdf_inj_w, ptdf_t;
  DevArr<float> ptdf_flow, lodf_worst, lodf_inv_cap;
  DevArr<float> ptdf_flow_rows;    // [rows][cap_lanes][line_pad] flows of the last gpf_ptdf_flows_rows
  int ptdf_rows_valid = 0;
  DevArr<float> lodf;              // [n_line][line_pad] line outage distribution factors of the PTDF topology, float32 (NaN column: islanding outage)
  std::vector<double> h_ptdf;      // [n_line][nb_tot]
  std::vector<double> h_br_bdc, h_shunt_fact;
  std::vector<int> h_gen_cnt;
  int ptdf_nb_pad = 0, ptdf_line_pad = 0;
  bool ptdf_ready = false;
  // per-lane topologies (gpf_ptdf_build_batch, gridpf_ptdf_batch.hpp): one PTDF^T / LODF block per distinct topology class of a lane range
  long long n_step_calls = 0, n_step_dispatches = 0;   // gpf_step_n calls / kernel dispatches they issued (gpf_get_counters)
  bool ptdf_batch = false;                 // the flows / screening calls run on the class tables of the last gpf_ptdf_build_batch
  int ptdfb_lane0 = 0, ptdfb_n = 0, ptdfb_classes = 0, ptdfb_slots = 0, ptdfb_kpad = 0, ptdfb_npad_max = 0, ptdfb_desc_stride = 0;
  DevArr<int> ptdfb_desc, ptdfb_order, ptdfb_blk_class, ptdfb_status;
  DevArr<double> ptdfb_work, ptdfb_t, ptdfb_inj_w;
  DevArr<float> ptdfb_lodf;
  std::vector<int> h_ptdfb_lane_class, h_ptdfb_status, h_ptdfb_desc;
  std::vector<std::vector<int>> h_ptdfb_bus;   // per class: compact bus index -> bus id (sub + (local - 1) * n_sub)
  double ptdfb_kernel_ms = 0.0;            // duration of the last build kernel (HIP events)
  // the build call returns once its kernel is QUEUED: class status + kernel time are fetched when somebody asks (gpf_ptdf_batch_info)
  Event ptdfb_ev_a, ptdfb_ev_b;
  HostPin<int> ptdfb_status_pin;
  bool ptdfb_pending = false;
  // device-side grouping + descriptors (gridpf_ptdf_group.hpp): their outputs, and the host mirrors fetched on demand
  DevArr<unsigned long long> ptdfg_hash;
  DevArr<int> ptdfg_lane_class, ptdfg_first, ptdfg_c2b, ptdfg_info;
  HostPin<int> ptdfg_info_pin;
  HostPin<int> ptdfg_back_pin;             // lane -> class map + descriptor headers, queued behind the factorisation
  bool ptdfb_prefetched = false;
  bool ptdfb_host_stale = false;           // h_ptdfb_lane_class / h_ptdfb_hdr are not what the device holds: ptdfb_fetch_host
  bool ptdfb_bus_stale = false;            // ... nor h_ptdfb_bus (only gpf_ptdf_batch_get reads it)
  std::vector<int> h_ptdfb_hdr;            // device path: the 4-int headers of the class descriptors (nr, n_act, n_pad, status); empty: h_ptdfb_desc has them
  DevArr<double> dc_inv_g;     // static DC inverse of the larger grids (gpf::SymDev::dc_inv_g)
  DevArr<double> stat_dbl;     // static blob of kernel S (gpf::StatOff)
  DevArr<int> stat_int;
  DevArr<int> flat_prog;       // flat programs of the substation graph (4 group widths)
  gpf::SymDev sym_dev{};
  gpf::DevParamsS h_params_s{};
  DevArr<gpf::DevParamsS> d_params_s;
  bool params_s_valid = false;
  // mixed batches: lanes without / with split substations are launched separately (single-busbar kernel / NB = n_busbar)
  DevArr<int> list_a, list_b, list_c;   // list_c: topology class of every lane of list_b
  // topology classes (gpf::TopoClassDev): bus-level graphs of the split topologies seen so far, each with its own symbolic program
  struct TopoClassHost { DevArr<int> tables, flat; gpf::TopoClassDev dev; int n_nodes, nslot, nslot_y; };
  std::vector<std::unique_ptr<TopoClassHost>> classes;
  std::unordered_map<std::string, int> class_of_key;
  // host mirror of the topology last SENT for every lane (gpf_set_topology skips the per-lane bookkeeping when a lane is
  // re-sent unchanged: agents resend whole batches with few changes); first entry INT_MIN = unknown
  std::vector<int> h_lane_topo, h_lane_sb;
  bool dev_topo_dirty = false;           // a kernel may have rewritten topology rows (cascade trips, scheduled outages): the host mirrors are not the device rows any more
  std::vector<int> lane_class;          // per lane: topology class (-1: no split substation / classes disabled)
  DevArr<gpf::TopoClassDev> d_classes;  // device copy of classes[*].dev
  size_t d_classes_count = 0;
  bool no_classes = false;              // GRIDPF_NO_CLASSES=1: split lanes run the NB = n_busbar kernel
  bool no_partition = false;     // GRIDPF_NO_PARTITION=1
  int ipw_override = 0;        // GRIDPF_IPW=1|2|4 (developer override of the instances-per-wavefront heuristic)
  int wpi_override = 0;        // GRIDPF_WPI=1|2 (developer override of the wavefronts-per-instance heuristic); 1 = deterministic
  int wpi_env = 0;
  bool no_yreg = false;        // GRIDPF_YREG=0: never keep the Ybus blocks in registers
  int stage_max = 2;           // GRIDPF_STAGE=0|1|2: highest static-table staging tier the planner may pick (developer / tests)
  int stage_force = -1;        // GRIDPF_FORCE_STAGE=0|1|2: take that tier whenever it fits the LDS, whatever it costs in residency (experiments)
  int dcf_env = -1;            // GRIDPF_DCF=0|1 (-1: not set)
  int cap_lanes = 0;           // lane buffers are padded to a multiple of 4 lanes (instance groups of a wavefront)
  std::vector<int> lane_mb;    // max live busbars in one substation, per lane
  int init_mb = 1;
  bool plan_valid = false;      // cached launch plan of the whole batch (invalidated by every topology mutation)
  LaunchPlan plan_cached{}, plan_b_cached{};   // plan_b: the split lanes of a mixed batch (sparse_nb == 0: none)
  // profiling
  bool profiling = false;      // per-launch event pairs (gpf_set_profiling(h, 2))
  bool window = false;         // one event pair around a window of launches (gpf_set_profiling(h, 1))
  Event win_a, win_b;
  bool win_marked = false;              // win_b was recorded by gpf_set_profiling(3) behind the last launch of the window
  long long win_launches = 0;
  std::vector<std::pair<Event, Event>> ev_pool;
  size_t ev_used = 0;
  double acc_ms = 0.0;
  long long acc_launches = 0;

  gpf::Bufs bufs() const {
    gpf::Bufs b{};
    b.inj = inj.p; b.topo = topo.p; b.shunt_bus = shunt_bus.p; b.out = out.p; b.topo_out = topo_out.p;
    b.shunt_bus_out = shunt_bus_out.p; b.line_status = line_status.p; b.status = status.p;
    b.bus_vm = bus_vm.p; b.bus_va = bus_va.p; b.work = work.p; b.work_stride = 0;
    b.chron = chron.p; b.lane_table = lane_table.p; b.lane_offset = lane_offset.p;
    b.lane_scale = has_scale ? lane_scale.p : nullptr;
    b.thermal_limit = thermal_limit.p; b.rho = rho.p; b.overflow_count = overflow_count.p; b.disc_round = disc_round.p;
    b.lane_gen_delta = has_delta ? lane_gen_delta.p : nullptr;
    b.maint = maint.n ? maint.p : nullptr;
    b.cooldown = cooldown.p; b.maint_dur = maint_dur.n ? maint_dur.p : nullptr; b.traj_cool = (traj_cap && traj_cool.n) ? traj_cool.p : nullptr;
    b.topo0 = topo0.p; b.done = done.p; b.episode = episode.p;
    b.traj_rho = traj_cap ? traj_rho.p : nullptr; b.traj_status = traj_cap ? traj_status.p : nullptr; b.traj_cap = traj_cap;
    const bool obs = traj_cap && (traj_what & GPF_TRAJ_OBS);
    b.traj_out = obs ? traj_out.p : nullptr; b.traj_topo = obs ? traj_topo.p : nullptr; b.traj_shb = obs ? traj_shb.p : nullptr;
    b.traj_lstat = obs ? traj_lstat.p : nullptr;
    b.lane_stride = cap_lanes; b.n_real_lanes = n_lanes;
    return b;
  }
};

// Rows [lane0, lane0 + n) of a lane-major device array with `stride` elements per lane, copied on the engine's stream (asynchronous:
// the caller synchronises).  No-op when the host pointer is null or the stride is 0.
template <typename T>
hipError_t rows_to_host(const gpf_engine* e, T* host, const DevArr<T>& arr, size_t stride, int lane0, int n) {
  if (!host || stride == 0) return hipSuccess;
  return hipMemcpyAsync(host, arr.p + (size_t)lane0 * stride, (size_t)n * stride * sizeof(T), hipMemcpyDeviceToHost, e->stream);
}
template <typename T>
hipError_t rows_to_device(const gpf_engine* e, const DevArr<T>& arr, const T* host, size_t stride, int lane0, int n) {
  if (!host || stride == 0) return hipSuccess;
  return hipMemcpyAsync(arr.p + (size_t)lane0 * stride, host, (size_t)n * stride * sizeof(T), hipMemcpyHostToDevice, e->stream);
}
// ... and rows [src, src + n) -> [dst, dst + n) of the same array
template <typename T>
hipError_t rows_copy(const gpf_engine* e, const DevArr<T>& arr, size_t stride, int src, int dst, int n) {
  if (stride == 0) return hipSuccess;
  return hipMemcpyAsync(arr.p + (size_t)dst * stride, arr.p + (size_t)src * stride, (size_t)n * stride * sizeof(T), hipMemcpyDeviceToDevice, e->stream);
}

// gridpf_capi.hip, the planner's bookkeeping: the host's record of one lane whose topology row is now `t` / `sb` (true: it changed), and
// "the lanes' rows were sent by the host" (their reset topology is their topology again)
bool note_lane_row(gpf_engine* e, int lane, const int* t, const int* sb);
void topo_unmoved(gpf_engine* e, int lane0, int n);
// ... lane `dst` takes lane `src`'s planning entries, and its mirror of the sent rows (else the mirror is unknown: a kernel wrote the row);
// the read-back of a moved-lane list of lanes in [lane_lo, lane_hi): count first, then ids and rows, note_lane_row and per_lane(lane) (may
// be empty) in lane order -- a count or a lane out of range: nothing is noted, GPF_E_DEVICE "<who> count)" / "<who> lane)"; and what is
// refused in a list of action items (kind, id, value) of `who` (*bus_items, may be null: an item sets or changes a bus)
void lane_inherit(gpf_engine* e, int dst, int src, bool copy_mirror);
int moved_list_readback(gpf_engine* e, MovedList& list, int lane_lo, int lane_hi, const char* who, const std::function<void(int)>& per_lane);
int check_action_items(gpf_engine* e, const char* who, int n_items, const int32_t* items, bool* bus_items);

// gridpf_capi_env.hip: the state pointers of the injection dynamics (no action pointers: upload_params_s adds its launch's), the
// feature's share of gpf_reset_lanes / gpf_copy_lanes, and simulate_env_copy_kernel: lanes dst0 + q, q < n_dst, take the state of lane
// src_lanes_dev[q / n_act] (gpf_fanout_n1, gpf_simulate_batch)
gpf::EnvDyn env_dyn(const gpf_engine* e);
int env_reset_lanes(gpf_engine* e, int lane0, int n);
hipError_t env_copy_lanes(gpf_engine* e, int src, int dst, int n);
int env_copy_from(gpf_engine* e, const int* src_lanes_dev, int n_act, int n_dst, int dst0);

// gridpf_capi_topo.hip: topo_prestep_kernel in front of a launch (acts: it carries topology actions) with the read-back of the lanes it
// moved to another topology class, topo_poststep_kernel behind it (list_resets: lanes that auto-reset are listed), the read-back of that
// list into the planner's bookkeeping (moved: the rows are action results, else reset topologies) and the feature's share of
// gpf_reset_lanes / gpf_copy_lanes / gpf_fanout_n1; in front of them the argument blocks of its kernels (grid maps and lane rows, the
// acting path's per-lane state), which the look-ahead's play kernel takes too
gpf::TopoDev topo_dev(const gpf_engine* e);
gpf::TopoLanes topo_lanes(const gpf_engine* e);
int topo_prestep(gpf_engine* e, bool acts);
int topo_poststep(gpf_engine* e, bool acts, int n_steps, bool list_resets);
int topo_readback(gpf_engine* e, bool moved);
int topo_reset_lanes(gpf_engine* e, int lane0, int n);
hipError_t topo_copy_lanes(gpf_engine* e, int src, int dst, int n);
int topo_fanout_lanes(gpf_engine* e, int src, int dst0, int n_out);

// gridpf_capi_opp.hip: the opponent's pre-step of a one-step launch (queued on the engine's stream) and its share of gpf_copy_lanes
int opponent_prestep(gpf_engine* e);
hipError_t opponent_copy_lanes(gpf_engine* e, int src, int dst, int n);
// gridpf_capi_alert.hip: the two side kernels of a one-step launch with alerts on (queued on the engine's stream), the alerts' share of
// gpf_copy_lanes / gpf_reset_lanes, and "off" (a new opponent or new areas change the alertable list)
int alert_prestep(gpf_engine* e);
int alert_poststep(gpf_engine* e);
hipError_t alert_copy_lanes(gpf_engine* e, int src, int dst, int n);
int alert_reset_lanes(gpf_engine* e, int lane0, int n);
void alerts_off(gpf_engine* e);

// gridpf_capi_reward.hip: the rewards' share of a one-step launch (the snapshot before the step, reward_kernel after it; topo_flags:
// the launch carried topology actions) and of gpf_reset_lanes
int reward_prestep(gpf_engine* e);
int reward_poststep(gpf_engine* e, bool topo_flags, bool combined = false);
int reward_reset_lanes(gpf_engine* e, int lane0, int n);

// gridpf_capi_episode.hip: episode_kernel, queued last in a one-step launch with a limit set (list_resets: truncated lanes are appended to
// ta_moved_list for the host's re-keying), the feature's share of gpf_reset_lanes / gpf_copy_lanes, and what gpf_set_rewards
// does to the returns (a new slot table starts them at 0)
int episode_poststep(gpf_engine* e, bool auto_reset, bool track_cooldown, bool list_resets);
int episode_reset_lanes(gpf_engine* e, int lane0, int n);
hipError_t episode_copy_lanes(gpf_engine* e, int src, int dst, int n);
int episode_rewards_changed(gpf_engine* e);

// gridpf_capi_cursor.hip: cursor_prestep_kernel, queued first in a one-step launch with the cursor on, the feature's share of
// gpf_copy_lanes, the skip byte of lanes [lane0, lane0 + n) (gpf_fanout_n1, gpf_simulate_batch: 1; gpf_set_lane_chronics: 0) and the
// read-back of lane_table / lane_offset into the host mirrors (queued; the caller synchronises)
int cursor_prestep(gpf_engine* e, int t);
hipError_t cursor_copy_lanes(gpf_engine* e, int src, int dst, int n);
hipError_t cursor_mark_lanes(gpf_engine* e, int lane0, int n, int skip);
hipError_t cursor_fetch_mirrors(gpf_engine* e);

// gridpf_capi_combined.hip: the three side kernels of a one-step launch in combined mode (acts: it carries topology actions; rules_on:
// the storage rule applies; screened: combined_screen ran in this launch) and the feature's share of gpf_reset_lanes / gpf_copy_lanes
int combined_screen(gpf_engine* e, bool acts, int rules_on);
int combined_cancel(gpf_engine* e, bool acts);
int combined_settle(gpf_engine* e, bool acts, bool screened);
int combined_reset_lanes(gpf_engine* e, int lane0, int n);
hipError_t combined_copy_lanes(gpf_engine* e, int src, int dst, int n);

// gridpf_capi.hip, for the fan: the plan of a lane range with the caller's device lane lists (list_a / list_b / list_c of the engine
// and the batch's cached plan are left alone), and gpf_runpf's launch on a range with a plan made that way
// (list_tail: a range that does not end on an instance group keeps the batch's group width, from a ghost-padded lane list)
int plan_launch_own(gpf_engine* e, int lane0, int n, LaunchPlan& p, LaunchPlan& pb, DevArr<int>* lists, bool list_tail = false);
int runpf_range(gpf_engine* e, int lane0, int n, int is_dc, int max_iter, double tol_mva, const LaunchPlan* pre_p, const LaunchPlan* pre_pb);
// ... the fan's plans brought up to date (no work while nothing invalidated the batch's plan), and the secondary lanes marked (1) or
// unmarked (0) in a host flag vector and, with the cursor on, in its skip bytes
int fan_plans(gpf_engine* e);
int fan_mark_lanes(gpf_engine* e, std::vector<char>& flags, int mark);

// gridpf_capi_n1.hip: fan_plans for the screen (in front of it the contingency lanes take their environments' planning entries), the
// screen itself, queued behind the step and the topology post-step of a one-step launch (fan-out, the power flows of the contingency
// lanes, values, summary), the GPF_RW_N1 slots of lanes [lane0, lane0 + n) from the table into `reward` and what gpf_set_rewards does to
// the slot indices (refusals included)
int n1_plans(gpf_engine* e);
int n1_screen(gpf_engine* e, int max_iter, double tol_mva);
int n1_fill_slots(gpf_engine* e, int lane0, int n, float* reward, long long row_stride);
int n1_check_slots(gpf_engine* e, int n_slot, const gpf_reward_slot* slots);
int n1_set_slots(gpf_engine* e, int n_slot, const gpf_reward_slot* slots);

// gridpf_capi.hip, for the look-ahead: simulate_prepare_kernel on scratch lanes dst0 + q, q < n_dst, of sources src_lanes_dev[q / n_act]
// (everything of a source that is not topology, and the chronics or forecast row to step on), one step of a lane range as gpf_simulate_batch
// takes it (no cooldown tracking, no auto-reset, no outage tables, no trajectory; pending injection actions stay pending), on a plan of
// the caller's, and the multi-step refusal's test
int simulate_prepare(gpf_engine* e, const int* src_lanes_dev, int n_act, int n_dst, int dst0, int t_obs, int time_step);
int simulate_step(gpf_engine* e, int lane0, int n, int time_step, const gpf_step_opts* o, const char* who, const LaunchPlan* pre_p, const LaunchPlan* pre_pb);
// gridpf_capi_lookahead.hip: the marks of the scratch lanes (their chronics cursor is an absolute row, they start no scenario of their
// own; gpf_set_lane_chronics clears the marks of every lane)
int la_mark_lanes(gpf_engine* e);

inline bool check_range(gpf_engine* e, int lane0, int n) { return e && lane0 >= 0 && n >= 0 && lane0 + n <= e->n_lanes; }

#pragma GCC visibility pop
