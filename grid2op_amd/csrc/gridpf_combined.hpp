// gridpf_combined.hpp -- combined topology + injection actions of the batched acting path (gpf_set_combined_actions, include/gridpf.h):
// what BaseEnv.step does with an action that has both parts, for every lane of a one-step launch.  Paths relative to the reference
// checkout:
//   value rules        BaseAction._check_for_ambiguity on redispatch (Action/baseAction.py:3621-3646), _is_storage_ambiguous (:3889-3918),
//                      _is_curtailment_ambiguous (:3929-3968): an ambiguous action does nothing in ALL its parts, is_ambiguous and not
//                      is_illegal -- combined_screen
//   the storage rule   PreventDiscoStorageModif (Rules/PreventDiscoStorageModif.py:39-46), between LookParam and PreventReconnection
//                      (Rules/DefaultRules.py:36-44): an illegal action does nothing in all its parts -- combined_screen
//   the flags          an ambiguous action never reaches the rules: ambiguous wins over illegal -- combined_merge
//   a cancelled        _prepare_redisp finds the target beyond pmax - pmin after the topology reached the backend action
//   redispatch         (Environment/baseEnv.py:3798, :3806, :3193-3201): the topology stays, nothing is booked for the action --
//                      combined_settle_kernel clears the lane's affected row in front of topo_poststep_kernel
// Three side kernels around kernels that stay as they are: a redispatch row of zeros, a storage row of zeros and a curtailment row of -1
// are "no action" to env_dynamics_step, a slot of -1 is "no action" to topo_prestep_kernel.
// Two parts: the rules (plain C++, run by the kernels and by the host emulator of tests/native/) and, for the one unit that defines
// GPF_COMBINED_KERNEL (gridpf_capi_combined.hip), the kernels.  Without hipcc only the rules exist: the header then needs no HIP header.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GPF_CB_HD __host__ __device__
#else
#define GPF_CB_HD
#endif

#include <math.h>
#include <stdint.h>

namespace gpf {

// the reason byte (= GPF_CB_* of include/gridpf.h); the value rules in the order the reference tests them
constexpr int CB_NONE = 0, CB_REDISP_FIXED_GEN = 1, CB_REDISP_RAMP_UP = 2, CB_REDISP_RAMP_DOWN = 3, CB_STORAGE_POWER = 4, CB_CURTAIL_RANGE = 5,
              CB_CURTAIL_FIXED_GEN = 6, CB_DISCO_STORAGE = 7, CB_TOPO_RULES = 8, CB_TOPO_AMBIGUOUS = 9;

// the grid's limits; ramps are the float64 of gpf_set_gen_limits and compared as the float32 the reference keeps (dt_float)
struct CombinedGrid {
  int n_gen, n_sto;
  const double* ramp_up; const double* ramp_down;       // [n_gen]
  const unsigned char* redispatchable;                  // [n_gen]
  const unsigned char* renewable;                       // [n_gen], or null: no generator is renewable
  const float* sto_max_prod; const float* sto_max_absorb;   // [n_sto], or null: the storage range is not checked
  const int* sto_pos;                                   // [n_sto] topo_vect position of every storage unit
};

struct CombinedVerdict { unsigned char ambiguous, illegal, reason; };

// the executor of the host emulator: pred(i) for i in [0, n), one after the other
struct CombinedSerial {
  template <typename Pred>
  bool any(int n, Pred pred) const { bool a = false; for (int i = 0; i < n; ++i) a = a || pred(i); return a; }
};

// The injection-side verdict of one lane.  redisp / storage / curtail: the lane's rows, null where that kind is not pending for the
// launch.  topo_row: the lane's topo_vect before the action.  sto_touched: bit k = the lane's topology entries set storage unit k to a
// busbar > 0 or change its bus (combined_entry_words, OR-ed over the lane's slots).  check_values: the value rules; rules_on: the
// storage rule (DefaultRules / RulesByArea; AlwaysLegal has none).
template <typename X>
GPF_CB_HD inline CombinedVerdict combined_screen(const X& x, const CombinedGrid& g, const float* redisp, const float* storage, const float* curtail,
                                                 const int* topo_row, unsigned long long sto_touched, int check_values, int rules_on) {
  CombinedVerdict v{0, 0, CB_NONE};
  if (check_values) {
    int why = CB_NONE;
    if (redisp) {
      if (x.any(g.n_gen, [&](int i) { return !g.redispatchable[i] && fabsf(redisp[i]) >= 1e-7f; })) why = CB_REDISP_FIXED_GEN;
      else if (x.any(g.n_gen, [&](int i) { return redisp[i] > (float)g.ramp_up[i]; })) why = CB_REDISP_RAMP_UP;
      else if (x.any(g.n_gen, [&](int i) { return -redisp[i] > (float)g.ramp_down[i]; })) why = CB_REDISP_RAMP_DOWN;
    }
    if (!why && storage && g.sto_max_prod &&
        x.any(g.n_sto, [&](int i) { return storage[i] < -g.sto_max_prod[i] || storage[i] > g.sto_max_absorb[i]; })) why = CB_STORAGE_POWER;
    if (!why && curtail) {
      if (x.any(g.n_gen, [&](int i) { return (curtail[i] < 0.f && fabsf(curtail[i] + 1.f) >= 1e-7f) || curtail[i] > 1.f; })) why = CB_CURTAIL_RANGE;
      else if (x.any(g.n_gen, [&](int i) { return !(g.renewable && g.renewable[i]) && fabsf(curtail[i] + 1.f) >= 1e-7f; })) why = CB_CURTAIL_FIXED_GEN;
    }
    if (why) { v.ambiguous = 1; v.reason = (unsigned char)why; return v; }
  }
  if (rules_on && storage &&
      x.any(g.n_sto, [&](int i) {
        const float p = storage[i];
        return topo_row[g.sto_pos[i]] < 0 && __builtin_isfinite(p) && fabsf(p) >= 1e-7f && !((sto_touched >> i) & 1ull);
      })) { v.illegal = 1; v.reason = CB_DISCO_STORAGE; }
  return v;
}

// The step's flags {is_illegal, is_ambiguous, is_illegal_redisp, reason}, packed in one word, from the topology part's own verdict, the screen's and "the step
// cancelled the redispatch".  An ambiguous action is not also illegal; the reason names the screen's rule before the topology part's.
GPF_CB_HD inline uint32_t combined_merge(bool topo_illegal, bool topo_ambiguous, CombinedVerdict s, bool illegal_redisp) {
  const bool amb = topo_ambiguous || s.ambiguous != 0;
  const bool ill = !amb && (topo_illegal || s.illegal != 0);
  const uint32_t why = s.ambiguous ? s.reason : topo_ambiguous ? CB_TOPO_AMBIGUOUS : s.illegal ? s.reason : topo_illegal ? CB_TOPO_RULES : CB_NONE;
  return (ill ? 1u : 0u) | (amb ? 1u << 8 : 0u) | (illegal_redisp ? 1u << 16 : 0u) | (why << 24);      // the four bytes, first byte lowest
}

// one byte per lane between the kernels: the screen's verdict
GPF_CB_HD inline unsigned char combined_pack(CombinedVerdict v) { return (unsigned char)((v.ambiguous ? 1 : 0) | (v.illegal ? 2 : 0) | (v.reason << 2)); }
GPF_CB_HD inline CombinedVerdict combined_unpack(unsigned char b) { return CombinedVerdict{(unsigned char)(b & 1), (unsigned char)((b >> 1) & 1), (unsigned char)(b >> 2)}; }

// One 64-bit word per table entry (gpf_upload_topo_actions): bit k = the entry sets storage unit k to a busbar > 0 or changes its bus.
// items: {kind, id, value} triples, kinds as GPF_ACT_* (0 = set_bus, 2 = change_bus).  Host only.
inline void combined_entry_words(int n_act, const int* off, const int* items, int n_sto, const int* sto_pos, unsigned long long* words) {
  for (int a = 0; a < n_act; ++a) {
    unsigned long long w = 0;
    for (int q = off[a]; q < off[a + 1]; ++q) {
      const int kind = items[3 * q], id = items[3 * q + 1], v = items[3 * q + 2];
      if (!((kind == 0 && v > 0) || kind == 2)) continue;
      for (int k = 0; k < n_sto && k < 64; ++k) if (sto_pos[k] == id) w |= 1ull << k;
    }
    words[a] = w;
  }
}

// ---- one lane with plain loops (the host emulator; the kernels below run the same rules with one wavefront per lane) -------------------
// before the topology pre-step: the verdict, and the lane's slots emptied on a verdict unless the topology part is ambiguous by itself
// (then the pre-step ignores it and keeps that verdict: the reference reports "ambiguous").  tab_amb: the table's static ambiguity flags.
inline CombinedVerdict combined_screen_serial(const CombinedGrid& g, const float* redisp, const float* storage, const float* curtail, const int* topo_row,
                                              int* slots, int n_slot, int n_act, const unsigned char* tab_amb, const unsigned long long* tab_word,
                                              int check_values, int rules_on) {
  unsigned long long touched = 0;
  bool tamb = false;
  for (int k = 0; slots && k < n_slot; ++k) {
    const int a = slots[k];
    if (a < -1 || a >= n_act) tamb = true;
    else if (a >= 0) { touched |= tab_word[a]; tamb = tamb || tab_amb[a] != 0; }
  }
  const CombinedVerdict v = combined_screen(CombinedSerial{}, g, redisp, storage, curtail, topo_row, touched, check_values, rules_on);
  if ((v.ambiguous || v.illegal) && !tamb) for (int k = 0; slots && k < n_slot; ++k) slots[k] = -1;
  return v;
}

// behind the topology pre-step: a verdict of either part leaves no injection action
inline void combined_cancel_serial(const CombinedGrid& g, bool topo_illegal, bool topo_ambiguous, CombinedVerdict s, float* redisp, float* storage, float* curtail) {
  if (!(topo_illegal || topo_ambiguous || s.ambiguous || s.illegal)) return;
  for (int i = 0; redisp && i < g.n_gen; ++i) redisp[i] = 0.f;
  for (int i = 0; storage && i < g.n_sto; ++i) storage[i] = 0.f;
  for (int i = 0; curtail && i < g.n_gen; ++i) curtail[i] = -1.f;
}

#if defined(__HIPCC__) && defined(GPF_COMBINED_KERNEL)
// the kernels' executor: element i is thread i % 64 of the wavefront, the verdict goes through __any (every thread ends with it)
struct CombinedWave {
  int tid;
  template <typename Pred>
  __device__ bool any(int n, Pred pred) const {
    bool a = false;
    for (int i = tid; i < n; i += 64) a = a || pred(i);
    return __any(a) != 0;
  }
};

// what the three kernels read and write (rows padded to the engine's lane capacity)
struct CombinedDev {
  CombinedGrid g;
  int dim_topo, n_line, n_sub, n_slot, n_act;
  int check_values, rules_on;
  int had_topo;                        // the launch carries topology actions (else the topology part's buffers are not read)
  int screened;                        // combined_screen_kernel ran in this launch (injection actions were pending)
  float* act_r; float* act_s; float* act_c;   // the launch's action rows [lanes][n_gen] / [lanes][n_sto] / [lanes][n_gen]; null: not pending
  const int* topo;                     // [lanes][dim_topo]
  int* slots;                          // [lanes][n_slot] the lanes' table indices of this launch
  const unsigned char* tab_amb;        // [n_act]
  const unsigned long long* tab_word;  // [n_act]
  const int* env_illegal;              // [lanes] cancelled redispatch actions since the reset
  int* ill_snap;                       // [lanes] ... before the step
  unsigned char* screen;               // [lanes] combined_pack of the screen's verdict
  const unsigned char* topo_flags;     // [lanes][2] the topology part's own verdict
  unsigned char* aff;                  // [lanes][n_line + n_sub] what the post-step books for the action
  unsigned char* flags;                // [lanes][4] the step's flags
};

constexpr int CB_WPB = 4;              // lanes (wavefronts) per block

// All three: one wavefront per lane, CB_WPB lanes per block, wave-uniform lane index, row loops of stride 64, verdicts by __any; no LDS,
// no scratch, no atomics, no block-wide barrier, plain vector stores.

// Queued in front of topo_prestep_kernel: it reads the storage units' busbars before the action.
__global__ __launch_bounds__(64 * CB_WPB) void combined_screen_kernel(CombinedDev d, int n_lanes) {
  const int tid = threadIdx.x & 63;
  const int lane = blockIdx.x * CB_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (lane >= n_lanes) return;
  unsigned long long touched = 0;
  bool tamb = false;
  int* slots = d.slots + (size_t)lane * d.n_slot;
  if (d.had_topo)
    for (int k = 0; k < d.n_slot; ++k) {                         // (uniform)
      const int a = slots[k];
      if (a < -1 || a >= d.n_act) tamb = true;
      else if (a >= 0) { touched |= d.tab_word[a]; tamb = tamb || d.tab_amb[a] != 0; }
    }
  const size_t g0 = (size_t)lane * d.g.n_gen, s0 = (size_t)lane * d.g.n_sto;
  const CombinedVerdict v = combined_screen(CombinedWave{tid}, d.g, d.act_r ? d.act_r + g0 : nullptr, d.act_s ? d.act_s + s0 : nullptr,
                                            d.act_c ? d.act_c + g0 : nullptr, d.topo + (size_t)lane * d.dim_topo, touched, d.check_values, d.rules_on);
  if (tid == 0) { d.screen[lane] = combined_pack(v); d.ill_snap[lane] = d.env_illegal[lane]; }
  if (!(v.ambiguous || v.illegal)) return;
  if (d.had_topo) {
    if (!tamb) for (int k = tid; k < d.n_slot; k += 64) slots[k] = -1;
    return;
  }
  // no topology part in this launch: nothing else can veto the lane, the cancel is done here and combined_cancel_kernel is not queued
  if (d.act_r) for (int i = tid; i < d.g.n_gen; i += 64) d.act_r[g0 + i] = 0.f;
  if (d.act_s) for (int i = tid; i < d.g.n_sto; i += 64) d.act_s[s0 + i] = 0.f;
  if (d.act_c) for (int i = tid; i < d.g.n_gen; i += 64) d.act_c[g0 + i] = -1.f;
}

// Queued behind topo_prestep_kernel (its run-time verdict) and in front of everything that reads the action rows, in the launches
// that carry topology actions.
__global__ __launch_bounds__(64 * CB_WPB) void combined_cancel_kernel(CombinedDev d, int n_lanes) {
  const int tid = threadIdx.x & 63;
  const int lane = blockIdx.x * CB_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (lane >= n_lanes) return;
  bool dirty = (d.screen[lane] & 3) != 0;
  if (d.had_topo) dirty = dirty || d.topo_flags[(size_t)lane * 2] != 0 || d.topo_flags[(size_t)lane * 2 + 1] != 0;
  if (!dirty) return;
  const size_t g0 = (size_t)lane * d.g.n_gen, s0 = (size_t)lane * d.g.n_sto;
  if (d.act_r) for (int i = tid; i < d.g.n_gen; i += 64) d.act_r[g0 + i] = 0.f;
  if (d.act_s) for (int i = tid; i < d.g.n_sto; i += 64) d.act_s[s0 + i] = 0.f;
  if (d.act_c) for (int i = tid; i < d.g.n_gen; i += 64) d.act_c[g0 + i] = -1.f;
}

// Queued behind the step and in front of topo_poststep_kernel: a redispatch the step cancelled takes the action's booking away; then the
// step's flags.
__global__ __launch_bounds__(64 * CB_WPB) void combined_settle_kernel(CombinedDev d, int n_lanes) {
  const int tid = threadIdx.x & 63;
  const int lane = blockIdx.x * CB_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (lane >= n_lanes) return;
  const bool ill_redisp = d.screened && d.env_illegal[lane] != d.ill_snap[lane];
  if (ill_redisp && d.had_topo) {
    unsigned char* aff = d.aff + (size_t)lane * (d.n_line + d.n_sub);
    for (int i = tid; i < d.n_line + d.n_sub; i += 64) aff[i] = 0;
  }
  const uint32_t f = combined_merge(d.had_topo && d.topo_flags[(size_t)lane * 2] != 0, d.had_topo && d.topo_flags[(size_t)lane * 2 + 1] != 0,
                                    combined_unpack(d.screened ? d.screen[lane] : (unsigned char)0), ill_redisp);
  if (tid == 0) reinterpret_cast<uint32_t*>(d.flags)[lane] = f;
}
#endif  // __HIPCC__ && GPF_COMBINED_KERNEL

}  // namespace gpf
