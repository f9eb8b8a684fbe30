// gridpf_lookahead.hpp -- the look-ahead screen of the batched acting path (gpf_set_lookahead / gpf_lookahead, include/gridpf.h): what an
// agent does with obs.simulate at every step (Observation/baseObservation.py:3365-3670 -> Environment/_obsEnv.py) -- simulate its K best
// actions, play the one with the lowest simulated rho.max() that is legal and does not end the episode -- for every environment lane in
// one call, with the candidates as indices into the uploaded action table, in a device buffer.  Environment i is lane i, its candidate k
// is played on scratch lane n_env + i K + k (the layout of the N-1 screen and of gpf_simulate_batch with dst_lane0 = n_env).  This header
// holds what is new:
//   the value rule    la_value: the maximum over the lines of the scratch lane's rho row as the step wrote it, +inf when the simulated
//                     step ended the episode
//   the ranking       la_playable (no flag set) and la_outranks, a total order: the lower value, then the lower slot
//   the maintenance   la_maintenance_ahead, the ONE statement of "the forecast time_step rows ahead has this line out" (_ObsEnv.init,
//                     Environment/_obsEnv.py:361-385), for gpf_simulate_batch on the host and la_play_kernel on the device
//   the kernels       la_play_kernel (one wavefront per scratch lane: the environment's topology-side state, maintenance ahead, steps 1-4
//                     of gridpf_topo.hpp through topo_play_lane), la_reduce_kernel (one wavefront per scratch lane) and la_summary_kernel
//                     (one wavefront per environment), for the one unit that defines GPF_LA_KERNEL (gridpf_capi_lookahead.hip)
//   the chain         gpf_set_lookahead_chain / gpf_lookahead_chain: the candidate, then do-nothing steps on the consecutive forecast rows
//                     la_chain_row of one observation (obs.get_forecast_env, Observation/baseObservation.py:4724-4842), the lines of
//                     la_maintenance_ahead out before each; per scratch lane the sticky record la_chain_step keeps (steps survived, peak
//                     over the survived steps, value = +inf from the failing step on) and per environment the fall-back slot
//                     la_chain_outranks picks; la_chain_kernel between two steps, la_chain_summary_kernel at the end
// A maximum of stored float32 values is exact in any order and the ranking is a total order, so the fixed butterfly of gridpf_n1.hpp
// (share t of 64 takes elements t, t + 64, ...; partners 32, 16, 8, 4, 2, 1) gives the same bits in every run.  Without hipcc only the
// rules exist: the header then needs no HIP header.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GPF_LA_HD __host__ __device__
#else
#define GPF_LA_HD
#endif

#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace gpf {

constexpr int LA_SHARES = 64;
constexpr int LA_ILLEGAL = 1, LA_AMBIGUOUS = 2, LA_DONE = 4;      // (= GPF_LA_* of include/gridpf.h)

// one candidate's value: rho_max is the maximum of the scratch lane's rho row, done its done flag after the simulated step
GPF_LA_HD inline float la_value(bool done, float rho_max) { return done ? INFINITY : rho_max; }
GPF_LA_HD inline bool la_playable(unsigned flags) { return flags == 0; }

// candidate (va, ka) outranks (vb, kb) as an environment's best; a slot index < 0: there is no such candidate (not playable)
GPF_LA_HD inline bool la_outranks(float va, int ka, float vb, int kb) {
  if (ka < 0) return false;
  if (kb < 0) return true;
  if (va != vb) return va < vb;
  return ka < kb;
}

// share t of the maximum over a row of n float32 (-inf: the share has no element)
GPF_LA_HD inline float la_strided_max(int t, int n, const float* row) {
  float acc = -INFINITY;
  for (int l = t; l < n; l += LA_SHARES) acc = fmaxf(acc, row[l]);
  return acc;
}

// the host emulator's maximum: the 64 shares one after the other, then the butterfly (every share ends with the same value)
inline float la_max_serial(int n, const float* row) {
  float a[LA_SHARES], b[LA_SHARES];
  for (int t = 0; t < LA_SHARES; ++t) a[t] = la_strided_max(t, n, row);
  for (int m = LA_SHARES / 2; m >= 1; m >>= 1) {
    for (int t = 0; t < LA_SHARES; ++t) b[t] = fmaxf(a[t], a[t ^ m]);
    for (int t = 0; t < LA_SHARES; ++t) a[t] = b[t];
  }
  return a[0];
}

// one environment's summary with plain loops (the host emulator; la_summary_kernel runs the same rules with one wavefront)
struct LaSummary { float best_value; int best, n_playable, n_done; };
inline LaSummary la_summary_serial(const float* value, const unsigned char* flags, int K) {
  LaSummary s{INFINITY, -1, 0, 0};
  for (int k = 0; k < K; ++k) {
    const bool ok = la_playable(flags[k]);
    if (la_outranks(value[k], ok ? k : -1, s.best_value, s.best)) { s.best_value = value[k]; s.best = k; }
    s.n_playable += ok ? 1 : 0;
    s.n_done += (flags[k] & LA_DONE) ? 1 : 0;
  }
  return s;
}

// Scheduled maintenance ahead of the observation (_ObsEnv.init, Environment/_obsEnv.py:361-385 with BaseEnv._update_vector_with_timestep,
// baseEnv.py:4768-4825): a forecast `time_step` >= 1 rows ahead of row idx has line l out when the line's NEXT maintenance (the first
// flagged row from idx on) covers row idx + time_step -- it begins there (first_ts_maintenance) or is under way (still_in_maintenance).
// M: one table [T][n_line].  Only rows idx .. idx + time_step are ever looked at.  Hazards are not forecast by the reference.
GPF_LA_HD inline bool la_maintenance_ahead(const unsigned char* M, int T, int n_line, int idx, int time_step, int l) {
  const int tgt = idx + time_step;
  if (time_step < 1 || tgt >= T) return false;
  int s = idx;
  while (s <= tgt && !M[(size_t)s * n_line + l]) ++s;                 // start of the next maintenance (idx itself: under way)
  if (s > tgt) return false;
  for (int r = s; r <= tgt; ++r) if (!M[(size_t)r * n_line + l]) return false;
  return true;
}

// ---- the chain: step 1 is the look-ahead's own step, steps 2 .. H are do-nothing steps on the forecast rows of the same observation ----
// row of the forecast tables ([table][T][n_h][n_chron], n_h rows per observation) that step h >= 1 of the observation at row idx runs on
GPF_LA_HD inline int la_chain_row(int n_h, int idx, int h) { return n_h * idx + (h - 1); }

// The sticky record of one scratch lane: the step kernel overwrites the lane's done flag at every step, the chain keeps the first failure.
// survived: steps completed before the first failure; peak: maximum of rho over the survived steps (-inf: none); value: maximum of the
// per-step values so far, +inf once the lane has failed.
struct LaChainState { int survived; float peak, value; };
GPF_LA_HD inline LaChainState la_chain_start() { return LaChainState{0, -INFINITY, -INFINITY}; }
// step h (1, 2, ... in order) left `done` and the row maximum rho_max: the step's value, +inf from the failing step on.  A lane that
// failed earlier is solved and ignored: whatever the later steps leave, its record stands.
GPF_LA_HD inline float la_chain_step(LaChainState& s, int h, bool done, float rho_max) {
  const bool alive = s.survived == h - 1 && !done;
  if (alive) { s.survived = h; s.peak = fmaxf(s.peak, rho_max); }
  const float vh = alive ? rho_max : INFINITY;
  s.value = fmaxf(s.value, vh);
  return vh;
}
GPF_LA_HD inline bool la_chain_failed(const LaChainState& s, int h) { return s.survived < h; }
// a fall-back is a slot whose action was played as asked: neither illegal nor ambiguous (it may well end the episode within the horizon)
GPF_LA_HD inline bool la_chain_eligible(unsigned flags) { return (flags & (unsigned)(LA_ILLEGAL | LA_AMBIGUOUS)) == 0; }
// candidate a outranks b as an environment's fall-back: more survived steps, then the lower peak, then the lower slot (a total order;
// a slot index < 0: no such candidate)
GPF_LA_HD inline bool la_chain_outranks(int sa, float pa, int ka, int sb, float pb, int kb) {
  if (ka < 0) return false;
  if (kb < 0) return true;
  if (sa != sb) return sa > sb;
  if (pa != pb) return pa < pb;
  return ka < kb;
}
// what play = 0 / 1 / 2 leaves as the environment's table index: nothing / the best slot's, else -1 / the best's, else the fall-back's, else -1
GPF_LA_HD inline int la_chain_pick(int play, int best, int fallback) { return best >= 0 ? best : (play == 2 ? fallback : -1); }

// one environment's fall-back with plain loops (the host emulator; la_chain_summary_kernel runs the same rules with one wavefront)
struct LaFallback { int slot, steps; };
inline LaFallback la_fallback_serial(const int* survived, const float* peak, const unsigned char* flags, int K) {
  int fs = 0, fk = -1;
  float fp = INFINITY;
  for (int k = 0; k < K; ++k)
    if (la_chain_outranks(survived[k], peak[k], la_chain_eligible(flags[k]) ? k : -1, fs, fp, fk)) { fs = survived[k]; fp = peak[k]; fk = k; }
  return LaFallback{fk, fk >= 0 ? fs : 0};
}

}  // namespace gpf

#if defined(__HIPCC__) && defined(GPF_LA_KERNEL)
#include "gridpf_topo.hpp"

namespace gpf {

// what the look-ahead's kernels read and write beyond the acting path's own blocks (TopoDev, TopoTab, TopoLanes)
struct LaDev {
  const int* cand;                   // [n_env][K] table indices, -1: do nothing
  unsigned char* flags;              // [n_env][K] LA_*
  float* value;                      // [n_env][K]
  int* best;                         // [n_env]
  float* best_value;                 // [n_env]
  int* info;                         // [n_env][2] {playable slots, done slots}
  int* list;                         // [1 + n_env K] count, then the scratch lanes whose class key / busbar count left the noted one
  int* list_rows;                    // [n_env K][dim_topo + n_shunt] their rows (slot order of `list`)
  int* noted;                        // [n_env K][dim_topo + n_shunt] the row the host last noted for every scratch lane
  const unsigned char* maint;        // [tables][T][n_line] scheduled maintenance alone, or null
  const int* lane_table;             // [lanes] the chronics cursors of the environments
  const int* lane_offset;
  const float* rho;                  // [lanes][n_line]
  const unsigned char* done;         // [lanes]
  int n_env, K, T, t_obs, time_step;
};

constexpr int LA_WPB = 4;            // wavefronts per block of the reduce and summary kernels

// Block q: scratch lane n_env + q becomes environment q / K as far as the topology side goes -- topology and shunt rows with the lines of
// the maintenance ahead out, substation cooldowns, last known busbars (the rest came with simulate_prepare_kernel) -- and plays entry
// cand[q] on it under the environment's rules.  The environment's lane is only read.
__global__ __launch_bounds__(64) void la_play_kernel(TopoDev g, TopoTab tab, TopoLanes s, TopoRules r, LaDev d) {
  extern __shared__ int lds[];
  const int q = blockIdx.x, tid = threadIdx.x;
  if (q >= d.n_env * d.K) return;
  const int D = g.dim_topo, L = g.n_line, S = g.n_sub, NS = g.n_shunt;
  const size_t src = (size_t)(q / d.K), dst = (size_t)d.n_env + q;
  const int* st = g.topo + src * D;
  int* dt = g.topo + dst * D;
  const unsigned char* M = nullptr;
  int idx = 0;
  if (d.maint && d.time_step >= 1) {
    M = d.maint + (size_t)d.lane_table[src] * d.T * L;
    idx = (d.t_obs + d.lane_offset[src]) % d.T;
    if (idx < 0) idx += d.T;
  }
  for (int i = tid; i < D; i += 64) if (s.pos_other[i] < 0) dt[i] = st[i];
  for (int l = tid; l < L; l += 64) {
    const int po = g.line_or_pos[l], pe = g.line_ex_pos[l];
    const bool out = M && la_maintenance_ahead(M, d.T, L, idx, d.time_step, l);
    dt[po] = out ? -1 : st[po];
    dt[pe] = out ? -1 : st[pe];
  }
  for (int i = tid; i < NS; i += 64) g.shunt_bus[dst * NS + i] = g.shunt_bus[src * NS + i];
  for (int i = tid; i < S; i += 64) s.sub_cd[dst * S + i] = s.sub_cd[src * S + i];
  for (int i = tid; i < D; i += 64) s.last_bus[dst * D + i] = s.last_bus[src * D + i];
  __syncthreads();
  const TopoLook k{d.cand[q], d.noted + (size_t)q * (D + NS), d.list, d.list_rows};
  const int verdict = topo_play_lane<false, true>(g, tab, s, r, TopoComp{}, lds, (int)dst, k, tid, 64);
  if (tid == 0) d.flags[q] = (unsigned char)verdict;            // (1 = LA_ILLEGAL, 2 = LA_AMBIGUOUS; la_reduce_kernel adds LA_DONE)
  __syncthreads();
  int* d0 = const_cast<int*>(g.topo0) + dst * D;                // the row an auto-reset would restore: the candidate's (as gpf_set_topology)
  for (int i = tid; i < D; i += 64) d0[i] = dt[i];
}

// One wavefront per scratch lane, LA_WPB per block; no LDS, no scratch, no atomics, no block-wide barrier.  Read-only on the lanes.
__global__ __launch_bounds__(64 * LA_WPB) void la_reduce_kernel(LaDev d, int n_line) {
  const int tid = threadIdx.x & 63;
  const int q = blockIdx.x * LA_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform: the rows are scalar addresses)
  if (q >= d.n_env * d.K) return;
  const size_t lane = (size_t)d.n_env + q;
  float a = la_strided_max(tid, n_line, d.rho + lane * n_line);
#pragma unroll
  for (int m = LA_SHARES / 2; m >= 1; m >>= 1) a = fmaxf(a, __shfl_xor(a, m));
  const bool done = d.done[lane] != 0;
  if (tid == 0) {
    d.value[q] = la_value(done, a);
    if (done) d.flags[q] = (unsigned char)(d.flags[q] | LA_DONE);
  }
}

// One wavefront per environment: thread t takes slots t, t + 64, ...; the ranking is a total order and the counts are integers, so the
// butterfly gives the same summary whatever the order.
__global__ __launch_bounds__(64 * LA_WPB) void la_summary_kernel(LaDev d) {
  const int tid = threadIdx.x & 63;
  const int env = blockIdx.x * LA_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (env >= d.n_env) return;
  const float* row = d.value + (size_t)env * d.K;
  const unsigned char* fl = d.flags + (size_t)env * d.K;
  float bv = INFINITY;
  int bk = -1, n_ok = 0, n_done = 0;
  for (int k = tid; k < d.K; k += LA_SHARES) {
    const unsigned f = fl[k];
    const bool ok = la_playable(f);
    if (la_outranks(row[k], ok ? k : -1, bv, bk)) { bv = row[k]; bk = k; }
    n_ok += ok ? 1 : 0;
    n_done += (f & LA_DONE) ? 1 : 0;
  }
#pragma unroll
  for (int m = LA_SHARES / 2; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(bv, m);
    const int ok = __shfl_xor(bk, m);
    if (la_outranks(ov, ok, bv, bk)) { bv = ov; bk = ok; }
    n_ok += __shfl_xor(n_ok, m);
    n_done += __shfl_xor(n_done, m);
  }
  if (tid == 0) {
    d.best[env] = bk; d.best_value[env] = bv;
    d.info[(size_t)env * 2] = n_ok; d.info[(size_t)env * 2 + 1] = n_done;
  }
}

// what the chain's kernels read and write beyond LaDev
struct LaChainDev {
  int* survived;                     // [n_env][K]
  float* peak;                       // [n_env][K]
  float* value_h;                    // [n_env][K][max_steps]
  int* fallback;                     // [n_env]
  int* fallback_steps;               // [n_env]
  int* lane_offset;                  // [lanes] (LaDev::lane_offset, writable: the scratch lanes' rows move)
  int* topo;                         // [lanes][dim_topo]
  int* topo0;                        // [lanes][dim_topo]
  const int* line_or_pos;            // [n_line]
  const int* line_ex_pos;
  int* act;                          // [lanes] the acting path's table indices (one slot per lane), written when play != 0
  int dim_topo, n_line, n_h, max_steps;
};

// Queued behind step h of the chain, one wavefront per scratch lane: the sticky reduce of step h, then -- advance != 0 -- the lane's move
// to step h + 1: its chronics cursor goes to the next forecast row of the same observation, and the lines whose maintenance covers that
// row go out in its topology row and in the row an auto-reset would restore.  No action: the next step is a do-nothing step.
__global__ __launch_bounds__(64 * LA_WPB) void la_chain_kernel(LaDev d, LaChainDev c, int h, int advance) {
  const int tid = threadIdx.x & 63;
  const int q = blockIdx.x * LA_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform: the rows are scalar addresses)
  if (q >= d.n_env * d.K) return;
  const int L = c.n_line;
  const size_t lane = (size_t)d.n_env + q;
  float a = la_strided_max(tid, L, d.rho + lane * L);
#pragma unroll
  for (int m = LA_SHARES / 2; m >= 1; m >>= 1) a = fmaxf(a, __shfl_xor(a, m));
  const bool done = d.done[lane] != 0;
  if (tid == 0) {
    LaChainState s = h == 1 ? la_chain_start() : LaChainState{c.survived[q], c.peak[q], d.value[q]};
    c.value_h[(size_t)q * c.max_steps + (h - 1)] = la_chain_step(s, h, done, a);
    c.survived[q] = s.survived; c.peak[q] = s.peak; d.value[q] = s.value;
    if (la_chain_failed(s, h)) d.flags[q] = (unsigned char)(d.flags[q] | LA_DONE);
  }
  if (!advance) return;
  const size_t src = (size_t)(q / d.K);
  int idx = (d.t_obs + d.lane_offset[src]) % d.T;
  if (idx < 0) idx += d.T;
  if (tid == 0) c.lane_offset[lane] = la_chain_row(c.n_h, idx, h + 1);
  if (!d.maint) return;
  const unsigned char* M = d.maint + (size_t)d.lane_table[src] * d.T * L;
  int* t = c.topo + lane * c.dim_topo;
  int* t0 = c.topo0 + lane * c.dim_topo;
  for (int l = tid; l < L; l += LA_SHARES) {
    if (!la_maintenance_ahead(M, d.T, L, idx, h + 1, l)) continue;
    const int po = c.line_or_pos[l], pe = c.line_ex_pos[l];
    t[po] = -1; t[pe] = -1;
    t0[po] = -1; t0[pe] = -1;
  }
}

// One wavefront per environment: la_summary_kernel's summary over the chain's value and flags, the fall-back slot, and -- play != 0 --
// the chosen slot's table index into the acting path's action buffer of the environment's lane.
__global__ __launch_bounds__(64 * LA_WPB) void la_chain_summary_kernel(LaDev d, LaChainDev c, int play) {
  const int tid = threadIdx.x & 63;
  const int env = blockIdx.x * LA_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (env >= d.n_env) return;
  const float* row = d.value + (size_t)env * d.K;
  const unsigned char* fl = d.flags + (size_t)env * d.K;
  const int* sv = c.survived + (size_t)env * d.K;
  const float* pk = c.peak + (size_t)env * d.K;
  float bv = INFINITY, fp = INFINITY;
  int bk = -1, n_ok = 0, n_done = 0, fk = -1, fs = 0;
  for (int k = tid; k < d.K; k += LA_SHARES) {
    const unsigned f = fl[k];
    const bool ok = la_playable(f);
    if (la_outranks(row[k], ok ? k : -1, bv, bk)) { bv = row[k]; bk = k; }
    if (la_chain_outranks(sv[k], pk[k], la_chain_eligible(f) ? k : -1, fs, fp, fk)) { fs = sv[k]; fp = pk[k]; fk = k; }
    n_ok += ok ? 1 : 0;
    n_done += (f & LA_DONE) ? 1 : 0;
  }
#pragma unroll
  for (int m = LA_SHARES / 2; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(bv, m);
    const int ok = __shfl_xor(bk, m);
    if (la_outranks(ov, ok, bv, bk)) { bv = ov; bk = ok; }
    const int os = __shfl_xor(fs, m), ofk = __shfl_xor(fk, m);
    const float op = __shfl_xor(fp, m);
    if (la_chain_outranks(os, op, ofk, fs, fp, fk)) { fs = os; fp = op; fk = ofk; }
    n_ok += __shfl_xor(n_ok, m);
    n_done += __shfl_xor(n_done, m);
  }
  if (tid == 0) {
    d.best[env] = bk; d.best_value[env] = bv;
    d.info[(size_t)env * 2] = n_ok; d.info[(size_t)env * 2 + 1] = n_done;
    c.fallback[env] = fk; c.fallback_steps[env] = fk >= 0 ? fs : 0;
    if (play) {
      const int slot = la_chain_pick(play, bk, fk);
      c.act[env] = slot >= 0 ? d.cand[(size_t)env * d.K + slot] : -1;
    }
  }
}

}  // namespace gpf
#endif  // __HIPCC__ && GPF_LA_KERNEL
