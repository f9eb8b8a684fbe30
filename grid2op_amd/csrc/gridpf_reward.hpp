// gridpf_reward.hpp -- the environment's rewards of the batched acting path (gpf_set_rewards, include/gridpf.h): what env.step returns as
// `reward` and info["rewards"], for every lane of a one-step launch.  Paths relative to the reference checkout:
//   RW_REDISP          RedispReward.__call__ (Reward/redispReward.py:169-211)
//   RW_L2RPN           L2RPNReward.__call__ (Reward/l2RPNReward.py:56-77)
//   RW_LINES_CAPACITY  LinesCapacityReward.__call__ (Reward/linesCapacityReward.py:49-62)
//   RW_ECONOMIC        EconomicReward.__call__ (Reward/economicReward.py:57-71)
//   RW_GAMEPLAY        GameplayReward.__call__ (Reward/gameplayReward.py:44-52)
// Two parts: the rule core (plain C++, the ONE statement of every formula: reward_value, on an executor that says how a reduction over a
// lane's elements runs) and the kernel.  Every reduction of every kind goes through reward_strided: share t of 64 takes elements t, t + 64,
// ... in order, the 64 shares are combined by a fixed butterfly (partners 32, 16, 8, 4, 2, 1).  All of it in float64 from the float32
// inputs, one rounding to float32 per slot: a lane's rewards are the same bits in every run and at every place in the batch.  The kernel's
// executor is a wavefront (share t = thread t, the butterfly through __shfl_xor); the host emulator of tests/native/ runs the same shares
// and the same butterfly with loops.  Without hipcc only the core exists: the header then needs no HIP header.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GPF_RW_HD __host__ __device__
#else
#define GPF_RW_HD
#endif

#include <math.h>
#include <stdint.h>

#include "gridpf_episode.hpp"

namespace gpf {

// kinds (= GPF_RW_* of include/gridpf.h) and the parameters p[] of each
constexpr int RW_REDISP = 1;          // p: alpha_redisp, max_regret, min_reward, reward_illegal_ambiguous, dts (hours per step)
constexpr int RW_L2RPN = 2;           // p: none
constexpr int RW_LINES_CAPACITY = 3;  // p: none
constexpr int RW_ECONOMIC = 4;        // p: worst_cost, reward_min, reward_max, dts
constexpr int RW_GAMEPLAY = 5;        // p: reward_min, reward_max
constexpr int RW_MAX_SLOTS = 8;
constexpr int RW_SHARES = 64;

struct RewardSlot { int32_t kind; double p[6]; };     // (= gpf_reward_slot)

// one lane's inputs: the float32 results of the step, the grid's thermal limits and costs, the lane's dispatch (null: none) and the
// storage set-points of its injection row (float64 there; the formulas take them as float32, which is what the dynamics wrote)
struct RewardRow {
  const float *gen_p, *load_p, *a_or, *rho, *thermal, *dispatch, *cost;
  const double* storage;
  const unsigned char* line_status;
  int n_gen, n_load, n_line, n_sto;
};

struct RwAdd { GPF_RW_HD double operator()(double a, double b) const { return a + b; } };
struct RwMax { GPF_RW_HD double operator()(double a, double b) const { return fmax(a, b); } };

// share t of a reduction over n elements: elements t, t + 64, ... combined in that order, starting from init
template <typename Term, typename Op>
GPF_RW_HD inline double reward_strided(int t, int n, double init, Term term, Op op) {
  double acc = init;
  for (int i = t; i < n; i += RW_SHARES) acc = op(acc, term(i));
  return acc;
}

// the executor of the host emulator: the 64 shares one after the other, then the butterfly (every share ends with the same value)
struct RewardSerial {
  template <typename Term, typename Op>
  double reduce(int n, double init, Term term, Op op) const {
    double a[RW_SHARES], b[RW_SHARES];
    for (int t = 0; t < RW_SHARES; ++t) a[t] = reward_strided(t, n, init, term, op);
    for (int m = RW_SHARES / 2; m >= 1; m >>= 1) {
      for (int t = 0; t < RW_SHARES; ++t) b[t] = op(a[t], a[t ^ m]);
      for (int t = 0; t < RW_SHARES; ++t) a[t] = b[t];
    }
    return a[0];
  }
};

#if defined(__clang__)
#define GPF_RW_NO_FMA _Pragma("clang fp contract(off)")
#else
#define GPF_RW_NO_FMA
#endif

// LinesCapacityReward with no line connected: numpy.interp(0, [0, 0], [0, 1]) (pinned against numpy by tests/test_reward_cpu.py)
constexpr double RW_LINES_CAPACITY_NONE = 1.0;

// One slot of one lane.  failed: the lane's episode-ending step (the engine's done = the reference's is_done and has_error);
// illegal / ambiguous: the reference's is_illegal / is_ambiguous of the step.  Out of the reference's domain: RW_REDISP without a
// generator that produces (the reference raises) is a quiet NaN; a zero load sum gives the IEEE quotient.  truncated: the step reached the
// lane's episode limit without failing (episode_truncated): the reference's is_done is failed || truncated, and two kinds read it --
// L2RPNReward returns 0 when is_done (l2RPNReward.py:57), RedispReward gives an illegal or ambiguous FINAL step reward_min
// (redispReward.py:171-176).
template <typename X>
GPF_RW_HD inline float reward_value(const X& x, const RewardSlot& s, const RewardRow& r, bool failed, bool illegal, bool ambiguous,
                                    bool truncated = false) {
  GPF_RW_NO_FMA
  const bool bad = illegal || ambiguous;
  const double* p = s.p;
  switch (s.kind) {
    case RW_REDISP: {
      if (failed) return (float)p[2];
      if (bad) return (float)(truncated ? p[2] : p[3]);
      const double sg = x.reduce(r.n_gen, 0.0, [&](int i) { return (double)r.gen_p[i]; }, RwAdd{});
      const double sl = x.reduce(r.n_load, 0.0, [&](int i) { return (double)r.load_p[i]; }, RwAdd{});
      const double sd = r.dispatch ? x.reduce(r.n_gen, 0.0, [&](int i) { return fabs((double)r.dispatch[i]); }, RwAdd{}) : 0.0;
      const double ss = x.reduce(r.n_sto, 0.0, [&](int i) { return fabs((double)(float)r.storage[i]); }, RwAdd{});
      // marginal cost: the dearest generator that produces (costs are >= 0: -1 says "none")
      const double mc = x.reduce(r.n_gen, -1.0, [&](int i) { return r.gen_p[i] > 0.f ? (double)r.cost[i] : -1.0; }, RwMax{});
      if (mc < 0.0) return __builtin_nanf("");
      const double regret = (mc * p[4]) * (((sg - sl) + p[0] * sd) + ss);
      return (float)((p[1] - regret) / sl);
    }
    case RW_L2RPN: {
      if (failed || truncated) return 0.f;
      const double v = x.reduce(r.n_line, 0.0, [&](int i) {
        const double rel = fmin(fabs((double)r.a_or[i]) / (fabs((double)r.thermal[i]) + (double)0.1f), 1.0);
        return fmax(1.0 - rel * rel, 0.0);
      }, RwAdd{});
      return (float)v;
    }
    case RW_LINES_CAPACITY: {
      if (failed || bad) return 0.f;
      const double n = x.reduce(r.n_line, 0.0, [&](int i) { return r.line_status[i] ? 1.0 : 0.0; }, RwAdd{});
      const double us = x.reduce(r.n_line, 0.0, [&](int i) { return r.line_status[i] ? (double)r.rho[i] : 0.0; }, RwAdd{});
      if (n == 0.0) return (float)RW_LINES_CAPACITY_NONE;
      const double u = fmin(fmax(us, 0.0), n);
      return (float)((n - u) / n);
    }
    case RW_ECONOMIC: {
      if (failed || bad) return (float)p[1];
      const double c = x.reduce(r.n_gen, 0.0, [&](int i) { return (double)r.gen_p[i] * (double)r.cost[i]; }, RwAdd{}) * p[3];
      const double v = fmin(fmax(p[0] - c, 0.0), p[0]);
      return (float)(p[1] + (p[2] - p[1]) * (v / p[0]));
    }
    case RW_GAMEPLAY:
      if (failed) return (float)p[0];
      if (bad) return (float)p[0] / 2.0f;
      return (float)p[1];
    default:
      return 0.f;                      // (unknown kinds are refused by gpf_set_rewards)
  }
}

#ifdef __HIPCC__
// the kernel's executor: share t is thread t of the wavefront, the butterfly goes through __shfl_xor (every thread ends with the same value)
struct RewardWave {
  int tid;
  template <typename Term, typename Op>
  __device__ double reduce(int n, double init, Term term, Op op) const {
    double a = reward_strided(tid, n, init, term, op);
#pragma unroll
    for (int m = RW_SHARES / 2; m >= 1; m >>= 1) a = op(a, __shfl_xor(a, m));
    return a;
  }
};

// what the kernel reads and writes
struct RewardDev {
  const float* out;                  // [lanes][n_out] results rows
  const double* inj;                 // [lanes][n_inj] injection rows (the storage set-points)
  const float* rho;                  // [lanes][n_line]
  const unsigned char* line_status;  // [lanes][n_line]
  const float* thermal;              // [n_line]
  const float* dispatch;             // [lanes][n_gen] actual dispatch / redispatch delta, or null: none
  const float* cost;                 // [n_gen] gen_cost_per_MW, or null (no slot reads it)
  const unsigned char* done;         // [lanes]
  const int* status;                 // [lanes][4], or null: done alone says "failed" (behind a step they agree)
  const unsigned char* topo_flags;   // [lanes][2] {illegal, ambiguous} of THIS launch's topology actions, or null: it carried none
  const int* ill_now;                // [lanes] cancelled redispatch actions since the reset, after the step ...
  const int* ill_snap;               // ... and before it; both null: no dynamics
  const unsigned char* eval_flags;   // [n][2] the caller's flags (gpf_rewards_eval), indexed from the range's first lane, or null
  const unsigned char* step_flags;   // [lanes][4] {illegal, ambiguous, illegal redispatch, reason} of the whole step (combined mode), or null
  const int* ep_limit;               // [lanes] episode limits (gpf_set_episode_limit), or null: off, or gpf_rewards_eval ...
  const int* episode;                // ... and the lanes' {steps survived, resets} after the step
  float* reward;                     // row of the range's first lane
  long long row_stride;
  int n_out, n_inj, off_gen_p, off_load_p, off_a_or, off_sto, n_gen, n_load, n_line, n_sto;
};

constexpr int RW_WPB = 4;            // lanes (wavefronts) per block

// One wavefront per lane, RW_WPB lanes per block, the slots in a wave-uniform loop; no LDS, no scratch, no atomics, no block-wide barrier.
// Queued last in a one-step launch (after the alert post-step), and by gpf_rewards_eval on the lanes' current state.  Read-only on the
// lanes' state: it writes the n_slot rewards of each lane of [lane0, lane0 + n).
__global__ __launch_bounds__(64 * RW_WPB) void reward_kernel(RewardDev d, const RewardSlot* slots, int n_slot, int lane0, int n) {
  const int tid = threadIdx.x & 63;
  const int k = blockIdx.x * RW_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (wave-uniform: the lane's rows are scalar addresses)
  if (k >= n) return;
  const size_t lane = (size_t)lane0 + k;
  bool failed = d.done[lane] != 0;
  if (d.status) failed = failed || d.status[lane * 4] != 0;
  bool illegal = false, ambiguous = false;
  if (d.topo_flags) { illegal = d.topo_flags[lane * 2] != 0; ambiguous = d.topo_flags[lane * 2 + 1] != 0; }
  if (d.ill_now) illegal = illegal || d.ill_now[lane] != d.ill_snap[lane];
  if (d.step_flags) { illegal = illegal || d.step_flags[lane * 4] != 0 || d.step_flags[lane * 4 + 2] != 0; ambiguous = ambiguous || d.step_flags[lane * 4 + 1] != 0; }
  if (d.eval_flags) { illegal = illegal || d.eval_flags[(size_t)k * 2] != 0; ambiguous = ambiguous || d.eval_flags[(size_t)k * 2 + 1] != 0; }
  const bool truncated = d.ep_limit && episode_truncated(d.episode[lane * 2], d.ep_limit[lane], failed);
  const float* row = d.out + lane * d.n_out;
  RewardRow r;
  r.gen_p = row + d.off_gen_p; r.load_p = row + d.off_load_p; r.a_or = row + d.off_a_or;
  r.rho = d.rho + lane * d.n_line; r.line_status = d.line_status + lane * d.n_line; r.thermal = d.thermal;
  r.dispatch = d.dispatch ? d.dispatch + lane * d.n_gen : nullptr; r.cost = d.cost;
  r.storage = d.inj + lane * d.n_inj + d.off_sto;
  r.n_gen = d.n_gen; r.n_load = d.n_load; r.n_line = d.n_line; r.n_sto = d.n_sto;
  float* o = d.reward + (size_t)k * d.row_stride;
  const RewardWave x{tid};
  for (int s = 0; s < n_slot; ++s) {
    const float v = reward_value(x, slots[s], r, failed, illegal, ambiguous, truncated);
    if (tid == 0) o[s] = v;
  }
}
#endif  // __HIPCC__

}  // namespace gpf
