// gridpf_n1.hpp -- the N-1 screen of the batched acting path (gpf_set_n1_screen, include/gridpf.h): the reference's N1Reward
// (Reward/n1Reward.py:64-101) for K watched lines of every environment lane of a one-step launch.  After env.step the reference copies the
// backend, takes line l_id out, runs ONE power flow and returns max(a_or / thermal_limit); here the copies are ordinary lanes behind the
// environment lanes (lane n_env + i K + k is contingency k of environment i), the power flows are the existing runpf kernels on that lane
// range, and this header holds what is new:
//   the value rule   n1_value, the ONE statement of it: is_done -> 0 (BaseReward's reward_min, which N1Reward never sets), not converged
//                    -> -1, else the maximum over the lines of a_or / th in float32 with th[th <= 1] = 1 (a_or, not rho)
//   the summary rule n1_outranks / n1_insecure: the worst contingency of an environment (a diverged one outranks every value, the lowest
//                    k wins a tie) and what counts as insecure (a value > 1, or diverged)
//   the kernels      n1_fanout_kernel (the contingency lanes' inputs from their environments' post-step state), n1_reduce_kernel (one
//                    wavefront per contingency lane), n1_summary_kernel (one wavefront per environment) and n1_slot_kernel (the table
//                    entries of GPF_RW_N1 slots into the rewards), for the one unit that defines GPF_N1_KERNEL (gridpf_capi_n1.hip)
// A reduction runs as the rewards' do: share t of 64 takes elements t, t + 64, ... in order, the shares meet in a fixed butterfly (partners
// 32, 16, 8, 4, 2, 1).  A maximum is exact in any order and the quotient is one correctly rounded float32 division, so a value is the same
// bits in every run and at every place in the batch.  Without hipcc only the rules exist: the header then needs no HIP header.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GPF_N1_HD __host__ __device__
#else
#define GPF_N1_HD
#endif

#include <math.h>
#include <stdint.h>

#include "gridpf_episode.hpp"

namespace gpf {

constexpr int N1_SHARES = 64;
constexpr int RW_N1 = 7;              // (= GPF_RW_N1 of include/gridpf.h) p[0]: index into the watched-line table
constexpr float N1_DONE = 0.f;        // BaseReward.reward_min
constexpr float N1_DIVERGED = -1.f;   // n1Reward.py:97-99

// one line's share of the maximum: th_lim[th_lim <= 1] = 1; a_or / th_lim
GPF_N1_HD inline float n1_term(float a_or, float th) { return a_or / (th <= 1.f ? 1.f : th); }

// share t of the maximum over n_line lines (-inf: the share has no line)
GPF_N1_HD inline float n1_strided(int t, int n_line, const float* a_or, const float* th) {
  float acc = -INFINITY;
  for (int l = t; l < n_line; l += N1_SHARES) acc = fmaxf(acc, n1_term(a_or[l], th[l]));
  return acc;
}

// the executor of the host emulator: the 64 shares one after the other, then the butterfly (every share ends with the same value)
struct N1Serial {
  float max_lines(int n_line, const float* a_or, const float* th) const {
    float a[N1_SHARES], b[N1_SHARES];
    for (int t = 0; t < N1_SHARES; ++t) a[t] = n1_strided(t, n_line, a_or, th);
    for (int m = N1_SHARES / 2; m >= 1; m >>= 1) {
      for (int t = 0; t < N1_SHARES; ++t) b[t] = fmaxf(a[t], a[t ^ m]);
      for (int t = 0; t < N1_SHARES; ++t) a[t] = b[t];
    }
    return a[0];
  }
};

// One contingency of one environment.  done: the environment's is_done (failed || truncated, as reward_value takes it); converged: the
// contingency lane's power flow; a_or: that lane's results; th: the thermal limits.
template <typename X>
GPF_N1_HD inline float n1_value(const X& x, bool done, bool converged, int n_line, const float* a_or, const float* th) {
  if (done) return N1_DONE;
  if (!converged) return N1_DIVERGED;
  return x.max_lines(n_line, a_or, th);
}

// the summary: contingency (va, ka) outranks (vb, kb) as an environment's worst; kb < 0: there is no b yet
GPF_N1_HD inline bool n1_diverged(float v) { return v == N1_DIVERGED; }
GPF_N1_HD inline bool n1_insecure(float v) { return n1_diverged(v) || v > 1.f; }
GPF_N1_HD inline bool n1_outranks(float va, int ka, float vb, int kb) {
  if (kb < 0) return ka >= 0;
  if (ka < 0) return false;
  const bool da = n1_diverged(va), db = n1_diverged(vb);
  if (da != db) return da;
  if (!da && va != vb) return va > vb;
  return ka < kb;
}

// one environment's summary with plain loops (the host emulator; n1_summary_kernel runs the same rules with one wavefront)
struct N1Summary { float worst; int arg_worst, n_insecure, n_diverged; };
inline N1Summary n1_summary_serial(const float* value, int K) {
  N1Summary s{0.f, -1, 0, 0};
  for (int k = 0; k < K; ++k) {
    if (n1_outranks(value[k], k, s.worst, s.arg_worst)) { s.worst = value[k]; s.arg_worst = k; }
    s.n_insecure += n1_insecure(value[k]) ? 1 : 0;
    s.n_diverged += n1_diverged(value[k]) ? 1 : 0;
  }
  return s;
}

#if defined(__HIPCC__) && defined(GPF_N1_KERNEL)
// the kernel's executor: share t is thread t of the wavefront, the butterfly goes through __shfl_xor
struct N1Wave {
  int tid;
  __device__ float max_lines(int n_line, const float* a_or, const float* th) const {
    float a = n1_strided(tid, n_line, a_or, th);
#pragma unroll
    for (int m = N1_SHARES / 2; m >= 1; m >>= 1) a = fmaxf(a, __shfl_xor(a, m));
    return a;
  }
};

// what the screen's kernels read and write.  Environment i is lane i, its contingency k lane n_env + i K + k.
struct N1Dev {
  const int* lines;                  // [K] watched lines (validated by gpf_set_n1_screen)
  double* inj;                       // [lanes][n_inj]
  int* topo;                         // [lanes][dim_topo]
  int* shunt_bus;                    // [lanes][n_shunt]
  const int* line_or_pos;            // [n_line] topo_vect position of the lines' ends
  const int* line_ex_pos;
  const float* out;                  // [lanes][n_out] results rows
  const int* status;                 // [lanes][4]
  const unsigned char* done;         // [lanes]
  const float* thermal;              // [n_line]
  const int* ep_limit;               // [lanes] episode limits, or null: off ...
  const int* episode;                // ... and the lanes' {steps survived, resets} after the step
  float* value;                      // [n_env][K]
  float* worst;                      // [n_env]
  int* info;                         // [n_env][3] {arg_worst, n_insecure, n_diverged}
  int n_env, K, n_inj, dim_topo, n_shunt, n_line, n_out, off_a_or;
};

constexpr int N1_WPB = 4;            // wavefronts per block of the reduce and summary kernels

// Block q: contingency lane n_env + q takes what runpf reads of environment q / K as the step left it -- injection row, topology row
// with line lines[q % K] out (both ends -1; a line that is already out leaves the base case), shunt buses.  Nothing comes from the host.
__global__ __launch_bounds__(64) void n1_fanout_kernel(N1Dev d) {
  const int q = blockIdx.x;
  if (q >= d.n_env * d.K) return;
  const size_t src = (size_t)(q / d.K), dst = (size_t)d.n_env + q;
  const int tid = threadIdx.x;
  const int ol = d.lines[q % d.K];
  const int po = d.line_or_pos[ol], pe = d.line_ex_pos[ol];
  const double* sinj = d.inj + src * d.n_inj;
  double* dinj = d.inj + dst * d.n_inj;
  for (int i = tid; i < d.n_inj; i += 64) dinj[i] = sinj[i];
  const int* st = d.topo + src * d.dim_topo;
  int* dt = d.topo + dst * d.dim_topo;
  for (int i = tid; i < d.dim_topo; i += 64) dt[i] = (i == po || i == pe) ? -1 : st[i];
  const int* ss = d.shunt_bus + src * d.n_shunt;
  int* ds = d.shunt_bus + dst * d.n_shunt;
  for (int i = tid; i < d.n_shunt; i += 64) ds[i] = ss[i];
}

// One wavefront per contingency lane, N1_WPB per block; no LDS, no scratch, no atomics, no block-wide barrier.  Read-only on the lanes.
__global__ __launch_bounds__(64 * N1_WPB) void n1_reduce_kernel(N1Dev d) {
  const int tid = threadIdx.x & 63;
  const int q = blockIdx.x * N1_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform: the rows are scalar addresses)
  if (q >= d.n_env * d.K) return;
  const size_t env = (size_t)(q / d.K), lane = (size_t)d.n_env + q;
  const bool failed = d.done[env] != 0;
  const bool truncated = d.ep_limit && episode_truncated(d.episode[env * 2], d.ep_limit[env], failed);
  const bool converged = d.status[lane * 4] == 0;
  const float v = n1_value(N1Wave{tid}, failed || truncated, converged, d.n_line, d.out + lane * d.n_out + d.off_a_or, d.thermal);
  if (tid == 0) d.value[q] = v;
}

// One wavefront per environment: thread t takes contingencies t, t + 64, ...; the ranking is a total order and the counts are integers, so
// the butterfly gives the same summary whatever the order.
__global__ __launch_bounds__(64 * N1_WPB) void n1_summary_kernel(N1Dev d) {
  const int tid = threadIdx.x & 63;
  const int env = blockIdx.x * N1_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (env >= d.n_env) return;
  const float* row = d.value + (size_t)env * d.K;
  float bv = 0.f;
  int bk = -1, n_ins = 0, n_div = 0;
  for (int k = tid; k < d.K; k += N1_SHARES) {
    const float v = row[k];
    if (n1_outranks(v, k, bv, bk)) { bv = v; bk = k; }
    n_ins += n1_insecure(v) ? 1 : 0;
    n_div += n1_diverged(v) ? 1 : 0;
  }
#pragma unroll
  for (int m = N1_SHARES / 2; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(bv, m);
    const int ok = __shfl_xor(bk, m);
    if (n1_outranks(ov, ok, bv, bk)) { bv = ov; bk = ok; }
    n_ins += __shfl_xor(n_ins, m);
    n_div += __shfl_xor(n_div, m);
  }
  if (tid == 0) {
    d.worst[env] = bv;
    d.info[(size_t)env * 3] = bk; d.info[(size_t)env * 3 + 1] = n_ins; d.info[(size_t)env * 3 + 2] = n_div;
  }
}

// GPF_RW_N1 slots: slot s of lane lane0 + r, r < n, takes value[lane][slot_idx[s]] when slot_idx[s] >= 0 and the lane is an environment
// (reward_kernel, which knows no such kind, left 0 there).  One thread per (lane, slot).
__global__ __launch_bounds__(256) void n1_slot_kernel(const float* __restrict__ value, const int* __restrict__ slot_idx, int n_slot, int n_env, int K,
                                                      int lane0, int n, float* __restrict__ reward, long long row_stride) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * n_slot) return;
  const int r = i / n_slot, s = i - r * n_slot, lane = lane0 + r;
  const int idx = slot_idx[s];
  if (idx < 0 || lane >= n_env) return;
  reward[(size_t)r * row_stride + s] = value[(size_t)lane * K + idx];
}
#endif  // __HIPCC__ && GPF_N1_KERNEL

}  // namespace gpf
