// gridpf_episode.hpp -- episode time limits of the batched acting path (gpf_set_episode_limit, include/gridpf.h): what BaseEnv.step calls
// `done` without an error, for every lane of a one-step launch.  Paths relative to the reference checkout:
//   the limit          chronics_handler.done() at max_episode_duration(), env.reset(options={"max step": N}) (Environment/baseEnv.py step)
//   the flags          terminated = has_error, truncated = is_done and not has_error -- episode_truncated, the ONE statement of the rule,
//                      called by reward_kernel (gridpf_reward.hpp), alert_poststep_kernel (gridpf_alert.hpp) and episode_kernel below
//   the length         env.nb_time_step of the episode that ended (the failing step counts) -- episode_length
//   the duration       EpisodeDurationReward.__call__ (Reward/episodeDurationReward.py:64-71) -- episode_duration_reward
//   the returns        a sequential float64 sum of the float32 rewards of gridpf_reward.hpp, one add per slot and launch -- episode_return_add
//   the reset          what the step kernel does for a failed lane under auto_reset (gridpf_sparse.hpp) and topo_poststep_kernel's reset
//                      branch (gridpf_topo.hpp: topo_reset_acting below, shared with it)
// Two parts: the rules (plain C++, run by the kernel and by the host emulator of tests/native/) and, for the one unit that defines
// GPF_EPISODE_KERNEL (gridpf_capi_episode.hip), the kernel.  Without hipcc only the rules exist: the header then needs no HIP header.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GPF_EP_HD __host__ __device__
#else
#define GPF_EP_HD
#endif

#include <stdint.h>

namespace gpf {

constexpr int EP_MAX_SLOTS = 8;       // row width of the returns (= GPF_REWARD_MAX_SLOTS: the rows do not move when the slots change)

// steps: the lane's episode[0] AFTER the step; limit: its step limit (0: none); done: the step failed.  A step that both fails and
// reaches the limit is terminated, not truncated (the reference's has_error case).
GPF_EP_HD inline bool episode_truncated(int steps, int limit, bool done) { return !done && limit > 0 && steps >= limit; }

// nb_time_step of the episode that ended in this launch (0: it goes on).  steps_before: episode[0] before the step.
GPF_EP_HD inline int episode_length(bool terminated, bool truncated, int steps_before, int steps_after) {
  return terminated ? steps_before + 1 : truncated ? steps_after : 0;
}

// EpisodeDurationReward: nb_time_step / (max_episode_duration x per_timestep) when the episode ended, else reward_min = 0; without a
// limit the reference's total_time_steps is infinite and the value is the length.  total_time_steps is float32 as dt_float keeps it.
GPF_EP_HD inline float episode_duration_reward(bool ended, int length, int limit, float per_timestep) {
  if (!ended) return 0.f;
  if (limit <= 0) return (float)length;
  const float total = (float)limit * per_timestep;
  return (float)((double)length / (double)total);
}

// one slot's running return after this launch's reward
GPF_EP_HD inline double episode_return_add(double running, float reward) { return running + (double)reward; }

// the acting path's state of a lane that starts a new episode (env.reset(): no substation cooldown, last known busbar = the reset
// topology, busbar 1 where it has an open end): elements first, first + stride, ...
GPF_EP_HD inline void topo_reset_acting(int* sub_cd, int* last_bus, const int* topo0_row, int n_sub, int dim_topo, int first, int stride) {
  for (int i = first; i < n_sub; i += stride) sub_cd[i] = 0;
  for (int i = first; i < dim_topo; i += stride) { const int v = topo0_row[i]; last_bus[i] = v >= 1 ? v : 1; }
}

// ---- one lane with plain loops (the host emulator; the kernel below runs the same rules with one wavefront per lane) ------------------
struct EpisodeLane {                  // what a launch leaves for one lane
  int terminated, truncated, length;
  float duration_reward;
};
struct EpisodeStats {                 // the lane's statistics across launches
  double running[EP_MAX_SLOTS], last[EP_MAX_SLOTS];
  int length_last, n_episodes, steps_prev;
};

// rewards: the n_slot float32 rewards of this launch (null: rewards are off).  Returns 1 when an episode ended in this launch for the
// first time (a truncated lane that is left alone re-flags on later launches, its statistics roll over once).
inline int episode_poststep_serial(int steps_after, int limit, int done, float per_timestep, const float* rewards, int n_slot,
                                   EpisodeLane& o, EpisodeStats& st) {
  const bool term = done != 0, trunc = episode_truncated(steps_after, limit, term);
  const bool fresh = term || (trunc && st.steps_prev < limit);
  o.terminated = term; o.truncated = trunc;
  o.length = episode_length(term, trunc, st.steps_prev, steps_after);
  o.duration_reward = episode_duration_reward(term || trunc, o.length, limit, per_timestep);
  for (int s = 0; rewards && s < n_slot; ++s) {
    const double r = episode_return_add(st.running[s], rewards[s]);
    if (fresh) { st.last[s] = r; st.running[s] = 0.0; } else st.running[s] = r;
  }
  if (fresh) { st.length_last = o.length; ++st.n_episodes; }
  st.steps_prev = steps_after;
  return fresh ? 1 : 0;
}

#if defined(__HIPCC__) && defined(GPF_EPISODE_KERNEL)
// what the kernel reads and writes (rows padded to the engine's lane capacity)
struct EpisodeDev {
  const int* limit;                  // [lanes]
  int* episode;                      // [lanes][2] {steps survived, resets}
  const unsigned char* done;         // [lanes]
  unsigned char* flags;              // [lanes][2] {terminated, truncated}
  int* length;                       // [lanes]
  float* duration;                   // [lanes]
  int* steps_prev;                   // [lanes] episode[lane][0] as the last launch left it
  const float* reward;               // [lanes][n_slot] rewards of this launch, or null: rewards are off
  double* ret_run; double* ret_last; // [lanes][EP_MAX_SLOTS]
  int* length_last; int* n_episodes; // [lanes]
  float per_timestep;
  int n_slot;
  // the reset of a truncated lane (auto_reset != 0)
  int auto_reset, dim_topo, n_line, n_sub, n_gen, n_sto, n_shunt;
  int* topo; const int* topo0; int* overflow_count;
  int* cooldown;                     // null: the launch does not track the line cooldowns
  // the environment dynamics, all null while they are off
  float* env_target; float* env_actual; float* env_prev; float* env_limit; float* env_amount_prev; float* env_curt_prev; float* env_charge;
  const float* env_charge0;          // [n_sto], or null: 0
  unsigned char* env_already; unsigned char* env_fresh; int* env_illegal;
  // the acting path, null while it is off
  int* sub_cd; int* last_bus;
  // re-keying by the host (null: nobody asked): count | lanes, and their reset rows [dim_topo + n_shunt]
  int* list; int* list_rows; const int* shunt_bus;
};

constexpr int EP_WPB = 4;            // lanes (wavefronts) per block

// One wavefront per lane, EP_WPB lanes per block; no LDS, no scratch, no block-wide barrier (blocks hold lanes that return early), row
// loops of stride 64, plain vector stores, one atomicAdd per truncated lane and only when the host asked for the list.  Queued last in a
// one-step launch, after reward_kernel: the rewards and the alert reward of a truncated step saw the step's state, this kernel then
// books the episode and, under auto_reset, puts a truncated lane where the step kernel puts a failed one.
__global__ __launch_bounds__(64 * EP_WPB) void episode_kernel(EpisodeDev d, int n_lanes) {
  const int tid = threadIdx.x & 63;
  const int lane = blockIdx.x * EP_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform: the lane's rows are scalar addresses)
  if (lane >= n_lanes) return;
  const int steps = d.episode[(size_t)lane * 2], resets = d.episode[(size_t)lane * 2 + 1];
  const int limit = d.limit[lane], before = d.steps_prev[lane];
  const bool term = d.done[lane] != 0, trunc = episode_truncated(steps, limit, term);
  const bool fresh = term || (trunc && before < limit);
  const int length = episode_length(term, trunc, before, steps);
  if (d.reward && tid < d.n_slot) {
    double* run = d.ret_run + (size_t)lane * EP_MAX_SLOTS + tid;
    const double r = episode_return_add(*run, d.reward[(size_t)lane * d.n_slot + tid]);
    if (fresh) { d.ret_last[(size_t)lane * EP_MAX_SLOTS + tid] = r; *run = 0.0; } else *run = r;
  }
  const bool reset = trunc && d.auto_reset != 0;
  if (tid == 0) {
    d.flags[(size_t)lane * 2] = term ? 1 : 0; d.flags[(size_t)lane * 2 + 1] = trunc ? 1 : 0;
    d.length[lane] = length;
    d.duration[lane] = episode_duration_reward(term || trunc, length, limit, d.per_timestep);
    if (fresh) { d.length_last[lane] = length; d.n_episodes[lane] += 1; }
    d.steps_prev[lane] = reset ? 0 : steps;
  }
  if (!reset) return;
  const int D = d.dim_topo, L = d.n_line;
  const int* t0 = d.topo0 + (size_t)lane * D;
  int* topo = d.topo + (size_t)lane * D;
  for (int i = tid; i < D; i += 64) topo[i] = t0[i];
  for (int l = tid; l < L; l += 64) d.overflow_count[(size_t)lane * L + l] = 0;
  if (d.cooldown) for (int l = tid; l < L; l += 64) d.cooldown[(size_t)lane * L + l] = 0;
  if (d.env_target) {                // env.reset(): dispatch cleared, storage back to its initial charge
    const size_t g0 = (size_t)lane * d.n_gen;
    for (int i = tid; i < d.n_gen; i += 64) {
      d.env_target[g0 + i] = 0.f; d.env_actual[g0 + i] = 0.f; d.env_prev[g0 + i] = 0.f; d.env_limit[g0 + i] = 1.f; d.env_already[g0 + i] = 0;
    }
    for (int i = tid; i < d.n_sto; i += 64) d.env_charge[(size_t)lane * d.n_sto + i] = d.env_charge0 ? d.env_charge0[i] : 0.f;
    if (tid == 0) { d.env_amount_prev[lane] = 0.f; d.env_curt_prev[lane] = 0.f; d.env_fresh[lane] = 1; d.env_illegal[lane] = 0; }
  }
  if (d.sub_cd) topo_reset_acting(d.sub_cd + (size_t)lane * d.n_sub, d.last_bus + (size_t)lane * D, t0, d.n_sub, D, tid, 64);
  if (tid == 0) { d.episode[(size_t)lane * 2] = 0; d.episode[(size_t)lane * 2 + 1] = resets + 1; }
  if (d.list) {                      // the lane is back on the class of its reset topology: the launch planner must learn it
    int slot = 0;
    if (tid == 0) { slot = atomicAdd(&d.list[0], 1); d.list[1 + slot] = lane; }
    slot = __builtin_amdgcn_readfirstlane(slot);
    int* dst = d.list_rows + (size_t)slot * (D + d.n_shunt);
    for (int i = tid; i < D; i += 64) dst[i] = t0[i];
    for (int i = tid; i < d.n_shunt; i += 64) dst[D + i] = d.shunt_bus[(size_t)lane * d.n_shunt + i];
  }
}
#endif  // __HIPCC__ && GPF_EPISODE_KERNEL

}  // namespace gpf
