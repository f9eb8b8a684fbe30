// gridpf_alert.hpp -- alerts and AlertReward of the batched acting path (gpf_set_alerts, include/gridpf.h): what BaseEnv.step keeps about the
// agent's alerts and the opponent's attacks in an environment with alertable lines, and the reward that scores the alerts, for every lane of
// a one-step launch.  Paths relative to the reference checkout:
//   the bookkeeping  BaseEnv._update_alert_properties (Environment/baseEnv.py:3295-3329), called after the opponent and before the power flow
//                    -- alert_update_line; BaseEnv._reset_alert (:1677-1685) -- alert_reset_line;
//   the reward       AlertReward (Reward/alertReward.py:105-207): _update_state (:144-156) -- alert_ring_update; the blackout branch
//                    (:158-170, 185-193) -- alert_window_first + alert_reward_blackout; the other branch (:194-206) --
//                    alert_reward_no_blackout; reset (:117-123) clears what alert_reset_aux clears.
// The alertable lines are the opponent's attackable lines (alerts_info.json {"by_line": "opponent"}), A <= 64 of them, and the reward's
// rings have R = time_window + 2 <= 64 rows: every boolean vector of the reference is ONE 64-bit word here (bit i = alertable line i) and
// every ring is R words.  Two parts: the rules (plain C++, the ONE statement of each, run by the kernels with one thread per alertable line
// and by the host emulator of tests/native/ with a loop over the lines) and the two kernels.  Without hipcc only the first exists: the
// header then needs no HIP header.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GPF_ALERT_HD __host__ __device__
#else
#define GPF_ALERT_HD
#endif

#include <stdint.h>

#include "gridpf_episode.hpp"

namespace gpf {

// the lane's block the observation reads: int32 [6 A + 1], sections of A elements at k * A (= GPF_ALERT_OBS_* of include/gridpf.h)
constexpr int AO_ACTIVE = 0;          // _last_alert (obs.active_alert)
constexpr int AO_SINCE_ALERT = 1;     // _time_since_last_alert
constexpr int AO_DURATION = 2;        // _alert_duration
constexpr int AO_SINCE_ATTACK = 3;    // _time_since_last_attack
constexpr int AO_UNDER_ALERT = 4;     // _attack_under_alert
constexpr int AO_USED = 5;            // _was_alert_used_after_attack
constexpr int AO_TOTAL = 6;           // _total_number_of_alert: ONE element at 6 A
GPF_ALERT_HD inline int alert_obs_ints(int A) { return 6 * A + 1; }
// the lane's words: uint64 [3 + 2 R]
constexpr int AX_ALREADY = 0;         // _is_already_attacked
constexpr int AX_CURRENT = 1;         // AlertReward._lines_currently_attacked
constexpr int AX_ID = 2;              // bits 0-31 AlertReward._current_id, bit 32: the lane's pre-step ran in this launch
constexpr int AX_RINGS = 3;           // _ts_attack [R], then _alert_launched [R]
constexpr uint64_t AX_RAN = (uint64_t)1 << 32;
// bit 33: this step may be the lane's truncated one (it reaches the episode limit unless it fails), so the pre-step left
// _was_alert_used_after_attack as the previous step's reward had set it: on a done without an error AlertReward returns its bonus BEFORE
// _update_state clears that array (alertReward.py:179-183), and the final observation shows the previous step's values.  The post-step
// clears it after all when the step was not truncated.
constexpr uint64_t AX_KEPT = (uint64_t)1 << 33;
GPF_ALERT_HD inline bool alert_may_truncate(int steps_before, int limit) { return limit > 0 && steps_before + 1 >= limit; }
GPF_ALERT_HD inline int alert_aux_words(int W) { return 3 + 2 * (W + 2); }

struct AlertCfg {
  int A, W;                           // alertable lines, ALERT_TIME_WINDOW
  float min_no_blackout, min_blackout, max_no_blackout, max_blackout;   // AlertReward's constants (float32, as dt_float keeps them)
};

GPF_ALERT_HD inline uint64_t alert_valid_bits(int A) { return A >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << A) - 1); }
GPF_ALERT_HD inline int alert_popcount(uint64_t x) { return __builtin_popcountll(x); }

// one alertable line's integers of the environment
struct AlertLine { int last, since_alert, duration, since_attack, under_alert; };

// BaseEnv._reset_alert (baseEnv.py:1677-1685) on one line
GPF_ALERT_HD inline void alert_reset_line(AlertLine& s, int& used) {
  s.last = 0; s.since_alert = -1; s.duration = 0; s.since_attack = -1; s.under_alert = 0; used = 0;
}

// BaseEnv._update_alert_properties (baseEnv.py:3304-3329) on one line.  raise: the agent's alert on it; att: the line is in the attack of
// this step; has_attack: the step has an attack at all (info["opponent_attack_line"] is not None); already: _is_already_attacked.
// Returns the line's new _is_already_attacked: set by an attack, NOT cleared for a line that leaves a continuing attack, cleared only by a
// step without attack.
GPF_ALERT_HD inline bool alert_update_line(int W, bool raise, bool att, bool has_attack, bool already, AlertLine& s) {
  s.last = raise ? 1 : 0;
  if (raise) s.since_alert = 0; else if (s.since_alert != -1) ++s.since_alert;
  s.duration = raise ? s.duration + 1 : 0;
  if (has_attack) {
    if (att && !already) s.since_attack = 0; else if (s.since_attack != -1) ++s.since_attack;
    already = already || att;
  } else {
    if (s.since_attack != -1) ++s.since_attack;
    already = false;
  }
  if (s.since_attack == 0) s.under_alert = 2 * s.last - 1;
  if (s.since_attack > W) s.under_alert = 0;
  return already;
}

// AlertReward.reset (alertReward.py:117-123) and the lane's _is_already_attacked
GPF_ALERT_HD inline void alert_reset_aux(int W, uint64_t* ax, int first, int stride) {
  for (int i = first; i < alert_aux_words(W); i += stride) ax[i] = 0;
}

// AlertReward._update_state (alertReward.py:125-152): the ring index advances, the newly attacked lines are noted in its row of _ts_attack
// (bits are only set: the row is cleared by a step without attack, or when it is scored), the alerts in its row of _alert_launched
GPF_ALERT_HD inline void alert_ring_update(int W, uint64_t* ax, uint64_t att, uint64_t raise) {
  const int R = W + 2;
  const int id = ((int)(uint32_t)ax[AX_ID] + 1) % R;
  uint64_t* ts = ax + AX_RINGS;
  uint64_t* al = ts + R;
  if (att == 0) { ax[AX_CURRENT] = 0; ts[id] = 0; }
  else { ts[id] |= att & ~ax[AX_CURRENT]; ax[AX_CURRENT] = att; }
  al[id] = raise;
  ax[AX_ID] = (uint64_t)(uint32_t)id | AX_RAN;
}

// ring row of position i of the window walk (rows current_id - W .. current_id, in that order)
GPF_ALERT_HD inline int alert_window_row(int W, int id, int i) { return ((id - W + i) % (W + 2) + (W + 2)) % (W + 2); }

// the blackout branch's walk (alertReward.py:158-169): every line takes the FIRST of the n rows where it is set.  row(i, ts, al) gives the
// two ring words of position i.  seen: the lines attacked in the window; alerted: those whose first row carries an alert on them.
template <typename Row>
GPF_ALERT_HD inline void alert_window_first(int n, Row row, uint64_t& seen, uint64_t& alerted) {
  seen = 0; alerted = 0;
  for (int i = 0; i < n; ++i) {
    uint64_t ts, al;
    row(i, ts, al);
    alerted |= ts & ~seen & al;
    seen |= ts;
  }
}

// the rewards: a count ratio (numpy's mean of a boolean vector) times a float32 constant plus a float32 constant, in float64 with two
// roundings (no fused multiply-add), stored as float32
#if defined(__clang__)
#define GPF_ALERT_NO_FMA _Pragma("clang fp contract(off)")
#else
#define GPF_ALERT_NO_FMA
#endif
GPF_ALERT_HD inline float alert_reward_blackout(const AlertCfg& c, uint64_t seen, uint64_t alerted) {
  GPF_ALERT_NO_FMA
  if (!seen) return 0.f;
  const double mean = (double)alert_popcount(alerted) / (double)alert_popcount(seen);
  const double prod = mean * (double)(float)(c.max_blackout - c.min_blackout);
  return (float)(prod + (double)c.min_blackout);
}
GPF_ALERT_HD inline float alert_reward_no_blackout(const AlertCfg& c, uint64_t lines, uint64_t alerts) {
  GPF_ALERT_NO_FMA
  if (!lines) return 0.f;
  const double mean = (double)alert_popcount(alerts & lines) / (double)alert_popcount(lines);
  const double prod = (double)(float)(c.min_no_blackout - c.max_no_blackout) * mean;
  return (float)(prod + (double)c.max_no_blackout);
}
// _was_alert_used_after_attack of one scored line: the two branches have opposite sign conventions, as in the reference
GPF_ALERT_HD inline int alert_used_blackout(bool alerted) { return alerted ? 1 : -1; }
GPF_ALERT_HD inline int alert_used_no_blackout(bool alerted) { return alerted ? -1 : 1; }

// ---- one lane with plain loops (the host emulator; the kernels below run the same rules with one thread per line) -----------------------
// ob: the lane's observation block, ax: its words.  steps_survived / done: the lane's episode[0] and done flag BEFORE the step.
// Returns 1 when the lane's bookkeeping ran (neither reset nor left alone).
inline int alert_prestep_serial(const AlertCfg& c, int* ob, uint64_t* ax, int steps_survived, int done, uint64_t raise, uint64_t att, int limit = 0) {
  const int A = c.A;
  if (steps_survived == 0) {
    for (int t = 0; t < A; ++t) {
      AlertLine s;
      alert_reset_line(s, ob[AO_USED * A + t]);
      ob[AO_ACTIVE * A + t] = s.last; ob[AO_SINCE_ALERT * A + t] = s.since_alert; ob[AO_DURATION * A + t] = s.duration;
      ob[AO_SINCE_ATTACK * A + t] = s.since_attack; ob[AO_UNDER_ALERT * A + t] = s.under_alert;
    }
    ob[AO_TOTAL * A] = 0;
    alert_reset_aux(c.W, ax, 0, 1);
    return 0;
  }
  if (done) { ax[AX_ID] &= ~AX_RAN; return 0; }
  raise &= alert_valid_bits(A); att &= alert_valid_bits(A);
  uint64_t already = 0;
  const bool kept = alert_may_truncate(steps_survived, limit);
  for (int t = 0; t < A; ++t) {
    AlertLine s{ob[AO_ACTIVE * A + t], ob[AO_SINCE_ALERT * A + t], ob[AO_DURATION * A + t], ob[AO_SINCE_ATTACK * A + t], ob[AO_UNDER_ALERT * A + t]};
    const bool b = alert_update_line(c.W, (raise >> t) & 1, (att >> t) & 1, att != 0, (ax[AX_ALREADY] >> t) & 1, s);
    already |= (uint64_t)(b ? 1 : 0) << t;
    ob[AO_ACTIVE * A + t] = s.last; ob[AO_SINCE_ALERT * A + t] = s.since_alert; ob[AO_DURATION * A + t] = s.duration;
    ob[AO_SINCE_ATTACK * A + t] = s.since_attack; ob[AO_UNDER_ALERT * A + t] = s.under_alert;
    if (!kept) ob[AO_USED * A + t] = 0;                                // (alertReward.py:156)
  }
  ob[AO_TOTAL * A] += alert_popcount(raise);
  ax[AX_ALREADY] = already;
  alert_ring_update(c.W, ax, att, raise);
  if (kept) ax[AX_ID] |= AX_KEPT;
  return 1;
}

// ... and its post-step: blackout = the lane's done flag AFTER the step (in the engine done = the step failed = has_error).  truncated:
// the step reached the lane's episode limit without failing: the reward is AlertReward's end-of-episode bonus and nothing is scored
// (alertReward.py:179-181).  Returns the reward.
inline float alert_poststep_serial(const AlertCfg& c, int* ob, uint64_t* ax, int blackout, bool truncated = false, float end_bonus = 0.f) {
  if (!(ax[AX_ID] & AX_RAN)) return 0.f;
  if (truncated) return end_bonus;
  const int A = c.A, W = c.W, id = (int)(uint32_t)ax[AX_ID];
  if (ax[AX_ID] & AX_KEPT) for (int t = 0; t < A; ++t) ob[AO_USED * A + t] = 0;
  uint64_t* ts = ax + AX_RINGS;
  const uint64_t* al = ts + (W + 2);
  if (blackout) {
    uint64_t seen, alerted;
    alert_window_first(W + 1, [&](int i, uint64_t& t_, uint64_t& a_) { const int r = alert_window_row(W, id, i); t_ = ts[r]; a_ = al[r]; }, seen, alerted);
    for (int t = 0; t < A; ++t) if ((seen >> t) & 1) ob[AO_USED * A + t] = alert_used_blackout((alerted >> t) & 1);
    return alert_reward_blackout(c, seen, alerted);
  }
  const int iw = alert_window_row(W, id, 0);
  const uint64_t lines = ts[iw], alerts = al[iw];
  for (int t = 0; t < A; ++t) if ((lines >> t) & 1) ob[AO_USED * A + t] = alert_used_no_blackout((alerts >> t) & 1);
  ts[iw] = 0;
  return alert_reward_no_blackout(c, lines, alerts);
}

#ifdef __HIPCC__
// the lanes' rows the kernels touch
struct AlertDev {
  int* obs;                          // [lanes][6 A + 1]
  unsigned long long* aux;           // [lanes][3 + 2 R]
  const unsigned long long* act;     // [lanes] the alert masks of this launch, or null: none
  float* reward;                     // [lanes]
  const unsigned char* done;         // [lanes]
  const int* episode;                // [lanes][2]
  const int* info;                   // the opponent's accepted line(s) of this launch: info[lane * info_lane + area * info_area]
  int info_lane, info_area;
  const int* lines;                  // [A] the alertable line ids (the opponent's list; grouped by area with areas)
  const int* area_of;                // [A] area of every alertable line (zeros without areas)
  const int* ep_limit;               // [lanes] episode limits (gpf_set_episode_limit), or null: off
  float end_bonus;                   // AlertReward.reward_end_episode_bonus
};

constexpr int ALERT_WPB = 4;         // lanes (wavefronts) per block

// The pre-step: one wavefront per lane, ALERT_WPB lanes per block, thread t owns alertable line t, no LDS.  Queued after the opponent's kernel
// and before the step.  Reads done and episode[lane][0] as the opponent does: a lane with no completed step in its episode is the
// env.reset() launch (its state is reset, its alert mask dropped); a done lane is left alone; otherwise the lane's alert mask (bits at or
// above A are dropped) and the attack the opponent just accepted go through alert_update_line and alert_ring_update.
__global__ __launch_bounds__(64 * ALERT_WPB) void alert_prestep_kernel(AlertCfg c, AlertDev d, int n_lanes) {
  const int tid = threadIdx.x & 63;
  const int lane = blockIdx.x * ALERT_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform: the lane's rows are scalar addresses)
  if (lane >= n_lanes) return;                                       // (no block-wide barrier below)
  const int A = c.A;
  const bool mine = tid < A;
  int* ob = d.obs + (size_t)lane * alert_obs_ints(A);
  uint64_t* ax = (uint64_t*)d.aux + (size_t)lane * alert_aux_words(c.W);
  if (d.episode[(size_t)lane * 2] == 0) {
    if (mine) {
      AlertLine s;
      int used;
      alert_reset_line(s, used);
      ob[AO_ACTIVE * A + tid] = s.last; ob[AO_SINCE_ALERT * A + tid] = s.since_alert; ob[AO_DURATION * A + tid] = s.duration;
      ob[AO_SINCE_ATTACK * A + tid] = s.since_attack; ob[AO_UNDER_ALERT * A + tid] = s.under_alert; ob[AO_USED * A + tid] = used;
    }
    if (tid == 0) ob[AO_TOTAL * A] = 0;
    alert_reset_aux(c.W, ax, tid, 64);
    return;
  }
  if (d.done[lane]) { if (tid == 0) ax[AX_ID] &= ~AX_RAN; return; }
  const uint64_t raise = d.act ? (uint64_t)d.act[lane] & alert_valid_bits(A) : 0;
  const bool att_t = mine && d.info[(size_t)lane * d.info_lane + (size_t)d.area_of[tid] * d.info_area] == d.lines[tid];
  const uint64_t att = __ballot(att_t);
  bool already = false;
  const bool kept = d.ep_limit && alert_may_truncate(d.episode[(size_t)lane * 2], d.ep_limit[lane]);
  if (mine) {
    AlertLine s{ob[AO_ACTIVE * A + tid], ob[AO_SINCE_ALERT * A + tid], ob[AO_DURATION * A + tid], ob[AO_SINCE_ATTACK * A + tid], ob[AO_UNDER_ALERT * A + tid]};
    already = alert_update_line(c.W, (raise >> tid) & 1, att_t, att != 0, (ax[AX_ALREADY] >> tid) & 1, s);
    ob[AO_ACTIVE * A + tid] = s.last; ob[AO_SINCE_ALERT * A + tid] = s.since_alert; ob[AO_DURATION * A + tid] = s.duration;
    ob[AO_SINCE_ATTACK * A + tid] = s.since_attack; ob[AO_UNDER_ALERT * A + tid] = s.under_alert;
    if (!kept) ob[AO_USED * A + tid] = 0;                              // (alertReward.py:156)
  }
  const uint64_t already_all = __ballot(already);
  if (tid == 0) {
    ob[AO_TOTAL * A] += alert_popcount(raise);
    ax[AX_ALREADY] = already_all;
    alert_ring_update(c.W, ax, att, raise);
    if (kept) ax[AX_ID] |= AX_KEPT;
  }
}

// The post-step: the same shape, queued after the step (and after topo_poststep_kernel where that runs).  A lane whose pre-step ran reads
// its done flag -- the step failed: the reference's blackout -- and scores one of AlertReward's two branches; in the blackout branch thread
// i holds the two ring words of window position i and the walk takes them in order through __shfl.  Other lanes get reward 0.
__global__ __launch_bounds__(64 * ALERT_WPB) void alert_poststep_kernel(AlertCfg c, AlertDev d, int n_lanes) {
  const int tid = threadIdx.x & 63;
  const int lane = blockIdx.x * ALERT_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (lane >= n_lanes) return;                                       // (no block-wide barrier below)
  const int A = c.A, W = c.W;
  int* ob = d.obs + (size_t)lane * alert_obs_ints(A);
  uint64_t* ax = (uint64_t*)d.aux + (size_t)lane * alert_aux_words(W);
  const uint64_t idw = ax[AX_ID];
  if (!(idw & AX_RAN)) { if (tid == 0) d.reward[lane] = 0.f; return; }
  if (d.ep_limit && episode_truncated(d.episode[(size_t)lane * 2], d.ep_limit[lane], d.done[lane] != 0)) {
    if (tid == 0) d.reward[lane] = d.end_bonus;                        // (alertReward.py:179-181: before _update_state, nothing is scored)
    return;
  }
  if ((idw & AX_KEPT) && tid < A) ob[AO_USED * A + tid] = 0;
  const int id = (int)(uint32_t)idw;
  uint64_t* ts = ax + AX_RINGS;
  const uint64_t* al = ts + (W + 2);
  float r;
  if (d.done[lane]) {
    const int row = alert_window_row(W, id, tid <= W ? tid : 0);
    const unsigned long long my_ts = ts[row], my_al = al[row];
    uint64_t seen, alerted;
    alert_window_first(W + 1, [&](int i, uint64_t& t_, uint64_t& a_) { t_ = __shfl(my_ts, i); a_ = __shfl(my_al, i); }, seen, alerted);
    if ((seen >> tid) & 1) ob[AO_USED * A + tid] = alert_used_blackout((alerted >> tid) & 1);
    r = alert_reward_blackout(c, seen, alerted);
  } else {
    const int iw = alert_window_row(W, id, 0);
    const uint64_t lines = ts[iw], alerts = al[iw];
    if ((lines >> tid) & 1) ob[AO_USED * A + tid] = alert_used_no_blackout((alerts >> tid) & 1);
    if (tid == 0 && lines) ts[iw] = 0;
    r = alert_reward_no_blackout(c, lines, alerts);
  }
  if (tid == 0) d.reward[lane] = r;
}
#endif  // __HIPCC__

}  // namespace gpf
