// gridpf_opponent.hpp -- the opponent of the batched acting path (gpf_set_opponent, include/gridpf.h): what BaseEnv.step does between the
// agent's action and the backend when the environment has an opponent, for every lane of a one-step launch.  Paths relative to the
// reference checkout:
//   the space      OpponentSpace.attack (Opponent/opponentSpace.py:144-249): budget, duration and cooldown automaton -- opp_decide + opp_finish;
//                  OpponentSpace.reset (:96-106) -- opp_reset; the cost is BaseActionBudget (Opponent/baseActionBudget.py:45-57): 1 per attacked line;
//   the opponents  RandomLineOpponent.attack (Opponent/randomLineOpponent.py:94-106), WeightedRandomOpponent.attack
//                  (Opponent/weightedRandomOpponent.py:139-164), GeometricOpponent.attack / sample_attack_times_and_durations
//                  (Opponent/geometricOpponent.py:169-293) -- opp_decide, opp_weight, opp_sample_schedule;
//   the effects    BaseEnv._aux_handle_attack (Environment/baseEnv.py:3148-3170) -- opp_apply: the attacked line is forced out of the lane's
//                  topology row (both ends -1, what a set_line_status -1 item of apply_topo_action does) and its cooldown raised to
//                  max(remaining duration, cooldown), BEFORE the step, whose end-of-step decrement then applies.
// The automaton is separated from its random numbers by a draw protocol: it consumes uniforms u in [0, 1) of a per-lane stream, one per
// event, in event order (opp_draw): from an uploaded table (the parity path) or from Philox4x32-10 (the production path).
//   WeightedRandom draws _next_attack_time        1 + floor(u * attack_period)
//   RandomLine picks among n connected lines      the floor(u * n)-th in attackable-list order
//   WeightedRandom / Geometric pick a line        the first index whose cumulative float64 weight is > u * total
//   Geometric samples its schedule (Philox only)  max(1, ceil(log1p(-u) / log1p(-p))), waiting time and duration alternating
// With areas set (gpf_set_opponent_areas) the lane plays GeometricOpponentMultiArea (Opponent/geometricOpponentMultiArea.py:88-149): one
// Geometric sub-opponent per area, each with its slice of the attackable list, its schedule and a row of OPP_AREA_STATE_INTS ints; all
// areas draw from the lane's ONE stream, in area order (opp_area_*, opponent_area_prestep_kernel).
// Three parts: the scalar rules (plain C++, the ONE statement of each rule, run by the kernel on one thread per lane and by the host
// emulator of tests/native/), the line choice (opp_weight + the threshold rule, summed by a wavefront scan on the device and by a plain
// loop in the emulator), and the kernels, for the one unit that defines GPF_OPPONENT_KERNEL (gridpf_capi_opp.hip; gridpf_cursor.hpp
// includes this header for Philox alone).  Without hipcc only the first two exist: the header then needs no HIP header.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GPF_OPP_HD __host__ __device__
#else
#define GPF_OPP_HD
#endif

#include <math.h>
#include <stdint.h>

namespace gpf {

// kinds and draw sources (= GPF_OPP_* of include/gridpf.h)
constexpr int OPP_NONE = 0, OPP_RANDOM_LINE = 1, OPP_WEIGHTED_RANDOM = 2, OPP_GEOMETRIC = 3;
constexpr int OPP_DRAWS_TABLE = 0, OPP_DRAWS_PHILOX = 1;
// per-lane state: the budget (double) + OPP_STATE_INTS ints (= GPF_OPP_S_* of include/gridpf.h)
constexpr int OPP_STATE_INTS = 14;
constexpr int OS_F32 = 0;            // the budget is still a numpy.float32 (no attack has been paid for since the reset)
constexpr int OS_DURATION = 1;       // current_attack_duration
constexpr int OS_COOLDOWN = 2;       // current_attack_cooldown
constexpr int OS_LINE = 3;           // last_attack: the attacked line, -1 for None
constexpr int OS_PREV_FAILS = 4;     // previous_fails
constexpr int OS_NEXT_TIME = 5;      // _next_attack_time, OPP_TIME_NONE for None (the reference counts it below zero after a refused attack)
constexpr int OS_COUNTER = 6;        // Geometric: _attack_counter
constexpr int OS_N_SCHED = 7;        // Geometric: _number_of_attacks (entries of the lane's schedule)
constexpr int OS_CURSOR = 8;         // draws consumed (table: since the upload; Philox: in this episode)
constexpr int OS_EPISODE = 9;        // resets of the lane's opponent so far (the Philox counter's episode word)
constexpr int OS_FLAGS = 10;         // sticky OPP_FLAG_* bits
constexpr int OS_INFO_LINE = 11;     // info["opponent_attack_line"] of the last launch (-1: none)
constexpr int OS_INFO_DURATION = 12; // info["opponent_attack_duration"] of the last launch
constexpr int OPP_TIME_NONE = INT32_MIN;
constexpr int OPP_FLAG_DRAWS_EXHAUSTED = 1, OPP_FLAG_SCHEDULE_CAPPED = 2;
// per (lane, area) state with areas set (= GPF_OPP_AS_* of include/gridpf.h); the lane's row then keeps OS_F32, OS_DURATION, OS_COOLDOWN,
// OS_PREV_FAILS, OS_CURSOR, OS_EPISODE, OS_FLAGS; OS_LINE / OS_INFO_LINE hold the accepted line of the lowest attacking area, OS_INFO_DURATION 1 or 0
constexpr int OPP_MAX_AREAS = 16;
constexpr int OPP_AREA_STATE_INTS = 8;
constexpr int OAS_COUNTER = 0;        // _new_attack_time_counters[a] (-1: the area is free)
constexpr int OAS_LINE = 1;           // _previous_attacks[a]: the line, -1 for None
constexpr int OAS_NEXT_TIME = 2;      // the sub-opponent's _next_attack_time
constexpr int OAS_ATTACK_COUNTER = 3; //                    _attack_counter
constexpr int OAS_N_SCHED = 4;        //                    _number_of_attacks
constexpr int OAS_INFO_LINE = 5;      // the area's line in the ACCEPTED attack of the last launch (-1: none)

struct OppCfg {
  int kind, n_att;
  const int* lines;          // [n_att] attackable line ids, in the order of the reference's lines_attacked
  const double* norm;        // [n_att] rho_normalization (ones when the caller gave none)
  int attack_period;         // WeightedRandom
  double hazard, recovery;   // Geometric: _attack_hazard_rate, _recovery_rate
  int min_dur;               //            _recovery_minimum_duration
  double log_ratio;          //            log(pmax_pmin_ratio)
  int episode_len;           //            _episode_max_time
  float init_budget, budget_per_ts;
  int max_duration, attack_cooldown;
  int source;
  uint32_t seed_lo, seed_hi;
  int lane_base, sched_cap, n_draw;
};

// one lane's rows
struct OppLane {
  double* budget;            // [1]
  int* st;                   // [OPP_STATE_INTS]
  const double* draws;       // [n_draw] (table source)
  int* sched;                // [sched_cap][2] {waiting time, duration} (Geometric)
  int global_lane;           // lane + lane_base
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter ctr[4], key[2] -> ctr
GPF_OPP_HD inline void philox4x32_10(uint32_t ctr[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * ctr[0], p1 = (uint64_t)0xCD9E8D57u * ctr[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ ctr[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ ctr[3] ^ k1, n3 = (uint32_t)p0;
    ctr[0] = n0; ctr[1] = n1; ctr[2] = n2; ctr[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// the uniform of a Philox output: 53 bits of its first two words
GPF_OPP_HD inline double opp_philox_u(uint32_t x0, uint32_t x1) { return ((double)(x0 >> 5) * 67108864.0 + (double)(x1 >> 6)) * (1.0 / 9007199254740992.0); }

// the next uniform of the lane's stream; false: the table is used up (sticky flag) -- the caller does not attack
GPF_OPP_HD inline bool opp_draw(const OppCfg& c, const OppLane& L, double& u) {
  int* s = L.st;
  if (c.source == OPP_DRAWS_PHILOX) {
    uint32_t x[4] = {(uint32_t)s[OS_CURSOR], (uint32_t)s[OS_EPISODE], (uint32_t)L.global_lane, 0u};
    philox4x32_10(x, c.seed_lo, c.seed_hi);
    u = opp_philox_u(x[0], x[1]);
    ++s[OS_CURSOR];
    return true;
  }
  if (!L.draws || s[OS_CURSOR] < 0 || s[OS_CURSOR] >= c.n_draw) { s[OS_FLAGS] |= OPP_FLAG_DRAWS_EXHAUSTED; return false; }
  u = L.draws[s[OS_CURSOR]++];
  return true;
}

// the inversion RandomState.geometric uses for p < 1/3, here for every p in (0, 1]
GPF_OPP_HD inline int opp_geometric(double u, double p) {
  const double x = ceil(log1p(-u) / log1p(-p));
  return x >= 1.0e9 ? 1000000000 : (x > 1.0 ? (int)x : 1);
}

// GeometricOpponent.sample_attack_times_and_durations (geometricOpponent.py:169-197) from the lane's own stream, up to sched_cap attacks:
// when the capacity is reached the schedule ends there (sticky OPP_FLAG_SCHEDULE_CAPPED)
GPF_OPP_HD inline void opp_sample_schedule_into(const OppCfg& c, const OppLane& L, int* sched, int* n_sched) {
  int n = 0;
  long long t = 0;
  while (t < c.episode_len) {
    if (n >= c.sched_cap) { L.st[OS_FLAGS] |= OPP_FLAG_SCHEDULE_CAPPED; break; }
    double u;
    if (!opp_draw(c, L, u)) break;
    const int wait = opp_geometric(u, c.hazard);
    t += wait;
    if (t < c.episode_len) {
      if (!opp_draw(c, L, u)) break;
      const int dur = c.min_dur + opp_geometric(u, c.recovery);
      sched[2 * n] = wait; sched[2 * n + 1] = dur;
      ++n;
      t += dur;
    }
  }
  *n_sched = n;
}
GPF_OPP_HD inline void opp_sample_schedule(const OppCfg& c, const OppLane& L) { opp_sample_schedule_into(c, L, L.sched, &L.st[OS_N_SCHED]); }

// OpponentSpace.reset (opponentSpace.py:96-106) + the opponent's reset: what env.reset() leaves.  The table cursor and an uploaded schedule
// stay (the recorded draws of a run go on across its resets); the Philox stream starts its next episode.
GPF_OPP_HD inline void opp_reset_space(const OppCfg& c, const OppLane& L) {
  int* s = L.st;
  *L.budget = (double)c.init_budget; s[OS_F32] = 1;
  s[OS_DURATION] = 0; s[OS_COOLDOWN] = c.attack_cooldown; s[OS_LINE] = -1; s[OS_PREV_FAILS] = 0;
  s[OS_NEXT_TIME] = OPP_TIME_NONE; s[OS_COUNTER] = 0;
  s[OS_EPISODE] += 1;
  s[OS_INFO_LINE] = -1; s[OS_INFO_DURATION] = 0;
  if (c.source == OPP_DRAWS_PHILOX) s[OS_CURSOR] = 0;
}
GPF_OPP_HD inline void opp_reset(const OppCfg& c, const OppLane& L) {
  opp_reset_space(c, L);
  if (c.source == OPP_DRAWS_PHILOX && c.kind == OPP_GEOMETRIC) opp_sample_schedule(c, L);
}

// what the scalar part asks of the line choice
constexpr int OPP_SEL_NONE = 0;      // no choice: `line` is the answer (-1: no attack)
constexpr int OPP_SEL_KTH = 1;       // the first index at which the count of connected lines exceeds thr (RandomLine)
constexpr int OPP_SEL_CDF = 2;       // the first index at which the cumulative weight exceeds u * total
struct OppAsk { int asked, sel, line, duration; double u; };    // duration -1: None

// OpponentSpace.attack's update of its variables (opponentSpace.py:183-185) on a budget and a lane row
GPF_OPP_HD inline void opp_space_tick(const OppCfg& c, double* budget, int* s) {
  // budget += budget_per_timestep: float32 + float32 while the budget is one (the double sum rounded once), float64 + float32 afterwards
  const double sum = *budget + (double)c.budget_per_ts;
  *budget = s[OS_F32] ? (double)(float)sum : sum;
  s[OS_DURATION] = s[OS_DURATION] > 1 ? s[OS_DURATION] - 1 : 0;
  s[OS_COOLDOWN] = s[OS_COOLDOWN] > 1 ? s[OS_COOLDOWN] - 1 : 0;
}

// GeometricOpponent.attack up to its draw of a line (geometricOpponent.py:234-293) on one opponent's _next_attack_time, _attack_counter
// and schedule of n entries (the lane's own, or an area's); c.lines / c.n_att are that opponent's attackable list
GPF_OPP_HD inline void opp_geometric_attack(const OppCfg& c, const OppLane& L, int prev_fails, int* next_time, int* counter, int n, const int* sched,
                                            int n_conn, OppAsk& a) {
  const int k = *counter;
  if (k >= n) return;
  if (prev_fails) *next_time = sched[2 * k] + sched[2 * (k > 0 ? k - 1 : n - 1) + 1];   // (index -1 of the reference's array: its last entry)
  if (*next_time == OPP_TIME_NONE) *next_time = 1 + sched[2 * k];
  const int dur = sched[2 * k + 1];
  *next_time -= 1;
  if (*next_time > 0) return;
  *counter = k + 1;                                                  // the attack is launched
  if (n_conn != c.n_att) return;                                     // `~status.all()`: given up when ANY attackable line is out
  if (c.n_att == 1) { a.line = c.lines[0]; a.duration = dur; return; }
  if (!opp_draw(c, L, a.u)) return;
  a.sel = OPP_SEL_CDF; a.duration = dur;
}

// OpponentSpace.attack up to the opponent's choice (opponentSpace.py:183-201) and the opponent's attack() up to its draw of a line.
// n_conn: connected attackable lines in the observation; w_pos: WeightedRandom's sum of weights is > 0.
GPF_OPP_HD inline void opp_decide(const OppCfg& c, const OppLane& L, int n_conn, bool w_pos, OppAsk& a) {
  int* s = L.st;
  opp_space_tick(c, L.budget, s);
  a.asked = 0; a.sel = OPP_SEL_NONE; a.line = -1; a.duration = -1; a.u = 0.0;
  if (s[OS_DURATION] > 0) { a.line = s[OS_LINE]; return; }           // the last attack continues
  if (s[OS_COOLDOWN] > c.attack_cooldown) return;                    // minimum time between two attacks not met
  a.asked = 1;
  if (c.kind == OPP_RANDOM_LINE) {
    a.duration = 0;
    if (n_conn == 0 || !opp_draw(c, L, a.u)) return;
    a.u = floor(a.u * n_conn); a.sel = OPP_SEL_KTH; a.duration = -1;
  } else if (c.kind == OPP_WEIGHTED_RANDOM) {
    a.duration = 0;
    if (s[OS_NEXT_TIME] == OPP_TIME_NONE) {
      double u;
      if (!opp_draw(c, L, u)) return;
      s[OS_NEXT_TIME] = 1 + (int)floor(u * c.attack_period);
    }
    s[OS_NEXT_TIME] -= 1;
    if (s[OS_NEXT_TIME] > 0 || n_conn == 0 || !w_pos || !opp_draw(c, L, a.u)) return;
    a.sel = OPP_SEL_CDF; a.duration = -1;
  } else if (c.kind == OPP_GEOMETRIC) {
    opp_geometric_attack(c, L, s[OS_PREV_FAILS], &s[OS_NEXT_TIME], &s[OS_COUNTER], s[OS_N_SCHED], L.sched, n_conn, a);
  }
}

// the weight of entry idx of the attackable list in the choice `sel` (0: cannot be chosen)
GPF_OPP_HD inline double opp_weight(const OppCfg& c, int sel, const float* rho, const unsigned char* status, int idx) {
  const int l = c.lines[idx];
  if (!status[l]) return 0.0;
  if (sel == OPP_SEL_KTH) return 1.0;
  if (c.kind == OPP_WEIGHTED_RANDOM) return (double)rho[l] / c.norm[idx];
  // Geometric: exp(log(pmax_pmin_ratio) / (n - 1) * rank), rank(i) = number of j with rho_j < rho_i, or rho_j == rho_i and j < i
  const float r = rho[l];
  int rank = 0;
  for (int j = 0; j < c.n_att; ++j) { const float rj = rho[c.lines[j]]; rank += (rj < r || (rj == r && j < idx)) ? 1 : 0; }
  return exp(c.log_ratio / (double)(c.n_att - 1) * (double)rank);
}

// the threshold a cumulative weight must exceed (RandomState.choice: cdf.searchsorted(u, side="right") on the normalised cumulative sum)
GPF_OPP_HD inline double opp_threshold(const OppAsk& a, double total) { return a.sel == OPP_SEL_KTH ? a.u : a.u * total; }

// OpponentSpace.attack from the opponent's answer on (opponentSpace.py:202-249): `line` / `duration` are the answer (-1: None)
GPF_OPP_HD inline void opp_finish(const OppCfg& c, const OppLane& L, int asked, int line, int duration) {
  int* s = L.st;
  if (asked) {
    if (duration < 0) duration = c.max_duration;
    int fails = 0;
    if (duration > c.max_duration) { line = -1; fails = 1; }
    if ((double)duration * (line >= 0 ? 1.0 : 0.0) > *L.budget) { line = -1; fails = 1; }
    if (line >= 0) { s[OS_DURATION] = duration; s[OS_COOLDOWN] += c.attack_cooldown; }
    s[OS_PREV_FAILS] = fails;
  } else {
    if (c.kind != OPP_RANDOM_LINE) s[OS_NEXT_TIME] = OPP_TIME_NONE;   // tell_attack_continues
    s[OS_PREV_FAILS] = 0;
  }
  if (line >= 0) { *L.budget -= 1.0; s[OS_F32] = 0; }                 // the integer cost of an attack widens the budget to float64
  s[OS_LINE] = line;
  s[OS_INFO_LINE] = line;
  s[OS_INFO_DURATION] = line >= 0 ? s[OS_DURATION] : 0;
}

// BaseEnv._aux_handle_attack (baseEnv.py:3158-3169) on the lane's topology row and line cooldowns
GPF_OPP_HD inline void opp_apply(const OppLane& L, int* topo_row, int* cooldown_row, const int* or_pos, const int* ex_pos) {
  const int line = L.st[OS_INFO_LINE], dur = L.st[OS_INFO_DURATION];
  if (line < 0) return;
  topo_row[or_pos[line]] = -1; topo_row[ex_pos[line]] = -1;
  if (cooldown_row[line] < dur) cooldown_row[line] = dur;
}

// One lane's pre-step with plain loops (the host emulator; the kernel below runs the same rules with the sums on a wavefront).
// steps_survived / done: the lane's episode[0] and done flag.  Returns 1 when the lane's opponent ran (neither reset nor left alone).
inline int opp_prestep_serial(const OppCfg& c, const OppLane& L, int steps_survived, int done, const float* rho, const unsigned char* status,
                              int* topo_row, int* cooldown_row, const int* or_pos, const int* ex_pos) {
  if (steps_survived == 0) { opp_reset(c, L); return 0; }
  if (done) return 0;
  int n_conn = 0;
  for (int i = 0; i < c.n_att; ++i) n_conn += status[c.lines[i]] ? 1 : 0;
  double total = 0.0;
  if (c.kind == OPP_WEIGHTED_RANDOM) for (int i = 0; i < c.n_att; ++i) total += opp_weight(c, OPP_SEL_CDF, rho, status, i);
  OppAsk a;
  opp_decide(c, L, n_conn, total > 0.0, a);
  if (a.sel != OPP_SEL_NONE) {
    if (a.sel == OPP_SEL_CDF && c.kind == OPP_GEOMETRIC) for (int i = 0; i < c.n_att; ++i) total += opp_weight(c, a.sel, rho, status, i);
    const double thr = opp_threshold(a, total);
    double cum = 0.0;
    int last = -1;
    a.line = -1;
    for (int i = 0; i < c.n_att && a.line < 0; ++i) {
      const double w = opp_weight(c, a.sel, rho, status, i);
      cum += w;
      if (w > 0.0) last = i;
      if (cum > thr) a.line = c.lines[i];
    }
    if (a.line < 0 && last >= 0) a.line = c.lines[last];              // (u * total rounded up to the total: the last line that can be chosen)
  }
  opp_finish(c, L, a.asked, a.line, a.duration);
  opp_apply(L, topo_row, cooldown_row, or_pos, ex_pos);
  return 1;
}

// ---- GeometricOpponentMultiArea (geometricOpponentMultiArea.py:88-149) under OpponentSpace.attack ------------------------------------
// the areas of a launch: area a attacks lines[offset[a] .. offset[a] + count[a]) (its entries of the descriptor's list, in that order)
struct OppAreas {
  int n_area;
  const int* lines;          // [n_att] the attackable lines grouped by area
  const int* offset;         // [n_area]
  const int* count;          // [n_area]
};
// one lane's area rows
struct OppAreaLane {
  int* st;                   // [n_area][OPP_AREA_STATE_INTS]
  int* sched;                // [n_area][sched_cap][2]
};

// area a's view of the configuration: the sub-opponent's attackable list
GPF_OPP_HD inline OppCfg opp_area_cfg(const OppCfg& c, const OppAreas& A, int a) {
  OppCfg ca = c;
  ca.lines = A.lines + A.offset[a]; ca.n_att = A.count[a];
  return ca;
}

// GeometricOpponentMultiArea.reset (:88-92) under OpponentSpace.reset: counters to -1, every sub-opponent reset (with the Philox source the
// areas sample their schedules in area order from the lane's stream); _previous_attacks (OAS_LINE) stays as it is, as in the reference
GPF_OPP_HD inline void opp_area_reset(const OppCfg& c, const OppLane& L, const OppAreas& A, const OppAreaLane& R) {
  opp_reset_space(c, L);
  for (int a = 0; a < A.n_area; ++a) {
    int* r = R.st + a * OPP_AREA_STATE_INTS;
    r[OAS_COUNTER] = -1; r[OAS_NEXT_TIME] = OPP_TIME_NONE; r[OAS_ATTACK_COUNTER] = 0; r[OAS_INFO_LINE] = -1;
    if (c.source == OPP_DRAWS_PHILOX) opp_sample_schedule_into(c, L, R.sched + (size_t)a * c.sched_cap * 2, &r[OAS_N_SCHED]);
  }
}

// OpponentSpace.attack up to its call of the opponent; returns 1 when the opponent is asked.  The returned duration of the multi-area
// opponent is always 1, so the space asks at every step; the other two branches are the reference's `tell_attack_continues` of the
// multi-area opponent ("I should not get there !"): here no area moves and nothing is attacked.
GPF_OPP_HD inline int opp_area_begin(const OppCfg& c, const OppLane& L) {
  opp_space_tick(c, L.budget, L.st);
  return L.st[OS_DURATION] == 0 && L.st[OS_COOLDOWN] <= c.attack_cooldown ? 1 : 0;
}

// one area's turn of GeometricOpponentMultiArea.attack (:127-148) up to its sub-opponent's draw of a line; ca: opp_area_cfg.
// a.asked: the area was free and its sub-opponent was called (else a.line is the line it goes on holding)
GPF_OPP_HD inline void opp_area_decide(const OppCfg& ca, const OppLane& L, int* r, const int* sched, int n_conn, OppAsk& a) {
  a.asked = 0; a.sel = OPP_SEL_NONE; a.line = -1; a.duration = -1; a.u = 0.0;
  r[OAS_COUNTER] = r[OAS_COUNTER] >= 0 ? r[OAS_COUNTER] - 1 : -1;
  if (r[OAS_COUNTER] >= 0) { r[OAS_NEXT_TIME] = OPP_TIME_NONE; a.line = r[OAS_LINE]; return; }   // the sub-opponent's tell_attack_continues
  a.asked = 1;
  opp_geometric_attack(ca, L, L.st[OS_PREV_FAILS], &r[OAS_NEXT_TIME], &r[OAS_ATTACK_COUNTER], r[OAS_N_SCHED], sched, n_conn, a);
}

// ... and from the sub-opponent's answer on: an attack of duration d books the area for d more steps (the line is held d + 1 steps)
GPF_OPP_HD inline void opp_area_book(int* r, const OppAsk& a) {
  if (!a.asked) return;
  if (a.line >= 0) r[OAS_COUNTER] = a.duration;
  r[OAS_LINE] = a.line;
}

// OpponentSpace.attack from the multi-area opponent's answer on (opponentSpace.py:202-249): the answer is the union of the areas' lines with
// duration 1, its cost one unit per line (baseActionBudget.py:55-56); a refused attack leaves the areas' bookings as they are
GPF_OPP_HD inline void opp_area_finish(const OppCfg& c, const OppLane& L, const OppAreas& A, const OppAreaLane& R, int asked) {
  int* s = L.st;
  int n = 0, first = -1;
  if (asked) {
    for (int a = 0; a < A.n_area; ++a) {
      const int l = R.st[a * OPP_AREA_STATE_INTS + OAS_LINE];
      if (l >= 0) { if (first < 0) first = l; ++n; }
    }
    int fails = 0;
    if (1 > c.max_duration) { n = 0; fails = 1; }
    if ((double)n > *L.budget) { n = 0; fails = 1; }
    if (n > 0) { s[OS_DURATION] = 1; s[OS_COOLDOWN] += c.attack_cooldown; }
    s[OS_PREV_FAILS] = fails;
  } else {
    s[OS_PREV_FAILS] = 0;
  }
  if (n > 0) { *L.budget -= (double)n; s[OS_F32] = 0; }               // the integer cost of an attack widens the budget to float64
  for (int a = 0; a < A.n_area; ++a) {
    int* r = R.st + a * OPP_AREA_STATE_INTS;
    r[OAS_INFO_LINE] = n > 0 ? r[OAS_LINE] : -1;
  }
  if (n == 0) first = -1;
  s[OS_LINE] = first;
  s[OS_INFO_LINE] = first;
  s[OS_INFO_DURATION] = n > 0 ? 1 : 0;
}

// BaseEnv._aux_handle_attack (baseEnv.py:3158-3169) for every line of the accepted union: out of the topology row, cooldown max(1, cooldown)
GPF_OPP_HD inline void opp_area_apply(const OppAreas& A, const OppAreaLane& R, int* topo_row, int* cooldown_row, const int* or_pos, const int* ex_pos) {
  for (int a = 0; a < A.n_area; ++a) {
    const int line = R.st[a * OPP_AREA_STATE_INTS + OAS_INFO_LINE];
    if (line < 0) continue;
    topo_row[or_pos[line]] = -1; topo_row[ex_pos[line]] = -1;
    if (cooldown_row[line] < 1) cooldown_row[line] = 1;
  }
}

// One lane's pre-step with areas, with plain loops (the host emulator; opponent_area_prestep_kernel runs the same rules with the sums on a
// wavefront).  Returns 1 when the lane's opponent ran.
inline int opp_area_prestep_serial(const OppCfg& c, const OppLane& L, const OppAreas& A, const OppAreaLane& R, int steps_survived, int done,
                                   const float* rho, const unsigned char* status, int* topo_row, int* cooldown_row, const int* or_pos,
                                   const int* ex_pos) {
  if (steps_survived == 0) { opp_area_reset(c, L, A, R); return 0; }
  if (done) return 0;
  const int asked = opp_area_begin(c, L);
  for (int ar = 0; asked && ar < A.n_area; ++ar) {
    const OppCfg ca = opp_area_cfg(c, A, ar);
    int* r = R.st + ar * OPP_AREA_STATE_INTS;
    int n_conn = 0;
    for (int i = 0; i < ca.n_att; ++i) n_conn += status[ca.lines[i]] ? 1 : 0;
    OppAsk a;
    opp_area_decide(ca, L, r, R.sched + (size_t)ar * c.sched_cap * 2, n_conn, a);
    if (a.sel != OPP_SEL_NONE) {
      double total = 0.0;
      for (int i = 0; i < ca.n_att; ++i) total += opp_weight(ca, a.sel, rho, status, i);
      const double thr = opp_threshold(a, total);
      double cum = 0.0;
      int last = -1;
      a.line = -1;
      for (int i = 0; i < ca.n_att && a.line < 0; ++i) {
        const double w = opp_weight(ca, a.sel, rho, status, i);
        cum += w;
        if (w > 0.0) last = i;
        if (cum > thr) a.line = ca.lines[i];
      }
      if (a.line < 0 && last >= 0) a.line = ca.lines[last];
    }
    opp_area_book(r, a);
  }
  opp_area_finish(c, L, A, R, asked);
  opp_area_apply(A, R, topo_row, cooldown_row, or_pos, ex_pos);
  return 1;
}


#if defined(__HIPCC__) && defined(GPF_OPPONENT_KERNEL)      // (the one unit that launches the kernels: gridpf_capi_opp.hip)
// the lanes' rows the kernel touches
struct OppDev {
  double* budget; int* state; const double* draws; int* sched;
  const float* rho; const unsigned char* line_status; const unsigned char* done; const int* episode;
  int* topo; int* cooldown; const int* or_pos; const int* ex_pos;
  int n_line, dim_topo;
};

constexpr int OPP_WPB = 4;           // lanes (wavefronts) per block

// cumulative weights of the attackable list on one wavefront: threads stride the list in chunks of 64, an inclusive scan over __shfl_up
// steps inside a chunk, the carry across chunks.  Returns the total; with `find`, *found = first index whose cumulative weight exceeds
// thr (else the last index with a positive weight, -1: none).
__device__ inline double opp_wave_scan(const OppCfg& c, int sel, const float* rho, const unsigned char* status, int tid, bool find, double thr,
                                       int* found) {
  double carry = 0.0;
  int hit = -1, last = -1;
  for (int c0 = 0; c0 < c.n_att; c0 += 64) {
    const int idx = c0 + tid;
    const double w = idx < c.n_att ? opp_weight(c, sel, rho, status, idx) : 0.0;
    double cum = w;
    for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(cum, o); if (tid >= o) cum += t; }
    cum += carry;
    carry = __shfl(cum, 63);
    if (find) {
      const unsigned long long pos = __ballot(w > 0.0), over = __ballot(cum > thr);
      if (pos) last = c0 + 63 - __clzll(pos);
      if (over) { hit = c0 + __ffsll(over) - 1; break; }              // (ballots are wave-uniform: so is the exit)
    }
  }
  if (find) *found = hit >= 0 ? hit : last;
  return carry;
}

// The opponent's pre-step: one wavefront per lane, OPP_WPB lanes per block, no LDS.  Launched on the engine's stream after
// topo_prestep_kernel and before the step, so that the attack wins over the agent's action.  Reads the lane's rho / line_status RESULT rows
// of its last step (the observation at time t), done and episode[lane][0]; a lane with no completed step in its episode is the reference's
// `observation is None` call (its state is reset, nothing else); a done lane is left alone.  Writes the lane's opponent state, both ends
// of the attacked line in its topology row and that line's cooldown.
__global__ __launch_bounds__(64 * OPP_WPB) void opponent_prestep_kernel(OppCfg c, OppDev d, int n_lanes) {
  const int tid = threadIdx.x & 63;
  const int lane = blockIdx.x * OPP_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform: the lane's rows are scalar addresses)
  if (lane >= n_lanes) return;                                       // (no block-wide barrier below)
  OppLane L;
  L.budget = d.budget + lane; L.st = d.state + (size_t)lane * OPP_STATE_INTS;
  L.draws = d.draws ? d.draws + (size_t)lane * c.n_draw : nullptr;
  L.sched = d.sched ? d.sched + (size_t)lane * c.sched_cap * 2 : nullptr;
  L.global_lane = lane + c.lane_base;
  if (d.episode[(size_t)lane * 2] == 0) { if (tid == 0) opp_reset(c, L); return; }
  if (d.done[lane]) return;
  const float* rho = d.rho + (size_t)lane * d.n_line;
  const unsigned char* status = d.line_status + (size_t)lane * d.n_line;
  int n_conn = 0;
  for (int c0 = 0; c0 < c.n_att; c0 += 64) {
    const int idx = c0 + tid;
    n_conn += __popcll(__ballot(idx < c.n_att && status[c.lines[idx]] != 0));
  }
  double total = 0.0;
  if (c.kind == OPP_WEIGHTED_RANDOM) total = opp_wave_scan(c, OPP_SEL_CDF, rho, status, tid, false, 0.0, nullptr);
  OppAsk a;
  a.asked = 0; a.sel = OPP_SEL_NONE; a.line = -1; a.duration = -1; a.u = 0.0;
  if (tid == 0) opp_decide(c, L, n_conn, total > 0.0, a);
  a.sel = __shfl(a.sel, 0); a.u = __shfl(a.u, 0);
  if (a.sel != OPP_SEL_NONE) {
    if (a.sel == OPP_SEL_CDF && c.kind == OPP_GEOMETRIC) total = opp_wave_scan(c, a.sel, rho, status, tid, false, 0.0, nullptr);
    int idx = -1;
    opp_wave_scan(c, a.sel, rho, status, tid, true, opp_threshold(a, total), &idx);
    a.line = idx >= 0 ? c.lines[idx] : -1;
  }
  if (tid == 0) {
    opp_finish(c, L, a.asked, a.line, a.duration);
    opp_apply(L, d.topo + (size_t)lane * d.dim_topo, d.cooldown + (size_t)lane * d.n_line, d.or_pos, d.ex_pos);
  }
}
// the lanes' area rows
struct OppAreaDev { int* state; int* sched; };

// The pre-step with areas: the same shape (one wavefront per lane, OPP_WPB lanes per block, no LDS, one launch per step whatever the number
// of areas).  The wavefront walks the areas in a wave-uniform loop, in area order -- the order in which they consume the lane's stream:
// count and scan on the area's slice of the attackable list, the scalar rules on thread 0; thread 0 then applies the space's combination
// and forces every accepted line out.  Reads and writes what opponent_prestep_kernel does, plus the lane's area rows.
__global__ __launch_bounds__(64 * OPP_WPB) void opponent_area_prestep_kernel(OppCfg c, OppDev d, OppAreas A, OppAreaDev ad, int n_lanes) {
  const int tid = threadIdx.x & 63;
  const int lane = blockIdx.x * OPP_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (lane >= n_lanes) return;                                       // (no block-wide barrier below)
  OppLane L;
  L.budget = d.budget + lane; L.st = d.state + (size_t)lane * OPP_STATE_INTS;
  L.draws = d.draws ? d.draws + (size_t)lane * c.n_draw : nullptr;
  L.sched = nullptr;
  L.global_lane = lane + c.lane_base;
  OppAreaLane R;
  R.st = ad.state + (size_t)lane * A.n_area * OPP_AREA_STATE_INTS;
  R.sched = ad.sched + (size_t)lane * A.n_area * c.sched_cap * 2;
  if (d.episode[(size_t)lane * 2] == 0) { if (tid == 0) opp_area_reset(c, L, A, R); return; }
  if (d.done[lane]) return;
  const float* rho = d.rho + (size_t)lane * d.n_line;
  const unsigned char* status = d.line_status + (size_t)lane * d.n_line;
  int asked = 0;
  if (tid == 0) asked = opp_area_begin(c, L);
  asked = __shfl(asked, 0);
  if (asked)
    for (int ar = 0; ar < A.n_area; ++ar) {
      const OppCfg ca = opp_area_cfg(c, A, ar);
      int* r = R.st + ar * OPP_AREA_STATE_INTS;
      int n_conn = 0;
      for (int c0 = 0; c0 < ca.n_att; c0 += 64) {
        const int idx = c0 + tid;
        n_conn += __popcll(__ballot(idx < ca.n_att && status[ca.lines[idx]] != 0));
      }
      OppAsk a;
      a.asked = 0; a.sel = OPP_SEL_NONE; a.line = -1; a.duration = -1; a.u = 0.0;
      if (tid == 0) opp_area_decide(ca, L, r, R.sched + (size_t)ar * c.sched_cap * 2, n_conn, a);
      a.sel = __shfl(a.sel, 0); a.u = __shfl(a.u, 0);
      if (a.sel != OPP_SEL_NONE) {
        const double total = opp_wave_scan(ca, a.sel, rho, status, tid, false, 0.0, nullptr);
        int idx = -1;
        opp_wave_scan(ca, a.sel, rho, status, tid, true, opp_threshold(a, total), &idx);
        a.line = idx >= 0 ? ca.lines[idx] : -1;
      }
      if (tid == 0) opp_area_book(r, a);
    }
  if (tid == 0) {
    opp_area_finish(c, L, A, R, asked);
    opp_area_apply(A, R, d.topo + (size_t)lane * d.dim_topo, d.cooldown + (size_t)lane * d.n_line, d.or_pos, d.ex_pos);
  }
}
#endif  // __HIPCC__ && GPF_OPPONENT_KERNEL

}  // namespace gpf
