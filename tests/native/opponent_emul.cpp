// Host emulator of the opponent's pre-step (grid2op_amd/csrc/gridpf_opponent.hpp), test infrastructure compiled with g++: the SAME scalar
// rules, weights and threshold rule as the library, with the kernel's wavefront sums done by plain loops (opp_prestep_serial).
//   g++ -O2 -std=c++17 -fPIC -shared opponent_emul.cpp -o libopponentemul.so          (tests/opponent_ref.py, ctypes)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DOPPONENT_EMUL_MAIN opponent_emul.cpp -o opponent_emul_san
// The second is a stand-alone program: every kind of opponent with both draw sources on a ring grid with more than 64 attackable lines,
// random line outages and state rows at the edges of what gpf_set_opponent_state accepts, checked for the invariants of the automaton.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_opponent.hpp"

struct opp_emul_cfg {
  int32_t kind, n_att; const int32_t* lines; const double* norm; int32_t attack_period; double hazard, recovery; int32_t min_dur; double ratio;
  int32_t episode_len; float init_budget, budget_per_ts; int32_t max_duration, attack_cooldown, source; uint32_t seed_lo, seed_hi;
  int32_t lane_base, sched_cap, n_draw;
};

static gpf::OppCfg to_cfg(const opp_emul_cfg& e) {
  gpf::OppCfg c{};
  c.kind = e.kind; c.n_att = e.n_att; c.lines = e.lines; c.norm = e.norm; c.attack_period = e.attack_period; c.hazard = e.hazard;
  c.recovery = e.recovery; c.min_dur = e.min_dur; c.log_ratio = e.kind == gpf::OPP_GEOMETRIC ? std::log(e.ratio) : 0.0; c.episode_len = e.episode_len;
  c.init_budget = e.init_budget; c.budget_per_ts = e.budget_per_ts; c.max_duration = e.max_duration; c.attack_cooldown = e.attack_cooldown;
  c.source = e.source; c.seed_lo = e.seed_lo; c.seed_hi = e.seed_hi; c.lane_base = e.lane_base; c.sched_cap = e.sched_cap; c.n_draw = e.n_draw;
  return c;
}

extern "C" void opp_emul_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out, double* u) {
  uint32_t x[4] = {ctr[0], ctr[1], ctr[2], ctr[3]};
  gpf::philox4x32_10(x, key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = x[i];
  *u = gpf::opp_philox_u(x[0], x[1]);
}

// one launch of opponent_prestep_kernel on n_lanes lanes of host memory (rows laid out as the engine's)
extern "C" int opp_emul_prestep(const opp_emul_cfg* e, int n_lanes, int n_line, int dim_topo, const int* or_pos, const int* ex_pos, double* budget,
                                int* state, const double* draws, int* sched, const int* steps_survived, const unsigned char* done,
                                const float* rho, const unsigned char* line_status, int* topo, int* cooldown) {
  const gpf::OppCfg c = to_cfg(*e);
  for (int i = 0; i < c.n_att; ++i) if (c.lines[i] < 0 || c.lines[i] >= n_line) return -1;
  for (int k = 0; k < n_lanes; ++k) {
    gpf::OppLane L;
    L.budget = budget + k; L.st = state + (size_t)k * gpf::OPP_STATE_INTS;
    L.draws = c.n_draw > 0 ? draws + (size_t)k * c.n_draw : nullptr;
    L.sched = sched + (size_t)k * (c.sched_cap > 0 ? c.sched_cap : 1) * 2;
    L.global_lane = k + c.lane_base;
    gpf::opp_prestep_serial(c, L, steps_survived[k], done[k], rho + (size_t)k * n_line, line_status + (size_t)k * n_line, topo + (size_t)k * dim_topo,
                            cooldown + (size_t)k * n_line, or_pos, ex_pos);
  }
  return 0;
}

#ifdef OPPONENT_EMUL_MAIN
namespace {
unsigned long long rng_state = 88172645463325252ull;
unsigned long long rnd64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
int rnd(int n) { return (int)(rnd64() % (unsigned long long)n); }
double rnd_u() { return (double)(rnd64() >> 11) * (1.0 / 9007199254740992.0); }
}  // namespace

int main() {
  const int L = 150, D = 2 * L, lanes = 7, steps = 400, cap = 5, n_draw = 60;
  std::vector<int> or_pos(L), ex_pos(L), lines(L - 3);
  for (int l = 0; l < L; ++l) { or_pos[l] = 2 * l; ex_pos[l] = 2 * l + 1; }
  for (int i = 0; i < L - 3; ++i) lines[i] = (i * 7 + 3) % L;             // a permutation prefix: distinct ids, more than two chunks of 64
  std::vector<double> norm(L - 3);
  for (auto& v : norm) v = 0.5 + rnd_u();
  long long attacks = 0, checks = 0;
  for (int kind = 1; kind <= 3; ++kind)
    for (int source = 0; source < 2; ++source)
      for (int n_att : {1, 2, 64, 65, L - 3}) {
        opp_emul_cfg e{};
        e.kind = kind; e.n_att = n_att; e.lines = lines.data(); e.norm = norm.data(); e.attack_period = 4; e.hazard = 0.3; e.recovery = 0.5; e.min_dur = 1;
        e.ratio = 4.0; e.episode_len = 60; e.init_budget = 3.f; e.budget_per_ts = 0.4f; e.max_duration = 4; e.attack_cooldown = 3; e.source = source;
        e.seed_lo = 12345u + kind; e.seed_hi = 99u; e.lane_base = 1000; e.sched_cap = cap; e.n_draw = n_draw;
        std::vector<double> budget(lanes, 3.0), draws((size_t)lanes * n_draw);
        for (auto& u : draws) u = rnd_u();
        draws[0] = 0.0; draws[1] = 1.0 - 1.0 / 9007199254740992.0;         // the ends of [0, 1)
        std::vector<int> state((size_t)lanes * gpf::OPP_STATE_INTS, 0), sched((size_t)lanes * cap * 2, 0), topo((size_t)lanes * D, 1), cool((size_t)lanes * L, 0);
        for (int k = 0; k < lanes; ++k) {
          int* s = &state[(size_t)k * gpf::OPP_STATE_INTS];
          s[gpf::OS_F32] = 1; s[gpf::OS_COOLDOWN] = 3; s[gpf::OS_LINE] = -1; s[gpf::OS_NEXT_TIME] = gpf::OPP_TIME_NONE; s[gpf::OS_INFO_LINE] = -1;
          if (kind == 3 && source == 0) { s[gpf::OS_N_SCHED] = cap; for (int i = 0; i < cap; ++i) { sched[((size_t)k * cap + i) * 2] = 1 + rnd(4); sched[((size_t)k * cap + i) * 2 + 1] = 1 + rnd(6); } }
        }
        std::vector<int> survived(lanes, 0);
        std::vector<unsigned char> done(lanes, 0), status((size_t)lanes * L, 1);
        std::vector<float> rho((size_t)lanes * L, 0.f);
        for (int t = 0; t < steps; ++t) {
          for (int k = 0; k < lanes; ++k)
            for (int l = 0; l < L; ++l) {
              const bool on = topo[(size_t)k * D + or_pos[l]] > 0 && topo[(size_t)k * D + ex_pos[l]] > 0;
              status[(size_t)k * L + l] = on ? 1 : 0;
              rho[(size_t)k * L + l] = on ? (float)(rnd(40) / 32.0) : 0.f;            // few values: ties, and zero weights
            }
          if (t == 200)                                                               // states at the edges of what the setter accepts
            for (int k = 0; k < lanes; ++k) {
              int* s = &state[(size_t)k * gpf::OPP_STATE_INTS];
              s[gpf::OS_PREV_FAILS] = 1; s[gpf::OS_COUNTER] = k == 0 ? 0 : rnd(cap + 2); s[gpf::OS_DURATION] = rnd(3); s[gpf::OS_LINE] = rnd(L + 1) - 1;
              budget[k] = k == 1 ? -1.0 : 0.25 * rnd(40);
            }
          if (opp_emul_prestep(&e, lanes, L, D, or_pos.data(), ex_pos.data(), budget.data(), state.data(), draws.data(), sched.data(), survived.data(),
                               done.data(), rho.data(), status.data(), topo.data(), cool.data()) != 0) { std::printf("FAIL: bad lines\n"); return 1; }
          for (int k = 0; k < lanes; ++k) {
            const int* s = &state[(size_t)k * gpf::OPP_STATE_INTS];
            const int line = s[gpf::OS_INFO_LINE], dur = s[gpf::OS_INFO_DURATION];
            ++checks;
            bool ok = line >= -1 && line < L && s[gpf::OS_DURATION] >= 0 && s[gpf::OS_COOLDOWN] >= 0 && s[gpf::OS_N_SCHED] <= cap;
            if (line >= 0 && survived[k] > 0 && !done[k]) {
              ++attacks;
              ok = ok && dur == s[gpf::OS_DURATION] && topo[(size_t)k * D + or_pos[line]] == -1 && topo[(size_t)k * D + ex_pos[line]] == -1 && cool[(size_t)k * L + line] >= dur && !s[gpf::OS_F32];
            } else if (!(survived[k] > 0 && done[k])) ok = ok && line == -1 && dur == 0;    // (a done lane is left alone: its info stands)
            if (!ok) { std::printf("FAIL: kind %d source %d n_att %d step %d lane %d\n", kind, source, n_att, t, k); return 1; }
            // the environment's side: one step survived, cooldowns count down, a line whose cooldown ran out comes back, rare game overs
            for (int l = 0; l < L; ++l) {
              int& cd = cool[(size_t)k * L + l];
              cd = cd > 0 ? cd - 1 : 0;
              if (cd == 0 && rnd(3) == 0) { topo[(size_t)k * D + or_pos[l]] = 1; topo[(size_t)k * D + ex_pos[l]] = 1; }
            }
            survived[k] = rnd(60) == 0 ? 0 : survived[k] + 1;
            done[k] = (survived[k] > 0 && rnd(200) == 0) ? 1 : 0;
          }
        }
      }
  // Philox4x32-10 known answers (Random123 kat_vectors)
  uint32_t x[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u};
  gpf::philox4x32_10(x, 0xa4093822u, 0x299f31d0u);
  if (x[0] != 0xd16cfe09u || x[1] != 0x94fdccebu || x[2] != 0x5001e420u || x[3] != 0x24126ea1u) { std::printf("FAIL: Philox known answer\n"); return 1; }
  if (attacks < 1000) { std::printf("FAIL: only %lld attacks\n", attacks); return 1; }
  std::printf("OK: %lld lane steps, %lld attacked\n", checks, attacks);
  return 0;
}
#endif
