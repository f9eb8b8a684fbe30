// cursor_emul.cpp -- the rule of grid2op_amd/csrc/gridpf_cursor.hpp compiled with g++ (no HIP): the shared library tests/cursor_ref.py
// loads, and with -DCURSOR_EMUL_MAIN a stand-alone program for -fsanitize=address,undefined that drives lanes through both policies and
// both draw sources on exactly sized tables.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_cursor.hpp"

extern "C" {

// one episode start of one lane (gridpf_cursor.hpp cursor_start); state: {table, offset, pos, next_pos, n_started, draws used, flags}
void cursor_emul_start(int n_order, const int* order, int policy, const double* cdf, int source, uint32_t seed_lo, uint32_t seed_hi, int lane_base,
                       int n_draw, const double* draws, int T, int first_row, int lane, int t, int* state) {
  gpf::CursorCfg c{};
  c.n_order = n_order; c.order = order; c.policy = policy; c.cdf = cdf; c.source = source; c.seed_lo = seed_lo; c.seed_hi = seed_hi;
  c.lane_base = lane_base; c.n_draw = n_draw; c.T = T;
  gpf::CursorLane L{};
  L.table = state; L.offset = state + 1; L.pos = state + 2; L.next_pos = state + 3; L.n_started = state + 4; L.draws_used = state + 5;
  L.flags = state + 6;
  L.draws = draws; L.first_row = first_row; L.global_lane = lane + lane_base;
  gpf::cursor_start(c, L, t);
}

// the uniform the Philox source gives an episode start
double cursor_emul_philox_u(uint32_t n_started, uint32_t global_lane, uint32_t seed_lo, uint32_t seed_hi) {
  uint32_t x[4] = {n_started, 0u, global_lane, gpf::CUR_PHILOX_STREAM};
  gpf::philox4x32_10(x, seed_lo, seed_hi);
  return gpf::opp_philox_u(x[0], x[1]);
}

int cursor_emul_state_ints() { return gpf::CUR_STATE_INTS; }

}  // extern "C"

#ifdef CURSOR_EMUL_MAIN
int main() {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  long checks = 0;
  for (int n : {1, 2, 3, 20})
    for (int policy : {gpf::CUR_SEQUENTIAL, gpf::CUR_SAMPLED})
      for (int source : {gpf::CUR_DRAWS_TABLE, gpf::CUR_DRAWS_PHILOX}) {
        std::vector<int> order(n);                                          // exactly sized: a read past them is a sanitizer report
        std::vector<double> cdf(n), draws(5);
        for (int i = 0; i < n; ++i) { order[i] = (i * 7 + 3) % n; cdf[i] = (double)(i + 1) / n; }
        for (double& u : draws) u = (double)(next() >> 11) / 9007199254740992.0;
        const int T = 11;
        int st[gpf::CUR_STATE_INTS] = {0, 0, -1, policy == gpf::CUR_SEQUENTIAL ? 0 : -1, 0, 0, 0};
        int expect = 0;
        for (int ep = 0; ep < 9; ++ep) {
          const int t = (int)(next() % 1000), first = ep % T;
          const int before_pos = st[2];
          if (ep == 4) st[3] = n - 1;                                       // set_id
          if (ep == 6) st[3] = n + 1;                                       // a bad value written on the device: wrapped, flagged
          cursor_emul_start(n, order.data(), policy, policy == gpf::CUR_SAMPLED ? cdf.data() : nullptr, source, 5u, 9u, 100, (int)draws.size(),
                            source == gpf::CUR_DRAWS_TABLE ? draws.data() : nullptr, T, first, 2, t, st);
          const int p = st[2];
          if (p < 0 || p >= n || st[0] != order[p]) { std::printf("FAIL: position\n"); return 1; }
          if (st[1] < 0 || st[1] >= T || (t + st[1]) % T != first) { std::printf("FAIL: offset\n"); return 1; }
          if (st[4] != ep + 1) { std::printf("FAIL: n_started\n"); return 1; }
          if (ep == 4 && p != n - 1) { std::printf("FAIL: next_pos not honoured\n"); return 1; }
          if (ep == 6 && (p != (n + 1) % n || !(st[6] & gpf::CUR_FLAG_NEXT_POS_WRAPPED))) { std::printf("FAIL: wrap\n"); return 1; }
          if (policy == gpf::CUR_SEQUENTIAL) {
            if (ep != 4 && ep != 6 && p != expect) { std::printf("FAIL: sequence\n"); return 1; }
            expect = (p + 1) % n;
            if (st[3] != expect || st[5] != 0) { std::printf("FAIL: next_pos\n"); return 1; }
          } else {
            if (st[3] != -1) { std::printf("FAIL: sampled next_pos\n"); return 1; }
            if (source == gpf::CUR_DRAWS_TABLE && st[5] == (int)draws.size() && (st[6] & gpf::CUR_FLAG_DRAWS_EXHAUSTED) && p != (before_pos < 0 ? 0 : before_pos)) {
              std::printf("FAIL: exhausted table\n"); return 1;
            }
          }
          ++checks;
        }
        if (policy == gpf::CUR_SAMPLED && source == gpf::CUR_DRAWS_TABLE && !(st[6] & gpf::CUR_FLAG_DRAWS_EXHAUSTED)) { std::printf("FAIL: flag\n"); return 1; }
      }
  std::printf("OK %ld checks\n", checks);
  return 0;
}
#endif
