// alert_emul.cpp -- the rule core of grid2op_amd/csrc/gridpf_alert.hpp compiled with g++ (no HIP): the shared library tests/alert_ref.py
// loads, and with -DALERT_EMUL_MAIN a stand-alone program for -fsanitize=address,undefined that drives the rules through resets, attacks
// that overlap, alerts on bit 63, both scoring branches and the largest and smallest windows.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_alert.hpp"

static gpf::AlertCfg cfg_of(int A, int W, const float* c) { return gpf::AlertCfg{A, W, c[0], c[1], c[2], c[3]}; }

extern "C" {

int alert_emul_prestep(int A, int W, const float* c, int* ob, uint64_t* ax, int steps_survived, int done, uint64_t raise, uint64_t att) {
  return gpf::alert_prestep_serial(cfg_of(A, W, c), ob, ax, steps_survived, done, raise, att);
}

float alert_emul_poststep(int A, int W, const float* c, int* ob, uint64_t* ax, int blackout) {
  return gpf::alert_poststep_serial(cfg_of(A, W, c), ob, ax, blackout);
}

}  // extern "C"

#ifdef ALERT_EMUL_MAIN
int main() {
  const float c[4] = {-1.f, -10.f, 1.f, 2.f};
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  long checks = 0;
  for (int A : {1, 22, 64})
    for (int W : {1, 4, 12, 62}) {
      // exactly sized rows: a write past a section is a sanitizer report
      std::vector<int> ob((size_t)gpf::alert_obs_ints(A), 7);
      std::vector<uint64_t> ax((size_t)gpf::alert_aux_words(W), ~(uint64_t)0);
      const uint64_t valid = gpf::alert_valid_bits(A);
      int survived = 0;
      uint64_t att = 0;
      for (int t = 0; t < 400; ++t) {
        const uint64_t r = next();
        const uint64_t raise = (r & next()) | ((r >> 11) & 1 ? (uint64_t)1 << 63 : 0);     // (bits above A are dropped by the rule)
        if ((r >> 20) % 5 == 0) att = next() & next() & valid; else if ((r >> 20) % 5 == 1) att = 0; else if ((r >> 20) % 5 == 2) att &= next();
        const int done_before = survived > 0 && (r >> 30) % 17 == 0;
        const int ran = alert_emul_prestep(A, W, c, ob.data(), ax.data(), survived, done_before, raise, att);
        const int blackout = (r >> 40) % 9 == 0;
        const float rew = alert_emul_poststep(A, W, c, ob.data(), ax.data(), blackout);
        if (!ran && rew != 0.f) { std::printf("FAIL: a reward on a lane that did not run\n"); return 1; }
        if (rew < -10.f || rew > 2.f) { std::printf("FAIL: reward %g out of range\n", rew); return 1; }
        if ((int)(uint32_t)ax[gpf::AX_ID] >= W + 2) { std::printf("FAIL: ring index\n"); return 1; }
        for (int i = 0; i < gpf::alert_aux_words(W); ++i)
          if (i != gpf::AX_ID && (ax[i] & ~valid)) { std::printf("FAIL: a bit above A in word %d\n", i); return 1; }
        survived = (blackout && ran) || (r >> 50) % 23 == 0 ? 0 : survived + 1;
        ++checks;
      }
    }
  std::printf("OK %ld steps\n", checks);
  return 0;
}
#endif
