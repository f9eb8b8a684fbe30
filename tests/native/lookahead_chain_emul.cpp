// lookahead_chain_emul.cpp -- the chain rules of grid2op_amd/csrc/gridpf_lookahead.hpp compiled with g++ (no HIP): the shared library
// tests/lookahead_chain_ref.py loads, and with -DLA_CHAIN_EMUL_MAIN a stand-alone program for -fsanitize=address,undefined that drives the
// sticky record, the fall-back ranking, the pick and the forecast row through every branch on exactly sized rows.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_lookahead.hpp"

extern "C" {

// One scratch lane over H steps: rho [H][n_line] and done [H] as the steps left them -> value_h [H], out_f = {value, peak}, out_i =
// {survived, failed}.  The row maximum is the library's strided share and butterfly.
void la_chain_emul_lane(int H, int n_line, const float* rho, const unsigned char* done, float* value_h, float* out_f, int* out_i) {
  gpf::LaChainState s = gpf::la_chain_start();
  for (int h = 1; h <= H; ++h)
    value_h[h - 1] = gpf::la_chain_step(s, h, done[h - 1] != 0, gpf::la_max_serial(n_line, rho + (size_t)(h - 1) * n_line));
  out_f[0] = s.value; out_f[1] = s.peak;
  out_i[0] = s.survived; out_i[1] = gpf::la_chain_failed(s, H) ? 1 : 0;
}

// out = {fallback, fallback_steps}
void la_chain_emul_fallback(int K, const int* survived, const float* peak, const unsigned char* flags, int* out) {
  const gpf::LaFallback f = gpf::la_fallback_serial(survived, peak, flags, K);
  out[0] = f.slot; out[1] = f.steps;
}

int la_chain_emul_outranks(int sa, float pa, int ka, int sb, float pb, int kb) { return gpf::la_chain_outranks(sa, pa, ka, sb, pb, kb) ? 1 : 0; }
int la_chain_emul_pick(int play, int best, int fallback) { return gpf::la_chain_pick(play, best, fallback); }
int la_chain_emul_row(int n_h, int idx, int h) { return gpf::la_chain_row(n_h, idx, h); }

}  // extern "C"

#ifdef LA_CHAIN_EMUL_MAIN
int main() {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  auto unif = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(next() >> 11) / 9007199254740992.0); };
  long checks = 0;
  for (int n : {1, 6, 20, 63, 64, 65, 129, 187})
    for (int H : {1, 2, 4, 12})
      for (int rep = 0; rep < 6; ++rep) {
        // exactly sized rows: a read past an array is a sanitizer report
        std::vector<float> rho((size_t)H * n), vh(H);
        std::vector<unsigned char> done(H);
        for (auto& r : rho) r = unif(0, 1.8);
        const int fail_at = rep == 0 ? 0 : (rep == 1 ? 1 : (int)(next() % (H + 1)));       // 0: never
        for (int h = 1; h <= H; ++h) done[h - 1] = (fail_at && h == fail_at) || (fail_at && h > fail_at && next() % 2);   // (later steps: anything)
        float f[2]; int i[2];
        la_chain_emul_lane(H, n, rho.data(), done.data(), vh.data(), f, i);
        const int want_s = fail_at ? fail_at - 1 : H;
        float peak = -INFINITY;
        for (int h = 1; h <= want_s; ++h) for (int l = 0; l < n; ++l) peak = std::fmax(peak, rho[(size_t)(h - 1) * n + l]);
        if (i[0] != want_s || i[1] != (fail_at ? 1 : 0) || f[1] != peak || f[0] != (fail_at ? INFINITY : peak)) { std::printf("FAIL: lane n = %d H = %d\n", n, H); return 1; }
        for (int h = 1; h <= H; ++h) {
          float m = -INFINITY;
          for (int l = 0; l < n; ++l) m = std::fmax(m, rho[(size_t)(h - 1) * n + l]);
          if (vh[h - 1] != (h <= want_s ? m : INFINITY)) { std::printf("FAIL: value_h\n"); return 1; }
        }
        // the fall-back on n slots against a plain search
        std::vector<int> sv(n);
        std::vector<float> pk(n);
        std::vector<unsigned char> fl(n);
        for (int k = 0; k < n; ++k) {
          sv[k] = (int)(next() % (H + 1)); pk[k] = sv[k] ? unif(0.2, 1.6) : -INFINITY;
          fl[k] = rep == 5 ? 1 : (unsigned char)(next() % 4 == 0 ? 1 + next() % 3 : 0);
          if (sv[k] < H) fl[k] |= 4;
        }
        if (n > 2) { sv[n / 2] = sv[n / 3]; pk[n / 2] = pk[n / 3]; }
        int out[2], arg = -1;
        la_chain_emul_fallback(n, sv.data(), pk.data(), fl.data(), out);
        for (int k = 0; k < n; ++k) {
          if (fl[k] & 3) continue;
          if (arg < 0 || sv[k] > sv[arg] || (sv[k] == sv[arg] && pk[k] < pk[arg])) arg = k;
        }
        if (out[0] != arg || out[1] != (arg < 0 ? 0 : sv[arg])) { std::printf("FAIL: fallback of n = %d\n", n); return 1; }
        ++checks;
      }
  if (la_chain_emul_pick(1, 3, 5) != 3 || la_chain_emul_pick(1, -1, 5) != -1 || la_chain_emul_pick(2, -1, 5) != 5 || la_chain_emul_pick(2, -1, -1) != -1 ||
      la_chain_emul_row(12, 7, 1) != 84 || la_chain_emul_row(12, 7, 12) != 95) { std::printf("FAIL: pick / row\n"); return 1; }
  std::printf("OK %ld rows\n", checks);
  return 0;
}
#endif
