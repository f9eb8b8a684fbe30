// lookahead_emul.cpp -- the rule core of grid2op_amd/csrc/gridpf_lookahead.hpp compiled with g++ (no HIP): the shared library
// tests/lookahead_ref.py loads, and with -DLA_EMUL_MAIN a stand-alone program for -fsanitize=address,undefined that drives the value, the
// summary and the maintenance-ahead predicate through every branch on exactly sized rows.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_lookahead.hpp"

extern "C" {

float la_emul_value(int done, int n_line, const float* rho) { return gpf::la_value(done != 0, gpf::la_max_serial(n_line, rho)); }

// best_value[1], info[3] = {best, n_playable, n_done}
void la_emul_summary(int K, const float* value, const unsigned char* flags, float* best_value, int* info) {
  const gpf::LaSummary s = gpf::la_summary_serial(value, flags, K);
  best_value[0] = s.best_value; info[0] = s.best; info[1] = s.n_playable; info[2] = s.n_done;
}

int la_emul_outranks(float va, int ka, float vb, int kb) { return gpf::la_outranks(va, ka, vb, kb) ? 1 : 0; }

// out[n_line]: the lines the forecast time_step rows ahead of row idx has out
void la_emul_maintenance(const unsigned char* M, int T, int n_line, int idx, int time_step, unsigned char* out) {
  for (int l = 0; l < n_line; ++l) out[l] = gpf::la_maintenance_ahead(M, T, n_line, idx, time_step, l) ? 1 : 0;
}

}  // extern "C"

#ifdef LA_EMUL_MAIN
int main() {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  auto unif = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(next() >> 11) / 9007199254740992.0); };
  long checks = 0;
  for (int n : {1, 6, 20, 63, 64, 65, 70, 128, 129, 187})
    for (int rep = 0; rep < 8; ++rep) {
      // exactly sized rows: a read past an array is a sanitizer report
      std::vector<float> rho(n);
      for (int i = 0; i < n; ++i) rho[i] = unif(0, 1.8);
      float want = -INFINITY;
      for (int i = 0; i < n; ++i) want = std::fmax(want, rho[i]);
      if (la_emul_value(0, n, rho.data()) != want) { std::printf("FAIL: value of n = %d\n", n); return 1; }
      if (la_emul_value(1, n, rho.data()) != INFINITY) { std::printf("FAIL: done\n"); return 1; }
      // the summary on n slots: ties go to the lowest slot, a flagged slot is never the best, no playable slot: -1 and +inf
      std::vector<float> v(n);
      std::vector<unsigned char> f(n);
      for (int i = 0; i < n; ++i) { v[i] = unif(0.2, 1.6); f[i] = rep == 7 ? 1 : (unsigned char)(next() % 4 == 0 ? 1 + next() % 7 : 0); }
      if (n > 2) v[n / 2] = v[n / 3];
      for (int i = 0; i < n; ++i) if (f[i] & 4) v[i] = INFINITY;
      float bv; int info[3];
      la_emul_summary(n, v.data(), f.data(), &bv, info);
      int arg = -1, ok = 0, dn = 0;
      for (int i = 0; i < n; ++i) { if (f[i] == 0 && (arg < 0 || v[i] < v[arg])) arg = i; ok += f[i] == 0; dn += (f[i] & 4) != 0; }
      if (info[0] != arg || bv != (arg < 0 ? INFINITY : v[arg]) || info[1] != ok || info[2] != dn) { std::printf("FAIL: summary of n = %d\n", n); return 1; }
      // maintenance ahead on an exactly sized table: rows idx .. idx + time_step only
      const int T = 5 + (int)(next() % 6), L = 1 + (int)(next() % 4);
      std::vector<unsigned char> M((size_t)T * L), out(L);
      for (auto& b : M) b = next() % 3 == 0;
      for (int idx = 0; idx < T; ++idx)
        for (int ts = 0; ts <= 3; ++ts) {
          la_emul_maintenance(M.data(), T, L, idx, ts, out.data());
          for (int l = 0; l < L; ++l) {
            bool w = false;
            if (ts >= 1 && idx + ts < T) {
              int s = idx;
              while (s < T && !M[(size_t)s * L + l]) ++s;
              if (s < T && s <= idx + ts) { w = true; for (int r = s; r <= idx + ts; ++r) w = w && M[(size_t)r * L + l]; }
            }
            if ((out[l] != 0) != w) { std::printf("FAIL: maintenance ahead\n"); return 1; }
          }
        }
      ++checks;
    }
  std::printf("OK %ld rows\n", checks);
  return 0;
}
#endif
