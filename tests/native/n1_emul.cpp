// n1_emul.cpp -- the rule core of grid2op_amd/csrc/gridpf_n1.hpp compiled with g++ (no HIP): the shared library tests/n1_ref.py loads, and
// with -DN1_EMUL_MAIN a stand-alone program for -fsanitize=address,undefined that drives the value and summary rules through every branch
// on exactly sized rows at the element counts around one, two and three strides.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_n1.hpp"

extern "C" {

float n1_emul_value(int done, int converged, int n_line, const float* a_or, const float* thermal) {
  return gpf::n1_value(gpf::N1Serial{}, done != 0, converged != 0, n_line, a_or, thermal);
}

// worst[1], info[3] = {arg_worst, n_insecure, n_diverged}
void n1_emul_summary(int K, const float* value, float* worst, int* info) {
  const gpf::N1Summary s = gpf::n1_summary_serial(value, K);
  worst[0] = s.worst; info[0] = s.arg_worst; info[1] = s.n_insecure; info[2] = s.n_diverged;
}

}  // extern "C"

#ifdef N1_EMUL_MAIN
int main() {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  auto unif = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(next() >> 11) / 9007199254740992.0); };
  long checks = 0;
  for (int n : {1, 20, 59, 63, 64, 65, 128, 129, 186, 193})
    for (int rep = 0; rep < 8; ++rep) {
      // exactly sized rows: a read past an array is a sanitizer report
      std::vector<float> a_or(n), th(n);
      for (int i = 0; i < n; ++i) { a_or[i] = unif(0, 900); th[i] = rep % 3 == 0 && i % 5 == 0 ? unif(0, 1) : unif(100, 800); }
      float want = -INFINITY;
      for (int i = 0; i < n; ++i) want = std::fmax(want, a_or[i] / (th[i] <= 1.f ? 1.f : th[i]));
      if (n1_emul_value(0, 1, n, a_or.data(), th.data()) != want) { std::printf("FAIL: value of n = %d\n", n); return 1; }
      if (n1_emul_value(1, 1, n, a_or.data(), th.data()) != 0.f || n1_emul_value(1, 0, n, a_or.data(), th.data()) != 0.f) { std::printf("FAIL: done\n"); return 1; }
      if (n1_emul_value(0, 0, n, a_or.data(), th.data()) != -1.f) { std::printf("FAIL: diverged\n"); return 1; }
      // the summary on n values: a diverged entry, when there is one, outranks the rest; ties go to the lowest index
      std::vector<float> v(n);
      for (int i = 0; i < n; ++i) v[i] = unif(0.2, 1.6);
      if (n > 2) v[n / 2] = v[n / 3];
      const int div_at = rep % 2 ? (int)(next() % (uint64_t)n) : -1;
      if (div_at >= 0) v[div_at] = -1.f;
      float worst; int info[3];
      n1_emul_summary(n, v.data(), &worst, info);
      int arg = 0, ins = 0, dv = 0;
      for (int i = 0; i < n; ++i) { if (v[i] > v[arg]) arg = i; ins += (v[i] > 1.f || v[i] == -1.f); dv += v[i] == -1.f; }
      if (div_at >= 0) arg = div_at;
      if (info[0] != arg || worst != v[arg] || info[1] != ins || info[2] != dv) { std::printf("FAIL: summary of n = %d\n", n); return 1; }
      ++checks;
    }
  std::printf("OK %ld rows\n", checks);
  return 0;
}
#endif
