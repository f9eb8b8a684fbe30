// combined_emul.cpp -- the rule core of grid2op_amd/csrc/gridpf_combined.hpp compiled with g++ (no HIP): the shared library
// tests/combined_ref.py loads, and with -DCOMBINED_EMUL_MAIN a stand-alone program for -fsanitize=address,undefined that drives lanes
// through every rule of the screen, the cancel and the merge on exactly sized rows.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_combined.hpp"

extern "C" {

// one lane in front of the topology pre-step (combined_screen_serial); rows may be null; out3: {ambiguous, illegal, reason}
void combined_emul_screen(int n_gen, int n_sto, const double* ramp_up, const double* ramp_down, const unsigned char* redispatchable,
                          const unsigned char* renewable, const float* max_prod, const float* max_absorb, const int* sto_pos, const float* redisp,
                          const float* storage, const float* curtail, const int* topo_row, int* slots, int n_slot, int n_act, const unsigned char* tab_amb,
                          const unsigned long long* tab_word, int check_values, int rules_on, unsigned char* out3) {
  const gpf::CombinedGrid g{n_gen, n_sto, ramp_up, ramp_down, redispatchable, renewable, max_prod, max_absorb, sto_pos};
  const gpf::CombinedVerdict v = gpf::combined_screen_serial(g, redisp, storage, curtail, topo_row, slots, n_slot, n_act, tab_amb, tab_word, check_values, rules_on);
  out3[0] = v.ambiguous; out3[1] = v.illegal; out3[2] = v.reason;
}

void combined_emul_cancel(int n_gen, int n_sto, int topo_illegal, int topo_ambiguous, int s_ambiguous, int s_illegal, float* redisp, float* storage,
                          float* curtail) {
  gpf::CombinedGrid g{};
  g.n_gen = n_gen; g.n_sto = n_sto;
  gpf::combined_cancel_serial(g, topo_illegal != 0, topo_ambiguous != 0, gpf::CombinedVerdict{(unsigned char)(s_ambiguous != 0), (unsigned char)(s_illegal != 0), 0},
                              redisp, storage, curtail);
}

uint32_t combined_emul_merge(int topo_illegal, int topo_ambiguous, int s_ambiguous, int s_illegal, int s_reason, int illegal_redisp) {
  const gpf::CombinedVerdict s{(unsigned char)(s_ambiguous != 0), (unsigned char)(s_illegal != 0), (unsigned char)s_reason};
  if (gpf::combined_unpack(gpf::combined_pack(s)).reason != s.reason) return 0xFFFFFFFFu;      // the byte between the kernels keeps the verdict
  return gpf::combined_merge(topo_illegal != 0, topo_ambiguous != 0, s, illegal_redisp != 0);
}

void combined_emul_words(int n_act, const int* off, const int* items, int n_sto, const int* sto_pos, unsigned long long* words) {
  gpf::combined_entry_words(n_act, off, items, n_sto, sto_pos, words);
}

}  // extern "C"

#ifdef COMBINED_EMUL_MAIN
#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAIL: %s\n", what); return 1; } ++checks; } while (0)
int main() {
  long checks = 0;
  // generator / storage counts around one stride of the kernels; every array exactly sized: a read past it is a sanitizer report
  for (int n_gen : {1, 6, 63, 64})
    for (int n_sto : {0, 2, 64}) {
      std::vector<double> ru(n_gen, 5.0), rd(n_gen, 4.0);
      std::vector<unsigned char> can(n_gen, 1), ren(n_gen, 0);
      can[n_gen - 1] = 0; ren[n_gen - 1] = 1;                              // the last generator: renewable, not redispatchable
      std::vector<float> mp(n_sto, 3.f), ma(n_sto, 2.f);
      std::vector<int> pos(n_sto), row(n_gen + n_sto, 1);
      for (int k = 0; k < n_sto; ++k) pos[k] = n_gen + k;
      // a table of three entries: nothing about storage, reconnects the last unit, ambiguous
      const std::vector<int> off = {0, 1, 1 + (n_sto ? 1 : 0), 1 + (n_sto ? 1 : 0)};
      std::vector<int> items = {1, 0, -1};
      if (n_sto) { items.push_back(0); items.push_back(pos[n_sto - 1]); items.push_back(1); }
      std::vector<unsigned long long> word(3);
      combined_emul_words(3, off.data(), items.data(), n_sto, pos.data(), word.data());
      CHECK(word[0] == 0 && word[2] == 0 && word[1] == (n_sto ? 1ull << (n_sto - 1) : 0ull), "entry words");
      const std::vector<unsigned char> amb = {0, 0, 1};
      auto run = [&](const float* r, const float* s, const float* c, int slot, int check, int rules, int* slot_after) {
        unsigned char o[3];
        int sl[1] = {slot};
        combined_emul_screen(n_gen, n_sto, ru.data(), rd.data(), can.data(), ren.data(), n_sto ? mp.data() : nullptr, n_sto ? ma.data() : nullptr,
                             pos.data(), r, s, c, row.data(), sl, 1, 3, amb.data(), word.data(), check, rules, o);
        if (slot_after) *slot_after = sl[0];
        return gpf::CombinedVerdict{o[0], o[1], o[2]};
      };
      std::vector<float> r(n_gen, 0.f), s(n_sto, 0.f), c(n_gen, -1.f);
      int after = 7;
      gpf::CombinedVerdict v = run(r.data(), n_sto ? s.data() : nullptr, c.data(), 0, 1, 1, &after);
      CHECK(!v.ambiguous && !v.illegal && v.reason == gpf::CB_NONE && after == 0, "a clean lane");
      v = run(nullptr, nullptr, nullptr, 0, 1, 1, &after);
      CHECK(!v.ambiguous && !v.illegal && after == 0, "no rows");
      r[n_gen - 1] = 1e-6f; v = run(r.data(), nullptr, nullptr, 0, 1, 1, &after); r[n_gen - 1] = 0.f;
      CHECK(v.ambiguous && !v.illegal && v.reason == gpf::CB_REDISP_FIXED_GEN && after == -1, "redispatch on a fixed generator");
      if (n_gen > 1) {
        r[0] = std::nextafterf(5.f, 6.f); v = run(r.data(), nullptr, nullptr, 0, 1, 1, &after);
        CHECK(v.ambiguous && v.reason == gpf::CB_REDISP_RAMP_UP && after == -1, "above ramp up");
        v = run(r.data(), nullptr, nullptr, 0, 0, 1, &after);
        CHECK(!v.ambiguous && after == 0, "check_values off");
        v = run(r.data(), nullptr, nullptr, 2, 1, 1, &after);
        CHECK(v.ambiguous && after == 2, "an ambiguous entry stays in its slot");
        v = run(r.data(), nullptr, nullptr, 9, 1, 1, &after);
        CHECK(v.ambiguous && after == 9, "an index outside the table stays in its slot");
        r[0] = 5.f; v = run(r.data(), nullptr, nullptr, 0, 1, 1, &after);
        CHECK(!v.ambiguous, "at ramp up");
        r[0] = -std::nextafterf(4.f, 5.f); v = run(r.data(), nullptr, nullptr, 0, 1, 1, &after);
        CHECK(v.ambiguous && v.reason == gpf::CB_REDISP_RAMP_DOWN, "below ramp down");
        r[0] = 0.f;
        c[0] = 0.5f; v = run(nullptr, nullptr, c.data(), 0, 1, 1, &after); c[0] = -1.f;
        CHECK(v.ambiguous && v.reason == gpf::CB_CURTAIL_FIXED_GEN, "curtailment on a fixed generator");
      }
      c[n_gen - 1] = 1.5f; v = run(nullptr, nullptr, c.data(), 0, 1, 1, &after);
      CHECK(v.ambiguous && v.reason == gpf::CB_CURTAIL_RANGE, "curtailment above 1");
      c[n_gen - 1] = -0.5f; v = run(nullptr, nullptr, c.data(), 0, 1, 1, &after);
      CHECK(v.ambiguous && v.reason == gpf::CB_CURTAIL_RANGE, "curtailment below 0");
      c[n_gen - 1] = 0.25f; v = run(nullptr, nullptr, c.data(), 0, 1, 1, &after);
      CHECK(!v.ambiguous && !v.illegal, "a legal curtailment");
      c[n_gen - 1] = -1.f;
      if (n_sto) {
        const int u = n_sto - 1;
        s[u] = std::nextafterf(2.f, 3.f); v = run(nullptr, s.data(), nullptr, 0, 1, 1, &after);
        CHECK(v.ambiguous && v.reason == gpf::CB_STORAGE_POWER, "storage above its absorption");
        s[u] = -std::nextafterf(3.f, 4.f); v = run(nullptr, s.data(), nullptr, 0, 1, 1, &after);
        CHECK(v.ambiguous && v.reason == gpf::CB_STORAGE_POWER, "storage below its production");
        s[u] = 1.f; row[pos[u]] = -1;
        v = run(nullptr, s.data(), nullptr, 0, 1, 1, &after);
        CHECK(!v.ambiguous && v.illegal && v.reason == gpf::CB_DISCO_STORAGE && after == -1, "the storage rule");
        v = run(nullptr, s.data(), nullptr, -1, 1, 1, &after);
        CHECK(v.illegal && after == -1, "the storage rule without a topology part");
        v = run(nullptr, s.data(), nullptr, 2, 1, 1, &after);
        CHECK(v.illegal && after == 2, "the storage rule and an ambiguous entry");
        v = run(nullptr, s.data(), nullptr, 1, 1, 1, &after);
        CHECK(!v.illegal && after == 1, "the same action reconnects the unit");
        v = run(nullptr, s.data(), nullptr, 0, 1, 0, &after);
        CHECK(!v.illegal && after == 0, "AlwaysLegal");
        s[u] = std::numeric_limits<float>::quiet_NaN(); v = run(nullptr, s.data(), nullptr, 0, 1, 1, &after);
        CHECK(!v.illegal && !v.ambiguous, "a NaN power is no action");
        s[u] = 0.f; row[pos[u]] = 1;
      }
      // cancel: either part's verdict leaves 0 / 0 / -1
      for (int bits = 0; bits < 16; ++bits) {
        std::vector<float> a(n_gen, 1.f), b(n_sto, 2.f), d(n_gen, 0.5f);
        combined_emul_cancel(n_gen, n_sto, bits & 1, bits & 2, bits & 4, bits & 8, a.data(), n_sto ? b.data() : nullptr, d.data());
        const bool hit = bits != 0;
        CHECK(a[n_gen - 1] == (hit ? 0.f : 1.f) && d[0] == (hit ? -1.f : 0.5f) && (!n_sto || b[n_sto - 1] == (hit ? 0.f : 2.f)), "cancel");
      }
    }
  // merge: an ambiguous action is not also illegal
  for (int bits = 0; bits < 32; ++bits) {
    const int ti = bits & 1, ta = (bits >> 1) & 1, sa = (bits >> 2) & 1, si = !sa && ((bits >> 3) & 1), ir = (bits >> 4) & 1;
    const uint32_t w = combined_emul_merge(ti, ta, sa, si, sa ? gpf::CB_STORAGE_POWER : si ? gpf::CB_DISCO_STORAGE : 0, ir);
    const int ill = w & 255, amb = (w >> 8) & 255, red = (w >> 16) & 255, why = w >> 24;
    CHECK(amb == (ta || sa) && ill == (!amb && (ti || si)) && red == ir, "merge flags");
    CHECK(why == (sa ? gpf::CB_STORAGE_POWER : ta ? gpf::CB_TOPO_AMBIGUOUS : si ? gpf::CB_DISCO_STORAGE : ti ? gpf::CB_TOPO_RULES : 0), "merge reason");
  }
  std::printf("OK %ld checks\n", checks);
  return 0;
}
#endif
