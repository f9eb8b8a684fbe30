// Host emulator of the legality-mask kernel (grid2op_amd/csrc/gridpf_topo_mask.hpp), test infrastructure compiled with g++: the SAME
// static ambiguity, summary builder and rule core as the library, with the kernel's bit sets built by plain loops.
//   g++ -O2 -std=c++17 -fPIC -shared topo_mask_emul.cpp -o libtopomaskemul.so          (tests/test_topo_mask_cpu.py, ctypes)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DTOPO_MASK_EMUL_MAIN topo_mask_emul.cpp -o topo_mask_emul_san
// The second is a stand-alone program: random tables on a ring grid with more than 64 lines and substations, the summary-based masks
// against a dense evaluation written like steps 2-3 of topo_prestep_kernel (gridpf_topo.hpp:140-167).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_topo_mask.hpp"

// table + grid maps + lane rows -> mask bytes [n_lanes][n_act] and the static ambiguity flags [n_act].  line_cd may be NULL (zeros).
extern "C" int topo_mask_emul(int dim_topo, int n_line, int n_sub, const int* or_pos, const int* ex_pos, const int* pos_sub, int n_act,
                              const int* act_off, const int* act_items, int rules_on, int max_line, int max_sub, int n_lanes, const int* topo,
                              const int* line_cd, const int* sub_cd, unsigned char* mask, unsigned char* amb_out) {
  const gpf::TopoMaskGrid g{dim_topo, n_line, n_sub, or_pos, ex_pos, pos_sub};
  std::vector<unsigned char> amb((size_t)n_act, 0);
  gpf::topo_static_ambiguity(g, n_act, act_off, act_items, amb.data());
  gpf::TopoMaskSummary s;
  if (!gpf::build_topo_mask_summary(g, n_act, act_off, act_items, amb.data(), s)) return -1;
  const gpf::TopoMaskTab tab = s.tab(amb.data(), n_act);
  const int wl = gpf::tm_words(n_line), ws = gpf::tm_words(n_sub);
  std::vector<unsigned long long> live(wl), lcd(wl), scd(ws);
  for (int k = 0; k < n_lanes; ++k) {
    std::fill(live.begin(), live.end(), 0ull); std::fill(lcd.begin(), lcd.end(), 0ull); std::fill(scd.begin(), scd.end(), 0ull);
    const int* row = topo + (size_t)k * dim_topo;
    for (int l = 0; l < n_line; ++l) {
      if (row[or_pos[l]] > 0 && row[ex_pos[l]] > 0) live[l >> 6] |= 1ull << (l & 63);
      if (line_cd && line_cd[(size_t)k * n_line + l] > 0) lcd[l >> 6] |= 1ull << (l & 63);
    }
    for (int i = 0; i < n_sub; ++i) if (sub_cd[(size_t)k * n_sub + i] > 0) scd[i >> 6] |= 1ull << (i & 63);
    for (int a = 0; a < n_act; ++a)
      mask[(size_t)k * n_act + a] = (unsigned char)gpf::topo_mask_eval(tab, a, live.data(), lcd.data(), scd.data(), rules_on, max_line, max_sub);
  }
  if (amb_out) for (int a = 0; a < n_act; ++a) amb_out[a] = amb[a];
  return 0;
}

#ifdef TOPO_MASK_EMUL_MAIN
namespace {
unsigned long long rng_state = 88172645463325252ull;
int rnd(int n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (int)(rng_state % (unsigned long long)n); }

// steps 2-3 of topo_prestep_kernel on dense arrays, every reason kept
unsigned dense_mask(int D, int L, int S, const int* or_pos, const int* ex_pos, const int* pos_sub, const int* items, int n_items, const int* row,
                    const int* line_cd, const int* sub_cd, int max_line, int max_sub) {
  std::vector<int> setv(D, 0), eff(D, 0), imp(L, 0), subf(S, 0);
  for (int k = 0; k < n_items; ++k) {
    const int kind = items[3 * k], id = items[3 * k + 1], v = items[3 * k + 2];
    if (kind == 0) setv[id] = v;
    else if (kind == 2) eff[id] = 1;
    else if (kind == 3 || (kind == 1 && v != 0)) imp[id] = 1;
  }
  for (int i = 0; i < D; ++i) eff[i] = (eff[i] || setv[i] != 0) ? 1 : 0;
  for (int l = 0; l < L; ++l) {
    const int po = or_pos[l], pe = ex_pos[l];
    const bool st = row[po] > 0 && row[pe] > 0, notc = !st;
    bool im = imp[l] != 0, clr = im && notc;
    const bool hit = (setv[po] > 0 && notc) || (setv[pe] > 0 && notc) || (setv[po] < 0 && st) || (setv[pe] < 0 && st);
    im = im || hit; clr = clr || hit;
    if (clr) { eff[po] = 0; eff[pe] = 0; }
    imp[l] = im ? 1 : 0;
  }
  for (int i = 0; i < D; ++i) if (eff[i]) subf[pos_sub[i]] = 1;
  unsigned m = 0;
  int nl = 0, ns = 0;
  for (int l = 0; l < L; ++l) if (imp[l]) { ++nl; if (line_cd[l] > 0) m |= gpf::TM_LINE_COOLDOWN; }
  for (int i = 0; i < S; ++i) if (subf[i]) { ++ns; if (sub_cd[i] > 0) m |= gpf::TM_SUB_COOLDOWN; }
  if (nl > max_line) m |= gpf::TM_TOO_MANY_LINES;
  if (ns > max_sub) m |= gpf::TM_TOO_MANY_SUBS;
  return m;
}
}  // namespace

int main() {
  // a ring of S substations: line l joins substations l and l + 1 (and a chord l -> l + 7 for l >= S); one load per substation
  const int S = 70, L = 100, D = 2 * L + S, n_act = 300, n_lanes = 40;
  std::vector<int> or_pos(L), ex_pos(L), pos_sub(D);
  for (int l = 0; l < L; ++l) {
    or_pos[l] = 2 * l; ex_pos[l] = 2 * l + 1;
    pos_sub[2 * l] = l % S; pos_sub[2 * l + 1] = (l < S ? l + 1 : l + 7) % S;
  }
  for (int i = 0; i < S; ++i) pos_sub[2 * L + i] = i;
  std::vector<int> off(1, 0), items;
  for (int a = 0; a < n_act; ++a) {
    const int n_items = rnd(6);
    for (int k = 0; k < n_items; ++k) {
      const int kind = rnd(4);
      items.push_back(kind);
      items.push_back(kind == 0 || kind == 2 ? rnd(D) : rnd(L));
      items.push_back(kind == 0 ? rnd(4) - 1 : kind == 1 ? rnd(3) - 1 : 0);
    }
    off.push_back((int)items.size() / 3);
  }
  std::vector<int> topo((size_t)n_lanes * D), lcd((size_t)n_lanes * L), scd((size_t)n_lanes * S);
  for (auto& v : topo) v = rnd(5) == 0 ? -1 : 1 + rnd(2);
  for (auto& v : lcd) v = rnd(6) == 0 ? 1 + rnd(3) : 0;
  for (auto& v : scd) v = rnd(6) == 0 ? 1 + rnd(3) : 0;
  std::vector<unsigned char> mask((size_t)n_lanes * n_act), amb(n_act);
  long long bad = 0, seen[6] = {0, 0, 0, 0, 0, 0};
  for (int max_rule = 1; max_rule <= 2; ++max_rule) {
    if (topo_mask_emul(D, L, S, or_pos.data(), ex_pos.data(), pos_sub.data(), n_act, off.data(), items.data(), 1, max_rule, max_rule, n_lanes, topo.data(),
                       lcd.data(), scd.data(), mask.data(), amb.data()) != 0) return 2;
    for (int k = 0; k < n_lanes; ++k)
      for (int a = 0; a < n_act; ++a) {
        const unsigned want = amb[a] ? gpf::TM_AMBIGUOUS
                                     : dense_mask(D, L, S, or_pos.data(), ex_pos.data(), pos_sub.data(), items.data() + 3 * (size_t)off[a], off[a + 1] - off[a],
                                                  topo.data() + (size_t)k * D, lcd.data() + (size_t)k * L, scd.data() + (size_t)k * S, max_rule, max_rule);
        const unsigned got = mask[(size_t)k * n_act + a];
        if (got != want) { if (bad++ < 5) std::printf("lane %d entry %d: mask %#x, dense evaluation %#x\n", k, a, got, want); }
        for (int b = 0; b < 5; ++b) seen[b] += (got >> b) & 1;
        seen[5] += got == 0;
      }
  }
  // AlwaysLegal: the ambiguous bit alone; no line cooldowns at all (NULL)
  if (topo_mask_emul(D, L, S, or_pos.data(), ex_pos.data(), pos_sub.data(), n_act, off.data(), items.data(), 0, 1, 1, n_lanes, topo.data(), nullptr,
                     scd.data(), mask.data(), amb.data()) != 0) return 2;
  for (size_t i = 0; i < mask.size(); ++i) if (mask[i] != (amb[i % n_act] ? gpf::TM_AMBIGUOUS : 0u)) ++bad;
  std::printf("topo_mask_emul self-test: %lld mismatches; bits seen %lld %lld %lld %lld %lld, legal %lld\n", bad, seen[0], seen[1], seen[2], seen[3],
              seen[4], seen[5]);
  for (int b = 0; b < 6; ++b) if (!seen[b]) return 3;
  return bad ? 1 : 0;
}
#endif
