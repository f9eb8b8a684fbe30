// Host emulator of the rules by area and the composite actions (grid2op_amd/csrc/gridpf_topo_mask.hpp), test infrastructure compiled with
// g++: the SAME run-time ambiguity (topo_dense_ambiguity), summary builder with areas, per-area rule core (topo_mask_eval_area) and area
// sets (topo_action_areas) as the library.  A composite is evaluated as the pre-step kernel treats it: the item lists of its non-empty
// slots concatenated in slot order into ONE entry.
//   g++ -O2 -std=c++17 -fPIC -shared topo_area_emul.cpp -o libtopoareaemul.so          (tests/test_topo_area_cpu.py, ctypes)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DTOPO_AREA_EMUL_MAIN topo_area_emul.cpp -o topo_area_emul_san
// The second is a stand-alone program: random tables and composites on a ring grid of three areas with more than 64 lines and
// substations, the summary-based masks against a dense per-area evaluation written like steps 1-3 of topo_prestep_kernel<true>.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_topo_mask.hpp"

// comps [n_comp][n_slot] table indices (-1: empty slot) -> the table of the concatenated entries; bad[c] = 1: an index outside the table
static void concat(int n_act, const int* act_off, const int* act_items, int n_comp, int n_slot, const int* comps, std::vector<int>& off,
                   std::vector<int>& items, std::vector<unsigned char>& bad) {
  off.assign(1, 0); items.clear(); bad.assign((size_t)n_comp, 0);
  for (int c = 0; c < n_comp; ++c) {
    for (int k = 0; k < n_slot; ++k) {
      const int a = comps[(size_t)c * n_slot + k];
      if (a < -1 || a >= n_act) bad[c] = 1;
      if (a < 0 || a >= n_act) continue;
      items.insert(items.end(), act_items + 3 * (size_t)act_off[a], act_items + 3 * (size_t)act_off[a + 1]);
    }
    off.push_back((int)items.size() / 3);
  }
}

// table + grid maps + areas (sub_area NULL: none, then n_area = 0) + lane rows -> mask bytes [n_lanes][n_act], ambiguity flags [n_act] and
// area sets [n_act] of the entries; with comps also masks [n_lanes][n_comp] and ambiguity [n_comp] of the composites.  line_cd may be NULL.
extern "C" int topo_area_emul(int dim_topo, int n_line, int n_sub, const int* or_pos, const int* ex_pos, const int* pos_sub, int n_act,
                              const int* act_off, const int* act_items, const int* sub_area, int rules_on, int max_line, int max_sub, int n_lanes,
                              const int* topo, const int* line_cd, const int* sub_cd, unsigned char* mask, unsigned char* amb_out, unsigned* areas_out,
                              int n_comp, int n_slot, const int* comps, unsigned char* comp_mask, unsigned char* comp_amb) {
  const gpf::TopoMaskGrid g{dim_topo, n_line, n_sub, or_pos, ex_pos, pos_sub};
  std::vector<int> c_off, c_items;
  std::vector<unsigned char> c_bad;
  if (n_comp) concat(n_act, act_off, act_items, n_comp, n_slot, comps, c_off, c_items, c_bad);
  const int wl = gpf::tm_words(n_line), ws = gpf::tm_words(n_sub);
  std::vector<unsigned long long> live(wl), lcd(wl), scd(ws);
  for (int pass = 0; pass < (n_comp ? 2 : 1); ++pass) {
    const int n = pass ? n_comp : n_act;
    const int* off = pass ? c_off.data() : act_off;
    const int* items = pass ? c_items.data() : act_items;
    unsigned char* out = pass ? comp_mask : mask;
    std::vector<unsigned char> amb((size_t)n, 0);
    gpf::topo_static_ambiguity(g, n, off, items, amb.data());        // (topo_dense_ambiguity on the entry's dense arrays)
    if (pass) for (int c = 0; c < n; ++c) amb[c] = amb[c] || c_bad[c];
    gpf::TopoMaskSummary s;
    if (!gpf::build_topo_mask_summary(g, n, off, items, amb.data(), s, sub_area)) return -1;
    const gpf::TopoMaskTab tab = s.tab(amb.data(), n);
    for (int k = 0; k < n_lanes; ++k) {
      std::fill(live.begin(), live.end(), 0ull); std::fill(lcd.begin(), lcd.end(), 0ull); std::fill(scd.begin(), scd.end(), 0ull);
      const int* row = topo + (size_t)k * dim_topo;
      for (int l = 0; l < n_line; ++l) {
        if (row[or_pos[l]] > 0 && row[ex_pos[l]] > 0) live[l >> 6] |= 1ull << (l & 63);
        if (line_cd && line_cd[(size_t)k * n_line + l] > 0) lcd[l >> 6] |= 1ull << (l & 63);
      }
      for (int i = 0; i < n_sub; ++i) if (sub_cd[(size_t)k * n_sub + i] > 0) scd[i >> 6] |= 1ull << (i & 63);
      for (int a = 0; a < n; ++a)                              // (the kernel's choice between the two rule cores)
        out[(size_t)k * n + a] = (unsigned char)((rules_on && sub_area)
                                                     ? gpf::topo_mask_eval_area(tab, a, live.data(), lcd.data(), scd.data(), max_line, max_sub)
                                                     : gpf::topo_mask_eval(tab, a, live.data(), lcd.data(), scd.data(), rules_on, max_line, max_sub));
    }
    unsigned char* ao = pass ? comp_amb : amb_out;
    if (ao) for (int a = 0; a < n; ++a) ao[a] = amb[a];
  }
  if (areas_out) gpf::topo_action_areas(g, n_act, act_off, act_items, sub_area, nullptr, areas_out);
  return 0;
}

#ifdef TOPO_AREA_EMUL_MAIN
namespace {
unsigned long long rng_state = 88172645463325252ull;
int rnd(int n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (int)(rng_state % (unsigned long long)n); }

// steps 1-3 of topo_prestep_kernel<true> on dense arrays, every reason kept; counts per area in plain ints
unsigned dense_mask(int D, int L, int S, const int* or_pos, const int* ex_pos, const int* pos_sub, const int* sub_area, const int* items, int n_items,
                    const int* row, const int* line_cd, const int* sub_cd, int max_line, int max_sub) {
  std::vector<int> setv(D, 0), chg(D, 0), eff(D, 0), setl(L, 0), swl(L, 0), imp(L, 0), subf(S, 0);
  for (int k = 0; k < n_items; ++k) {
    const int kind = items[3 * k], id = items[3 * k + 1], v = items[3 * k + 2];
    if (kind == 0) setv[id] = v;
    else if (kind == 2) chg[id] = 1;
    else if (kind == 1) { setl[id] = v; if (v != 0) imp[id] = 1; }
    else if (kind == 3) { swl[id] = 1; imp[id] = 1; }
  }
  if (gpf::topo_dense_ambiguity(D, L, or_pos, ex_pos, setv.data(), chg.data(), setl.data(), swl.data(), 0, 1)) return gpf::TM_AMBIGUOUS;
  for (int i = 0; i < D; ++i) eff[i] = (chg[i] || setv[i] != 0) ? 1 : 0;
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
  int nl[16] = {0}, ns[16] = {0};
  for (int l = 0; l < L; ++l) if (imp[l]) { ++nl[sub_area[pos_sub[or_pos[l]]]]; if (line_cd[l] > 0) m |= gpf::TM_LINE_COOLDOWN; }
  for (int i = 0; i < S; ++i) if (subf[i]) { ++ns[sub_area[i]]; if (sub_cd[i] > 0) m |= gpf::TM_SUB_COOLDOWN; }
  for (int k = 0; k < 16; ++k) { if (nl[k] > max_line) m |= gpf::TM_TOO_MANY_LINES; if (ns[k] > max_sub) m |= gpf::TM_TOO_MANY_SUBS; }
  return m;
}
}  // namespace

int main() {
  // a ring of S substations in three areas: line l joins substations l and l + 1 (and a chord l -> l + 7 for l >= S); one load per substation
  const int S = 70, L = 100, D = 2 * L + S, n_act = 300, n_lanes = 24, n_comp = 200, n_slot = 3;
  std::vector<int> or_pos(L), ex_pos(L), pos_sub(D), sub_area(S);
  for (int l = 0; l < L; ++l) {
    or_pos[l] = 2 * l; ex_pos[l] = 2 * l + 1;
    pos_sub[2 * l] = l % S; pos_sub[2 * l + 1] = (l < S ? l + 1 : l + 7) % S;
  }
  for (int i = 0; i < S; ++i) { pos_sub[2 * L + i] = i; sub_area[i] = i < 20 ? 0 : i < 45 ? 1 : 2; }
  std::vector<int> off(1, 0), items;
  for (int a = 0; a < n_act; ++a) {
    const int n_items = rnd(4);
    for (int k = 0; k < n_items; ++k) {
      const int kind = rnd(4);
      items.push_back(kind);
      items.push_back(kind == 0 || kind == 2 ? rnd(D) : rnd(L));
      items.push_back(kind == 0 ? rnd(4) - 1 : kind == 1 ? rnd(3) - 1 : 0);
    }
    off.push_back((int)items.size() / 3);
  }
  std::vector<int> comps((size_t)n_comp * n_slot);
  for (auto& v : comps) v = rnd(4) == 0 ? -1 : rnd(n_act);
  comps[0] = n_act;                                            // an index outside the table: ambiguous
  int lg = 0, other = 0;                                       // one index in several slots: the longest entry three times, twice with
  for (int a = 0; a < n_act; ++a) if (off[a + 1] - off[a] > off[lg + 1] - off[lg]) lg = a;       // another entry, an entry around a gap
  while (other == lg || off[other + 1] == off[other]) ++other;
  const int dup[3][3] = {{lg, lg, lg}, {lg, lg, other}, {other, -1, other}};
  for (int c = 0; c < 3; ++c) for (int k = 0; k < n_slot; ++k) comps[(size_t)(1 + c) * n_slot + k] = dup[c][k];
  std::vector<int> topo((size_t)n_lanes * D), lcd((size_t)n_lanes * L), scd((size_t)n_lanes * S);
  for (auto& v : topo) v = rnd(5) == 0 ? -1 : 1 + rnd(2);
  for (auto& v : lcd) v = rnd(8) == 0 ? 1 + rnd(3) : 0;
  for (auto& v : scd) v = rnd(8) == 0 ? 1 + rnd(3) : 0;
  std::vector<unsigned char> mask((size_t)n_lanes * n_act), amb(n_act), cmask((size_t)n_lanes * n_comp), camb(n_comp);
  std::vector<unsigned> areas(n_act);
  std::vector<int> c_off, c_items;
  std::vector<unsigned char> c_bad;
  concat(n_act, off.data(), items.data(), n_comp, n_slot, comps.data(), c_off, c_items, c_bad);
  long long bad = 0, seen[6] = {0, 0, 0, 0, 0, 0};
  for (int max_rule = 1; max_rule <= 2; ++max_rule) {
    if (topo_area_emul(D, L, S, or_pos.data(), ex_pos.data(), pos_sub.data(), n_act, off.data(), items.data(), sub_area.data(), 1, max_rule, max_rule,
                       n_lanes, topo.data(), lcd.data(), scd.data(), mask.data(), amb.data(), areas.data(), n_comp, n_slot, comps.data(), cmask.data(),
                       camb.data()) != 0) return 2;
    for (int k = 0; k < n_lanes; ++k) {
      for (int a = 0; a < n_act; ++a) {
        const unsigned want = dense_mask(D, L, S, or_pos.data(), ex_pos.data(), pos_sub.data(), sub_area.data(), items.data() + 3 * (size_t)off[a],
                                         off[a + 1] - off[a], topo.data() + (size_t)k * D, lcd.data() + (size_t)k * L, scd.data() + (size_t)k * S, max_rule, max_rule);
        const unsigned got = mask[(size_t)k * n_act + a];
        if (got != want) { if (bad++ < 5) std::printf("lane %d entry %d: mask %#x, dense evaluation %#x\n", k, a, got, want); }
      }
      for (int c = 0; c < n_comp; ++c) {
        const unsigned want = c_bad[c] ? gpf::TM_AMBIGUOUS
                                       : dense_mask(D, L, S, or_pos.data(), ex_pos.data(), pos_sub.data(), sub_area.data(), c_items.data() + 3 * (size_t)c_off[c],
                                                    c_off[c + 1] - c_off[c], topo.data() + (size_t)k * D, lcd.data() + (size_t)k * L, scd.data() + (size_t)k * S,
                                                    max_rule, max_rule);
        const unsigned got = cmask[(size_t)k * n_comp + c];
        if (got != want) { if (bad++ < 5) std::printf("lane %d composite %d: mask %#x, dense evaluation %#x\n", k, c, got, want); }
        for (int b = 0; b < 5; ++b) seen[b] += (got >> b) & 1;
        seen[5] += got == 0;
      }
    }
  }
  // the area sets: every substation and line an entry names lies in them
  for (int a = 0; a < n_act; ++a)
    for (int q = off[a]; q < off[a + 1]; ++q) {
      const int kind = items[3 * q], id = items[3 * q + 1];
      const unsigned need = (kind == 0 || kind == 2) ? 1u << sub_area[pos_sub[id]]
                                                     : (1u << sub_area[pos_sub[or_pos[id]]]) | (1u << sub_area[pos_sub[ex_pos[id]]]);
      if ((areas[a] & need) != need) ++bad;
    }
  // no areas: the whole-grid rule core, bit 0 alone in the area sets
  if (topo_area_emul(D, L, S, or_pos.data(), ex_pos.data(), pos_sub.data(), n_act, off.data(), items.data(), nullptr, 1, 1, 1, n_lanes, topo.data(), nullptr,
                     scd.data(), mask.data(), amb.data(), areas.data(), 0, 0, nullptr, nullptr, nullptr) != 0) return 2;
  for (int a = 0; a < n_act; ++a) if (areas[a] != (off[a + 1] > off[a] ? 1u : 0u)) ++bad;
  std::printf("topo_area_emul self-test: %lld mismatches; composite bits seen %lld %lld %lld %lld %lld, legal %lld\n", bad, seen[0], seen[1], seen[2],
              seen[3], seen[4], seen[5]);
  for (int b = 0; b < 6; ++b) if (!seen[b]) return 3;
  return bad ? 1 : 0;
}
#endif
