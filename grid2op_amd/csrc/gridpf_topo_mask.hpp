// gridpf_topo_mask.hpp -- legality masks of the uploaded topology action table (gpf_topo_action_mask, include/gridpf.h): for every
// (lane, table entry) what steps 1-3 of topo_prestep_kernel (gridpf_topo.hpp) would decide if the lane played the entry now, without playing
// it.  Paths relative to the reference checkout:
//   ambiguity  BaseAction._check_for_ambiguity (Action/baseAction.py:3668-3760), static per entry: topo_static_ambiguity;
//   impact     BaseAction.get_topological_impact (Action/baseAction.py:1782-2020) with the lane's line status;
//   legality   Rules/LookParam.py:28-53 + Rules/PreventReconnection.py:23-60 against the lane's line and substation cooldowns.
// Three parts: the static per-entry summary built on the host at upload (build_topo_mask_summary), the rule core of one (lane, entry)
// (topo_mask_eval, topo_mask_eval_area over topo_mask_rules: plain C++, the ONE statement of the mask's rules, run by the kernel and by
// the host emulators of tests/native/), and, for the one unit that defines GPF_TOPO_KERNEL (gridpf_capi_topo.hip), the kernel.  Without
// hipcc only the first two exist: the header then needs no HIP header.
//
// Areas (gpf_set_topo_areas; Rules/rulesByArea.py:120-140, _lookparam_byarea): every substation carries one area, a line the area of its
// ORIGIN substation (rulesByArea.py:91), and the two limits hold per area.  The summary then carries the area in bits 26-29 of every line
// word and substation word, and topo_mask_eval_area runs the same rules (topo_mask_rules) with a counter per area: sixteen saturating
// 8-bit counters held in two 64-bit registers.
// The ambiguity rules are stated once (topo_dense_ambiguity) for the upload and for the composite actions of topo_prestep_kernel.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GPF_TM_HD __host__ __device__
#else
#define GPF_TM_HD
#endif

#include <algorithm>
#include <utility>
#include <vector>

namespace gpf {

// reason bits of a mask byte (= GPF_MASK_* of include/gridpf.h); 0: the entry would be applied
constexpr unsigned TM_TOO_MANY_LINES = 0x01, TM_TOO_MANY_SUBS = 0x02, TM_LINE_COOLDOWN = 0x04, TM_SUB_COOLDOWN = 0x08, TM_AMBIGUOUS = 0x10;

// item kinds of the {kind, id, value} encoding (= GPF_ACT_*)
constexpr int TM_SET_BUS = 0, TM_SET_LINE_STATUS = 1, TM_CHANGE_BUS = 2, TM_CHANGE_LINE_STATUS = 3;

// A line word: what get_topological_impact needs of one line of one entry.  Bits 0-19 the line; STATUS: a line-status item names it
// (aff_lines whatever the status); OR_POS / OR_NEG, EX_POS / EX_NEG: sign of set_bus at its origin / extremity; END: as a line-end
// candidate (below), the end meant is the extremity.
constexpr int TM_LINE_BITS = 20, TM_LINE_MASK = (1 << TM_LINE_BITS) - 1;
constexpr int TM_STATUS = 1 << 20, TM_OR_POS = 1 << 21, TM_OR_NEG = 1 << 22, TM_EX_POS = 1 << 23, TM_EX_NEG = 1 << 24, TM_END = 1 << 25;
// A substation word: bits 0-19 the substation; ALWAYS: affected whatever the line status (a set_bus / change_bus on an element that is
// not a line end).
constexpr int TM_SUB_ALWAYS = 1 << 20;
// Bits 26-29 of a line word / substation word: the area of the line (of its origin substation) / of the substation; 0 without areas.
constexpr int TM_AREA_SHIFT = 26, TM_MAX_AREAS = 16, TM_AREA_MAX_LIMIT = 254;

// The static summary of the table.  off [n_act + 1][3]: first line word, first substation record, first line-end candidate of every
// entry (an ambiguous entry has none).  line: one word per line the entry can put into aff_lines (status item, or set_bus != 0 on an
// end).  sub [][2]: one record per substation the entry can put into aff_subs = {substation word, number of its line-end
// candidates}; the candidates of an entry's records follow each other in `end`.  end: line words (with TM_END) of the line ends
// that carry an "effective change" (set_bus != 0 or change_bus): the change counts unless the line's own impact clears it.
struct TopoMaskTab { const int* off; const int* line; const int* sub; const int* end; const unsigned char* amb; int n_act; };

GPF_TM_HD inline bool tm_bit(const unsigned long long* w, int i) { return (w[i >> 6] >> (i & 63)) & 1ull; }

// get_topological_impact of one line: in service `st` -> (in aff_lines, clears the effective changes of its two ends)
GPF_TM_HD inline void tm_line_impact(int w, bool st, bool& im, bool& clr) {
  const bool notc = !st;
  im = (w & TM_STATUS) != 0;
  clr = im && notc;
  const bool hit = ((w & (TM_OR_POS | TM_EX_POS)) && notc) || ((w & (TM_OR_NEG | TM_EX_NEG)) && st);
  im = im || hit;
  clr = clr || hit;
}

// The two counters of the limits: one count over the whole grid, or one per area.  bump(word): a line / substation word is counted
// (in its area, bits 26-29 of the word); over(limit): the count, or some area's, exceeds the limit.
struct TmGridCount {
  int n = 0;
  GPF_TM_HD void bump(int) { ++n; }
  GPF_TM_HD bool over(int limit) const { return n > limit; }
};
// Sixteen saturating 8-bit counters in two 64-bit words: counter k is byte k & 7 of word k >> 3 (limit <= TM_AREA_MAX_LIMIT: exact).
struct TmAreaCount {
  unsigned long long lo = 0, hi = 0;
  GPF_TM_HD void bump(int word) {
    const int area = (word >> TM_AREA_SHIFT) & (TM_MAX_AREAS - 1), sh = (area & 7) * 8;
    const bool up = (area & 8) != 0;
    const unsigned long long w = up ? hi : lo;
    const unsigned long long nw = ((w >> sh) & 0xFFull) != 0xFFull ? w + (1ull << sh) : w;
    if (up) hi = nw; else lo = nw;
  }
  GPF_TM_HD bool over(int limit) const {
    bool o = false;
    for (int k = 0; k < 8; ++k) o = o || (int)((lo >> (8 * k)) & 0xFFull) > limit || (int)((hi >> (8 * k)) & 0xFFull) > limit;
    return o;
  }
};

// The rules of a mask byte, stated once for both counters: entry `a` (not ambiguous) of one lane under rules that are on.
template <class Count>
GPF_TM_HD inline unsigned topo_mask_rules(const TopoMaskTab& t, int a, const unsigned long long* live, const unsigned long long* line_cd,
                                          const unsigned long long* sub_cd, int max_line, int max_sub) {
  unsigned m = 0;
  Count n_lines, n_subs;
  const int* o = t.off + 3 * a;
  for (int q = o[0]; q < o[3]; ++q) {
    const int w = t.line[q], l = w & TM_LINE_MASK;
    bool im, clr;
    tm_line_impact(w, tm_bit(live, l), im, clr);
    if (im) { n_lines.bump(w); if (tm_bit(line_cd, l)) m |= TM_LINE_COOLDOWN; }
  }
  int c = o[2];
  for (int q = o[1]; q < o[4]; ++q) {
    const int w = t.sub[2 * q], nc = t.sub[2 * q + 1];
    bool aff = (w & TM_SUB_ALWAYS) != 0;
    for (int k = 0; k < nc; ++k) {
      const int e = t.end[c + k];
      bool im, clr;
      tm_line_impact(e, tm_bit(live, e & TM_LINE_MASK), im, clr);
      aff = aff || !clr;
    }
    c += nc;
    if (aff) { n_subs.bump(w); if (tm_bit(sub_cd, w & TM_LINE_MASK)) m |= TM_SUB_COOLDOWN; }
  }
  if (n_lines.over(max_line)) m |= TM_TOO_MANY_LINES;
  if (n_subs.over(max_sub)) m |= TM_TOO_MANY_SUBS;
  return m;
}

// The mask byte of entry `a` for one lane.  live / line_cd / sub_cd: the lane's bit sets (line in service = both ends > 0, line
// cooldown > 0, substation cooldown > 0; bit i of word i / 64).  rules_on = 0: AlwaysLegal.
GPF_TM_HD inline unsigned topo_mask_eval(const TopoMaskTab& t, int a, const unsigned long long* live, const unsigned long long* line_cd,
                                         const unsigned long long* sub_cd, int rules_on, int max_line, int max_sub) {
  if (t.amb[a]) return TM_AMBIGUOUS;
  if (!rules_on) return 0;
  return topo_mask_rules<TmGridCount>(t, a, live, line_cd, sub_cd, max_line, max_sub);
}

// The same byte with the two limits held per area (rules on; the words of `t` carry their areas): TOO_MANY_LINES / TOO_MANY_SUBS mean
// "in some area".  max_line, max_sub <= TM_AREA_MAX_LIMIT.
GPF_TM_HD inline unsigned topo_mask_eval_area(const TopoMaskTab& t, int a, const unsigned long long* live, const unsigned long long* line_cd,
                                              const unsigned long long* sub_cd, int max_line, int max_sub) {
  if (t.amb[a]) return TM_AMBIGUOUS;
  return topo_mask_rules<TmAreaCount>(t, a, live, line_cd, sub_cd, max_line, max_sub);
}

// The ambiguity rules of the topology kinds (BaseAction._check_for_ambiguity, Action/baseAction.py:3668-3760) on the dense arrays of one
// action -- setv [dim_topo] set_bus value, chg [dim_topo] change_bus, setl [n_line] set_line_status value, swl [n_line]
// change_line_status, each filled item by item (a later item of a position / line replaces an earlier one).  The ONE statement of these
// rules: run per table entry at upload (topo_static_ambiguity) and per lane on a composite action (topo_prestep_kernel, gridpf_topo.hpp).
// Looks at positions and lines tid, tid + nth, ...; the action is ambiguous when any of the nth calls says so.
GPF_TM_HD inline bool topo_dense_ambiguity(int dim_topo, int n_line, const int* or_pos, const int* ex_pos, const int* setv, const int* chg,
                                           const int* setl, const int* swl, int tid, int nth) {
  bool a = false;
  for (int p = tid; p < dim_topo; p += nth) a = a || (chg[p] && setv[p] != 0);              // set_bus and change_bus of one element
  for (int l = tid; l < n_line; l += nth) {
    const int po = or_pos[l], pe = ex_pos[l];
    a = a || (swl[l] && setl[l] != 0)                                                      // set and change of one line status
        || (setv[po] == -1 && setv[pe] > 0) || (setv[pe] == -1 && setv[po] > 0)             // one end set to -1, the other to a bus
        || (setl[l] == -1 && (setv[po] > 0 || setv[pe] > 0 || chg[po] || chg[pe]))           // disconnected and (re)assigned / changed
        || (setl[l] == 1 && (setv[po] == -1 || setv[pe] == -1 || chg[po] || chg[pe]));       // reconnected and disconnected / changed
  }
  return a;
}

// ---- host: static ambiguity + summary of a table, once per upload ---------------------------------------------------------------

struct TopoMaskGrid { int dim_topo, n_line, n_sub; const int* or_pos; const int* ex_pos; const int* pos_sub; };

// static ambiguity of every entry (BaseAction._check_for_ambiguity, Action/baseAction.py:3668-3760 -- the topology kinds)
inline void topo_static_ambiguity(const TopoMaskGrid& g, int n_act, const int* act_off, const int* act_items, unsigned char* amb) {
  std::vector<int> setv(g.dim_topo), chg(g.dim_topo), setl(g.n_line), swl(g.n_line);
  for (int k = 0; k < n_act; ++k) {
    std::fill(setv.begin(), setv.end(), 0); std::fill(chg.begin(), chg.end(), 0); std::fill(setl.begin(), setl.end(), 0); std::fill(swl.begin(), swl.end(), 0);
    for (int q = act_off[k]; q < act_off[k + 1]; ++q) {
      const int kind = act_items[3 * q], id = act_items[3 * q + 1], v = act_items[3 * q + 2];
      if (kind == TM_SET_BUS) setv[id] = v;
      else if (kind == TM_CHANGE_BUS) chg[id] = 1;
      else if (kind == TM_SET_LINE_STATUS) setl[id] = v;
      else if (kind == TM_CHANGE_LINE_STATUS) swl[id] = 1;
    }
    const bool a = topo_dense_ambiguity(g.dim_topo, g.n_line, g.or_pos, g.ex_pos, setv.data(), chg.data(), setl.data(), swl.data(), 0, 1);
    amb[k] = a ? 1 : 0;
  }
}

struct TopoMaskSummary {
  std::vector<int> off, line, sub, end;
  TopoMaskTab tab(const unsigned char* amb, int n_act) const { return TopoMaskTab{off.data(), line.data(), sub.data(), end.data(), amb, n_act}; }
};

// The dense per-entry arrays are those of step 2 of topo_prestep_kernel, filled item by item in the same way (a later set_bus of a
// position replaces an earlier one; a line-status item with a value != 0 marks its line for good).  false: a line or substation id
// does not fit the 20 bits of a word.  sub_area [n_sub] (NULL: no areas): the area, < TM_MAX_AREAS, every line word and substation word
// carries (a line: its origin substation's).
inline bool build_topo_mask_summary(const TopoMaskGrid& g, int n_act, const int* act_off, const int* act_items, const unsigned char* amb,
                                    TopoMaskSummary& s, const int* sub_area = nullptr) {
  if (g.n_line > TM_LINE_MASK || g.n_sub > TM_LINE_MASK) return false;
  std::vector<int> setv(g.dim_topo, 0), eff(g.dim_topo, 0), imp(g.n_line, 0), other(g.dim_topo, -1), line_of(g.dim_topo, -1);
  for (int l = 0; l < g.n_line; ++l) {
    other[g.or_pos[l]] = g.ex_pos[l]; other[g.ex_pos[l]] = g.or_pos[l];
    line_of[g.or_pos[l]] = l; line_of[g.ex_pos[l]] = l;
  }
  s.off.assign(3 * ((size_t)n_act + 1), 0); s.line.clear(); s.sub.clear(); s.end.clear();
  std::vector<int> lines, poss;                              // lines / positions the entry's items name
  std::vector<std::pair<int, int>> cand;                     // (substation, line word of a line-end candidate or -1: always)
  for (int a = 0; a < n_act; ++a) {
    s.off[3 * a] = (int)s.line.size(); s.off[3 * a + 1] = (int)(s.sub.size() / 2); s.off[3 * a + 2] = (int)s.end.size();
    if (amb[a]) continue;
    lines.clear(); poss.clear(); cand.clear();
    for (int q = act_off[a]; q < act_off[a + 1]; ++q) {
      const int kind = act_items[3 * q], id = act_items[3 * q + 1], v = act_items[3 * q + 2];
      if (kind == TM_SET_BUS) { setv[id] = v; poss.push_back(id); }
      else if (kind == TM_CHANGE_BUS) { eff[id] = 1; poss.push_back(id); }
      else if (kind == TM_CHANGE_LINE_STATUS || (kind == TM_SET_LINE_STATUS && v != 0)) { imp[id] = 1; lines.push_back(id); }
    }
    for (int p : poss) { if (setv[p] != 0) eff[p] = 1; if (line_of[p] >= 0) lines.push_back(line_of[p]); }
    std::sort(lines.begin(), lines.end()); lines.erase(std::unique(lines.begin(), lines.end()), lines.end());
    std::sort(poss.begin(), poss.end()); poss.erase(std::unique(poss.begin(), poss.end()), poss.end());
    auto word = [&](int l) {
      const int po = g.or_pos[l], pe = g.ex_pos[l];
      return l | (imp[l] ? TM_STATUS : 0) | (setv[po] > 0 ? TM_OR_POS : 0) | (setv[po] < 0 ? TM_OR_NEG : 0) | (setv[pe] > 0 ? TM_EX_POS : 0) |
             (setv[pe] < 0 ? TM_EX_NEG : 0);
    };
    auto area = [&](int sub) { return sub_area ? sub_area[sub] << TM_AREA_SHIFT : 0; };
    for (int l : lines) { const int w = word(l); if (w & ~TM_LINE_MASK) s.line.push_back(w | area(g.pos_sub[g.or_pos[l]])); }
    for (int p : poss) if (eff[p]) {
      const int l = line_of[p];
      cand.emplace_back(g.pos_sub[p], l < 0 ? -1 : word(l) | (p == g.ex_pos[l] ? TM_END : 0));
    }
    std::sort(cand.begin(), cand.end());
    for (size_t i = 0; i < cand.size();) {
      size_t j = i;
      int always = 0, n_end = 0;
      for (; j < cand.size() && cand[j].first == cand[i].first; ++j) {
        if (cand[j].second < 0) always = TM_SUB_ALWAYS; else { s.end.push_back(cand[j].second); ++n_end; }
      }
      s.sub.push_back(cand[i].first | always | area(cand[i].first)); s.sub.push_back(n_end);
      i = j;
    }
    for (int p : poss) { setv[p] = 0; eff[p] = 0; }
    for (int l : lines) imp[l] = 0;
  }
  s.off[3 * (size_t)n_act] = (int)s.line.size(); s.off[3 * (size_t)n_act + 1] = (int)(s.sub.size() / 2); s.off[3 * (size_t)n_act + 2] = (int)s.end.size();
  return true;
}

// Bit k of areas[a]: entry `a` can touch area k -- the area of every substation it names and of BOTH end substations of every line it
// names (a status item, or a set_bus / change_bus on a line end), ambiguous entries included.  sub_area NULL: one area, bit 0.
// shunt_sub [n_shunt] (may be NULL: shunt items are skipped).
inline void topo_action_areas(const TopoMaskGrid& g, int n_act, const int* act_off, const int* act_items, const int* sub_area,
                              const int* shunt_sub, unsigned* areas) {
  std::vector<int> line_of(g.dim_topo, -1);
  for (int l = 0; l < g.n_line; ++l) { line_of[g.or_pos[l]] = l; line_of[g.ex_pos[l]] = l; }
  auto bit = [&](int sub) { return 1u << (sub_area ? sub_area[sub] : 0); };
  auto ends = [&](int l) { return bit(g.pos_sub[g.or_pos[l]]) | bit(g.pos_sub[g.ex_pos[l]]); };
  for (int a = 0; a < n_act; ++a) {
    unsigned m = 0;
    for (int q = act_off[a]; q < act_off[a + 1]; ++q) {
      const int kind = act_items[3 * q], id = act_items[3 * q + 1];
      if (kind == TM_SET_BUS || kind == TM_CHANGE_BUS) { m |= bit(g.pos_sub[id]); if (line_of[id] >= 0) m |= ends(line_of[id]); }
      else if (kind == TM_SET_LINE_STATUS || kind == TM_CHANGE_LINE_STATUS) m |= ends(id);
      else if (shunt_sub) m |= bit(shunt_sub[id]);
    }
    areas[a] = m;
  }
}

// 64-bit words of a bit set over n elements
GPF_TM_HD inline int tm_words(int n) { return (n + 63) >> 6; }

#if defined(__HIPCC__) && defined(GPF_TOPO_KERNEL)
// the lane rows and grid maps the kernel reads (line_cd may be NULL: no line cooldowns, all zero)
struct TopoMaskLanes {
  const int* topo; const int* line_cd; const int* sub_cd; const int* or_pos; const int* ex_pos;
  int dim_topo, n_line, n_sub;
};

constexpr int TM_CHUNK = 256;      // table entries of one wavefront (4 per thread): the lane's bit sets are rebuilt per chunk

// One wavefront per (lane, chunk of TM_CHUNK entries): blockIdx.x = lane - lane0, blockIdx.y strides over the chunks.  The lane's state
// is reduced once to three bit sets in LDS (one __ballot per 64 lines / substations), thread t then evaluates entries t, t + 64, ...
// of the chunk, so that the wavefront's 64 byte stores to the lane's row are contiguous.  Dynamic LDS: (2 * tm_words(n_line) +
// tm_words(n_sub)) * 8 bytes.  Reads only; writes bytes [0, n_act) of rows [0, n) of `out`.  by_area (uniform): the rules are on and
// areas are set -- the limits hold per area.
__global__ __launch_bounds__(64) void topo_mask_kernel(TopoMaskTab tab, TopoMaskLanes s, int rules_on, int max_line, int max_sub, int lane0,
                                                       int n, unsigned char* __restrict__ out, long long row_stride, int by_area) {
  extern __shared__ unsigned long long tm_sets[];
  const int k = blockIdx.x, tid = threadIdx.x;
  if (k >= n) return;
  const size_t lane = (size_t)lane0 + k;
  const int L = s.n_line, S = s.n_sub, wl = tm_words(L), ws = tm_words(S);
  unsigned long long* live = tm_sets;
  unsigned long long* lcd = live + wl;
  unsigned long long* scd = lcd + wl;
  const int* trow = s.topo + lane * s.dim_topo;
  for (int c = 0; c < wl; ++c) {
    const int l = c * 64 + tid;
    bool st = false, cd = false;
    if (l < L) {
      st = trow[s.or_pos[l]] > 0 && trow[s.ex_pos[l]] > 0;
      cd = s.line_cd && s.line_cd[lane * L + l] > 0;
    }
    const unsigned long long b0 = __ballot(st), b1 = __ballot(cd);
    if (tid == 0) { live[c] = b0; lcd[c] = b1; }
  }
  for (int c = 0; c < ws; ++c) {
    const int i = c * 64 + tid;
    const unsigned long long b = __ballot(i < S && s.sub_cd[lane * S + i] > 0);
    if (tid == 0) scd[c] = b;
  }
  __syncthreads();
  unsigned char* orow = out + (long long)k * row_stride;
  for (long long a0 = (long long)blockIdx.y * TM_CHUNK; a0 < tab.n_act; a0 += (long long)gridDim.y * TM_CHUNK) {
    const int a1 = (int)(a0 + TM_CHUNK < tab.n_act ? a0 + TM_CHUNK : tab.n_act);
    if (by_area)
      for (int a = (int)a0 + tid; a < a1; a += 64) orow[a] = (unsigned char)topo_mask_eval_area(tab, a, live, lcd, scd, max_line, max_sub);
    else
      for (int a = (int)a0 + tid; a < a1; a += 64) orow[a] = (unsigned char)topo_mask_eval(tab, a, live, lcd, scd, rules_on, max_line, max_sub);
  }
}
#endif  // __HIPCC__ && GPF_TOPO_KERNEL

}  // namespace gpf
