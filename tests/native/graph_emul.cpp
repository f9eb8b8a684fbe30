// graph_emul.cpp -- the rule core of grid2op_amd/csrc/gridpf_graph.hpp behind loops, compiled with g++ (no HIP): the shared library
// tests/graph_ref.py loads, and with -DGRAPH_EMUL_MAIN a stand-alone program for -fsanitize=address,undefined that drives random
// topologies of a small ring grid (open lines, split substations, elements alone on a busbar, parallel lines) on exactly sized arrays.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_graph.hpp"

extern "C" {

// one lane.  dims = {n_sub, n_busbar, n_load, n_gen, n_sto, n_line, n_shunt, dim_topo}; out_off = the 13 columns of the results row in
// the order p_or q_or v_or p_ex q_ex v_ex gen_p gen_q load_p load_q storage_p shunt_p shunt_q; sub_cd may be null.
// Writes idx [index width], feat [NB][4], dense [3][NB][NB] (may be null).
void graph_emul_lane(const int* dims, const int* load_sub, const int* load_pos, const int* gen_sub, const int* gen_pos, const int* sto_sub,
                     const int* sto_pos, const int* lor_sub, const int* lor_pos, const int* lex_sub, const int* lex_pos, const int* shunt_sub,
                     const int* out_off, const int* topo, const int* shunt_bus, const float* out, const int* sub_cd, int over, int* idx,
                     float* feat, float* dense) {
  gpf::GraphGrid g{};
  g.n_sub = dims[0]; g.n_busbar = dims[1]; g.n_load = dims[2]; g.n_gen = dims[3]; g.n_sto = dims[4]; g.n_line = dims[5]; g.n_shunt = dims[6];
  g.dim_topo = dims[7];
  g.load_sub = load_sub; g.load_pos = load_pos; g.gen_sub = gen_sub; g.gen_pos = gen_pos; g.sto_sub = sto_sub; g.sto_pos = sto_pos;
  g.lor_sub = lor_sub; g.lor_pos = lor_pos; g.lex_sub = lex_sub; g.lex_pos = lex_pos; g.shunt_sub = shunt_sub;
  g.o_p_or = out_off[0]; g.o_q_or = out_off[1]; g.o_v_or = out_off[2]; g.o_p_ex = out_off[3]; g.o_q_ex = out_off[4]; g.o_v_ex = out_off[5];
  g.o_gen_p = out_off[6]; g.o_gen_q = out_off[7]; g.o_load_p = out_off[8]; g.o_load_q = out_off[9]; g.o_sto_p = out_off[10];
  g.o_sh_p = out_off[11]; g.o_sh_q = out_off[12];
  const std::vector<int> blob = gpf::graph_build_tab(g);
  const gpf::GraphTab T = gpf::graph_tab_view(blob.data(), blob.data());
  const gpf::GraphRow r{topo, shunt_bus, out, sub_cd};
  gpf::graph_lane_serial(T, r, over != 0, idx, feat, dense);
}

}  // extern "C"

#ifdef GRAPH_EMUL_MAIN
int main() {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  auto unif = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(next() >> 11) / 9007199254740992.0); };
  long checks = 0;
  for (int ns : {2, 5, 33, 70})
    for (int nbb : {1, 2, 3}) {
      // a ring of ns substations with one parallel line on the first pair (reversed), one load and one generator per substation, a
      // storage unit and a shunt on every third; topo_vect: per substation load, gen, [storage], the line ends
      const int nl = ns + 1, n_load = ns, n_gen = ns, n_sto = (ns + 2) / 3, n_sh = n_sto;
      std::vector<int> load_sub(n_load), load_pos(n_load), gen_sub(n_gen), gen_pos(n_gen), sto_sub(n_sto), sto_pos(n_sto), sh_sub(n_sh);
      std::vector<int> lor_sub(nl), lex_sub(nl), lor_pos(nl), lex_pos(nl);
      for (int l = 0; l < ns; ++l) { lor_sub[l] = l; lex_sub[l] = (l + 1) % ns; }
      lor_sub[ns] = 1 % ns; lex_sub[ns] = 0;
      int pos = 0;
      for (int s = 0; s < ns; ++s) {
        load_sub[s] = s; load_pos[s] = pos++; gen_sub[s] = s; gen_pos[s] = pos++;
        if (s % 3 == 0) { sto_sub[s / 3] = s; sto_pos[s / 3] = pos++; sh_sub[s / 3] = s; }
        for (int l = 0; l < nl; ++l) { if (lor_sub[l] == s) lor_pos[l] = pos++; if (lex_sub[l] == s) lex_pos[l] = pos++; }
      }
      const int dim_topo = pos, nb = ns * nbb;
      const int dims[8] = {ns, nbb, n_load, n_gen, n_sto, nl, n_sh, dim_topo};
      int off[13], at = 0;
      const int w[13] = {nl, nl, nl, nl, nl, nl, n_gen, n_gen, n_load, n_load, n_sto, n_sh, n_sh};
      for (int i = 0; i < 13; ++i) { off[i] = at; at += w[i]; }
      const int width = 1 + n_load + n_gen + n_sto + 2 * nl + n_sh + nb;
      for (int rep = 0; rep < 24; ++rep) {
        // exactly sized rows: a read or write past an array is a sanitizer report
        std::vector<int> topo(dim_topo), shb(n_sh), cd(ns), idx(width);
        std::vector<float> out(at), feat((size_t)nb * 4), dense((size_t)3 * nb * nb);
        for (auto& t : topo) t = (int)(next() % 11 == 0 ? -1 : 1 + next() % nbb);
        for (int l = 0; l < nl; ++l) if (topo[lor_pos[l]] < 0 || topo[lex_pos[l]] < 0) topo[lor_pos[l]] = topo[lex_pos[l]] = -1;
        for (auto& b : shb) b = (int)(next() % 5 == 0 ? -1 : 1 + next() % nbb);
        for (auto& c : cd) c = (int)(next() % 4);
        for (auto& x : out) x = unif(-90, 90);
        graph_emul_lane(dims, load_sub.data(), load_pos.data(), gen_sub.data(), gen_pos.data(), sto_sub.data(), sto_pos.data(), lor_sub.data(),
                        lor_pos.data(), lex_sub.data(), lex_pos.data(), sh_sub.data(), off, topo.data(), shb.data(), out.data(),
                        rep % 2 ? cd.data() : nullptr, rep % 12 == 11, idx.data(), feat.data(), rep % 3 ? dense.data() : nullptr);
        const int n_bus = idx[0];
        if (n_bus < 0 || n_bus > nb) { std::printf("FAIL: n_bus\n"); return 1; }
        for (int i = 1; i < width - nb; ++i) if (idx[i] < -1 || idx[i] >= n_bus) { std::printf("FAIL: compact id out of range\n"); return 1; }
        for (int k = 0; k < nb; ++k) {
          const int g = idx[width - nb + k];
          if ((k < n_bus) != (g >= 0) || g >= nb || (k > 0 && k < n_bus && g <= idx[width - nb + k - 1])) { std::printf("FAIL: bus_global\n"); return 1; }
        }
        for (float x : feat) if (!std::isfinite(x)) { std::printf("FAIL: feature\n"); return 1; }
        ++checks;
      }
    }
  std::printf("OK %ld lanes\n", checks);
  return 0;
}
#endif
