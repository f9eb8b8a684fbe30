// step_features_main.cpp -- table-driven check of the host function that computes the launch-feature word of a step launch
// (grid2op_amd/csrc/gridpf_host.hpp: gpf_step_features; bits: gridpf_common.hpp FEAT_*).  Stand-alone program, host code only:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tests/native/step_features_main.cpp -o step_features && ./step_features
// The headline launch description (bench.py: contiguous lanes, jitter, rebalancing, observation trajectory on, nothing else) sets every
// bit; for every bit, the one change of the description that violates its assumption clears exactly that bit.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_host.hpp"

namespace {

struct Launch {
  gpf::StepArgs sa;
  gpf::DevParamsS hp;
  const int* list;
  int n_l, ipw;
};

template <class T>
T* some() { static long long cell[2]; return reinterpret_cast<T*>(cell); }     // a pointer that is not null (never dereferenced)

Launch headline() {
  Launch L;
  std::memset(&L.sa, 0, sizeof L.sa);
  std::memset(&L.hp, 0, sizeof L.hp);
  L.sa.t = 3; L.sa.T = 288; L.sa.rebalance_on = 1; L.sa.rebalance = 1.02; L.sa.nb_ts_allowed = 2; L.sa.max_rounds = 16; L.sa.lane0 = 0;
  L.sa.n_steps = 16; L.sa.nb_ts_reco = -1; L.sa.hard_overflow = 2.f; L.sa.soft_overflow = 1.f;
  gpf::Bufs& b = L.hp.b;
  b.lane_scale = some<const float>();
  b.traj_out = some<float>(); b.traj_topo = some<int>(); b.traj_shb = some<int>(); b.traj_lstat = some<unsigned char>();
  b.traj_rho = some<float>(); b.traj_status = some<signed char>(); b.traj_cap = 16;
  b.lane_stride = 4100; b.n_real_lanes = 4096;
  L.hp.dcf = 1;
  L.list = nullptr; L.n_l = 4096; L.ipw = 2;
  return L;
}

struct Case { const char* what; unsigned cleared; std::function<void(Launch&)> change; };

}  // namespace

int main() {
  static const int lanes[4] = {0, 1, 2, 3};
  const std::vector<Case> cases = {
      {"cascade on", gpf::FEAT_NO_CASCADE, [](Launch& L) { L.sa.cascade = 1; }},
      {"auto-reset on", gpf::FEAT_NO_AUTO_RESET, [](Launch& L) { L.sa.auto_reset = 1; }},
      {"warm start on", gpf::FEAT_COLD_START, [](Launch& L) { L.sa.warm_start = 1; }},
      {"DC step", gpf::FEAT_AC, [](Launch& L) { L.sa.is_dc = 1; }},
      {"cooldowns maintained (0 steps)", gpf::FEAT_NO_COOLDOWN, [](Launch& L) { L.sa.nb_ts_reco = 0; }},
      {"cooldowns maintained (10 steps)", gpf::FEAT_NO_COOLDOWN, [](Launch& L) { L.sa.nb_ts_reco = 10; }},
      {"no rebalancing", gpf::FEAT_REBALANCE, [](Launch& L) { L.sa.rebalance_on = 0; }},
      {"kept state", gpf::FEAT_NO_KEEP, [](Launch& L) { L.sa.keep.p = some<unsigned char>(); }},
      {"lane list", gpf::FEAT_CONTIGUOUS | gpf::FEAT_NO_GHOST, [](Launch& L) { L.list = lanes; L.n_l = 4; }},
      {"maintenance table", gpf::FEAT_NO_MAINT, [](Launch& L) { L.hp.b.maint = some<const unsigned char>(); }},
      {"outage durations alone", gpf::FEAT_NO_MAINT, [](Launch& L) { L.hp.b.maint_dur = some<const unsigned short>(); }},
      {"redispatch delta", gpf::FEAT_NO_GEN_DELTA, [](Launch& L) { L.hp.b.lane_gen_delta = some<const float>(); }},
      {"no jitter", gpf::FEAT_LANE_SCALE, [](Launch& L) { L.hp.b.lane_scale = nullptr; }},
      {"trajectory off", gpf::FEAT_TRAJ_OBS, [](Launch& L) {
         gpf::Bufs& b = L.hp.b;
         b.traj_out = nullptr; b.traj_topo = nullptr; b.traj_shb = nullptr; b.traj_lstat = nullptr; b.traj_rho = nullptr; b.traj_status = nullptr; b.traj_cap = 0; }},
      {"rho / status trajectory only", gpf::FEAT_TRAJ_OBS, [](Launch& L) {
         gpf::Bufs& b = L.hp.b; b.traj_out = nullptr; b.traj_topo = nullptr; b.traj_shb = nullptr; b.traj_lstat = nullptr; }},
      {"one trajectory buffer missing", gpf::FEAT_TRAJ_OBS, [](Launch& L) { L.hp.b.traj_lstat = nullptr; }},
      {"more steps than trajectory rows", gpf::FEAT_TRAJ_OBS, [](Launch& L) { L.sa.n_steps = 17; }},
      {"no room for the DC factors", gpf::FEAT_DCF, [](Launch& L) { L.hp.dcf = 0; }},
      {"odd lane count: the last group is padded", gpf::FEAT_NO_GHOST, [](Launch& L) { L.n_l = 4095; L.hp.b.n_real_lanes = 4095; }},
      {"range runs past the real lanes", gpf::FEAT_NO_GHOST, [](Launch& L) { L.sa.lane0 = 2; }},
      {"sub-range inside the real lanes", 0u, [](Launch& L) { L.sa.lane0 = 64; L.n_l = 128; }},
      {"another time index", 0u, [](Launch& L) { L.sa.t = 100; L.sa.n_steps = 4; }},
      {"another rebalancing target", 0u, [](Launch& L) { L.sa.rebalance = 1.05; }},
  };
  int bad = 0;
  const Launch H = headline();
  const unsigned wh = gpf_step_features(H.sa, H.hp, H.list, H.n_l, H.ipw);
  if (wh != gpf::FEAT_ALL) { std::printf("FAIL headline: word %u, expected %u\n", wh, (unsigned)gpf::FEAT_ALL); ++bad; }
  unsigned seen = 0;
  for (const Case& c : cases) {
    Launch L = headline();
    c.change(L);
    const unsigned w = gpf_step_features(L.sa, L.hp, L.list, L.n_l, L.ipw);
    if (w != (gpf::FEAT_ALL & ~c.cleared)) { std::printf("FAIL %s: word %u, expected %u\n", c.what, w, (unsigned)(gpf::FEAT_ALL & ~c.cleared)); ++bad; }
    seen |= c.cleared;
  }
  if (seen != gpf::FEAT_ALL) { std::printf("FAIL: bits %u have no violating case\n", (unsigned)(gpf::FEAT_ALL & ~seen)); ++bad; }
  {                                                               // a launch that assumes nothing
    Launch L = headline();
    for (const Case& c : cases) c.change(L);
    L.sa.lane0 = 2; L.list = lanes;
    const unsigned w = gpf_step_features(L.sa, L.hp, L.list, L.n_l, L.ipw);
    if (w != 0u) { std::printf("FAIL everything on: word %u, expected 0\n", w); ++bad; }
  }
  std::printf("%s: %zu cases, headline word %u\n", bad ? "FAILED" : "ok", cases.size(), wh);
  return bad ? 1 : 0;
}
