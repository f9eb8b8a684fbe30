// gridpf_lane_fan.hpp -- the lane split the N-1 screen and the look-ahead share, and the host half of a moved-lane list's read-back.
// Plain C++, nothing of HIP: tests/native/lane_fan_main.cpp is built from it with g++ alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

enum class FanOwner { none, n1_screen, lookahead };

// Lanes [0, n_env) are environments, lane n_env + i K + k is secondary lane (i, k): contingency k of environment i for the N-1 screen,
// scratch lane (i, k) for the look-ahead.  One feature at a time owns the lanes behind the environments; host_only: that is only
// recorded, on a header-only handle (every refusal holds there, nothing runs).  Each of the two ranges has a launch plan pair and three
// device lane lists of its own (LaunchPlan and DevArr<int> in the engine); the plans hold while the batch's plan_valid and plans_valid
// both hold, and plans_gen counts how often they were made anew.
template <class Plan, class List>
struct LaneFanT {
  struct Range { Plan p{}, pb{}; List lists[3]; };
  FanOwner owner = FanOwner::none;
  bool host_only = false, plans_valid = false;
  int n_env = 0, K = 0;
  long long plans_gen = 0;
  Range env, sec;

  int n_sec() const { return n_env * K; }
  int lane(int i, int k) const { return n_env + i * K + k; }
  bool owned_by(FanOwner o) const { return owner == o; }                 // on, or recorded on a header-only handle
  bool on(FanOwner o) const { return owner == o && !host_only; }
  bool on() const { return owner != FanOwner::none && !host_only; }
  void claim(FanOwner o, int n_env_, int K_, bool host_only_) { owner = o; n_env = n_env_; K = K_; host_only = host_only_; plans_valid = false; }
  void release() {
    for (int i = 0; i < 3; ++i) { env.lists[i].release(); sec.lists[i].release(); }
    claim(FanOwner::none, 0, 0, false);
  }
};

// A moved-lane list as the host fetched it: `count | lane ids [cap] | rows [cap][w]`, cap = lane_hi - lane_lo.  The kernels append in any
// order; the host notes the lanes in lane order, so that topology classes are created in the order gpf_set_topology would create them.
enum { MOVED_OK = 0, MOVED_BAD_COUNT = 1, MOVED_BAD_LANE = 2 };

inline bool moved_list_count_ok(int cnt, int lane_lo, int lane_hi) { return cnt <= lane_hi - lane_lo; }

// note(lane, row) for every listed lane, ascending; nothing is noted unless the count fits and every id is in [lane_lo, lane_hi)
template <class F>
int moved_list_visit(const int* block, size_t w, int lane_lo, int lane_hi, F&& note) {
  const int cnt = block[0];
  if (cnt <= 0) return MOVED_OK;
  if (!moved_list_count_ok(cnt, lane_lo, lane_hi)) return MOVED_BAD_COUNT;
  const int* ids = block + 1;
  const int* rows = ids + (lane_hi - lane_lo);
  std::vector<int> order(cnt);
  for (int i = 0; i < cnt; ++i) {
    if (ids[i] < lane_lo || ids[i] >= lane_hi) return MOVED_BAD_LANE;
    order[i] = i;
  }
  std::sort(order.begin(), order.end(), [ids](int a, int b) { return ids[a] < ids[b]; });
  for (int i : order) note(ids[i], rows + (size_t)i * w);
  return MOVED_OK;
}
