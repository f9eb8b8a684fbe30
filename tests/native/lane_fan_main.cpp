// lane_fan_main.cpp -- the host-only half of the lane fan (grid2op_amd/csrc/gridpf_lane_fan.hpp): the split's index arithmetic and what a
// fetched moved-lane list yields.  Stand-alone program, plain C++:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/lane_fan_main.cpp -o lane_fan && ./lane_fan
#include <cstdio>
#include <utility>
#include <vector>

#include "../../grid2op_amd/csrc/gridpf_lane_fan.hpp"

namespace {

int bad = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAIL %s\n", what); ++bad; }
}

struct List { bool held = false; void release() { held = false; } };      // stands in for the engine's device lane lists
using Fan = LaneFanT<int, List>;

void fan_arithmetic(int n_env, int K) {
  Fan f;
  expect(!f.on() && f.owned_by(FanOwner::none) && f.n_sec() == 0, "a new fan is nobody's");
  f.plans_valid = true;
  f.claim(FanOwner::n1_screen, n_env, K, false);
  expect(f.on() && f.on(FanOwner::n1_screen) && !f.on(FanOwner::lookahead) && !f.plans_valid, "claimed: on, plans to be made");
  expect(f.n_sec() == n_env * K, "n_sec");
  std::vector<char> seen((size_t)n_env + f.n_sec(), 0);      // every lane behind the environments is exactly one (i, k), in order
  int next = n_env;
  for (int i = 0; i < n_env; ++i)
    for (int k = 0; k < K; ++k) {
      const int lane = f.lane(i, k);
      expect(lane == next++, "lanes of (i, k) are consecutive");
      expect(lane >= n_env && lane < n_env + f.n_sec() && !seen[lane], "lane(i, k) in range, once");
      seen[lane] = 1;
    }
  expect(next == n_env + f.n_sec(), "the secondary range is covered");
  f.claim(FanOwner::lookahead, n_env, K, true);
  expect(!f.on() && !f.on(FanOwner::lookahead) && f.owned_by(FanOwner::lookahead), "recorded on a header-only handle: owned, not on");
  f.env.lists[0].held = f.sec.lists[2].held = true;
  f.release();
  expect(f.owned_by(FanOwner::none) && f.n_env == 0 && f.K == 0 && !f.host_only, "released");
  expect(!f.env.lists[0].held && !f.sec.lists[2].held, "... with its lane lists");
}

// a fetched block `count | ids [cap] | rows [cap][w]` for lanes [lo, hi); row i holds 100 * ids[i] + column
std::vector<int> block_of(int cnt, const std::vector<int>& ids, int lo, int hi, int w) {
  const int cap = hi - lo;
  std::vector<int> b(1 + (size_t)cap + (size_t)cap * w, -7);
  b[0] = cnt;
  for (size_t i = 0; i < ids.size(); ++i) {
    b[1 + i] = ids[i];
    for (int c = 0; c < w; ++c) b[1 + cap + i * w + c] = 100 * ids[i] + c;
  }
  return b;
}

using Noted = std::vector<std::pair<int, int>>;      // (lane, first element of its row)
int visit(const std::vector<int>& block, int w, int lo, int hi, Noted& noted) {
  return moved_list_visit(block.data(), (size_t)w, lo, hi, [&](int lane, const int* row) {
    for (int c = 0; c < w; ++c) expect(row[c] == 100 * lane + c, "a lane comes with its own row");
    noted.emplace_back(lane, row[0]);
  });
}

}  // namespace

int main() {
  fan_arithmetic(1, 1);
  fan_arithmetic(3, 2);
  fan_arithmetic(2, 64);

  const int lo = 3, hi = 9, w = 5;
  {
    Noted n;
    expect(visit(block_of(3, {8, 5, 3}, lo, hi, w), w, lo, hi, n) == MOVED_OK, "three ids in descending order are accepted");
    expect(n == Noted{{3, 300}, {5, 500}, {8, 800}}, "... and come out ascending");
  }
  {
    Noted n;
    expect(visit(block_of(0, {}, lo, hi, w), w, lo, hi, n) == MOVED_OK && n.empty(), "an empty list notes nothing");
  }
  {
    Noted n;
    expect(!moved_list_count_ok(hi - lo + 1, lo, hi) && moved_list_count_ok(hi - lo, lo, hi), "the capacity is the number of lanes of the range");
    expect(visit(block_of(hi - lo + 1, {3, 4}, lo, hi, w), w, lo, hi, n) == MOVED_BAD_COUNT && n.empty(), "a count above the capacity is refused");
  }
  {
    Noted n;
    expect(visit(block_of(3, {4, 2, 5}, lo, hi, w), w, lo, hi, n) == MOVED_BAD_LANE && n.empty(), "an id below lane_lo is refused, nothing noted");
  }
  {
    Noted n;
    expect(visit(block_of(3, {4, 5, 9}, lo, hi, w), w, lo, hi, n) == MOVED_BAD_LANE && n.empty(), "an id equal to lane_hi is refused, nothing noted");
  }
  std::printf("%s\n", bad ? "FAILED" : "ok: lane fan");
  return bad ? 1 : 0;
}
