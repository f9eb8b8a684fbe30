// gridpf_cursor.hpp -- the chronics cursor of the batched acting path (gpf_set_chronics_cursor, include/gridpf.h): what Environment.reset
// does to the time series, for every lane of a one-step launch that starts an episode.  Paths relative to the reference checkout:
//   the order       Multifolder._order (Chronics/multiFolder.py:361-395: the scenarios left by the filter, shuffled or not) -- CursorCfg::order
//   the next one    Multifolder.next_chronics (:290-295): the next position of _order, wrapping -- the sequential policy of cursor_pick
//   a sampled one   Multifolder.sample_next_chronics (:341-359) with RandomState.choice: probabilities as float32 over their float32 sum,
//                   a float64 cumulative sum over its last entry, one uniform, searchsorted(side="right") -- cursor_search on the cdf the
//                   host built that way
//   a chosen one    env.set_id(k) / env.reset(options={"time serie id": k}) (Environment/environment.py: chronics_handler.tell_id) -- a
//                   next_pos >= 0, honoured under both policies
//   the first row   row 0 of the scenario is the reset observation; options={"init ts": k} starts at row k -- first_row and cursor_offset
// The rule draws from the opponent's generator (philox4x32_10 / opp_philox_u of gridpf_opponent.hpp) on a counter of its own, or from an
// uploaded table of uniforms (the parity path).  Two parts: the rule (plain C++, the ONE statement of it, run by the kernel on one thread
// per lane and by the host emulator of tests/native/) and, for the one unit that defines GPF_CURSOR_KERNEL (gridpf_capi_cursor.hip), the
// kernel.  Without hipcc only the rule exists: the header then needs no HIP header.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GPF_CUR_HD __host__ __device__
#else
#define GPF_CUR_HD
#endif

#include <stdint.h>

#include "gridpf_opponent.hpp"

namespace gpf {

// policies and draw sources (= GPF_CURSOR_* of include/gridpf.h; the sources are the opponent's)
constexpr int CUR_SEQUENTIAL = 0, CUR_SAMPLED = 1;
constexpr int CUR_DRAWS_TABLE = 0, CUR_DRAWS_PHILOX = 1;
// sticky flags of a lane: its draw table was used up (the lane restarted its current scenario); a next_pos written on the device was
// outside [0, n_order) (it was taken modulo n_order)
constexpr int CUR_FLAG_DRAWS_EXHAUSTED = 1, CUR_FLAG_NEXT_POS_WRAPPED = 2;
constexpr int CUR_STATE_INTS = 7;     // rows of gpf_get_cursor_state: {table, offset, pos, next_pos, n_started, draws used, flags}
constexpr uint32_t CUR_PHILOX_STREAM = 0x63757273u;   // fourth counter word: the opponent's is 0, so the streams differ under one seed

struct CursorCfg {
  int n_order;
  const int* order;          // [n_order] table indices, each < the number of uploaded tables
  int policy;
  const double* cdf;         // [n_order] (sampled), non-decreasing, last entry 1
  int source;
  uint32_t seed_lo, seed_hi;
  int lane_base, n_draw;
  int T;                     // rows of a table
};

// one lane's words
struct CursorLane {
  int* table; int* offset;   // lane_table / lane_offset of the engine: what every kernel of the launch reads
  int* pos; int* next_pos; int* n_started; int* draws_used; int* flags;
  const double* draws;       // [n_draw] (table source), or null
  int first_row;             // the row the first launch of an episode reads
  int global_lane;           // lane + lane_base
};

// the offset with which chron_row_index(t, offset, T) (gridpf_common.hpp) is `row`: in [0, T)
GPF_CUR_HD inline int cursor_offset(int row, int t, int T) {
  int off = (int)(((long long)row - (long long)t) % T);
  if (off < 0) off += T;
  return off;
}

// searchsorted(cdf, u, side="right"): the first index whose entry is > u (n - 1 at most: the last entry is 1 and u < 1)
GPF_CUR_HD inline int cursor_search(const double* cdf, int n, double u) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] > u) hi = mid; else lo = mid + 1;
  }
  return lo < n ? lo : n - 1;
}

// the next uniform of the lane's stream; false: the table is used up (sticky flag)
GPF_CUR_HD inline bool cursor_draw(const CursorCfg& c, const CursorLane& L, double& u) {
  if (c.source == CUR_DRAWS_PHILOX) {
    uint32_t x[4] = {(uint32_t)*L.n_started, 0u, (uint32_t)L.global_lane, CUR_PHILOX_STREAM};
    philox4x32_10(x, c.seed_lo, c.seed_hi);
    u = opp_philox_u(x[0], x[1]);
    ++*L.draws_used;
    return true;
  }
  if (!L.draws || *L.draws_used < 0 || *L.draws_used >= c.n_draw) { *L.flags |= CUR_FLAG_DRAWS_EXHAUSTED; return false; }
  u = L.draws[(*L.draws_used)++];
  return true;
}

// the position in `order` of the episode that starts now.  A next_pos >= 0 is taken (sequential: the one after it becomes next_pos;
// sampled: next_pos goes back to -1); without one the sequential policy follows the episode under way and the sampled one draws.
GPF_CUR_HD inline int cursor_pick(const CursorCfg& c, const CursorLane& L) {
  const int n = c.n_order;
  int p = *L.next_pos;
  if (p >= n) { p %= n; *L.flags |= CUR_FLAG_NEXT_POS_WRAPPED; }
  if (c.policy == CUR_SEQUENTIAL) {
    if (p < 0) p = (*L.pos + 1 < 0 ? 0 : *L.pos + 1) % n;
    *L.next_pos = (p + 1) % n;
    return p;
  }
  *L.next_pos = -1;
  if (p >= 0) return p;
  double u;
  if (!cursor_draw(c, L, u)) return *L.pos < 0 ? 0 : *L.pos % n;       // the lane restarts its current scenario
  return cursor_search(c.cdf, n, u);
}

// the ONE statement of the rule: the lane starts an episode in the launch at time index t
GPF_CUR_HD inline void cursor_start(const CursorCfg& c, const CursorLane& L, int t) {
  const int p = cursor_pick(c, L);
  *L.table = c.order[p];
  *L.offset = cursor_offset(L.first_row, t, c.T);
  *L.pos = p;
  ++*L.n_started;
}

#if defined(__HIPCC__) && defined(GPF_CURSOR_KERNEL)
// what the kernel reads and writes (rows padded to the engine's lane capacity)
struct CursorDev {
  const int* episode;                // [lanes][2] {steps survived, resets}: [0] == 0 before the step is an episode start
  const unsigned char* skip;         // [lanes] 1: a scratch lane of gpf_simulate_batch or a contingency lane of gpf_fanout_n1 (left alone)
  int* table; int* offset;           // [lanes] lane_table / lane_offset
  int* pos; int* next_pos; int* n_started; int* draws_used; int* flags;   // [lanes]
  const int* first_row;              // [lanes]
  const double* draws;               // [lanes][n_draw], or null
};

constexpr int CUR_BLOCK = 256;       // lanes (threads) per block

// One thread per lane: three words read by the great majority of lanes, whose episode goes on (episode[lane][0] != 0: early return); a
// lane that starts an episode reads and writes seven words more.  No LDS, no scratch, no barrier, no atomics, plain vector stores.
// Queued first in a one-step launch: the opponent's and the alerts' pre-steps, the step kernel and the observation kernel behind it
// read the lane_table / lane_offset it leaves.
__global__ __launch_bounds__(CUR_BLOCK) void cursor_prestep_kernel(CursorCfg c, CursorDev d, int t, int n_lanes) {
  const int lane = blockIdx.x * CUR_BLOCK + threadIdx.x;
  if (lane >= n_lanes) return;
  if (d.episode[(size_t)lane * 2] != 0 || d.skip[lane]) return;
  CursorLane L;
  L.table = d.table + lane; L.offset = d.offset + lane; L.pos = d.pos + lane; L.next_pos = d.next_pos + lane;
  L.n_started = d.n_started + lane; L.draws_used = d.draws_used + lane; L.flags = d.flags + lane;
  L.draws = d.draws ? d.draws + (size_t)lane * c.n_draw : nullptr;
  L.first_row = d.first_row[lane];
  L.global_lane = lane + c.lane_base;
  cursor_start(c, L, t);
}
#endif  // __HIPCC__ && GPF_CURSOR_KERNEL

}  // namespace gpf
