// gridpf_obs.hpp -- observation vectors assembled on the device (gpf_set_obs_spec / gpf_obs_vector, include/gridpf.h).
//
// What the reference builds for the agent after every env.step (paths relative to the reference checkout): BaseObservation._update_obs_complete
// (Observation/baseObservation.py:4464-4540) fills the attributes, GridObjects.to_vect (Space/GridObjects.py) concatenates them as float32 in
// the order of CompleteObservation.attr_list_vect (Observation/completeObservation.py:140-212), gym_compat.BoxGymObsSpace maps each element to
// (x - subtract) / divide.  Here: ONE gather kernel on the engine's stream turns the lane-major buffers of four dtypes the step kernel leaves
// behind (results row, rho, line status, topo_vect, counters, cooldowns, the state of the injection dynamics) into one float32 row per lane.
//
// Mapping: one wavefront per environment row, OBS_WPB rows per block (a 14-substation row is ~440 floats: a block per row would leave three
// of four wavefronts idle); the segment table is wavefront-uniform, read through scalar loads and kept in SGPRs; the lanes of the wavefront
// stride the elements of a segment, so source and destination rows are read / written coalesced, 16 bytes per lane where the float sources
// and the destination are aligned.  No LDS, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gridpf.h"
#include "gridpf_common.hpp"

namespace gpf {

constexpr int OBS_WPB = 4;                   // environment rows (wavefronts) per block
constexpr int OBS_SEG_INTS = 5;              // {kind, source offset, length, destination offset, flags}
constexpr int OBS_GO_ZERO = 0, OBS_GO_KEEP = 1, OBS_GO_MINUS1 = 2, OBS_GO_ONE = 3;   // flags bits 0-1: value of a game-over lane
constexpr int OBS_F_AFFINE = 4;              // flags bit 2 (set by the library): some element of the segment has subtract != 0 or divide != 1

// every pointer may be null where its comment says so: the source then reads as the stated constant
struct ObsSrc {
  const float* out;                 // [rows][n_out]      (trajectory mode: traj_out, rows = [step][lane capacity])
  const float* rho;                 // [rows][n_line]
  const unsigned char* line_status; // [rows][n_line]
  const int* topo_vect;             // [rows][dim_topo]
  const int* shunt_bus;             // [rows][n_shunt]
  const double* inj;                // [lanes][n_inj] injection rows (generator set-points at inj_gen_p_off)                (no per-step copy)
  const int* overflow;              // [lanes][n_line]                                      (no per-step copy)
  const int* cooldown;              // [lanes][n_line] or null: 0
  const short* cooldown16;          // trajectory mode: [rows][n_line] (saturated int16 copy), else null
  const int* sub_cd;                // [lanes][n_sub] or null: 0
  const float *target, *actual;     // [lanes][n_gen] or null: 0
  const float* charge;              // [lanes][n_sto] or null: 0
  const float* limit;               // [lanes][n_gen] or null: 1
  const double *pmin, *pmax, *ramp_up, *ramp_down;   // [n_gen] or null: margins 0
  const unsigned char* renewable;   // [n_gen] or null: none
  const unsigned char* done;        // [lanes]
  const signed char* traj_status;   // trajectory mode: [rows] GPF_ST_* of the step (!= 0: game over)
  const int* episode;               // [lanes][2]
  const int* lane_table;            // [lanes]
  const int* lane_offset;           // [lanes]
  const long long* clock_start;     // [n_tables] minutes since 1970-01-01 00:00 of row 0, or null (no calendar segment in the spec)
  const int* maint_next;            // [n_tables][T][n_line] or null: -1
  const int* maint_durn;            // [n_tables][T][n_line] or null: 0
  const float* thermal_limit;       // [n_line]
  const int* alert;                 // [lanes][6 alert_A + 1] the alert block (gpf_set_alerts), or null (its kinds are then refused by the host)     (no per-step copy)
  int alert_A;
  int T, t, step_minutes, max_step; // chronics rows per table (0: none uploaded), time index of step 0 of the rows
  int n_out, n_line, dim_topo, n_shunt, n_sub, n_gen, n_sto, gen_p_off, n_inj, inj_gen_p_off;
  long long lane_stride;            // trajectory mode: rows per step (the lane capacity)
  int traj;
};

struct ObsDate { int year, month, day, hour, minute, weekday; };

// civil date of `minutes` since 1970-01-01 00:00 (>= 0): days -> year / month / day by the era arithmetic of the proleptic Gregorian calendar
// (400-year eras of 146 097 days, the year starting in March); weekday as datetime.weekday() (Monday = 0; 1970-01-01 was a Thursday)
__host__ __device__ inline ObsDate obs_civil(long long minutes) {
  const long long days = minutes / 1440;
  const int mod = (int)(minutes - days * 1440);
  const long long z = days + 719468;
  const long long era = z / 146097;
  const int doe = (int)(z - era * 146097);
  const int yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const int doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const int mp = (5 * doy + 2) / 153;
  ObsDate d;
  d.day = doy - (153 * mp + 2) / 5 + 1;
  d.month = mp < 10 ? mp + 3 : mp - 9;
  d.year = (int)(yoe + era * 400) + (d.month <= 2 ? 1 : 0);
  d.hour = mod / 60;
  d.minute = mod % 60;
  d.weekday = (int)((days + 3) % 7);
  return d;
}

// rows [0, n_steps * n): row r = step r / n, lane lane0 + r % n.  dst row r at dst + r * row_stride.
__global__ __launch_bounds__(64 * OBS_WPB) void obs_gather_kernel(ObsSrc S, const int* __restrict__ seg, int n_seg, const float* __restrict__ sub,
                                                                   const float* __restrict__ div, float* __restrict__ dst, long long row_stride,
                                                                   int lane0, int n, int n_rows, int step0, int game_over_fill) {
  const int ln = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int r = blockIdx.x * OBS_WPB + wave; r < n_rows; r += gridDim.x * OBS_WPB) {       // wavefront-uniform
    const int step = r / n;
    const int lane = lane0 + (r - step * n);
    const size_t srow = S.traj ? (size_t)(step0 + step) * S.lane_stride + lane : (size_t)lane;   // row of the per-step buffers
    const bool over = game_over_fill && (S.traj ? gptr(S.traj_status)[srow] != 0 : gptr(S.done)[lane] != 0);
    // the chronics row the step read (K9's index) dates it and positions the maintenance look-ahead
    const int tab = gptr(S.lane_table)[lane];
    const int crow = S.T > 0 ? chron_row_index(S.t + step0 + step, gptr(S.lane_offset)[lane], S.T) : 0;
    ObsDate date{};
    if (S.clock_start) date = obs_civil(gptr(S.clock_start)[tab] + (long long)crow * S.step_minutes);
    const auto drow = (GPF_GLOBAL float*)dst + (size_t)r * row_stride;
    for (int s = 0; s < n_seg; ++s) {
      const int kind = seg[OBS_SEG_INTS * s], so = seg[OBS_SEG_INTS * s + 1], len = seg[OBS_SEG_INTS * s + 2], d0 = seg[OBS_SEG_INTS * s + 3],
                flags = seg[OBS_SEG_INTS * s + 4];
      const bool affine = (flags & OBS_F_AFFINE) != 0;
      const int go = flags & 3;
      const auto sb = gptr(sub) + d0;
      const auto dv = gptr(div) + d0;
      const auto dp = drow + d0;
      auto emit = [&](auto load) {          // lanes stride the elements of the segment
        for (int i = ln; i < len; i += 64) {
          float x = load(i);
          if (affine) x = (x - sb[i]) / dv[i];
          dp[i] = x;
        }
      };
      if (over && go != OBS_GO_KEEP) { const float v = go == OBS_GO_MINUS1 ? -1.f : go == OBS_GO_ONE ? 1.f : 0.f; emit([&](int) { return v; }); continue; }
      switch (kind) {
        case GPF_OBS_CONST: { const float v = __int_as_float(so); emit([&](int) { return v; }); break; }
        case GPF_OBS_OUT:
        case GPF_OBS_RHO: {
          const auto sp = kind == GPF_OBS_OUT ? gptr(S.out) + srow * S.n_out + so : gptr(S.rho) + srow * S.n_line + so;
          // 16 bytes per lane where source, destination and the affine arrays are aligned (uniform test); the tail element-wise
          typedef float v4f __attribute__((ext_vector_type(4)));
          const bool vec = (((size_t)sp | (size_t)dp) & 15) == 0 && (d0 & 3) == 0 && len >= 4;
          const int nv = vec ? len >> 2 : 0;
          for (int i = ln; i < nv; i += 64) {
            v4f x = ((GPF_GLOBAL const v4f*)sp)[i];
            if (affine) x = (x - ((GPF_GLOBAL const v4f*)sb)[i]) / ((GPF_GLOBAL const v4f*)dv)[i];
            ((GPF_GLOBAL v4f*)dp)[i] = x;
          }
          for (int i = 4 * nv + ln; i < len; i += 64) {
            float x = sp[i];
            if (affine) x = (x - sb[i]) / dv[i];
            dp[i] = x;
          }
          break;
        }
        case GPF_OBS_LINE_STATUS: { const auto sp = gptr(S.line_status) + srow * S.n_line + so; emit([&](int i) { return sp[i] ? 1.f : 0.f; }); break; }
        case GPF_OBS_TOPO_VECT: { const auto sp = gptr(S.topo_vect) + srow * S.dim_topo + so; emit([&](int i) { return (float)sp[i]; }); break; }
        case GPF_OBS_SHUNT_BUS: { const auto sp = gptr(S.shunt_bus) + srow * S.n_shunt + so; emit([&](int i) { return (float)sp[i]; }); break; }
        case GPF_OBS_OVERFLOW: { const auto sp = gptr(S.overflow) + (size_t)lane * S.n_line + so; emit([&](int i) { return (float)sp[i]; }); break; }
        case GPF_OBS_COOLDOWN_LINE: {
          if (S.cooldown16) { const auto sp = gptr(S.cooldown16) + srow * S.n_line + so; emit([&](int i) { return (float)sp[i]; }); }
          else if (S.cooldown) { const auto sp = gptr(S.cooldown) + (size_t)lane * S.n_line + so; emit([&](int i) { return (float)sp[i]; }); }
          else emit([&](int) { return 0.f; });
          break;
        }
        case GPF_OBS_COOLDOWN_SUB: {
          if (S.sub_cd) { const auto sp = gptr(S.sub_cd) + (size_t)lane * S.n_sub + so; emit([&](int i) { return (float)sp[i]; }); }
          else emit([&](int) { return 0.f; });
          break;
        }
        case GPF_OBS_TARGET_DISPATCH:
        case GPF_OBS_ACTUAL_DISPATCH:
        case GPF_OBS_CURTAILMENT_LIMIT: {
          const float* base = kind == GPF_OBS_TARGET_DISPATCH ? S.target : kind == GPF_OBS_ACTUAL_DISPATCH ? S.actual : S.limit;
          const float none = kind == GPF_OBS_CURTAILMENT_LIMIT ? 1.f : 0.f;
          if (base) { const auto sp = gptr(base) + (size_t)lane * S.n_gen + so; emit([&](int i) { return sp[i]; }); }
          else emit([&](int) { return none; });
          break;
        }
        case GPF_OBS_STORAGE_CHARGE: {
          if (S.charge) { const auto sp = gptr(S.charge) + (size_t)lane * S.n_sto + so; emit([&](int i) { return sp[i]; }); }
          else emit([&](int) { return 0.f; });
          break;
        }
        case GPF_OBS_MARGIN_UP:
        case GPF_OBS_MARGIN_DOWN: {
          if (!S.pmax) { emit([&](int) { return 0.f; }); break; }
          const auto gp = gptr(S.out) + srow * S.n_out + S.gen_p_off + so;
          const bool up = kind == GPF_OBS_MARGIN_UP;
          emit([&](int i) {
            const int g_ = so + i;
            const float p = gp[i];
            const float room = up ? (float)gptr(S.pmax)[g_] - p : p - (float)gptr(S.pmin)[g_];
            const float ramp = up ? (float)gptr(S.ramp_up)[g_] : (float)gptr(S.ramp_down)[g_];
            float m = (room != room || room < ramp) ? room : ramp;     // np.minimum: a NaN result row stays NaN
            if (S.renewable && gptr(S.renewable)[g_]) m = 0.f;
            return m < 0.f ? 0.f : m;       // (NaN stays NaN, as numpy's `x[x < 0] = 0` leaves it)
          });
          break;
        }
        case GPF_OBS_GEN_P_BEFORE_CURTAIL: {
          const auto ip = gptr(S.inj) + (size_t)lane * S.n_inj + S.inj_gen_p_off + so;
          emit([&](int i) { return (S.renewable && gptr(S.renewable)[so + i]) ? (float)ip[i] : 0.f; });
          break;
        }
        case GPF_OBS_GEN_P_DELTA: {
          const auto ip = gptr(S.inj) + (size_t)lane * S.n_inj + S.inj_gen_p_off + so;
          const auto gp = gptr(S.out) + srow * S.n_out + S.gen_p_off + so;
          emit([&](int i) { return gp[i] - (float)ip[i]; });
          break;
        }
        case GPF_OBS_CALENDAR: {
          const int v = so == 0 ? date.year : so == 1 ? date.month : so == 2 ? date.day : so == 3 ? date.hour : so == 4 ? date.minute : date.weekday;
          emit([&](int) { return (float)v; });
          break;
        }
        case GPF_OBS_CURRENT_STEP: {
          const int v = gptr(S.episode)[2 * (size_t)lane] + (gptr(S.done)[lane] ? 1 : 0);
          emit([&](int) { return (float)v; });
          break;
        }
        case GPF_OBS_MAX_STEP: { const float v = (float)S.max_step; emit([&](int) { return v; }); break; }
        case GPF_OBS_DELTA_TIME: { const float v = (float)S.step_minutes; emit([&](int) { return v; }); break; }
        case GPF_OBS_TIME_NEXT_MAINTENANCE:
        case GPF_OBS_DURATION_NEXT_MAINTENANCE: {
          const bool nx = kind == GPF_OBS_TIME_NEXT_MAINTENANCE;
          const int* base = nx ? S.maint_next : S.maint_durn;
          if (base) { const auto sp = gptr(base) + ((size_t)tab * S.T + crow) * S.n_line + so; emit([&](int i) { return (float)sp[i]; }); }
          else emit([&](int) { return nx ? -1.f : 0.f; });
          break;
        }
        case GPF_OBS_THERMAL_LIMIT: { const auto sp = gptr(S.thermal_limit) + so; emit([&](int i) { return sp[i]; }); break; }
        case GPF_OBS_ACTIVE_ALERT:
        case GPF_OBS_TIME_SINCE_LAST_ALERT:
        case GPF_OBS_ALERT_DURATION:
        case GPF_OBS_TOTAL_NUMBER_OF_ALERT:
        case GPF_OBS_TIME_SINCE_LAST_ATTACK:
        case GPF_OBS_ATTACK_UNDER_ALERT:
        case GPF_OBS_WAS_ALERT_USED_AFTER_ATTACK: {
          const int sec = kind == GPF_OBS_ACTIVE_ALERT ? GPF_ALERT_OBS_ACTIVE : kind == GPF_OBS_TIME_SINCE_LAST_ALERT ? GPF_ALERT_OBS_SINCE_ALERT
                        : kind == GPF_OBS_ALERT_DURATION ? GPF_ALERT_OBS_DURATION : kind == GPF_OBS_TOTAL_NUMBER_OF_ALERT ? GPF_ALERT_OBS_TOTAL
                        : kind == GPF_OBS_TIME_SINCE_LAST_ATTACK ? GPF_ALERT_OBS_SINCE_ATTACK : kind == GPF_OBS_ATTACK_UNDER_ALERT ? GPF_ALERT_OBS_UNDER_ALERT
                        : GPF_ALERT_OBS_USED;
          const auto sp = gptr(S.alert) + (size_t)lane * (6 * S.alert_A + 1) + sec * S.alert_A + so;
          emit([&](int i) { return (float)sp[i]; });
          break;
        }
        default: break;                     // (kinds are validated on the host)
      }
    }
  }
}

}  // namespace gpf
