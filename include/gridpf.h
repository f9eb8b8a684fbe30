/* gridpf.h -- C ABI of libgridpf.so: the MI355X-native batched power-flow engine behind the
 * grid2op Backend plugin surface.
 *
 * The reference (Grid2op/grid2op, 100 % Python) has no FFI of its own: its Backend plugin calls the
 * third-party package pandapower.  This header declares the entry points a grid2op Backend binds
 * instead (via ctypes, see INTEGRATION.md and grid2op_amd/_capi.py); each one cites the reference
 * interface it replaces.  Paths are relative to the reference checkout.
 *
 * Conventions: every function returns 0 on success and a negative GPF_E_* code on failure (message via
 * gpf_last_error()); no exception crosses the ABI; the caller owns every host buffer; a handle is
 * thread-compatible (use one handle per host thread); all work of a handle is queued on ONE HIP
 * stream owned by the handle and the gpf_get_* calls synchronise that stream.
 *
 * A "lane" is one independent grid instance (one environment copy or one N-1 contingency).  All
 * per-lane buffers are lane-major: row `lane` of a [n_lanes][stride] array.
 *
 * Units (same as grid2op/Backend/backend.py:563-760): MW, MVAr, kV, A, degrees; buses are LOCAL bus
 * ids 1..n_busbar, -1 = disconnected; generator voltage setpoints are in per unit.
 */
#ifndef GRIDPF_H
#define GRIDPF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPF_OK 0
#define GPF_E_INVALID (-1)   /* bad argument                                  */
#define GPF_E_DEVICE (-2)    /* HIP runtime error (no device, OOM, launch)    */
#define GPF_E_CAPACITY (-3)  /* grid too large for the compiled kernels       */
#define GPF_E_UNSUPPORTED (-4) /* optional facility not available on this host (gpf_jit_enable without hipcc) */

/* per-lane solver status written by gpf_runpf / gpf_step (status[lane*4 + 0]) */
#define GPF_ST_CONVERGED 0
#define GPF_ST_MAXITER 1     /* Newton did not reach the tolerance in max_iter iterations */
#define GPF_ST_ISLANDED 2    /* an active bus is not connected to a reference bus         */
#define GPF_ST_NOSLACK 3     /* no in-service slack generator                             */
#define GPF_ST_SINGULAR 4    /* zero / non finite pivot                                   */
#define GPF_ST_CAPACITY 5    /* more active buses than the handle was sized for           */
#define GPF_ST_NOTRUN (-1)

#define GPF_MAX_BUSBAR 64          /* busbars per substation a grid may have (the reference takes any n_busbar_per_sub,
                                      pandaPowerBackend.py:562-577; grid2op/tests/test_issue_l2g_128.py:218 uses 6)                  */
#define GPF_MAX_BUSBAR_BLOCKS 3    /* ... of which the NB = n_busbar block kernels cover 1..3.  Lanes with split substations normally
                                      run the single-busbar kernel on the bus-level graph of their topology class (any busbar count);
                                      only the developer fallback GRIDPF_NO_CLASSES=1 / a class that cannot be built needs the block
                                      kernels and is refused beyond 3 busbars (GPF_E_CAPACITY, at launch planning)                   */

typedef struct gpf_engine* gpf_handle;

/* Static description of one grid = what PandaPowerBackend.load_grid + _init_private_attrs derive
 * from the grid file (grid2op/Backend/pandaPowerBackend.py:356-617, 670-874) plus the per-unit
 * branch model pandapower's pd2ppc/makeYbus builds.  Arrays are copied by gpf_create.            */
typedef struct gpf_grid_desc {
  int32_t n_sub, n_busbar;                 /* global bus = sub + (local-1)*n_sub (GridObjects.py:4683) */
  int32_t n_line, n_gen, n_load, n_storage, n_shunt, dim_topo;
  double sn_mva;
  const double* sub_vn_kv;                 /* [n_sub]                                              */
  const int32_t* line_or_sub;              /* [n_line] lines first, then trafos (:462-471)         */
  const int32_t* line_ex_sub;
  const int32_t* line_or_pos_topo_vect;    /* [n_line] positions in topo_vect (GridObjects.py:1409) */
  const int32_t* line_ex_pos_topo_vect;
  const double* br_y;                      /* [n_line][8] yff.re,yff.im,yft.re,yft.im,ytf.re,ytf.im,ytt.re,ytt.im (pu) */
  const double* br_bdc;                    /* [n_line] 1/(x*ratio) DC susceptance (pu)             */
  const int32_t* gen_sub;                  /* [n_gen]                                              */
  const int32_t* gen_pos_topo_vect;
  const double* gen_min_q;                 /* [n_gen] MVAr, used for the Q split of co-located gens */
  const double* gen_max_q;
  const uint8_t* gen_slack;                /* [n_gen] 1 = slack generator (reference bus follows it) */
  const int32_t* load_sub;                 /* [n_load]                                             */
  const int32_t* load_pos_topo_vect;
  const int32_t* storage_sub;              /* [n_storage]                                          */
  const int32_t* storage_pos_topo_vect;
  const int32_t* shunt_sub;                /* [n_shunt]                                            */
  const double* shunt_fact;                /* [n_shunt] step*(vn_bus/vn_shunt)^2                   */
  /* pristine lane state (what reset() restores, pandaPowerBackend.py:334-354, 872) */
  const double* init_inj;                  /* [n_inj] see gpf_layout                               */
  const int32_t* init_topo;                /* [dim_topo]                                           */
  const int32_t* init_shunt_bus;           /* [n_shunt]                                            */
} gpf_grid_desc;

/* Row layouts of the per-lane buffers (offsets in elements). */
typedef struct gpf_layout {
  /* injections row (double): what apply_action scatters (pandaPowerBackend.py:925-969) */
  int32_t n_inj;
  int32_t inj_gen_p, inj_gen_vm, inj_load_p, inj_load_q, inj_storage_p, inj_storage_q, inj_shunt_p, inj_shunt_q;
  /* results row (float = grid2op dt_float): what _fetch_data_pf_converged gathers (:1122-1218) */
  int32_t n_out;
  int32_t out_p_or, out_q_or, out_v_or, out_a_or, out_theta_or;
  int32_t out_p_ex, out_q_ex, out_v_ex, out_a_ex, out_theta_ex;
  int32_t out_gen_p, out_gen_q, out_gen_v, out_gen_theta;
  int32_t out_load_p, out_load_q, out_load_v, out_load_theta;
  int32_t out_storage_p, out_storage_q, out_storage_v, out_storage_theta;
  int32_t out_shunt_p, out_shunt_q, out_shunt_v;
  /* chronics row (float): load_p[n_load], load_q[n_load], prod_p[n_gen], prod_v[n_gen] (kV) */
  int32_t n_chron;
  int32_t chron_load_p, chron_load_q, chron_prod_p, chron_prod_v;
  int32_t nb_total;                        /* n_sub*n_busbar: row length of the bus voltage buffers */
} gpf_layout;

const char* gpf_last_error(void);
/* ABI version of the library = GPF_ABI_VERSION of the header it was built from.  A binding MUST compare the two before any other
 * call (grid2op_amd/_capi.py does): 300 = round 4 (gpf_set_trajectory(h, cap, what), 22 device pointers, GPF_ST_REDISPATCH,
 * gpf_device_pointers_n); 310 = + gpf_jit_*, GPF_E_UNSUPPORTED, gpf_set_profiling mode 3; 321 = 28 device pointers (action buffers and
 * dispatch / charge state of the environment dynamics), gpf_lane_actions_on_device; 322 = + gpf_get_results_pinned; 323 = gpf_step_opts::track_cooldown,
 * GPF_DEVICE_NONE (header-only handles); 324 = 32 device pointers, topology actions in the batched step (gpf_upload_topo_actions ...);
 * 325 = 33 device pointers, observation vectors assembled on the device (gpf_set_obs_spec ...).
 * gpf_set_topo_areas / gpf_set_topo_slots / gpf_get_topo_action_areas were added under 326 without raising it: three new symbols, no
 * struct, argument list or default behaviour changed, so a binding written against the earlier 326 header works unchanged (a binding
 * that needs them finds out by looking the symbols up). */
#define GPF_ABI_VERSION 326
int gpf_version(void);
/* Bitwise run-to-run reproducibility is the DEFAULT on every grid: the same lane inputs give bit-identical results from run to
 * run and whatever the lane's position in the batch (grid2op's determinism contract: same seeds -> same episode,
 * grid2op/Environment/baseEnv.py seed()).  Small grids are solved by one wavefront per lane (the LDS applies the atomics of a
 * wavefront in a fixed order); grids with >= 64 substations by 2 wavefronts per lane whose accumulations are arranged so that no
 * sum depends on the interleaving of the two (accumulation loops on wavefront 0, every destination of an LU pass owned by one
 * wavefront, per-wavefront partial sums added in a fixed order).  flag != 0 additionally forces ONE wavefront per lane on the
 * large grids (~20 % slower there; kept for cross-checks -- its results differ from the 2-wavefront kernel's in the last bits,
 * each variant being reproducible in itself). */
int gpf_set_deterministic(gpf_handle h, int32_t flag);
/* Number of HIP devices visible to this process (0 and GPF_OK when there is none): what a single-process caller
 * shards its lane batch over (grid2op_amd/sharding.py ShardedEngine; the reference's own parallelism is one process per
 * environment, Runner/runner.py:1071-1253, Environment/baseMultiProcessEnv.py:293). */
int gpf_device_count(int32_t* n_devices);

/* load_grid (pandaPowerBackend.py:356): build an engine with `n_lanes` lanes on HIP device `device`.
 * Every lane starts in the pristine state.
 * device = GPF_DEVICE_NONE: a HEADER-ONLY handle -- every host-side step of the construction runs (validation, symbolic analysis of the
 * substation graph, static tables, launch planning for `n_lanes` lanes) but nothing is allocated on a device, and none is needed: what
 * works on it is gpf_jit_source (the header the grid-specialised kernels are compiled with -- pure grid arithmetic), gpf_get_plan (the
 * kernel variant a launch over all lanes would take), gpf_get_layout, gpf_n_lanes and gpf_destroy; every other entry point fails with
 * GPF_E_DEVICE.  It is how the ahead-of-time objects of a NEW grid are prepared on a machine without a GPU
 * (python -m grid2op_amd.aot). */
#define GPF_DEVICE_NONE (-1)
int gpf_create(const gpf_grid_desc* desc, int32_t n_lanes, int32_t device, gpf_handle* out);
/* close (pandaPowerBackend.py:1411-1423) */
int gpf_destroy(gpf_handle h);
int gpf_get_layout(gpf_handle h, gpf_layout* out);
int gpf_n_lanes(gpf_handle h);
/* Lane capacity of the per-lane device buffers (n_lanes rounded up, plus padding lanes the kernels use for instance groups). */
int gpf_lane_capacity(gpf_handle h);

/* apply_action, injection half (pandaPowerBackend.py:925-969): overwrite rows lane0..lane0+n-1.
 * inj is [n][n_inj] double. */
int gpf_set_injections(gpf_handle h, int32_t lane0, int32_t n, const double* inj);
/* apply_action, topology half (:920-922, 941-951, 964-975): topo is [n][dim_topo] local bus ids
 * (the layout of _BackendAction.current_topo.values), shunt_bus is [n][n_shunt] (may be NULL). */
int gpf_set_topology(gpf_handle h, int32_t lane0, int32_t n, const int32_t* topo, const int32_t* shunt_bus);
int gpf_get_injections(gpf_handle h, int32_t lane0, int32_t n, double* inj);
int gpf_get_topology(gpf_handle h, int32_t lane0, int32_t n, int32_t* topo, int32_t* shunt_bus);
/* _disconnect_line (:1464-1475): both ends of line `line_id` of lane `lane` go to -1. */
int gpf_disconnect_line(gpf_handle h, int32_t lane, int32_t line_id);
/* reset (:334-354): back to the pristine state. */
int gpf_reset_lanes(gpf_handle h, int32_t lane0, int32_t n);
/* copy (:1289-1409): device-side copy of the complete state (inputs and last results; with gpf_set_env_dynamics on also the
 * dispatch / storage / curtailment state of the environment's injection dynamics) of `n` lanes. */
int gpf_copy_lanes(gpf_handle h, int32_t src_lane0, int32_t dst_lane0, int32_t n);
/* N-1 fan-out (Reward/n1Reward.py:75-99, Observation/_obsEnv.py:321-503): lanes dst0+k (k < n_out)
 * become copies of `src_lane` (injections, topology, shunts; with gpf_set_env_dynamics on also its dispatch / storage /
 * curtailment state) with line out_lines[k] disconnected (out_lines[k] < 0: plain copy). */
int gpf_fanout_n1(gpf_handle h, int32_t src_lane, int32_t dst_lane0, int32_t n_out, const int32_t* out_lines);

/* runpf (pandaPowerBackend.py:1220-1255 -> pp.runpp / pp.rundcpp :1078-1120): one AC Newton-Raphson
 * (init="dc", <= max_iter iterations, ||F||inf < tol_mva/sn_mva) or DC power flow per lane, then the
 * result extraction of _fetch_data_pf_converged.  Asynchronous (queued on the handle's stream). */
int gpf_runpf(gpf_handle h, int32_t lane0, int32_t n, int32_t is_dc, int32_t max_iter, double tol_mva);

/* The single-environment plugin path in ONE call (what HipBackend.runpf does per power flow): gpf_set_injections +
 * gpf_set_topology + gpf_runpf + gpf_get_results for one lane through a device-mapped pinned host block (one dispatch
 * reads the inputs from it into the lane's rows, one writes the result rows back into it; no staged copies), synchronised once
 * (apply_action pandaPowerBackend.py:902-975, runpf :1220-1255, getters :1566-1619).  inj [n_inj], topo [dim_topo],
 * shunt_bus [n_shunt] (required when the grid has shunts); output pointers as in gpf_get_results (any may be NULL).
 * Synchronous. */
int gpf_solve_lane(gpf_handle h, int32_t lane, const double* inj, const int32_t* topo, const int32_t* shunt_bus, int32_t is_dc,
                   int32_t max_iter, double tol_mva, float* out, int32_t* topo_vect, int32_t* shunt_bus_out, uint8_t* line_status,
                   int32_t* status, double* bus_vm, double* bus_va);

/* gpf_get_results without the second host copy: the rows asked for (bit k of `what`: 0 out, 1 topo_vect, 2 shunt_bus, 3 line_status,
 * 4 status, 5 bus_vm, 6 bus_va, 7 rho [n][n_line] float32) are copied by DMA into a pinned block the engine owns and ptrs[k] (k < 8)
 * points at piece k inside it (NULL: not asked for) -- valid until the next call of this function.  A host agent that reads every
 * lane's rows at every step gets the PCIe rate instead of the pageable-copy rate.  Synchronous. */
int gpf_get_results_pinned(gpf_handle h, int32_t lane0, int32_t n, int32_t what, void** ptrs /* [8] */);

/* Getters (pandaPowerBackend.py:1566-1619, 278-301, 1439-1462, 1486): synchronise, then copy rows
 * lane0..lane0+n-1.  Any pointer may be NULL.
 *   out         [n][n_out]    float   (NaN everywhere when the lane did not converge, :1257-1287)
 *   topo_vect   [n][dim_topo] int32   (-1 everywhere when not converged)
 *   shunt_bus   [n][n_shunt]  int32
 *   line_status [n][n_line]   uint8
 *   status      [n][4]        int32   {GPF_ST_*, n_iter, n_active_bus, n_cascade_rounds}
 *   bus_vm/va   [n][nb_total] double  pu / degrees, NaN for inactive buses (pre-cast parity checks) */
int gpf_get_results(gpf_handle h, int32_t lane0, int32_t n, float* out, int32_t* topo_vect, int32_t* shunt_bus,
                    uint8_t* line_status, int32_t* status, double* bus_vm, double* bus_va);

/* ---- batched environment stepping (device-resident chronics) ----------------
 * chronics: [n_tables][T][n_chron] float, resident in HBM.  Lane k reads row
 * (t + lane_offset[k]) mod T of table lane_table[k]; loads are multiplied by lane_scale[k][0..2*n_load)
 * (NULL = 1); if `rebalance` != 0 the non-slack prod_p are rescaled so that sum(prod_p) =
 * rebalance * sum(load_p) (Environment/baseEnv.py:2516-2563 feeds these 4 vectors each step). */
int gpf_upload_chronics(gpf_handle h, int32_t n_tables, int32_t T, const float* data);
/* Scheduled maintenance of the uploaded chronics tables: [n_tables][T][n_line] uint8, 1 = the line is in maintenance at that
 * row (maintenance.csv, grid2op/Chronics/gridStateFromFile.py:520-600 -> the "maintenance" modification the environment applies
 * every step, Environment/baseEnv.py:2516-2563): gpf_step / gpf_step_n force such a line out of service; it stays out afterwards
 * (nothing reconnects it for a DoNothing agent).  NULL removes the table. */
int gpf_upload_maintenance(gpf_handle h, int32_t n_tables, int32_t T, const uint8_t* data);
/* Hazards of the uploaded chronics tables (hazards.csv, Chronics/gridStateFromFile.py:478-490: unplanned outages), same shape and
 * same effect on the backend as the maintenance table -- the line is forced out of service at the rows where it is flagged (the
 * "hazards" modification the environment applies every step); the two tables are independent, the device applies their union. */
int gpf_upload_hazards(gpf_handle h, int32_t n_tables, int32_t T, const uint8_t* data);
/* Remaining duration (steps, incl. the current one) of the maintenance / hazard under way at every row, [n_tables][T][n_line] uint16: what the
 * line cooldowns are raised to during an outage (gpf_step_opts::track_cooldown; GridValue.get_maintenance_duration_1d / get_hazard_duration_1d,
 * grid2op/Chronics/gridValue.py:339).  By default the library derives it from the uploaded outage tables (one backward scan); a caller whose
 * tables are a WINDOW of longer chronics passes the true values here, because an outage that runs past the end of the window looks shorter than it
 * is.  Used where an outage table flags the line; NULL: back to the derived values. */
int gpf_upload_outage_durations(gpf_handle h, int32_t n_tables, int32_t T, const uint16_t* data);
int gpf_set_lane_chronics(gpf_handle h, const int32_t* lane_table, const int32_t* lane_offset, const float* lane_scale);
int gpf_set_thermal_limits(gpf_handle h, const float* limit_a /* [n_line] */);
/* One DoNothing env.step for every lane (Environment/baseEnv.py:3562 -> Backend.next_grid_state
 * backend.py:1433-1521): chronics row -> injections -> AC power flow -> results -> overflow counters;
 * when `cascade` != 0 lines above hard_overflow*limit (or soft-overflowed for more than nb_ts_allowed
 * steps) are tripped and the power flow re-run, at most max_rounds times.  is_dc != 0 runs the DC power flow
 * instead (Parameters.ENV_DC, grid2op/Parameters.py:273 -> runpf(is_dc=True)).  Asynchronous. */
int gpf_step(gpf_handle h, int32_t t, int32_t max_iter, double tol_mva, double rebalance, int32_t cascade,
             float hard_overflow, float soft_overflow, int32_t nb_ts_allowed, int32_t max_rounds, int32_t is_dc);
/* Options of gpf_step_n (the arguments of gpf_step, plus auto_reset). */
typedef struct gpf_step_opts {
  int32_t max_iter;
  double tol_mva;
  double rebalance;
  int32_t cascade;
  float hard_overflow, soft_overflow;
  int32_t nb_ts_allowed, max_rounds;
  int32_t is_dc;
  int32_t auto_reset;    /* != 0: a lane whose step fails (game over: BaseEnv.step sets done when the backend diverges,
                            Environment/baseEnv.py:3847-3931) restarts at the next step from the topology the host sent last
                            (gpf_set_topology / gpf_reset_lanes), overflow counters cleared -- what env.reset() does to the
                            backend (Environment/environment.py:1418 reset_grid); the chronics cursor runs on, unless
                            gpf_set_chronics_cursor is on: then the lane's next launch starts a scenario */
  int32_t warm_start;    /* != 0 (OPT-IN, NOT what PandaPowerBackend does): steps 2..n of a launch start Newton from the previous
                            step's voltages while the lane's topology stands, instead of the DC initialisation pandapower
                            performs on every runpf (pandaPowerBackend.py:1086 _pf_init = "dc"; LightSimBackend-style warm start).
                            Same solution within the solver tolerance, fewer iterations: n_iter and the last digits differ
                            from the reference's.  Default 0 = the reference's algorithm. */
  int32_t track_cooldown; /* != 0: maintain the environment's LINE COOLDOWNS (BaseEnv._times_before_line_status_actionable =
                            obs.time_before_cooldown_line, Environment/baseEnv.py:3352-3358, 2590-2597) at every converged step: decremented,
                            set to nb_ts_reco for a line the protections trip in the step, raised to the remaining duration of a
                            maintenance / hazard under way (the uploaded outage tables).  0 (what a zero-initialised struct says, like every
                            other field): the counters are left alone (gpf_step: always).  Read with gpf_get_cooldown /
                            gpf_get_trajectory_cooldown; cleared by gpf_reset_lanes and by an auto-reset, copied by gpf_copy_lanes,
                            gpf_fanout_n1 and gpf_simulate_batch -- whose scratch step never maintains them (one look-ahead step on the
                            forecast tables: the source's counters are what obs.simulate starts from, _obsEnv.py:321-428).
                            (Cooldowns caused by the agents' own line / substation actions: the acting path of gpf_upload_topo_actions
                            books them on the device when it is enabled; otherwise they belong to the caller -- a DoNothing step has none.) */
  int32_t nb_ts_reco;    /* Parameters.NB_TIMESTEP_RECONNECTION (default 10; >= 0): the cooldown of a line the protections trip;
                            only read when track_cooldown != 0 */
} gpf_step_opts;
/* n_steps consecutive DoNothing env.step (t0, t0+1, ...) of every lane in ONE launch.  Every step does the whole of gpf_step;
 * between the steps of a launch the lane state stays on chip and whatever only depends on the topology (element->bus maps, bus
 * types, Ybus, the factored DC matrix) is kept until a line trips or a lane fails.
 * n_steps = 1 (an agent that acts between any two steps: the reference's loop, Environment/baseEnv.py:3562-3931): a lane whose topology
 * row, shunt buses and shunt set-points are those the engine was created with loads that topology-only state from one blob the engine
 * keeps (written by the first such launch) instead of rebuilding it; every other lane rebuilds.  Results are bit-identical either way,
 * and equal to the same steps inside one multi-step launch bit for bit (GRIDPF_KEEP=0 at gpf_create: always rebuild).
 * What is retrievable afterwards: the getters (gpf_get_results, gpf_get_step_outputs, device views) return the LAST step only --
 * without a trajectory buffer each step overwrites the lane's result row, so the observations of the earlier steps never exist in
 * HBM.  gpf_set_trajectory(h, cap, GPF_TRAJ_OBS) keeps the complete backend observation of EVERY step (what BaseEnv.step hands
 * to the observation after each env.step: Environment/baseEnv.py:3562-3931 -> Observation/completeObservation.py:140-211 reads
 * the backend's flows / voltages / injections, topo_vect and line status); GPF_TRAJ_RHO keeps rho + status only.
 * n_steps must not exceed the capacity of a trajectory buffer that is set.  Asynchronous. */
int gpf_step_n(gpf_handle h, int32_t t0, int32_t n_steps, const gpf_step_opts* opts);
/* Per-lane additive generator set-point delta in MW, [n_lanes][n_gen] (NULL: none): the redispatch the environment adds to the
 * chronics' prod_p every step (actual_dispatch, Environment/baseEnv.py:2211-2470, 3650-3700). */
int gpf_set_lane_redispatch(gpf_handle h, const float* delta_mw);
/* The environment's redispatching automaton (BaseEnv._compute_dispatch_vect, Environment/baseEnv.py:2211-2470), batched: for
 * every lane the redispatch the agents ask for is projected on pmin / pmax / ramp limits under the zero-sum constraint
 * sum(x) = rhs (rhs = storage power - curtailment + detached MW, :2335-2340) and added to the actual dispatch.
 * gpf_set_gen_limits: the generator characteristics of prods_charac.csv ([n_gen] each), eps_poly as BaseEnv._epsilon_poly.
 * gpf_redispatch: rows of lanes lane0..lane0+n-1, [n][n_gen]: new_p (chronics set-points of the step), prev_p (set-points of
 * the previous step incl. dispatch, BaseEnv._gen_activeprod_t_redisp), actual / target dispatch, modified (generators touched
 * by an action this step); ok[n] = 0 where the reference raises ImpossibleRedispatching (the row is then returned unchanged);
 * actual_after [n][n_gen] float.  apply != 0 also stores the result as the lanes' redispatch delta (gpf_set_lane_redispatch)
 * for the following gpf_step.  Synchronous. */
int gpf_set_gen_limits(gpf_handle h, const double* pmin, const double* pmax, const double* ramp_up, const double* ramp_down,
                       const uint8_t* redispatchable, double eps_poly);
int gpf_redispatch(gpf_handle h, int32_t lane0, int32_t n, const double* new_p, const double* prev_p, const double* actual,
                   const double* target, const uint8_t* modified, const double* rhs, int32_t apply, uint8_t* ok, float* actual_after);
/* ---- injection dynamics of the environment inside the stepped batch (BASELINE configs[3]: storage + redispatch actions) ------
 * What BaseEnv.step does to the generator / storage set-points between the chronics and the backend, evaluated by gpf_step_n at
 * EVERY step of a launch: the storage state of charge with its efficiencies, Emin / Emax clamping and losses
 * (Environment/baseEnv.py:2829-2905 _compute_storage, :2777-2790 _withdraw_storage_losses), the accumulation of the agents'
 * redispatch into the target dispatch (:2101-2115), the _make_redisp gate (:2188-2209) and the ramp- / pmin- / pmax-limited
 * zero-sum projection (:2211-2470 _compute_dispatch_vect; exact solution of the separable QP, as gpf_redispatch), then
 * prod_p = chronics + actual dispatch (:3830 set_redispatch) and the storage power (:3831 set_storage).  A lane whose projection is
 * infeasible ends its episode (status GPF_ST_REDISPATCH; ImpossibleRedispatching :3227-3247).  Curtailment
 * (_aux_handle_curtailment_without_limit, :2956-2982): renewable generators are capped at limit * pmax, the change of the curtailed
 * total joins the right-hand side of the projection.  An ILLEGAL redispatch -- the accumulated target beyond pmax - pmin or below
 * pmin - pmax (_prepare_redisp :2140-2173) -- is cancelled as the reference cancels it: taken back out of the target, the storage
 * part of the step undone (:3189-3212).  Not modelled: detachment, generator up / down times, the dispatch of switched-off generators
 * (Parameters.ALLOW_DISPATCH_GEN_SWITCH_OFF = False), LIMIT_INFEASIBLE_CURTAILMENT_STORAGE_ACTION.
 *   gpf_set_storage_params : storage_Emax / Emin / loss / charging & discharging efficiency / initial charge [n_storage], the
 *                            step length and Parameters.ACTIVATE_STORAGE_LOSS.
 *   gpf_set_env_dynamics   : on != 0 switches the dynamics on (needs gpf_set_gen_limits, and gpf_set_storage_params on a grid
 *                            with storage units) and resets the state of every lane (dispatch 0, initial charge); tol_poly as
 *                            BaseEnv._tol_poly.  Needs n_gen and n_storage <= the lanes an instance owns (16 / 32 / 64).
 *   gpf_set_lane_actions   : the agents' actions of the NEXT launch: redispatch [n_lanes][n_gen] MW (added to the target dispatch
 *                            by the launch's first step, then consumed) and storage power [n_lanes][n_storage] MW (applied by the
 *                            first step only -- grid2op's semantics of a storage action -- or, hold_storage != 0, by every step
 *                            until replaced); NULL = none.  The arrays are copied into pinned staging before the call returns;
 *                            the upload rides the engine's stream, nothing is synchronised.
 *   gpf_set_gen_renewable  : gen_renewable [n_gen] (NULL: no curtailment);  gpf_set_lane_curtailment: the curtailment action of
 *                            the NEXT launch, [n_lanes][n_gen] ratios of pmax in [0, 1], -1 = no change (consumed by the first
 *                            step; the limits then live in the lanes' state, like BaseEnv._limit_curtailment).
 *   gpf_get/set_env_state  : target / actual dispatch, previous set-points (_gen_activeprod_t_redisp), already-modified mask
 *                            [n][n_gen], state of charge [n][n_storage], previous storage amount [n], curtailment limits
 *                            [n][n_gen], previous curtailed total [n] (what an environment restored from an observation hands
 *                            over, baseEnv.py:4879-4882); any pointer may be NULL.
 * gpf_reset_lanes also resets the dynamics of the lanes. */
#define GPF_ST_REDISPATCH 6   /* the redispatch projection is infeasible: game over (ImpossibleRedispatching) */
int gpf_set_storage_params(gpf_handle h, const double* emax, const double* emin, const double* loss, const double* eff_charge,
                           const double* eff_discharge, const float* charge0, double delta_time_seconds, int32_t activate_loss);
int gpf_set_env_dynamics(gpf_handle h, int32_t on, double tol_poly);
int gpf_set_lane_actions(gpf_handle h, const float* redispatch, const float* storage_power, int32_t hold_storage);
/* The same hand-over for agents that live ON THE DEVICE (a policy network next to the engine): the caller has written the actions of
 * the next launch into the engine's own action buffers -- gpf_device_pointers_n entries 22 (redispatch [lanes][n_gen] MW), 23 (storage
 * power [lanes][n_storage] MW), 24 (curtailment [lanes][n_gen], ratios in [0, 1] or -1: NOT validated here) -- on the engine's stream
 * or ordered before the next launch; the flags say which of them hold an action (the others count as "none").  Nothing crosses PCIe,
 * nothing is synchronised.  Consumption is as for gpf_set_lane_actions / gpf_set_lane_curtailment: the launch's first step takes the
 * actions; afterwards the redispatch buffer (and the storage buffer unless hold_storage) counts as empty until declared again. */
int gpf_lane_actions_on_device(gpf_handle h, int32_t redispatch, int32_t storage_power, int32_t curtailment, int32_t hold_storage);
int gpf_set_gen_renewable(gpf_handle h, const uint8_t* renewable);
int gpf_set_lane_curtailment(gpf_handle h, const float* limit);
int gpf_get_env_state(gpf_handle h, int32_t lane0, int32_t n, float* target, float* actual, float* prev_p, uint8_t* already_modified,
                      float* charge, float* amount_prev, float* curtail_limit, float* curtail_prev);
/* count[n]: steps since the lane's last reset whose action was CANCELLED as an illegal redispatch (what BaseEnv.step reports as
 * info["is_illegal_redisp"] / the IllegalRedispatching exception of that step, baseEnv.py:2140-2173, 3400-3425); copied with the lane
 * by gpf_copy_lanes / gpf_fanout_n1 / gpf_simulate_batch, cleared by gpf_reset_lanes and auto-reset. */
int gpf_get_env_illegal(gpf_handle h, int32_t lane0, int32_t n, int32_t* count);
/* overwrite the counters (a lane moved between engines / devices through the host carries its count: ShardedEngine.copy_lanes) */
int gpf_set_env_illegal(gpf_handle h, int32_t lane0, int32_t n, const int32_t* count);
int gpf_set_env_state(gpf_handle h, int32_t lane0, int32_t n, const float* target, const float* actual, const float* prev_p,
                      const uint8_t* already_modified, const float* charge, const float* amount_prev, const float* curtail_limit,
                      const float* curtail_prev);

/* ---- batched obs.simulate (Observation/baseObservation.py:3365-3670 simulate -> Environment/_obsEnv.py: the forecast
 * injections of `time_step` steps ahead + a candidate action on a copy of the observation's grid state, one env.step of that copy) --
 * gpf_upload_forecasts: the *_forecasted tables of the uploaded chronics (Chronics/gridStateFromFileWithForecasts.py:311-353:
 * forecast h_id of chronics row r is row n_horizons * r + h_id), [n_tables][T][n_horizons][n_chron] float, same row layout as
 * the chronics; NULL removes them.
 * gpf_simulate_batch: for each of the n_src source lanes (environments whose current observation is the step at time index t_obs)
 * and each of the n_act candidate actions, lane dst_lane0 + b * n_act + k becomes a copy of source lane b (topology, shunts,
 * storage / shunt set-points, redispatch delta, jitter, protection counters) with action k applied to the topology as
 * _BackendAction.__iadd__ applies it (Action/_backendAction.py:836-919: line status first -- a reconnected end goes back to its
 * last known busbar, `last_bus` [n_src][dim_topo] or NULL = busbar 1 --, then change_bus, then set_bus, then lines with one open
 * end are opened / lines reconnected by a bus assignment get their other end back), and ONE launch steps all n_src * n_act lanes
 * with the injections of the forecast `time_step` steps ahead (time_step = 0: the current chronics row, i.e. the observation's own
 * injections) under `opts` (cascade, thermal limits, is_dc ... as gpf_step_n; one step).  Results: the getters on the
 * destination range (gpf_get_results, gpf_get_step_outputs -> rho).  The destination lanes are scratch lanes: their chronics
 * cursor and counters are overwritten.  Actions: act_off[n_act + 1] offsets into act_items[][3] = {kind, id, value}:
 *   GPF_ACT_SET_BUS {topo_vect position, bus (-1 | 1..n_busbar)}   GPF_ACT_CHANGE_BUS {topo_vect position, -}
 *   GPF_ACT_SET_LINE_STATUS {line id, +1 | -1}                      GPF_ACT_CHANGE_LINE_STATUS {line id, -}
 *   GPF_ACT_SET_SHUNT_BUS {shunt id, bus}
 * With the injection dynamics on (gpf_set_env_dynamics) every scratch lane also inherits its source's dispatch / storage /
 * curtailment state (what _ObsEnv is initialised with) and takes ONE do-nothing step of the dynamics on the simulated injections
 * (the candidates are topology actions); the sources' state and the per-lane actions waiting for the next gpf_step_n are untouched.
 * A scratch lane cannot be the SOURCE of a later call -- its chronics cursor is an absolute row (of the forecast tables when it simulated
 * a forecast), not an offset to the time index (GPF_E_INVALID; gpf_set_lane_chronics puts every lane back on the chronics).
 * Asynchronous launch (the topology bookkeeping before it synchronises once). */
#define GPF_ACT_SET_BUS 0
#define GPF_ACT_SET_LINE_STATUS 1
#define GPF_ACT_CHANGE_BUS 2
#define GPF_ACT_CHANGE_LINE_STATUS 3
#define GPF_ACT_SET_SHUNT_BUS 4
int gpf_upload_forecasts(gpf_handle h, int32_t n_tables, int32_t T, int32_t n_horizons, const float* data);
int gpf_simulate_batch(gpf_handle h, int32_t t_obs, int32_t time_step, int32_t n_src, const int32_t* src_lanes, int32_t n_act,
                       const int32_t* act_off, const int32_t* act_items, const int32_t* last_bus, int32_t dst_lane0,
                       const gpf_step_opts* opts);

/* ---- topology actions in the batched step (what BaseEnv.step does between the agent and the backend for the topology part of an
 * action, Environment/baseEnv.py:3562-3931, on the device for every lane; grid2op_amd/csrc/gridpf_topo.hpp) ------------------------------
 * A launch of gpf_step_n that carries topology actions takes, for every lane, the entry act_topo[lane] of an uploaded action table
 * (-1: do nothing) and, before the step: rejects an ambiguous entry (BaseAction._check_for_ambiguity, Action/baseAction.py:3668-3760:
 * static per entry, computed here at upload; an index outside the table written on the device counts as ambiguous), computes its
 * impact with the lane's line status before the step (get_topological_impact, Action/baseAction.py:1782-2020), checks the rules
 * (Rules/DefaultRules.py = LookParam.py:28-53 + PreventReconnection.py:23-60 against the lane's line and substation cooldowns), turns an
 * ambiguous or illegal action into do-nothing with its flag set (baseEnv.py:3700-3770) and applies a legal one to the lane's topology
 * row as gpf_simulate_batch does (a reconnected end goes back to the lane's last known busbar).  After the step (baseEnv.py:3346-3395):
 * lines the action affected whose cooldown is below cooldown_line get cooldown_line (after the step's own cooldown update --
 * gpf_step_opts::track_cooldown), substation cooldowns are decremented and the affected substations set to cooldown_sub, and the last
 * known busbar of every connected element is updated (_BackendAction.update_state, Action/_backendAction.py:1533-1555).  A
 * multi-step launch without actions decrements the substation cooldowns by its step count.  A lane that auto-resets is cleared (no
 * substation cooldown, last known busbar = its reset topology); a lane whose step failed without auto-reset books nothing.
 * Rules:
 *   - a launch that carries topology actions must be a one-step launch (GPF_E_INVALID otherwise: the line-cooldown rule needs the
 *     action step's trips and outages);
 *   - topology actions and injection actions (gpf_set_lane_actions / gpf_lane_actions_on_device / gpf_set_lane_curtailment, a held
 *     storage action included) pending for the same launch: GPF_E_INVALID, unless gpf_set_combined_actions (below) turned combined
 *     actions on: in the reference the illegality of either part cancels both;
 *   - cooldown_line > 0 needs gpf_step_opts::track_cooldown on the action launch (GPF_E_INVALID otherwise): the agents' line cooldowns
 *     are counted down by the launches that maintain the line cooldowns, never by the acting path itself;
 *   - an auto-reset puts a lane an action moved to another topology class back on its reset topology: after such a one-step launch the
 *     host reads those lanes back and re-keys them (one more synchronisation, only while moved lanes exist); a MULTI-step launch with
 *     auto_reset while any lane is on a moved class is refused (GPF_E_INVALID: the plan of a launch cannot follow a reset inside it);
 *   - the pending indices are consumed by the launch that takes them, also when it fails after the pre-step (the rows may already be
 *     rewritten: reset or re-send the lanes after a failed launch);
 *   - PreventDiscoStorageModif cannot fire on a pure topology action; it is part of the combined actions of gpf_set_combined_actions.
 *     RulesByArea (l2rpn_idf_2023) is covered by gpf_set_topo_areas / gpf_set_topo_slots below.
 * The launch planner needs every lane's topology class: the pre-step kernel lists the lanes whose class key or busbar count changed
 * and the host reads that one compact list back (skipped when no entry of the table can change a class).  The auto-reset target
 * (the rows last sent with gpf_set_topology) is not changed by an action.
 *   gpf_set_topo_rules        : on != 0: DefaultRules with Parameters.MAX_SUB_CHANGED / MAX_LINE_STATUS_CHANGED; on = 0: AlwaysLegal.
 *                               cooldown_sub / cooldown_line: NB_TIMESTEP_COOLDOWN_SUB / NB_TIMESTEP_COOLDOWN_LINE (0: not booked).
 *   gpf_upload_topo_actions   : the table in the encoding of gpf_simulate_batch (act_off[n_act + 1], act_items[][3], validated the same
 *                               way); ambiguous[n_act] (may be NULL) receives the static ambiguity flags.  n_act = 0 empties it.
 *   gpf_set_lane_topo_actions : index[n_lanes][n_slot] of the NEXT launch from the host (NULL: none); consumed by that launch.
 *   gpf_topo_actions_on_device: on != 0: the next launch takes the indices written into the device buffer act_topo (gpf_device_pointers
 *                               entry 28) on the engine's stream or ordered before the launch; consumed by that launch.
 *   gpf_get/set_sub_cooldown  : [n][n_sub] obs.time_before_cooldown_sub.      gpf_get/set_last_bus: [n][dim_topo] busbars 1..n_busbar.
 *   gpf_get_topo_flags        : [n][2] {is_illegal, is_ambiguous} of the last launch that carried actions.
 * The first of these calls enables the acting path (buffers for every lane); gpf_reset_lanes / auto-reset clear its state,
 * gpf_copy_lanes / gpf_fanout_n1 copy it. */
int gpf_set_topo_rules(gpf_handle h, int32_t on, int32_t max_sub_changed, int32_t max_line_status_changed, int32_t cooldown_sub,
                       int32_t cooldown_line);
int gpf_upload_topo_actions(gpf_handle h, int32_t n_act, const int32_t* act_off, const int32_t* act_items, uint8_t* ambiguous);
int gpf_set_lane_topo_actions(gpf_handle h, const int32_t* index);
int gpf_topo_actions_on_device(gpf_handle h, int32_t on);
int gpf_get_sub_cooldown(gpf_handle h, int32_t lane0, int32_t n, int32_t* sub_cooldown);
int gpf_set_sub_cooldown(gpf_handle h, int32_t lane0, int32_t n, const int32_t* sub_cooldown);
int gpf_get_last_bus(gpf_handle h, int32_t lane0, int32_t n, int32_t* last_bus);
int gpf_set_last_bus(gpf_handle h, int32_t lane0, int32_t n, const int32_t* last_bus);
int gpf_get_topo_flags(gpf_handle h, int32_t lane0, int32_t n, uint8_t* flags);

/* ---- rules by area and composite actions (Rules/rulesByArea.py: RulesByArea, the rules l2rpn_idf_2023 is played under: the limits hold
 * per area and an agent acts in every area at the same step) ------------------------------------------------------------------------
 *   gpf_set_topo_areas : sub_area[n_sub], the area in [0, n_area) of every substation, 1 <= n_area <= 16, every area holding at least one
 *                        substation (GPF_E_INVALID otherwise).  n_area = 0 or sub_area = NULL: whole-grid limits again (the default).  A line
 *                        belongs to the area of its ORIGIN substation (rulesByArea.py:91), tie lines too.  With gpf_set_topo_rules(on = 1)
 *                        an action is then illegal when in ANY area the affected lines of that area exceed max_line_status_changed, or the
 *                        affected substations of that area exceed max_sub_changed (_lookparam_byarea, rulesByArea.py:120-140);
 *                        PreventReconnection stays per element.  With areas set the two limits must not exceed 254 (GPF_E_INVALID).  Areas
 *                        belong to the rules, not to lanes: resets and lane copies do not touch them.  May be called before or after the
 *                        upload of the table.
 *   gpf_set_topo_slots : 1 <= n_slot <= 8 (default 1) table entries per lane and step: act_topo becomes [lane capacity][n_slot] (another
 *                        buffer: fetch gpf_device_pointers again), all slots empty; pending indices are dropped.  A lane's action is the
 *                        CONCATENATION, in slot order, of the item lists of its non-empty slots (-1: empty; all empty: do nothing), treated
 *                        exactly as a single table entry with that item list would be: the dense arrays are filled item by item (a later
 *                        set_bus of a position replaces an earlier one), ambiguity is decided at run time on them by the rules of the
 *                        upload (an index outside the table in any slot: ambiguous), impact, legality and the cooldown booking are those
 *                        of the union, and the list is applied ONCE (every line-status item before any bus item -- applying slot after
 *                        slot would be another action).  One index may sit in several slots of a lane: its items then stand
 *                        several times in the list, as they would in such an entry.  GPF_E_INVALID (here or from
 *                        gpf_upload_topo_actions) when n_slot times the longest entry of the table does not fit the pre-step kernel's
 *                        64 KiB of LDS.
 *   gpf_get_topo_action_areas : areas[n_act], bit k set when the entry can touch area k: the area of every substation it names and of BOTH
 *                        end substations of every line it names through a status item or a line-end set_bus / change_bus (an ambiguous
 *                        entry: everything it names).  Without areas every non-empty entry has bit 0.  Static; works on a header-only handle.
 * With areas set GPF_MASK_TOO_MANY_LINES / GPF_MASK_TOO_MANY_SUBS of the legality masks below mean "in some area".  The mask stays one byte
 * per (lane, ENTRY).  Factorisation guarantee: if the non-empty slots of a lane hold entries with pairwise disjoint area sets
 * (gpf_get_topo_action_areas), the composite is applied (is_illegal = is_ambiguous = 0) EXACTLY WHEN every one of those entries has mask
 * byte 0 for that lane.  Proof: disjoint area sets mean the entries name disjoint elements, lines and substations (an entry's set holds
 * the areas of both ends of every line it names).  So (1) no item of one entry overwrites or meets an item of another in the dense
 * arrays, and every ambiguity rule looks at one element or at one line and its two ends: the composite is ambiguous iff one entry is;
 * (2) a line's impact depends on its own items and status, a substation's on its own elements and their lines: the composite's
 * aff_lines / aff_subs are the disjoint unions of the entries'; (3) an affected line or substation of an entry lies in one of that
 * entry's areas, so each area's counts come from one entry only: a limit is exceeded in some area iff it is for one entry alone;
 * (4) the cooldown rules are per element.  A policy with one head per area can therefore mask each head by its own columns. */
int gpf_set_topo_areas(gpf_handle h, int32_t n_area, const int32_t* sub_area /* [n_sub] */);
int gpf_set_topo_slots(gpf_handle h, int32_t n_slot);
int gpf_get_topo_action_areas(gpf_handle h, uint32_t* areas /* [n_act] */);

/* ---- legality masks of the action table (what a policy with a discrete head over the table needs before every step) -- for lane k
 * and table entry a one byte, 0 exactly when a launch that carried act_topo[k] = a right now would apply the entry (is_illegal =
 * is_ambiguous = 0 in gpf_get_topo_flags), else the OR of ALL the reasons that hold (the reference reports the first):
 *   GPF_MASK_TOO_MANY_LINES  aff_lines.sum() > max_line_status_changed            (Rules/LookParam.py:28-53)
 *   GPF_MASK_TOO_MANY_SUBS   aff_subs.sum() > max_sub_changed                     (Rules/LookParam.py:28-53)
 *   GPF_MASK_LINE_COOLDOWN   an affected line has a line cooldown > 0             (Rules/PreventReconnection.py:23-60)
 *   GPF_MASK_SUB_COOLDOWN    an affected substation has a substation cooldown > 0 (Rules/PreventReconnection.py:23-60)
 *   GPF_MASK_AMBIGUOUS       the entry's static ambiguity flag; such an entry carries this bit alone (no impact is computed for it)
 * aff_lines / aff_subs are BaseAction.get_topological_impact (Action/baseAction.py:1782-2020) with the lane's line status (both ends of
 * its current topology row > 0) -- the arithmetic of the pre-step of gpf_step_n, evaluated for every entry by ONE side kernel
 * (grid2op_amd/csrc/gridpf_topo_mask.hpp) from a static per-entry summary built by gpf_upload_topo_actions.  With gpf_set_topo_rules(on = 0)
 * only GPF_MASK_AMBIGUOUS occurs.  The inputs are the lanes' topology rows, line cooldowns and substation cooldowns as they stand when the
 * call is ordered on the engine's stream; the call only reads: no lane state, pending index, flag or affected row changes; a lane whose
 * episode is done is evaluated from its rows like any other.
 *   gpf_topo_action_mask     : rows of lanes [lane0, lane0 + n) -> out_dev (device memory, row k at out_dev + k * row_stride bytes,
 *                              row_stride >= n_act; only the first n_act bytes of a row are written) or, out_dev = NULL, rows lane0.. of the
 *                              engine-owned [lane capacity][n_act] buffer (gpf_device_pointers_n entry 33, re-allocated with the table).
 *                              Asynchronous on the engine's stream.
 *   gpf_get_topo_action_mask : the same into the engine-owned buffer, then the rows on the host ([n][n_act], dense); synchronous.
 * GPF_E_INVALID: no table (or an empty one), a lane range outside the engine, row_stride < n_act, a header-only handle. */
#define GPF_MASK_TOO_MANY_LINES 0x01
#define GPF_MASK_TOO_MANY_SUBS 0x02
#define GPF_MASK_LINE_COOLDOWN 0x04
#define GPF_MASK_SUB_COOLDOWN 0x08
#define GPF_MASK_AMBIGUOUS 0x10
int gpf_topo_action_mask(gpf_handle h, int32_t lane0, int32_t n, uint8_t* out_dev, int64_t row_stride);
int gpf_get_topo_action_mask(gpf_handle h, int32_t lane0, int32_t n, uint8_t* host_out);

/* ---- the opponent of the batched acting path (grid2op_amd/csrc/gridpf_opponent.hpp): the reference's OpponentSpace
 * (Opponent/opponentSpace.py:144-249: budget, attack duration and attack cooldown) with one of its three single-area line opponents --
 * RandomLineOpponent (Opponent/randomLineOpponent.py:94-106), WeightedRandomOpponent (Opponent/weightedRandomOpponent.py:139-164),
 * GeometricOpponent (Opponent/geometricOpponent.py:169-293) -- run for every lane by ONE side kernel (opponent_prestep_kernel) queued after the
 * topology pre-step and before the step of a ONE-STEP gpf_step_n launch, so that the attack is added after the agent's action and wins
 * (Environment/baseEnv.py:3148-3170, called at :3839): the attacked line is forced out of the lane's topology row (both ends -1) at every
 * step of the attack's duration, its line cooldown is raised to max(remaining duration, cooldown) before the step's own decrement (a fresh
 * attack of duration 3 shows 2 in the next observation); the agent's legality was decided on the cooldowns from before the attack.
 * The opponent reads the lane's rho and line_status RESULT rows of its last step (the observation at time t).  A lane with no completed
 * step in its episode (steps survived = 0: a fresh lane, after gpf_reset_lanes, after an auto-reset) is the reference's `observation is
 * None` call of env.reset(): its opponent is reset (OpponentSpace.reset, :96-106), nothing else happens, not even the budget increment.  A
 * done lane without auto-reset is left alone.  The budget restates numpy's arithmetic: float32 until the first paid attack step, whose
 * integer cost widens it to float64; float32 increments are then added in float64; a reset goes back to float32.
 * Random numbers: the automaton consumes uniforms u in [0, 1) of a per-lane stream, one per event in event order:
 *   WeightedRandom draws _next_attack_time : 1 + floor(u * attack_period);   RandomLine picks among n connected lines : the floor(u * n)-th
 *   in attackable-list order;   WeightedRandom / Geometric pick a line : the first index whose cumulative float64 weight is > u * total
 *   (RandomState.choice's cdf.searchsorted(u, side="right"));   Geometric samples its schedule (GPF_OPP_DRAWS_PHILOX only) :
 *   max(1, ceil(log1p(-u) / log1p(-p))), waiting time and duration alternating (sample_attack_times_and_durations, :169-197).
 *   GPF_OPP_DRAWS_TABLE  : gpf_upload_opponent_draws uploads draws[lanes][n_draw]; every lane has a cursor, set to 0 by the upload and NOT by
 *                          a reset (a recorded run goes on across its resets); a lane whose cursor runs past the table stops attacking and
 *                          raises the sticky GPF_OPP_FLAG_DRAWS_EXHAUSTED.  The Geometric schedule comes from gpf_upload_opponent_schedule.
 *   GPF_OPP_DRAWS_PHILOX : Philox4x32-10, key (seed_lo, seed_hi), counter (draw index in the episode, the lane's opponent resets so far,
 *                          lane + lane_base, 0), u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53.  The kernel fills the lane's Geometric schedule
 *                          itself when it resets the lane, up to schedule_cap attacks: if the capacity is reached the schedule ENDS there
 *                          (sticky GPF_OPP_FLAG_SCHEDULE_CAPPED) -- size it for the episode (episode_max_time * hazard rate, with margin).
 *   gpf_set_opponent         : NULL or kind GPF_OPP_NONE turns the opponent off (gpf_step_n then launches nothing for it).  Everything is
 *                              validated before the device is touched: line ids in [0, n_line) and distinct, at least one line, init_budget
 *                              >= 0 (opponentSpace.py:77), attack_period > 0 (weightedRandomOpponent.py:93), rho_normalization finite and > 0,
 *                              hazard and recovery rates in (0, 1] (the rates of geometricOpponent.py:117-135 exist), pmax_pmin_ratio > 0,
 *                              a finite episode_max_time > 0 (geometricOpponent.py:149-155), attack_duration / attack_cooldown >= 0,
 *                              schedule_cap > 0.  Every lane's opponent starts reset; the sticky flags are cleared.
 *   gpf_upload_opponent_draws    : table source; draws[n_lanes][n_draw] doubles in [0, 1); cursors back to 0.
 *   gpf_upload_opponent_schedule : Geometric, table source; schedule[n_lanes][schedule_cap][2] = {waiting time, duration} and count[n_lanes]
 *                                  entries (<= schedule_cap): what the opponent's reset sampled, for the lanes' NEXT resets too until replaced.
 *   gpf_get_opponent_state   : budget[n] and state[n][GPF_OPP_STATE_INTS] of lanes [lane0, lane0 + n) (either may be NULL); entries
 *                              GPF_OPP_S_INFO_LINE / _DURATION are info["opponent_attack_line"] (a line id, -1: none) and
 *                              info["opponent_attack_duration"] of the last launch (baseEnv.py:3890-3892).  Synchronous.
 *   gpf_set_opponent_state   : the same rows written (tests start from arbitrary states).
 * gpf_step_n with an opponent set refuses n_steps != 1 (the choice needs the previous step's rho) and track_cooldown == 0 (the attacked
 * line's cooldown is only counted down by a launch that maintains the line cooldowns).  gpf_copy_lanes copies the opponent state;
 * gpf_fanout_n1 and gpf_simulate_batch never run the opponent and leave its state alone. */
#define GPF_OPP_NONE 0
#define GPF_OPP_RANDOM_LINE 1
#define GPF_OPP_WEIGHTED_RANDOM 2
#define GPF_OPP_GEOMETRIC 3
#define GPF_OPP_DRAWS_TABLE 0
#define GPF_OPP_DRAWS_PHILOX 1
#define GPF_OPP_STATE_INTS 14
#define GPF_OPP_S_BUDGET_IS_F32 0  /* the budget is still a numpy.float32 */
#define GPF_OPP_S_DURATION 1       /* current_attack_duration */
#define GPF_OPP_S_COOLDOWN 2       /* current_attack_cooldown */
#define GPF_OPP_S_LINE 3           /* last_attack: the attacked line, -1 for None */
#define GPF_OPP_S_PREVIOUS_FAILS 4
#define GPF_OPP_S_NEXT_TIME 5      /* _next_attack_time; GPF_OPP_TIME_NONE for None (the reference counts it below zero after a refused attack) */
#define GPF_OPP_S_COUNTER 6        /* Geometric: _attack_counter */
#define GPF_OPP_S_N_SCHEDULE 7     /* Geometric: _number_of_attacks */
#define GPF_OPP_S_CURSOR 8         /* draws consumed */
#define GPF_OPP_S_EPISODE 9        /* resets of the lane's opponent so far */
#define GPF_OPP_S_FLAGS 10         /* sticky GPF_OPP_FLAG_* */
#define GPF_OPP_S_INFO_LINE 11
#define GPF_OPP_S_INFO_DURATION 12
#define GPF_OPP_TIME_NONE (-2147483647 - 1)
#define GPF_OPP_FLAG_DRAWS_EXHAUSTED 1
#define GPF_OPP_FLAG_SCHEDULE_CAPPED 2
typedef struct gpf_opponent_desc {
  int32_t kind;                        /* GPF_OPP_* */
  int32_t n_lines;
  const int32_t* line_ids;             /* [n_lines] attackable lines, in the order of the reference's lines_attacked */
  const double* rho_normalization;     /* [n_lines] or NULL (ones): WeightedRandom */
  int32_t attack_period;               /* WeightedRandom */
  double attack_hazard_rate;           /* Geometric: 1 / (ts_per_hour * (attack_every_xxx_hour - average_attack_duration_hour)) */
  double recovery_rate;                /*            1 / (ts_per_hour * (average_attack_duration_hour - minimum_attack_duration_hour)) */
  int32_t recovery_minimum_duration;   /*            int(minimum_attack_duration_hour * ts_per_hour) */
  double pmax_pmin_ratio;
  int32_t episode_max_time;            /*            env.max_episode_duration() */
  float init_budget;                   /* opponent_init_budget (numpy.float32 in the reference) */
  float budget_per_ts;                 /* opponent_budget_per_ts */
  int32_t attack_duration;             /* opponent_attack_duration */
  int32_t attack_cooldown;             /* opponent_attack_cooldown */
  int32_t draw_source;                 /* GPF_OPP_DRAWS_* */
  uint32_t seed_lo;
  uint32_t seed_hi;
  int32_t lane_base;                   /* global index of lane 0 (a sharded engine draws what one engine would) */
  int32_t schedule_cap;                /* Geometric: attacks per episode the lane's schedule can hold */
} gpf_opponent_desc;
int gpf_set_opponent(gpf_handle h, const gpf_opponent_desc* desc);
int gpf_upload_opponent_draws(gpf_handle h, int32_t n_draw, const double* draws);
int gpf_upload_opponent_schedule(gpf_handle h, const int32_t* schedule, const int32_t* count);
int gpf_get_opponent_state(gpf_handle h, int32_t lane0, int32_t n, double* budget, int32_t* state);
int gpf_set_opponent_state(gpf_handle h, int32_t lane0, int32_t n, const double* budget, const int32_t* state);

/* ---- the multi-area opponent: GeometricOpponentMultiArea (Opponent/geometricOpponentMultiArea.py:18-204), the opponent l2rpn_idf_2023
 * ships.  gpf_set_opponent_areas cuts the attackable list of a GPF_OPP_GEOMETRIC opponent into areas; every area is one GeometricOpponent
 * with the descriptor's rates, its own slice of the list (its entries in descriptor order: that order decides the cdf), its own schedule
 * and a row of GPF_OPP_AREA_STATE_INTS ints.  ONE side kernel (opponent_area_prestep_kernel) runs them for every lane, one launch per step
 * whatever the number of areas.  What a step does (attack(), :126-149, under OpponentSpace.attack, opponentSpace.py:177-249):
 *   - every area's counter goes down by one, clamped at -1; the areas are visited in area order;
 *   - a free area (counter -1) calls its sub-opponent's attack() (geometricOpponent.py:230-293) with the space's previous_fails -- the same
 *     flag for every area of the step; a line with duration d sets counter = d and _previous_attacks = that line, no line sets None;
 *   - any other area gets tell_attack_continues (geometricOpponent.py:199-200: _next_attack_time = None) and contributes its line again:
 *     an attack of duration d holds its line for d + 1 steps;
 *   - the answer is the union of the contributed lines with duration 1, so the space asks at every step: 1 > attack_duration drops the
 *     attack and sets previous_fails (even when there was none); the cost is one unit per line (baseActionBudget.py:46-57); cost > budget
 *     drops the attack and sets previous_fails, but the areas have booked their counters and lines, which therefore come back at the next
 *     step; an accepted attack sets current_attack_duration = 1, current_attack_cooldown += attack_cooldown, budget -= cost;
 *   - every line of the accepted union is forced out and its cooldown raised to max(1, cooldown) before the step (baseEnv.py:3148-3170).
 *   - reset() (:88-92): counters to -1, every sub-opponent reset (counter 0, _next_attack_time None, schedule resampled); _previous_attacks
 *     is LEFT as it is.
 * attack_cooldown > 1 cannot be played: with cooldown c two consecutive attacking steps leave current_attack_cooldown = 2 c, and after the
 * next decrement 2 c - 1 > c for every c >= 2 sends the space into its minimum-time-between-attacks branch, which calls the multi-area
 * opponent's own tell_attack_continues: RuntimeError("I should not get there !") (:152-153).  A state written by hand can still reach that
 * branch (GPF_OPP_S_COOLDOWN above attack_cooldown + 1): then no area moves and nothing is attacked at that step.
 * Draws: the lane's ONE stream, one uniform per event in event order -- within a step, area order; on a Philox reset the areas sample their
 * schedules in area order; a sub-opponent with a single line draws nothing.  The two sticky flags stay per lane.
 * The lane's row with areas set: BUDGET_IS_F32, DURATION (0 or 1), COOLDOWN, PREVIOUS_FAILS, CURSOR, EPISODE, FLAGS keep their meaning; LINE and
 * INFO_LINE hold the accepted line of the lowest attacking area (-1: none), INFO_DURATION 1 or 0; NEXT_TIME, COUNTER, N_SCHEDULE are unused.
 *   gpf_set_opponent_areas  : after gpf_set_opponent with kind GPF_OPP_GEOMETRIC; area_of_line[i] in [0, n_area) is the area of entry i of
 *                             the descriptor's line_ids.  n_area = 0 goes back to the single-area opponent; gpf_set_opponent itself clears
 *                             the areas.  Every lane's opponent starts reset.  Refused before the device is touched (on a header-only handle
 *                             too): no opponent or not Geometric, n_area outside [0, GPF_OPP_MAX_AREAS], an entry outside [0, n_area), an
 *                             empty area, attack_cooldown > 1.
 *   gpf_upload_opponent_area_schedule : table source; schedule[n_lanes][n_area][schedule_cap][2] and count[n_lanes][n_area].
 *   gpf_get_opponent_area_state / gpf_set_opponent_area_state : state[n][n_area][GPF_OPP_AREA_STATE_INTS].  The setter refuses a line outside
 *                             the area's list (unless -1), a counter below -1, N_SCHEDULE outside [0, schedule_cap]; with areas set
 *                             gpf_set_opponent_state refuses DURATION > 1.
 *   gpf_get_opponent_attack_lines : attacked[n][n_line], info["opponent_attack_line"] of the last launch (with or without areas).
 * gpf_copy_lanes copies area state and area schedules; gpf_step_n keeps its two refusals; gpf_fanout_n1 and gpf_simulate_batch never run
 * the opponent. */
#define GPF_OPP_MAX_AREAS 16
#define GPF_OPP_AREA_STATE_INTS 8
#define GPF_OPP_AS_COUNTER 0         /* _new_attack_time_counters[a]; -1: the area is free */
#define GPF_OPP_AS_LINE 1            /* _previous_attacks[a]: the line, -1 for None */
#define GPF_OPP_AS_NEXT_TIME 2       /* the sub-opponent's _next_attack_time; GPF_OPP_TIME_NONE for None */
#define GPF_OPP_AS_ATTACK_COUNTER 3  /*                    _attack_counter */
#define GPF_OPP_AS_N_SCHEDULE 4      /*                    _number_of_attacks */
#define GPF_OPP_AS_INFO_LINE 5       /* the area's line in the ACCEPTED attack of the last launch, -1 for none */
                                     /* 6, 7: reserved, always 0 */
int gpf_set_opponent_areas(gpf_handle h, int32_t n_area, const int32_t* area_of_line);
int gpf_upload_opponent_area_schedule(gpf_handle h, const int32_t* schedule, const int32_t* count);
int gpf_get_opponent_area_state(gpf_handle h, int32_t lane0, int32_t n, int32_t* state);
int gpf_set_opponent_area_state(gpf_handle h, int32_t lane0, int32_t n, const int32_t* state);
int gpf_get_opponent_attack_lines(gpf_handle h, int32_t lane0, int32_t n, uint8_t* attacked);

/* ---- alerts and AlertReward of the batched acting path (grid2op_amd/csrc/gridpf_alert.hpp): the bookkeeping of an environment whose
 * alerts_info.json says {"by_line": "opponent"} (l2rpn_idf_2023), for every lane of a one-step launch, in two side kernels -- one queued
 * after the opponent's kernel and before the step, one after the step; the step, power-flow, topology and opponent kernels are not
 * involved, and with alerts off gpf_step_n launches nothing for them.  The A alertable lines are the current opponent's attackable lines in
 * its order (with areas: grouped by area, descriptor order inside an area -- the reference's flattened lines_attacked).
 *   - BaseEnv._update_alert_properties (Environment/baseEnv.py:3295-3329) runs in every step that reaches the backend, after the opponent
 *     and before the power flow: last_alert, time_since_last_alert, alert_duration, total_number_of_alert, then with an attack
 *     (info["opponent_attack_line"] is not None: here a non-zero row of gpf_get_opponent_attack_lines; an attack refused for budget is none)
 *     time_since_last_attack = 0 on the lines attacked for the first time, +1 on the others that are not -1, is_already_attacked set on the
 *     attacked lines and NOT cleared on a line that leaves a continuing attack; without an attack +1 and is_already_attacked cleared; then
 *     attack_under_alert = 2 last_alert - 1 where time_since_last_attack == 0 and 0 where it exceeds time_window.
 *   - BaseEnv._reset_alert (:1677-1685) on the lane's env.reset() launch (no completed step in its episode) and gpf_reset_lanes.
 *   - AlertReward (Reward/alertReward.py:105-207): two boolean rings of time_window + 2 rows; per step the ring index advances, the newly
 *     attacked lines are noted, the alerts are noted, was_alert_used_after_attack is cleared; a step that fails (the engine's done: the
 *     reference's blackout, done and has_error) gives every line attacked in the last time_window + 1 rows the alert of the FIRST row where
 *     it was noted: was_alert_used_after_attack = 2 alert - 1, reward = mean(alert) (max_blackout - min_blackout) + min_blackout (0 without
 *     such a line); any other step scores the row time_window steps back: was_alert_used_after_attack = 1 - 2 alert, reward =
 *     (min_no_blackout - max_no_blackout) mean(alert) + max_no_blackout, the row is cleared.  The mean is a count ratio in float64, the
 *     result float32.  reward_end_episode_bonus applies when done comes without an error (alertReward.py:179-181): that is a step
 *     truncated by gpf_set_episode_limit, which carries the bonus; without a limit the engine has no such done.  Alarms, the alert budget and
 *     _is_alert_illegal (always False in the reference) are not modelled; the agent's alert survives an illegal or ambiguous topology action
 *     (baseEnv.py:3716-3766), so alerts are booked whatever gpf_get_topo_flags says.
 *   gpf_set_alerts      : NULL turns alerts off, as gpf_set_opponent and gpf_set_opponent_areas do.  Refused before the device is touched
 *                         (on a header-only handle too): no opponent, more than GPF_ALERT_MAX_LINES attackable lines, time_window outside
 *                         [1, GPF_ALERT_MAX_WINDOW], a constant that is not finite.  Every lane starts reset.
 *   gpf_set_lane_alerts : mask[n_lanes] for the NEXT launch, bit i = an alert on alertable line i (NULL: none); a bit at or above A is
 *                         GPF_E_INVALID.  gpf_alerts_on_device(h, 1): the next launch takes the masks the caller wrote into the device buffer
 *                         (gpf_alert_device_pointers entry 0); there the kernel drops the bits at or above A, which are outside the feature's
 *                         domain.  Both are consumed by the launch, like the topology actions.
 *   gpf_get_alert_state / gpf_set_alert_state : state[n][gpf_alert_state_ints] int32 rows, A = number of alertable lines, R = time_window + 2:
 *                         [0, 7 A) seven arrays of A: last_alert, is_already_attacked, time_since_last_alert, alert_duration,
 *                         time_since_last_attack, attack_under_alert, was_alert_used_after_attack; [7 A] total_number_of_alert; [7 A + 1]
 *                         AlertReward._current_id; [7 A + 2] 1: the lane's bookkeeping ran in the last launch (its post-step scores it);
 *                         [7 A + 3, 8 A + 3) _lines_currently_attacked; then _ts_attack [R][A] and _alert_launched [R][A].  The row length is
 *                         8 A + 3 + 2 R A (gpf_alert_state_ints(h, &n) returns it).  The setter refuses booleans outside {0, 1}, a
 *                         _current_id outside [0, R), counters below -1 / 0.
 *   gpf_get_alert_reward: reward[n] of the last launch (0 on a lane that was reset or left alone).
 *   gpf_alert_device_pointers : out[0] the alert masks uint64 [lane capacity], out[1] the rewards float32 [lane capacity], out[2] the
 *                         observation block int32 [lane capacity][6 A + 1]: sections of A at GPF_ALERT_OBS_* x A, total_number_of_alert at
 *                         6 A.  n must be GPF_N_ALERT_POINTERS.  (A call of its own: the length of gpf_device_pointers' table is fixed.)
 * gpf_copy_lanes copies the alert state, gpf_reset_lanes resets it; gpf_fanout_n1 and gpf_simulate_batch leave it alone (AlertReward
 * returns 0 inside simulate); gpf_step_n with alerts on keeps the opponent's two refusals. */
#define GPF_ALERT_MAX_LINES 64
#define GPF_ALERT_MAX_WINDOW 62
#define GPF_N_ALERT_POINTERS 3
#define GPF_ALERT_OBS_ACTIVE 0
#define GPF_ALERT_OBS_SINCE_ALERT 1
#define GPF_ALERT_OBS_DURATION 2
#define GPF_ALERT_OBS_SINCE_ATTACK 3
#define GPF_ALERT_OBS_UNDER_ALERT 4
#define GPF_ALERT_OBS_USED 5
#define GPF_ALERT_OBS_TOTAL 6
typedef struct gpf_alert_desc {
  int32_t time_window;             /* Parameters.ALERT_TIME_WINDOW (12) */
  float reward_min_no_blackout;    /* -1 */
  float reward_min_blackout;       /* -10 */
  float reward_max_no_blackout;    /* 1 */
  float reward_max_blackout;       /* 2 */
} gpf_alert_desc;
int gpf_set_alerts(gpf_handle h, const gpf_alert_desc* desc);
int gpf_set_lane_alerts(gpf_handle h, const uint64_t* mask);
int gpf_alerts_on_device(gpf_handle h, int32_t on);
int gpf_alert_state_ints(gpf_handle h, int32_t* n_ints);
int gpf_get_alert_state(gpf_handle h, int32_t lane0, int32_t n, int32_t* state);
int gpf_set_alert_state(gpf_handle h, int32_t lane0, int32_t n, const int32_t* state);
int gpf_get_alert_reward(gpf_handle h, int32_t lane0, int32_t n, float* reward);
int gpf_alert_device_pointers(gpf_handle h, void** out, int32_t n);

/* ---- the environment's rewards of the batched acting path (grid2op_amd/csrc/gridpf_reward.hpp): what env.step returns as `reward` and
 * info["rewards"], for every lane of a ONE-STEP launch, in one side kernel queued last (after the alert post-step); the step, power-flow,
 * topology, opponent and alert kernels are not involved, and with rewards off gpf_step_n launches nothing for them.  A lane has up to
 * GPF_REWARD_MAX_SLOTS slots (the reference's reward_class + other_rewards); a slot is a kind and its parameters p[]:
 *   GPF_RW_REDISP (Reward/redispReward.py:169-211)  p = alpha_redisp, max_regret, min_reward, reward_illegal_ambiguous, dts
 *       failed: min_reward; illegal or ambiguous: reward_illegal_ambiguous; else
 *       (max_regret - mc dts (sum gen_p - sum load_p + alpha sum|actual_dispatch| + sum|storage_power|)) / sum load_p, mc the largest
 *       gen_cost_per_mw over the generators whose gen_p of this step is > 0.  dts: hours per step (delta_time_seconds / 3600).
 *   GPF_RW_L2RPN (Reward/l2RPNReward.py:56-77)      no p.  failed: 0; else sum over the lines of
 *       max(1 - min(|a_or| / (|thermal_limit| + float32(0.1)), 1)^2, 0); the flags play no part.
 *   GPF_RW_LINES_CAPACITY (Reward/linesCapacityReward.py:49-62)  no p.  failed, illegal or ambiguous: 0; else with n connected lines and
 *       u = clip(sum rho[connected], 0, n): (n - u) / n.
 *   GPF_RW_ECONOMIC (Reward/economicReward.py:57-71) p = worst_cost, reward_min, reward_max, dts.  failed, illegal or ambiguous: reward_min;
 *       else with c = sum(gen_p cost) dts: reward_min + (reward_max - reward_min) clip(worst_cost - c, 0, worst_cost) / worst_cost.
 *   GPF_RW_GAMEPLAY (Reward/gameplayReward.py:44-52) p = reward_min, reward_max.  failed: reward_min; illegal or ambiguous: reward_min / 2
 *       (a float32 division); else reward_max.
 * failed is the lane's failed step, the engine's done (with auto-reset the done byte still says that the step failed).  Without an episode
 * limit the reference's is_done and has_error coincide; with one (gpf_set_episode_limit) is_done is failed OR truncated, and the two kinds
 * that read it follow: GPF_RW_L2RPN is 0 on a truncated step, GPF_RW_REDISP gives an illegal or ambiguous truncated step min_reward
 * (redispReward.py:171-176; a legal truncated step gets the formula).  gpf_rewards_eval never sees a truncated step.  illegal = the topology flag of THIS launch (a launch without
 * topology actions has none, whatever gpf_get_topo_flags still holds) OR "a redispatch action was cancelled in this step" (the change of
 * gpf_get_env_illegal over the step, from a device-side snapshot queued before it when rewards and dynamics are both on); ambiguous = the
 * topology flag.  The reference's is_illegal_reco cannot occur (generator switch-off is not modelled).
 * Inputs: gen_p / load_p / a_or of the float32 results row, rho, line_status, the thermal limits; actual_dispatch = the dynamics' actual
 * dispatch with gpf_set_env_dynamics on, else the lanes' gpf_set_lane_redispatch delta, else zero; storage_power = the storage set-points
 * of the lane's injection row as float32 (with the dynamics on the step wrote them: the power AFTER _compute_storage's clamps).
 * Arithmetic: every sum, product and maximum in float64 from the float32 inputs, share t of 64 takes elements t, t + 64, ... in order,
 * the shares are combined by a fixed butterfly, the slot is rounded ONCE to float32: the same bits in every run and at every place in
 * the batch.  Out of the reference's domain: GPF_RW_REDISP with no generator at gen_p > 0 (the reference raises) writes a quiet NaN; a
 * zero load sum gives the IEEE quotient; GPF_RW_LINES_CAPACITY with no line connected gives 1, what numpy.interp returns for xp = [0, 0].
 *   gpf_set_rewards   : n_slot = 0 or slots = NULL turns rewards off.  Refused before the device is touched (on a header-only handle too):
 *                       more than GPF_REWARD_MAX_SLOTS slots, an unknown kind, a parameter that is not finite, dts <= 0, GPF_RW_REDISP /
 *                       GPF_RW_ECONOMIC without gen_cost_per_mw [n_gen] or with a cost that is negative or not finite.  Rewards start at 0.
 *   gpf_get_rewards   : reward[n][n_slot] of the last launch (0 on a lane that was reset since).  GPF_E_INVALID while rewards are off and
 *                       when the last gpf_step_n was a multi-step launch (it queues nothing for rewards).
 *   gpf_rewards_eval  : the same rules on the lanes' CURRENT state (a state restored or copied into a lane), read-only, queued on the
 *                       engine's stream.  failed here is done or a non-zero status; flags_dev is a DEVICE array [n][2] {illegal, ambiguous}
 *                       (NULL: none).  out_dev = NULL writes the engine-owned rows of the lanes; else rows of row_stride >= n_slot floats.
 *   gpf_reward_device_pointers : out[0] the engine-owned rewards, float32 [lane capacity][n_slot].  n must be GPF_N_REWARD_POINTERS.
 * gpf_reset_lanes zeroes the lanes' rewards; gpf_copy_lanes, gpf_fanout_n1 and gpf_simulate_batch leave them alone. */
#define GPF_REWARD_MAX_SLOTS 8
#define GPF_N_REWARD_POINTERS 1
#define GPF_RW_REDISP 1
#define GPF_RW_L2RPN 2
#define GPF_RW_LINES_CAPACITY 3
#define GPF_RW_ECONOMIC 4
#define GPF_RW_GAMEPLAY 5
#define GPF_RW_N1 7                /* N1Reward (Reward/n1Reward.py:64-101): p[0] = index into the watched lines of gpf_set_n1_screen (below) */
typedef struct gpf_reward_slot {
  int32_t kind;                    /* GPF_RW_* */
  double p[6];                     /* the kind's parameters, in the order above; the rest is ignored */
} gpf_reward_slot;
int gpf_set_rewards(gpf_handle h, int32_t n_slot, const gpf_reward_slot* slots, const float* gen_cost_per_mw);
int gpf_get_rewards(gpf_handle h, int32_t lane0, int32_t n, float* reward);
int gpf_rewards_eval(gpf_handle h, int32_t lane0, int32_t n, const uint8_t* flags_dev, float* out_dev, int64_t row_stride);
int gpf_reward_device_pointers(gpf_handle h, void** out, int32_t n);

/* ---- episode time limits of the batched acting path (grid2op_amd/csrc/gridpf_episode.hpp): the reference's done WITHOUT an error -- the
 * episode ends at max_episode_duration() (chronics_handler.done(), or env.reset(options={"max step": N})) -- for every lane of a ONE-STEP
 * launch, in one side kernel queued last (after the reward kernel: the rewards and the alert reward of a truncated step see the step's
 * state before the reset); the step, power-flow and topology kernels are not involved, and with the feature off gpf_step_n launches
 * nothing for it.  gpf_get_episode and the done byte keep their meaning: the step failed.
 *   limit[lane]     int32 steps, 0: none.  The lane's steps are counted as gpf_get_episode counts them (episode[lane][0], every launch since
 *                   the lane's last reset counts): after gpf_reset_lanes the N-th launch of a lane with limit N is the truncated one, as the
 *                   N-th env.step after env.reset(options={"max step": N}).  (A loop that spends a launch on the reset observation, as the
 *                   opponent and the alerts expect, counts that launch too.)
 *   terminated      the lane's done byte.  truncated = !terminated && limit > 0 && steps survived >= limit, on the state after the step; a
 *                   step that fails at the limit is terminated (the reference's has_error case).
 *   length          env.nb_time_step of the episode that ended in this launch (the limit on truncation; steps survived + 1 on failure: the
 *                   reference counts the failing step), 0 while the episode goes on.
 *   duration_reward EpisodeDurationReward (Reward/episodeDurationReward.py:64-71): length / (limit x per_timestep) when terminated or
 *                   truncated (the length itself with limit 0), else 0; float32, the product in float32 as dt_float keeps total_time_steps.
 *   rewards         see gpf_set_rewards: the reference's is_done is failed || truncated.
 *   alert reward    a truncated lane whose alert pre-step ran gets alert_end_bonus (AlertReward.reward_end_episode_bonus) instead of the
 *                   window scoring (alertReward.py:179-181).  The reference returns it BEFORE _update_state runs, so the final observation's
 *                   was_alert_used_after_attack is what the PREVIOUS step's reward left (it is not cleared, :156); the other six alert
 *                   attributes are the environment's and do not differ.  The engine reproduces that.
 *   returns         with rewards on: return_running[lane][slot] float64 takes every launch's float32 reward, widened, ONE add per slot and
 *                   launch in launch order (bit-reproducible); when an episode ends the total with the final step's reward moves to
 *                   return_last, length_last takes the length, n_episodes goes up by one and the running total restarts at 0, with or
 *                   without auto_reset.  Rows are GPF_REWARD_MAX_SLOTS wide, the slots beyond n_slot stay 0; gpf_set_rewards zeroes them.
 *   auto_reset      a truncated lane leaves the launch as a failed lane does: topology row = its topo0 row, overflow counters and (when the
 *                   launch tracks them) line cooldowns 0, the dynamics' target / actual / previous / already-modified dispatch, curtailment
 *                   limit and scalars, fresh flag and illegal count cleared, storage charge = charge0, sub_cooldown 0, last_bus from topo0,
 *                   episode = {0, resets + 1} -- the opponent and the alerts then reset themselves at the next launch, and with
 *                   gpf_set_chronics_cursor on the lane then starts a scenario (off: the chronics cursor runs on).  The results row, rho, rewards and flags stay those of the final step: the terminal observation.  The host
 *                   re-keys a lane an action had moved to another topology class exactly as for a failure.  Without auto_reset a truncated
 *                   lane is left alone: it reports truncated again at every later launch, its statistics roll over once.
 *   gpf_set_episode_limit : lane_max_steps [n_lanes] (NULL: max_steps for every lane).  NULL, or max_steps 0 without a table, turns the
 *                   feature off.  Refused before the device is touched (on a header-only handle too): a negative limit, a per_timestep that
 *                   is not finite or not positive, a bonus that is not finite.  A new limit on a running feature keeps the statistics.
 *                   While a limit is set gpf_step_n refuses n_steps != 1.
 *   gpf_get_episode_ends  : terminated [n], truncated [n], length [n], duration_reward [n] of the last launch; any pointer may be NULL.
 *   gpf_get_episode_stats : return_running / return_last [n][GPF_REWARD_MAX_SLOTS], length_last [n], n_episodes [n]; any may be NULL.
 *   gpf_episode_device_pointers : out[0] limits int32 [lanes], out[1] flags uint8 [lanes][2] {terminated, truncated}, out[2] length int32,
 *                   out[3] duration_reward float32, out[4] return_running, out[5] return_last float64 [lanes][GPF_REWARD_MAX_SLOTS],
 *                   out[6] length_last, out[7] n_episodes int32 [lanes] (lanes = gpf_lane_capacity).  n must be GPF_N_EPISODE_POINTERS.
 *   The getters fail with "episode limits are off" while the feature is off.
 * gpf_reset_lanes zeroes every episode buffer of the lanes (not their limits); gpf_copy_lanes copies them with the limits; gpf_fanout_n1
 * and gpf_simulate_batch leave them alone.  OUT OF SCOPE: truncation inside multi-step launches, CombinedReward (the scenario
 * of the next episode: gpf_set_chronics_cursor below; N1Reward: gpf_set_n1_screen below). */
#define GPF_N_EPISODE_POINTERS 8
typedef struct gpf_episode_desc {
  int32_t max_steps;               /* the limit of every lane (0: none) ... */
  const int32_t* lane_max_steps;   /* ... or one per lane [n_lanes] (NULL: max_steps) */
  float per_timestep;              /* EpisodeDurationReward.per_timestep (1) */
  float alert_end_bonus;           /* AlertReward.reward_end_episode_bonus (1) */
} gpf_episode_desc;
int gpf_set_episode_limit(gpf_handle h, const gpf_episode_desc* desc);
int gpf_get_episode_ends(gpf_handle h, int32_t lane0, int32_t n, uint8_t* terminated, uint8_t* truncated, int32_t* length, float* duration_reward);
int gpf_get_episode_stats(gpf_handle h, int32_t lane0, int32_t n, double* return_running, double* return_last, int32_t* length_last,
                          int32_t* n_episodes);
int gpf_episode_device_pointers(gpf_handle h, void** out, int32_t n);

/* ---- the N-1 screen of the batched acting path (grid2op_amd/csrc/gridpf_n1.hpp): the reference's N1Reward (Reward/n1Reward.py:64-101),
 * one per watched line, for every environment lane of a ONE-STEP launch.  After env.step the reference copies the backend's state, takes
 * line l_id out (n1Reward.py:78-88), runs one power flow (:89-96) and returns max(a_or / thermal_limit) (:97-101).  Here the copies are
 * ordinary lanes: lanes [0, n_env) are the environments, lane n_env + i K + k is contingency k of environment i.  While the screen is on
 *   - gpf_step_n steps lanes [0, n_env) only (their results are bit-identical to a launch without the screen) and refuses n_steps != 1; every other side kernel of the launch runs over all lanes as before, and every getter reads the
 *     contingency lanes like any lane: lane n_env + i K + k holds the whole post-contingency observation;
 *   - behind the step and the topology post-step, in front of the reward and episode kernels, the launch queues: n1_fanout_kernel (the
 *     contingency lane takes the environment's injection row, its topology row -- after the agent's action, the opponent's attack,
 *     maintenance and protection trips -- with both ends of the watched line at -1, and its shunt buses; a watched line that is already
 *     out leaves the base case), ONE plain AC power flow of lanes [n_env, n_env (1 + K)) with the launch's max_iter and tol_mva (DC
 *     initialisation, no cascade, no dynamics, no cooldowns: what gpf_runpf does), n1_reduce_kernel and n1_summary_kernel.  No host
 *     work per environment or per contingency and no synchronisation: the watched lines were uploaded once, the plans of the two lane
 *     ranges are cached with lane lists of their own and re-made only after something invalidated the batch's plan (a topology class
 *     of an environment lane changed, a reset, gpf_set_topology ...); the contingency lanes then take their environments' planning
 *     entries (a single line outage never changes a lane's topology class);
 *   - value[i][k] float32: is_done (failed or truncated, as the rewards take it) -> 0 (BaseReward's reward_min, N1Reward sets none); the
 *     power flow did not converge -> -1; else max over the lines of a_or / th with th[th <= 1] = 1, ONE float32 division per line and an
 *     exact maximum (share t of 64 takes lines t, t + 64, ..., a fixed butterfly): the same bits in every run and at every lane;
 *   - summary of environment i: arg_worst = the contingency that ranks first (a diverged one outranks every value, then the larger
 *     value, then the lower k), worst = its value (-1 when one diverged), n_insecure = the values > 1 or diverged, n_diverged;
 *   - a reward slot of kind GPF_RW_N1 with p[0] = k is value[lane][k] on an environment lane (0 on a contingency lane): it enters the
 *     episode returns like any slot, and gpf_rewards_eval returns the last launch's table entry for it.  gpf_set_rewards refuses the
 *     kind while the screen is off and an index outside [0, K); more than GPF_REWARD_MAX_SLOTS watched lines are read from the table.
 * Instance groups: on small grids the step kernel packs 4 (<= 8 substations) or 2 (<= 24) lanes into a wavefront.  The environment lanes
 * keep the groups, and so the bits, of a launch without the screen whatever n_env is: a range that does not end on a group runs from a
 * lane list padded with ghost lanes.  The contingency range is planned as gpf_runpf plans a lane range (narrower groups when it does
 * not start on one: choose n_env a multiple of the group width for the fastest power flows).
 *   gpf_set_n1_screen : lines [n_lines] watched line ids; n_lines = 0 turns the screen off.  Refused before the device is touched (on a
 *                       header-only handle too): a negative n_lines, a line id outside [0, n_line), n_env <= 0, n_env (1 + n_lines) >
 *                       n_lanes, and any change while a GPF_RW_N1 slot is set (set the rewards anew afterwards).  The contingency lanes
 *                       start no scenario of their own (the chronics cursor's skip byte, as after gpf_fanout_n1).
 *   gpf_get_n1_values : value[n][K] of environments [lane0, lane0 + n) within [0, n_env), of the last launch (0 before the first).
 *   gpf_get_n1_summary: worst [n] float32, arg_worst / n_insecure / n_diverged [n] int32; any pointer may be NULL.
 *   gpf_n1_device_pointers : out[0] value float32 [n_env][K], out[1] worst float32 [n_env], out[2] int32 [n_env][3] {arg_worst,
 *                       n_insecure, n_diverged}, out[3] the watched lines int32 [K].  n must be GPF_N_N1_POINTERS.
 *   The getters fail with "the N-1 screen is off" while it is off.
 * OUT OF SCOPE: a DC or LODF screen (gpf_lodf_screen), other contingencies than single lines, the screen inside multi-step launches,
 * gpf_simulate_batch or trajectory mode, skipping the power flows of lanes that are done (solved and ignored). */
#define GPF_N_N1_POINTERS 4
int gpf_set_n1_screen(gpf_handle h, int32_t n_env, const int32_t* lines, int32_t n_lines);
int gpf_get_n1_values(gpf_handle h, int32_t lane0, int32_t n, float* value);
int gpf_get_n1_summary(gpf_handle h, int32_t lane0, int32_t n, float* worst, int32_t* arg_worst, int32_t* n_insecure, int32_t* n_diverged);
int gpf_n1_device_pointers(gpf_handle h, void** out, int32_t n);

/* ---- the look-ahead screen: per-lane candidates of the action table simulated on the device (grid2op_amd/csrc/gridpf_lookahead.hpp) ----
 * What an agent does with obs.simulate at every step (Observation/baseObservation.py:3365-3670 -> Environment/_obsEnv.py): simulate its
 * K best actions and play the one with the lowest simulated rho.max() that is legal and does not end the episode.  Here environment i
 * is lane i < n_env, its candidates are K indices into the uploaded action table (gpf_upload_topo_actions) in a device buffer, and
 * candidate (i, k) is played on scratch lane n_env + i K + k -- the layout of the N-1 screen and of gpf_simulate_batch with
 * dst_lane0 = n_env.  One gpf_lookahead call:
 *   - the scratch lane takes everything gpf_simulate_batch copies from a source (injection row, protection counters, line cooldowns,
 *     chronics table and the absolute chronics / forecast row, jitter, redispatch delta, dynamics state) and the environment's topology
 *     and shunt rows, substation cooldowns and last known busbars, all from the device;
 *   - scheduled maintenance ahead of the observation takes its lines out before the action (_ObsEnv.init, _obsEnv.py:361-385: the rule
 *     of gpf_simulate_batch, stated once for both);
 *   - entry cand[i][k] goes through steps 1-4 of the acting path (ambiguity, impact, LookParam + PreventReconnection with the
 *     environment's cooldowns and gpf_set_topo_rules, _BackendAction.__iadd__): the code of the topology pre-step, not a copy.  -1 is the
 *     do-nothing candidate; an index outside the table is ambiguous; an ambiguous or illegal entry leaves the do-nothing row and its flag;
 *   - the scratch lanes are stepped ONCE as gpf_simulate_batch steps them (no cooldown tracking, no auto-reset, no outage tables, no
 *     opponent), time_step 0 on the observation's own injections, time_step >= 1 on the uploaded forecasts;
 *   - value[i][k] float32 = the maximum over the lines of the scratch lane's rho row as the step wrote it (a maximum of stored float32:
 *     exact in any order), +inf when the simulated step ended the episode; flags[i][k] = GPF_LA_ILLEGAL | GPF_LA_AMBIGUOUS (what
 *     sim_info["is_illegal"] / ["is_ambiguous"] say; for a valid index, set exactly when gpf_topo_action_mask's byte is non-zero) |
 *     GPF_LA_DONE; best[i] = the slot with flags == 0 and the lowest value, the lowest k on a tie, -1 (best_value +inf) when no slot is
 *     playable; info[i] = {playable slots, done slots}.
 * The environment lanes are only read: their rows, cooldowns, flags, pending actions and the planner's record of them stay as they were.
 * Nothing plays the choice: write table[cand[i][best[i]]] (or -1) into act_topo and step.  While the look-ahead is set gpf_step_n steps
 * lanes [0, n_env) only and refuses multi-step launches; the scratch lanes stay readable (gpf_get_results, gpf_get_step_outputs) on
 * their range.  Host work: one read-back of the count of scratch lanes whose topology class or busbar count left the one the planner
 * noted, then only those lanes' rows; the plans of the two lane ranges are cached.  Forecast horizons beyond 1 use the observation's
 * cooldowns unchanged (the reference counts them down by time_step - 1).
 *   gpf_set_lookahead : n_cand = 0 switches it off.  Refused before the device is touched (on a header-only handle too): no action
 *                       table, composite slots (gpf_set_topo_slots > 1), rules by area (gpf_set_topo_areas), n_env <= 0,
 *                       n_env (1 + n_cand) > n_lanes, the N-1 screen on (and gpf_set_n1_screen while this is set: both claim the lanes
 *                       behind the environments), a grid whose rows do not fit the 64 KiB of LDS of the play kernel.
 *   gpf_lookahead     : cand [n_env][n_cand] from the host, or NULL: what is in the engine-owned device buffer (out[0] below), written
 *                       on the engine's stream.  Refused: off, a horizon without forecasts (gpf_simulate_batch's reason), combined mode
 *                       with injection actions pending, the table checks above.
 *   gpf_get_lookahead : the outputs of environments [env0, env0 + n) of the last call; any pointer may be NULL.
 *   gpf_lookahead_device_pointers : out[0] cand int32 [n_env][K], out[1] value float32 [n_env][K], out[2] flags uint8 [n_env][K], out[3]
 *                       best int32 [n_env], out[4] best_value float32 [n_env], out[5] info int32 [n_env][2].  n must be
 *                       GPF_N_LOOKAHEAD_POINTERS.
 *   The getters fail with "the look-ahead is off" while it is off.
 * OUT OF SCOPE: composite slots and rules by area, injection candidates (redispatch, storage, curtailment), a scratch lane as an
 * environment (chained horizons and playing the choice inside the call: the look-ahead chain below), the opponent inside the look-ahead,
 * simulated rewards as a pinned feature (gpf_rewards_eval on the scratch range works as after gpf_simulate_batch), the look-ahead inside
 * multi-step launches. */
#define GPF_N_LOOKAHEAD_POINTERS 6
#define GPF_LA_ILLEGAL 1
#define GPF_LA_AMBIGUOUS 2
#define GPF_LA_DONE 4
int gpf_set_lookahead(gpf_handle h, int32_t n_env, int32_t n_cand);
int gpf_lookahead(gpf_handle h, int32_t t_obs, int32_t time_step, const int32_t* cand, const gpf_step_opts* opts);
int gpf_get_lookahead(gpf_handle h, int32_t env0, int32_t n, float* value, uint8_t* flags, int32_t* best, float* best_value, int32_t* info);
int gpf_lookahead_device_pointers(gpf_handle h, void** out, int32_t n);

/* ---- the look-ahead chain: candidates held over several forecast steps (grid2op_amd/csrc/gridpf_lookahead.hpp) ----
 * What agents do with obs.get_forecast_env() (Observation/baseObservation.py:4724-4842) or chained sim_obs.simulate: play the candidate,
 * do nothing for the rest of the forecast horizon, keep the action only if the grid survives -- a line above its limit that the
 * protections trip nb_ts_allowed steps later, the cascade behind the trip and a maintenance that begins two steps ahead are invisible
 * to a one-step look-ahead.  A chain of n_steps = H on the scratch lanes of gpf_set_lookahead, scratch lane q = (environment i, slot k):
 *   - step 1 is exactly gpf_lookahead(t_obs, 1): the lane becomes its environment (protection counters included), the candidate is played
 *     under the environment's rules, the lane is stepped once on forecast row n_h idx (idx: the observation's row);
 *   - steps h = 2 .. H: the lane's chronics cursor moves to forecast row n_h idx + (h - 1), every line whose scheduled maintenance covers
 *     row idx + h (the rule of the look-ahead, from the table it keeps) goes out in the lane's topology row and in the row an auto-reset
 *     would restore, no action is played, and the scratch range is stepped once more on the cached plan.  The step kernel counts the
 *     overflows and trips lines on its own; with gpf_set_env_dynamics on every step is one more do-nothing step of the dynamics.  There
 *     is no read-back and no re-planning between steps: a line outage never changes a lane's planning class;
 *   - per step, sticky (the step kernel overwrites `done` at every step): survived[q] = the steps completed before the first failure (H:
 *     none failed, 0: step 1 failed); later steps of a failed lane are solved and ignored; value_h[q][h - 1] = the maximum of the lane's
 *     float32 rho row after step h, +inf from the failing step on;
 *   - value[q] = the maximum of value_h over the horizon (+inf if the lane failed anywhere), GPF_LA_DONE = it failed anywhere; value,
 *     flags, best, best_value and info keep the meaning of gpf_lookahead with "the step" read as "the chain" (the look-ahead's own
 *     buffers: gpf_get_lookahead); peak[q] = the maximum over the survived steps only, -inf when survived is 0;
 *   - fallback[i] = among the slots that are neither illegal nor ambiguous the one with the most survived steps, then the lowest peak,
 *     then the lowest k (-1: none), fallback_steps[i] its survived steps: what an agent plays when every candidate fails in the horizon;
 *   - play = 1 writes the table index of slot best[i] (-1 without one) into the acting path's action buffer of lane i (act_topo), play =
 *     2 that of best[i], else of fallback[i], else -1, and marks the buffer as written on the device (gpf_topo_actions_on_device(1)): the
 *     next gpf_step_n plays the choice.  play = 0 leaves the buffer and the pending actions alone.
 * n_steps = 1 is gpf_lookahead(t_obs, 1) bit for bit.  The environment lanes are only read (play writes their action index alone).
 *   gpf_set_lookahead_chain : max_steps = 0 releases it, and so does gpf_set_lookahead(.., 0) or a new gpf_set_lookahead.  Refused before
 *                       the device is touched: negative max_steps, the look-ahead off.
 *   gpf_lookahead_chain : cand as gpf_lookahead.  Refused before the device is touched: the look-ahead off, the chain off, n_steps < 1,
 *                       n_steps > max_steps, n_steps > the uploaded forecast horizons (gpf_lookahead's refusal of that horizon), play
 *                       outside 0 .. 2, play without one action slot per lane, and everything gpf_lookahead refuses.
 *   gpf_get_lookahead_chain : environments [env0, env0 + n) of the last call: survived int32 [n][K], peak float32 [n][K], value_h float32
 *                       [n][K][max_steps] (columns < n_steps of the last call), fallback / fallback_steps int32 [n]; any may be NULL.
 *   gpf_lookahead_chain_device_pointers : out[0] survived, out[1] peak, out[2] value_h, out[3] fallback, out[4] fallback_steps.  n must be
 *                       GPF_N_LOOKAHEAD_CHAIN_POINTERS.
 *   The getters fail with "the chain is off" while it is off.
 * OUT OF SCOPE: candidates after step 1; cooldown counting on the scratch lanes (do-nothing steps need none: the observation's
 * cooldowns stand); hazards and the opponent inside the chain; the chain as ONE multi-step launch over the consecutive forecast rows
 * (bit-identical by the guarantee of multi-step launches, and the next speed-up); composite slots and areas. */
#define GPF_N_LOOKAHEAD_CHAIN_POINTERS 5
int gpf_set_lookahead_chain(gpf_handle h, int32_t max_steps);
int gpf_lookahead_chain(gpf_handle h, int32_t t_obs, int32_t n_steps, const int32_t* cand, int32_t play, const gpf_step_opts* opts);
int gpf_get_lookahead_chain(gpf_handle h, int32_t env0, int32_t n, int32_t* survived, float* peak, float* value_h, int32_t* fallback,
                            int32_t* fallback_steps);
int gpf_lookahead_chain_device_pointers(gpf_handle h, void** out, int32_t n);

/* ---- combined topology + injection actions of the batched acting path (grid2op_amd/csrc/gridpf_combined.hpp): one action with a
 * topology part (the table indices above) and an injection part (redispatch / storage / curtailment rows), lane by lane, in a one-step
 * launch.  OFF by default: without this call gpf_step_n refuses such a launch and queues exactly what it queued before.  Paths relative
 * to the reference checkout (Environment/baseEnv.py step):
 *   1. ambiguity is tested on the whole action (Action/baseAction.py:3621-3668, _is_storage_ambiguous :3889-3927,
 *      _is_curtailment_ambiguous :3929-3968): an ambiguous action does nothing in ALL its parts, is_ambiguous and not is_illegal.  The
 *      injection-side rules are value rules, compared in float32 (check_values): a redispatch with |x| >= 1e-7 on a generator that is
 *      not redispatchable, above gen_max_ramp_up, below -gen_max_ramp_down; a storage power outside [-storage_max_p_prod,
 *      storage_max_p_absorb]; a curtailment < 0 (other than -1, "no change") or > 1, or on a generator that is not renewable;
 *   2. the rules run in the order LookParam, PreventDiscoStorageModif, PreventReconnection (baseEnv.py:3754-3767,
 *      Rules/DefaultRules.py:36-44); an illegal action does nothing in all its parts, is_illegal.  PreventDiscoStorageModif
 *      (Rules/PreventDiscoStorageModif.py:39-46) fires on a storage unit whose topo_vect entry before the action is < 0 when the action
 *      gives it a finite power with |p| >= 1e-7 and neither sets it to a busbar > 0 nor changes its bus (with gpf_set_topo_rules on = 0,
 *      AlwaysLegal, it does not exist);
 *   3. the surviving topology reaches the backend action (baseEnv.py:3798) before the redispatch is prepared (:3806): a redispatch the
 *      step cancels as illegal (the case gpf_get_env_illegal counts) leaves the topology applied and books NOTHING for the action -- no
 *      line cooldown, no substation cooldown (:3193-3201, :3373) --, is_illegal_redisp.
 * Three side kernels (one wavefront per lane, no LDS, no atomics) around kernels that stay as they are; queue order of a one-step launch:
 * cursor, SCREEN, topology pre-step, CANCEL, opponent, alert pre-step, reward pre-step, step, SETTLE, topology post-step, alert
 * post-step, rewards, episode.  The screen is queued only when injection actions are pending, the cancel only when topology actions are
 * pending too (else the screen cancels), settle in every one-step launch: three, two or one more dispatch.
 * With check_values on the value rules hold for EVERY lane of the launch, pure injection lanes included (what makes device-written float
 * actions safe), and so does PreventDiscoStorageModif.  A verdict rewrites the lane's rows of the pending action buffers to 0 / 0 / -1
 * and, unless the topology part is ambiguous by its table entry, the lane's slots of act_topo to -1: both are consumed by the launch.
 * gpf_step_n with the mode on:
 *   - topology and injection actions pending for the same launch are accepted;
 *   - a held storage action (hold_storage != 0) pending together with topology actions: GPF_E_INVALID (a combined action cannot suppress
 *     one step of a held action); without topology actions a held storage action stays outside the screen;
 *   - a launch that carries actions of either kind must be a one-step launch.
 * The rewards (gpf_set_rewards) read the flags of the whole step.  Composite actions (gpf_set_topo_slots > 1): the screen tells a
 * topology part that is ambiguous by ONE of its entries; a composite that is ambiguous only between its entries, on a lane where
 * PreventDiscoStorageModif also fires, reports is_illegal where the reference reports is_ambiguous (the action is void either way).
 * OUT OF SCOPE: held storage actions combined with topology, LIMIT_INFEASIBLE_CURTAILMENT_STORAGE_ACTION, minimum up / down times
 * (is_illegal_reco), the value rules against prod_p injections (baseAction.py:3648-3661), anything inside multi-step launches.
 *   gpf_set_combined_actions : needs gpf_set_env_dynamics on and the acting path enabled (GPF_E_INVALID otherwise).  NULL or on = 0: off,
 *                   the refusal of combined launches is back.  storage_max_p_prod / storage_max_p_absorb [n_storage]: may both be NULL
 *                   without storage units or with check_values = 0 (then the storage range is not checked).
 *   gpf_get_action_flags : flags[n][4] {is_illegal, is_ambiguous, is_illegal_redisp, reason} of the last one-step launch in combined mode,
 *                   merged as the reference merges them (an ambiguous action is not also illegal); reason: GPF_CB_*, the screen's rule
 *                   before the topology part's.  gpf_get_topo_flags keeps its meaning, the topology part's own verdict (of the slots
 *                   the screen left).  gpf_reset_lanes clears the flags, gpf_copy_lanes copies them; a lane that auto-resets keeps the
 *                   flags of its final step, as it keeps its topology flags.
 *   gpf_combined_device_pointers : out[0] flags uint8 [lanes][4] (lanes = gpf_lane_capacity).  n must be GPF_N_COMBINED_POINTERS.
 * gpf_simulate_batch and gpf_fanout_n1 leave these buffers alone. */
#define GPF_N_COMBINED_POINTERS 1
#define GPF_CB_NONE 0
#define GPF_CB_REDISP_FIXED_GEN 1      /* redispatch on a generator that is not redispatchable */
#define GPF_CB_REDISP_RAMP_UP 2
#define GPF_CB_REDISP_RAMP_DOWN 3
#define GPF_CB_STORAGE_POWER 4         /* storage power outside the unit's range */
#define GPF_CB_CURTAIL_RANGE 5         /* curtailment < 0 (not -1) or > 1 */
#define GPF_CB_CURTAIL_FIXED_GEN 6     /* curtailment on a generator that is not renewable */
#define GPF_CB_DISCO_STORAGE 7         /* PreventDiscoStorageModif */
#define GPF_CB_TOPO_RULES 8            /* LookParam / PreventReconnection on the topology part */
#define GPF_CB_TOPO_AMBIGUOUS 9        /* the topology part is ambiguous */
typedef struct gpf_combined_desc {
  int32_t on;
  int32_t check_values;
  const float* storage_max_p_prod;
  const float* storage_max_p_absorb;
} gpf_combined_desc;
int gpf_set_combined_actions(gpf_handle h, const gpf_combined_desc* desc);
int gpf_get_action_flags(gpf_handle h, int32_t lane0, int32_t n, uint8_t* flags);
int gpf_combined_device_pointers(gpf_handle h, void** out, int32_t n);

/* ---- the chronics cursor: each new episode starts a scenario, on the device (grid2op_amd/csrc/gridpf_cursor.hpp) ----------------------
 * What Environment.reset does to the time series (Environment/environment.py reset: chronics_handler.next_chronics(), then row 0 of the
 * new scenario is the reset observation), for every lane of a one-step launch (gpf_step_n with n_steps = 1).  ONE side kernel,
 * cursor_prestep_kernel, is queued FIRST in the launch, before the opponent's, the topology actions' and the alerts' pre-steps and before
 * the step kernel; with the feature off nothing is launched and no other kernel changes.
 *   episode start   a lane starts an episode in a launch when its episode[lane][0] (gpf_get_episode: steps survived) is 0 before the step:
 *                   its first launch, the launch after gpf_reset_lanes, the launch after the one in which it failed or was truncated under
 *                   auto_reset.  It is the test the opponent and the alerts use for their own reset.  The lane then takes a position p of
 *                   `order`, sets lane_table = order[p] and lane_offset so that the row gpf_step_n reads at this launch's time index,
 *                   (t + lane_offset) mod T, is first_row, sets pos = p and counts n_started up.
 *   when it moves   at the START of the new episode, not at the end of the old one: after the launch that ended an episode lane_table /
 *                   lane_offset still describe the step that ended it, so the terminal gpf_obs_vector (calendar, time / duration of the
 *                   next maintenance), the rewards and a gpf_simulate_batch from that lane belong to the OLD scenario; after the next
 *                   launch they belong to the new one.
 *   sequential      Multifolder.next_chronics (Chronics/multiFolder.py:290-295): p = next_pos, then next_pos = (p + 1) mod n_order.
 *   sampled         Multifolder.sample_next_chronics (multiFolder.py:341-359) + RandomState.choice: ONE uniform u in [0, 1) per episode
 *                   start, p = the first index with cdf[p] > u (searchsorted side="right").  cdf [n_order] is built by the caller as the
 *                   reference and numpy build it: the probabilities as float32 over their float32 sum, a float64 cumulative sum over its
 *                   last entry.  The device samples POSITIONS of `order`; the reference indexes positions by scenario id on a filtered or
 *                   shuffled order (multiFolder.py:356-358), the same thing whenever order is 0 .. n - 1.
 *   next_pos        int32 [lanes] on the device, writable between launches (gpf_cursor_device_pointers): env.set_id(k) /
 *                   env.reset(options={"time serie id": k}) (Environment/environment.py set_id: chronics_handler.tell_id).  A value >= 0 is
 *                   taken under both policies; the sequential policy leaves the position after it, the sampled policy leaves -1 and draws
 *                   only when it finds a negative value (the sequential policy then follows pos).  The first episode after
 *                   gpf_set_chronics_cursor takes the next_pos of the descriptor as it is.  A value >= n_order written on the device is
 *                   taken modulo n_order and sets GPF_CURSOR_FLAG_NEXT_POS_WRAPPED.
 *   first_row       0 for a loop that spends a launch on the reset observation (the opponent's and the alerts' loops), 1 for one that does
 *                   not, k or k + 1 for env.reset(options={"init ts": k}); one value, or one per lane.
 *   draws           GPF_OPP_DRAWS_TABLE: gpf_upload_cursor_draws gives every lane n_draw float64 uniforms, consumed in order; a used-up
 *                   table sets the sticky GPF_CURSOR_FLAG_DRAWS_EXHAUSTED and the lane restarts its current scenario at first_row.
 *                   GPF_OPP_DRAWS_PHILOX: Philox4x32-10 keyed by the seed on the counter {n_started, 0, lane + lane_base, "curs"}: the
 *                   stream depends on the global lane alone (shards with their lane_base equal one engine) and differs from the
 *                   opponent's under the same seed.
 *   gpf_set_chronics_cursor : NULL turns the feature off.  Refused with GPF_E_INVALID and a message: an empty order, a cdf that is not
 *                   non-decreasing to 1 (sampled), a negative first_row, a next_pos >= n_order, an unknown policy or draw source (these
 *                   on a header-only handle too); no chronics uploaded, an order entry >= n_tables, a first_row >= T.  Every call starts
 *                   the lanes' cursor state afresh (pos -1, n_started 0, no draws); lane_table / lane_offset stay until a lane starts an
 *                   episode.  While it is on: gpf_step_n refuses n_steps != 1 (a restart inside a launch cannot be followed);
 *                   gpf_upload_chronics refuses fewer tables than an order entry needs or fewer rows than a first_row;
 *                   gpf_set_lane_chronics stays legal and positions a lane until its next episode start; gpf_reset_lanes needs nothing
 *                   (it zeroes episode, so the next launch starts a scenario, as env.reset() does); gpf_copy_lanes copies the cursor
 *                   state with lane_table / lane_offset; the contingency lanes of gpf_fanout_n1 and the scratch lanes of
 *                   gpf_simulate_batch are left alone by the kernel until gpf_set_lane_chronics puts them back on the tables;
 *                   gpf_simulate_batch reads its source lanes' two words back before it looks for the maintenance ahead of them.
 *   gpf_upload_cursor_draws : draws [n_lanes][n_draw] in [0, 1); the lanes' draw counters restart at 0.
 *   gpf_get_cursor_state / gpf_set_cursor_state : rows [n][GPF_CURSOR_STATE_INTS] = {table, offset, pos, next_pos, n_started, draws
 *                   used, flags} (a learner's checkpoint; the setter validates table, pos and next_pos).
 *   gpf_cursor_device_pointers : out[0] next_pos (writable), out[1] pos, out[2] n_started, int32 [lanes] (lanes = gpf_lane_capacity).
 * OUT OF SCOPE: scenarios of different lengths (the loader truncates them to one T; the episode's length is the caller's:
 * gpf_set_episode_limit), chunked or generated chronics, anything inside multi-step launches. */
#define GPF_CURSOR_SEQUENTIAL 0
#define GPF_CURSOR_SAMPLED 1
#define GPF_CURSOR_FLAG_DRAWS_EXHAUSTED 1
#define GPF_CURSOR_FLAG_NEXT_POS_WRAPPED 2
#define GPF_CURSOR_STATE_INTS 7
#define GPF_N_CURSOR_POINTERS 3
typedef struct gpf_cursor_desc {
  int32_t n_order;                 /* positions of the order (> 0) */
  const int32_t* order;            /* [n_order] table indices: Multifolder._order after filter and shuffle */
  int32_t policy;                  /* GPF_CURSOR_SEQUENTIAL / GPF_CURSOR_SAMPLED */
  const double* cdf;               /* [n_order], sampled only */
  int32_t first_row;               /* the row the first launch of an episode reads ... */
  const int32_t* lane_first_row;   /* ... or one per lane [n_lanes] (NULL: first_row) */
  int32_t next_pos;                /* the position the first episode takes (< 0: none) ... */
  const int32_t* lane_next_pos;    /* ... or one per lane [n_lanes] (NULL: next_pos) */
  int32_t draw_source;             /* GPF_OPP_DRAWS_TABLE / GPF_OPP_DRAWS_PHILOX */
  uint32_t seed_lo, seed_hi;       /* Philox key */
  int32_t lane_base;               /* global index of lane 0 (sharding) */
} gpf_cursor_desc;
int gpf_set_chronics_cursor(gpf_handle h, const gpf_cursor_desc* desc);
int gpf_upload_cursor_draws(gpf_handle h, int32_t n_draw, const double* draws);
int gpf_get_cursor_state(gpf_handle h, int32_t lane0, int32_t n, int32_t* state);
int gpf_set_cursor_state(gpf_handle h, int32_t lane0, int32_t n, const int32_t* state);
int gpf_cursor_device_pointers(gpf_handle h, void** out, int32_t n);

/* ---- observation vectors assembled on the device (what an agent reads: obs.to_vect(), Space/GridObjects.py to_vect over
 * CompleteObservation.attr_list_vect, Observation/completeObservation.py:140-212, filled by BaseObservation._update_obs_complete,
 * Observation/baseObservation.py:4464-4540; with subtract / divide what gym_compat.BoxGymObsSpace(attr_to_keep, subtract, divide) puts on
 * top of it, gym_compat/box_gym_obsspace.py) -- one float32 row per lane, gathered from the engine's buffers by ONE side kernel on the
 * engine's stream (grid2op_amd/csrc/gridpf_obs.hpp); the step and power-flow kernels are not involved.
 *   gpf_set_obs_clock : the calendar of row 0 of each chronics table, start_minutes[n_tables] minutes since 1970-01-01 00:00 (>= 0), the step
 *                       length in minutes (> 0) and the episode length obs.max_step reports.  A lane's date is that of the chronics row its
 *                       last step read -- (t + lane_offset) mod T of its table, the row index of gpf_step_n for the last time index of the last
 *                       launch (t = 0 before any launch).
 *   gpf_set_obs_spec  : n_seg <= 64 segments[n_seg][5] = {source kind (GPF_OBS_*), source offset, length, destination offset, flags}
 *                       and the per-element affine map value = (x - subtract[i]) / divide[i] in float32 (arrays of `dim` floats; NULL: 0 / 1;
 *                       a segment whose elements all have 0 and 1 is a plain cast, bit for bit).  Source offsets are columns of the results row
 *                       (GPF_OBS_OUT), the calendar field 0..5 = year, month, day, hour, minute, weekday (GPF_OBS_CALENDAR), the float bits of
 *                       the value (GPF_OBS_CONST), an element offset otherwise.  flags bits 0-1: what a lane whose last step ended its episode
 *                       writes when game_over_fill != 0 (BaseObservation.set_game_over, baseObservation.py:1551-1700): 0 zeros, 1 the value as
 *                       computed (calendar, counters, constants), 2 minus one, 3 one.  Everything is validated on the host before the device is
 *                       touched: kinds, source ranges against the grid's sizes, destination ranges that tile [0, dim) without overlap or gap,
 *                       divide != 0.  Sources: GPF_OBS_RHO / GPF_OBS_OVERFLOW are the buffers gpf_step / gpf_step_n maintain (gpf_runpf does NOT
 *                       refresh them); buffers that were never allocated (line / substation cooldowns, the state of the injection dynamics)
 *                       read as zeros, the curtailment limit as 1; the generator margins (baseObservation.py:4393-4410, float32) are zeros until
 *                       gpf_set_gen_limits was called, renewables from gpf_set_gen_renewable; time / duration of the next maintenance are
 *                       GridValue.get_maintenance_time_1d / get_maintenance_duration_1d (Chronics/gridValue.py:264-410) of the uploaded
 *                       MAINTENANCE table at the lane's row (-1 / 0 without a table); current_step is the lane's steps survived, plus one on a
 *                       lane whose last step ended its episode (BaseEnv.nb_time_step counts the failing step); gen_p_before_curtail /
 *                       gen_p_delta read the generator set-points of the lane's injection row as the last launch left them (the reference's
 *                       values while no curtailment limit is acting on the lane).
 *   gpf_obs_vector    : rows of lanes [lane0, lane0 + n) -> out_dev (device memory, row k at out_dev + k * row_stride floats, row_stride >= dim;
 *                       only the first dim floats of a row are written) or, out_dev = NULL, rows lane0.. of the engine-owned [lane capacity][dim]
 *                       buffer (gpf_device_pointers_n entry 32).  Asynchronous on the engine's stream.
 *   gpf_obs_vector_trajectory : [n_steps][n][dim] (dense) of steps [step0, step0 + n_steps) of the last multi-step launch from the per-step
 *                       copies of GPF_TRAJ_OBS (GPF_E_INVALID without them); out_dev must not be NULL.  Calendar and maintenance attributes advance
 *                       with the steps; a step whose status is not converged counts as game over.  Attributes without a per-step copy
 *                       (GPF_OBS_OVERFLOW, GPF_OBS_COOLDOWN_SUB, the dispatch / charge / curtailment state, GPF_OBS_CURRENT_STEP, the two set-point
 *                       attributes) are refused by name.
 *                       GPF_OBS_COOLDOWN_LINE reads the int16 per-step copy of a launch that maintained the line cooldowns
 *                       (gpf_step_opts::track_cooldown) and the lanes' own counters, which then stand for all its steps, of one that did not; a
 *                       failed step has no copy, so with game_over_fill off the attribute is refused in this mode after a tracking launch.
 *   gpf_get_obs_vector: gpf_obs_vector into the engine-owned buffer, then the rows on the host ([n][dim]); synchronous. */
#define GPF_OBS_CONST 0
#define GPF_OBS_OUT 1
#define GPF_OBS_RHO 2
#define GPF_OBS_LINE_STATUS 3
#define GPF_OBS_TOPO_VECT 4
#define GPF_OBS_SHUNT_BUS 5
#define GPF_OBS_OVERFLOW 6
#define GPF_OBS_COOLDOWN_LINE 7
#define GPF_OBS_COOLDOWN_SUB 8
#define GPF_OBS_TARGET_DISPATCH 9
#define GPF_OBS_ACTUAL_DISPATCH 10
#define GPF_OBS_STORAGE_CHARGE 11
#define GPF_OBS_CURTAILMENT_LIMIT 12
#define GPF_OBS_MARGIN_UP 13
#define GPF_OBS_MARGIN_DOWN 14
#define GPF_OBS_CALENDAR 15
#define GPF_OBS_CURRENT_STEP 16
#define GPF_OBS_MAX_STEP 17
#define GPF_OBS_DELTA_TIME 18
#define GPF_OBS_TIME_NEXT_MAINTENANCE 19
#define GPF_OBS_DURATION_NEXT_MAINTENANCE 20
#define GPF_OBS_THERMAL_LIMIT 21
#define GPF_OBS_GEN_P_BEFORE_CURTAIL 22   /* renewables: the generator set-point the last launch left in the injection row, others 0 */
#define GPF_OBS_GEN_P_DELTA 23            /* gen_p of the power flow minus that set-point (what the slack absorbed), float32 */
/* the alert attributes (Observation/baseObservation.py:4630-4636, 5142-5143): the lane's alert block (gpf_set_alerts), A elements each and
 * ONE for the total; refused by gpf_set_obs_spec while alerts are off and, by name, in trajectory mode (no per-step copy).  A game-over
 * lane (:1681-1687) writes 0 / 0 / 0 / 0 and -1 for the first five below and KEEPS the environment's values of the last two: the flags
 * of their segments say so (0, 0, 0, 0, 2, 1, 1). */
#define GPF_OBS_ACTIVE_ALERT 24
#define GPF_OBS_TIME_SINCE_LAST_ALERT 25
#define GPF_OBS_ALERT_DURATION 26
#define GPF_OBS_TOTAL_NUMBER_OF_ALERT 27
#define GPF_OBS_TIME_SINCE_LAST_ATTACK 28
#define GPF_OBS_ATTACK_UNDER_ALERT 29
#define GPF_OBS_WAS_ALERT_USED_AFTER_ATTACK 30
#define GPF_OBS_N_KINDS 31
#define GPF_OBS_MAX_SEGMENTS 64
int gpf_set_obs_clock(gpf_handle h, int32_t n_tables, const int64_t* start_minutes, int32_t step_minutes, int32_t max_step);
int gpf_set_obs_spec(gpf_handle h, int32_t n_seg, const int32_t* segments, int32_t dim, const float* subtract, const float* divide,
                     int32_t game_over_fill);
int gpf_obs_vector(gpf_handle h, int32_t lane0, int32_t n, float* out_dev, int64_t row_stride);
int gpf_obs_vector_trajectory(gpf_handle h, int32_t step0, int32_t n_steps, int32_t lane0, int32_t n, float* out_dev);
int gpf_get_obs_vector(gpf_handle h, int32_t lane0, int32_t n, float* host_out);

/* ---- the observation as a bus graph, assembled on the device (what graph-network policies read: BaseObservation.bus_connectivity_matrix,
 * flow_bus_matrix and the node table of get_energy_graph, Observation/baseObservation.py:2081-2445, 2679-2710) -- one read-only side kernel on
 * the engine's stream (grid2op_amd/csrc/gridpf_graph.hpp) over the lanes' CURRENT rows (topo_vect, shunt buses, the float32 results row, the
 * substation cooldowns), as gpf_obs_vector reads them.  Definitions:
 *   NB = n_sub * n_busbar.  Global bus id g = sub + (busbar - 1) * n_sub (GridObjects.local_bus_to_global).  A line is CONNECTED when both
 *   of its topo_vect entries are > 0.  A global bus is LIVE when it holds an end of a connected line (_aux_fun_get_bus, :2081-2118); n_bus is
 *   the number of live buses; the COMPACT id of a live bus is its rank among the live buses in ascending g.
 * Index row, int32 [lane][width], the sections GPF_GRAPH_* in this order: n_bus (1) | load_bus (n_load) | gen_bus (n_gen) | storage_bus
 *   (n_storage) | line_or_bus (n_line) | line_ex_bus (n_line) | shunt_bus (n_shunt) | bus_global (NB): the compact id of each element's bus,
 *   and g of compact bus k (-1 for k >= n_bus).  An element whose busbar is <= 0, both ends of a line that is not connected and an element on
 *   a busbar that is not live get -1.
 * Node features, float32 [lane][NB][GPF_GRAPH_N_FEATURES], rows k >= n_bus all zero:
 *   0 p  float64 sum from the float32 results row, starting at 0: + the bus's generators in index order, - its loads, - its storage units,
 *        - its shunts, each class in index order; rounded once (the diagonal of flow_bus_matrix(active_flow=True), :2386-2432)
 *   1 q  the same with gen_q, load_q, shunt_q (storage contributes nothing)
 *   2 v  v_ex of the highest-index connected line with its extremity on the bus, else v_or of the highest-index connected line with its
 *        origin on it (the overwrite order of :2694-2695)
 *   3 cooldown  time_before_cooldown_sub of the bus's substation; 0 while the engine does not track it (gpf_set_topo_rules)
 * Dense planes (optional), float32 [lane][3][NB][NB], zero outside [n_bus][n_bus]:
 *   0 bus_connectivity_matrix (:2199-2205): 1 on the live diagonal and at [or][ex], [ex][or] of every connected line
 *   1, 2 flow_bus_matrix, active and reactive (:2434-2441): the diagonal is the node's p / q; for i != j entry [i][j] is minus the float64
 *        sum, over the connected lines in index order, of p_or of a line from i to j and p_ex of a line from j to i, rounded once (parallel
 *        lines add up, as the reference's duplicate csr entries do)
 * Game-over lanes (done), with game_over_fill != 0: n_bus = 1, every element section 0, bus_global[0] = 0 and the rest -1, features and
 *   planes zero (:2163-2177, 2321-2330); with 0 the rows are computed from whatever the lane's buffers hold.
 * Deviations from the reference, on purpose: disconnected elements get the -1 its docstrings promise (it returns the LAST bus, tmplate[-1]);
 *   a shunt on any busbar is mapped by local_bus_to_global (its formula, :2350-2354, is only right on busbar 1); each sum is one float64
 *   sum (it sums float32).  No floating-point atomics: results are the same bits in every run, at every place in the batch and in the host
 *   emulator of tests/native/graph_emul.cpp.
 *   gpf_set_graph_obs : on != 0 builds the static tables (substation -> elements, lines by substation pair) from the grid, on = 0 frees
 *                       them.  GPF_E_INVALID when NB > GPF_GRAPH_MAX_BUS.
 *   gpf_graph_layout  : offsets[GPF_GRAPH_N_SECTIONS] and widths[..] of the index row's sections, *index_width and *nb; any may be NULL.
 *                       Works on a header-only handle.
 *   gpf_graph_obs     : rows of lanes [lane0, lane0 + n) -> caller-owned DEVICE buffers index_out [n][width], features_out [n][NB][4]
 *                       and, unless NULL, dense_out [n][3][NB][NB], all dense.  Asynchronous on the engine's stream (a
 *                       memset of dense_out is queued ahead of the kernel).  Lane range, NULL outputs and "feature off" are refused before
 *                       the device is touched.
 *   gpf_graph_obs_host: the same into HOST arrays; synchronous. */
#define GPF_GRAPH_N_BUS 0
#define GPF_GRAPH_LOAD_BUS 1
#define GPF_GRAPH_GEN_BUS 2
#define GPF_GRAPH_STORAGE_BUS 3
#define GPF_GRAPH_LINE_OR_BUS 4
#define GPF_GRAPH_LINE_EX_BUS 5
#define GPF_GRAPH_SHUNT_BUS 6
#define GPF_GRAPH_BUS_GLOBAL 7
#define GPF_GRAPH_N_SECTIONS 8
#define GPF_GRAPH_N_FEATURES 4
#define GPF_GRAPH_MAX_BUS 1024
int gpf_set_graph_obs(gpf_handle h, int32_t on, int32_t game_over_fill);
int gpf_graph_layout(gpf_handle h, int32_t* offsets, int32_t* widths, int32_t* index_width, int32_t* nb);
int gpf_graph_obs(gpf_handle h, int32_t lane0, int32_t n, int32_t* index_out, float* features_out, float* dense_out);
int gpf_graph_obs_host(gpf_handle h, int32_t lane0, int32_t n, int32_t* index_out, float* features_out, float* dense_out);

/* Trajectory buffers of multi-step launches (n_steps_cap = 0 or what = 0 releases them).
 *   GPF_TRAJ_RHO: rho [cap][n_lanes][n_line] and status [cap][n_lanes] of every step of the last gpf_step_n.
 *   GPF_TRAJ_OBS: in addition the complete backend observation of every step -- results row out [cap][n_lanes][n_out]
 *                 (layout of gpf_get_results), topo_vect [..][dim_topo], shunt_bus [..][n_shunt], line_status [..][n_line]:
 *                 every step of the launch then writes its rows to HBM (1 observation per env.step, as the reference
 *                 returns one per BaseEnv.step); the lane's own rows still return the last step.
 * gpf_get_trajectory / gpf_get_trajectory_obs copy steps [step0, step0+n_steps) of lanes [lane0, lane0+n) -- only steps written
 * by the LAST gpf_step_n are retrievable (GPF_E_INVALID beyond).  Any output pointer may be NULL. */
#define GPF_TRAJ_RHO 1
#define GPF_TRAJ_OBS 2
int gpf_set_trajectory(gpf_handle h, int32_t n_steps_cap, int32_t what);
int gpf_get_trajectory(gpf_handle h, int32_t step0, int32_t n_steps, int32_t lane0, int32_t n, float* rho, int8_t* status);
int gpf_get_trajectory_obs(gpf_handle h, int32_t step0, int32_t n_steps, int32_t lane0, int32_t n, float* out, int32_t* topo_vect,
                           int32_t* shunt_bus, uint8_t* line_status);
/* Episode bookkeeping of the batched steps: done [n] (1: the lane's last step ended its episode), steps_and_resets [n][2]
 * {steps survived since the last (auto-)reset, number of auto-resets}. */
int gpf_get_episode(gpf_handle h, int32_t lane0, int32_t n, uint8_t* done, int32_t* steps_and_resets);
/* The environment's protection counters of lanes lane0..lane0+n-1 (BaseEnv._timestep_overflow, Environment/baseEnv.py:3346-3370:
 * consecutive steps each line has spent above its thermal limit), [n][n_line]: what an environment restored from an observation
 * hands over (Environment/_obsEnv.py init copies obs.timestep_overflow).  gpf_step / gpf_step_n maintain them on the device. */
int gpf_set_overflow_count(gpf_handle h, int32_t lane0, int32_t n, const int32_t* overflow_count);
/* The lanes' line cooldowns (gpf_step_opts::track_cooldown), [n][n_line]; gpf_set_cooldown: what an environment restored from an observation
 * hands over (obs.time_before_cooldown_line).  gpf_get_trajectory_cooldown: the counters after every step of the last multi-step launch,
 * int16 [n_steps][n][n_line] (saturating at 32767), kept with any trajectory (gpf_set_trajectory). */
int gpf_get_cooldown(gpf_handle h, int32_t lane0, int32_t n, int32_t* line_cooldown);
int gpf_set_cooldown(gpf_handle h, int32_t lane0, int32_t n, const int32_t* line_cooldown);
int gpf_get_trajectory_cooldown(gpf_handle h, int32_t step0, int32_t n_steps, int32_t lane0, int32_t n, int16_t* line_cooldown);
/* rho = a_or / thermal_limit (backend.py:1145-1168) and overflow counters of the last gpf_step. */
int gpf_get_step_outputs(gpf_handle h, int32_t lane0, int32_t n, float* rho, int32_t* overflow_count,
                         int32_t* disc_round);

/* ---- DC sensitivity (PTDF) path ------------------------------------------------------------------------------
 * The reference solves B' theta = P from scratch on every DC power flow (pp.rundcpp, pandaPowerBackend.py:1090).
 * For a FIXED topology the DC branch flows are linear in the bus injections: p_or = PTDF * P_bus.
 * gpf_ptdf_build factorises the DC system of the topology currently held by `lane` (host side, once) and keeps the
 * PTDF on the device; gpf_ptdf_flows evaluates lanes [lane0, lane0+n) from their current injection rows (as left
 * by gpf_set_injections / gpf_step) with one FP64 MFMA GEMM (asynchronous); gpf_get_ptdf_flows copies the active
 * power flows at the origin side (MW, float32 [n][n_line]; the extremity side is the negative, DC has no losses).
 * Errors: no in-service slack generator / islanded topology -> GPF_E_INVALID. */
int gpf_ptdf_build(gpf_handle h, int32_t lane);
int gpf_ptdf_get(gpf_handle h, double* ptdf /* [n_line][n_sub*n_busbar] row-major, MW per MW */);
int gpf_ptdf_flows(gpf_handle h, int32_t lane0, int32_t n);
int gpf_get_ptdf_flows(gpf_handle h, int32_t lane0, int32_t n, float* p_or);
/* ---- the same for PER-LANE topologies: the DC matrices of every DISTINCT topology of a lane range factorised ON THE DEVICE ------------
 * The reference factorises B' of whatever topology each environment has on every DC call (pp.rundcpp, pandaPowerBackend.py:1090;
 * N1Reward once per contingency, grid2op/Reward/n1Reward.py:70-99).  gpf_ptdf_build_batch groups lanes [lane0, lane0 + n) by their
 * CURRENT topology rows (as on the device: lines tripped by a cascade included) into classes and, in ONE launch with one workgroup per
 * class, assembles the reduced B', inverts it with a blocked Gauss-Jordan whose panel / trailing updates run on the FP64 matrix cores
 * (v_mfma_f64_16x16x4_f64; 2 n^3 flops per class) and forms PTDF^T and (with_lodf != 0) the LODF table of the class
 * (grid2op_amd/csrc/gridpf_ptdf_batch.hpp).  The host only does the integer work per class (live buses, compact numbering, the
 * connectivity check of rundcpp(check_connectivity=True)).  Afterwards gpf_ptdf_flows / gpf_ptdf_flows_rows / gpf_lodf_screen evaluate
 * every lane against the tables of ITS class (gpf_ptdf_flows and gpf_lodf_screen must be called on exactly [lane0, lane0 + n),
 * gpf_ptdf_flows_rows needs the batch built for all lanes); lanes of a class without sensitivities (islanded topology, no in-service
 * slack, singular pivot) get NaN flows instead of an error.  gpf_ptdf_build switches back to the single-topology tables.
 * Capacity: at most 256 active non-reference buses per topology (GPF_E_CAPACITY).  *n_classes (may be NULL) = distinct topologies. */
int gpf_ptdf_build_batch(gpf_handle h, int32_t lane0, int32_t n, int32_t with_lodf, int32_t* n_classes);
/* lane_class[n]: class of every lane of the built range; class_status[n_classes]: 0 ok, 1 singular pivot, 2 islanded, 3 no in-service
 * slack; class_n[n_classes]: dimension of the reduced B' of the class; *kernel_ms: duration of the build kernel (HIP events).  Any
 * pointer may be NULL. */
int gpf_ptdf_batch_info(gpf_handle h, int32_t* lane_class, int32_t* class_status, int32_t* class_n, double* kernel_ms);
/* tables of one class in the layout of gpf_ptdf_get: ptdf [n_line][n_sub*n_busbar], lodf [n_line][n_line] (either may be NULL) */
int gpf_ptdf_batch_get(gpf_handle h, int32_t cls, double* ptdf, double* lodf);
/* The same over n_rows CONSECUTIVE CHRONICS ROWS of every lane in ONE launch (M = n_lanes x n_rows rows of the GEMM): row j of lane k
 * is chronics row (t0 + j + lane_offset[k]) mod T of table lane_table[k] turned into injections exactly as gpf_step does (loads x
 * lane_scale, non-slack prod_p rescaled to rebalance x sum(load) when rebalance > 0, + the lane's redispatch delta; storage and shunt
 * set-points from the lane's injection row), i.e. the DC flows of the next n_rows DoNothing env steps of the whole batch for the
 * fixed topology of gpf_ptdf_build -- what rundcpp would return at each of them (pandaPowerBackend.py:1090).  Asynchronous;
 * gpf_get_ptdf_flows_rows copies rows [row0, row0 + n_rows) of lanes [lane0, lane0 + n): float32 [n_rows][n][n_line] MW at the origin. */
int gpf_ptdf_flows_rows(gpf_handle h, int32_t t0, int32_t n_rows, double rebalance);
int gpf_get_ptdf_flows_rows(gpf_handle h, int32_t row0, int32_t n_rows, int32_t lane0, int32_t n, float* p_or);
/* DC N-1 screening on top of the PTDF path (what N1Reward / obs.simulate loops do one contingency at a time,
 * grid2op/Reward/n1Reward.py:70-99): post-outage flows are f_l + LODF[l][k] * f_k, so for every lane of the range and
 * every single-line outage k this returns the largest post-outage loading max_l |f_l + LODF[l][k] f_k| / cap_mw[l]
 * (cap_mw NULL: the largest |flow| in MW), computed from the flows left by the last gpf_ptdf_flows; outages that island
 * the grid give +inf.  Synchronous; worst is [n][n_line]. */
int gpf_lodf_screen(gpf_handle h, int32_t lane0, int32_t n, const float* cap_mw, float* worst);

/* ---- measurement ---------------------------------------------------------------------------------------- */
int gpf_sync(gpf_handle h);
/* Event timing of the solver launches on the handle's stream.  mode 0: off.  mode 1 (window): ONE event pair around all
 * launches issued until the next gpf_get_kernel_time / gpf_set_profiling call -- no per-launch events, so back-to-back
 * launches stay back-to-back (a per-launch pair costs ~7 us of stream time per launch on MI355X); the window time divided
 * by the launch count is the average launch duration when the stream never runs dry.  mode 2: every launch is bracketed
 * by its own event pair (exact per-kernel durations, perturbs throughput).  mode 3 (inside a window): the window ENDS at this
 * point of the stream -- the closing event is recorded right behind the launches issued so far (asynchronous, no wait), so that
 * host work between the last launch and the next gpf_get_kernel_time (a barrier with other ranks, say) is not part of the window;
 * without it the window ends when gpf_get_kernel_time / gpf_set_profiling is called. */
int gpf_set_profiling(gpf_handle h, int32_t mode);
/* Sum of the event-measured durations (ms) and number of solver launches since the last call (closes the running
 * window of mode 1 and opens the next one). */
int gpf_get_kernel_time(gpf_handle h, double* total_ms, int64_t* n_launches);
/* out[2] = {gpf_step / gpf_step_n / gpf_simulate_batch step launches since gpf_create, kernel dispatches they issued}.  A batch of a few
 * residency rounds of equal lanes (e.g. 2 048 lanes of a 118-substation grid: 2 x the 1 024 resident blocks) goes out as one dispatch per
 * round, back to back on the engine's stream (gridpf_launch_step.hip); everything else is one dispatch per launch. */
int gpf_get_counters(gpf_handle h, int64_t out[2]);
/* Diagnostics (no reference counterpart): the kernel configuration a launch over ALL lanes would use right now.
 * out[0] busbars per block (1: single-busbar kernel; 2, 3: NB = n_busbar kernel), out[1] instances per wavefront,
 * out[2] wavefronts per instance, out[3] static-table staging tier (0 global memory, 1 program + pair table in LDS, 2 all),
 * out[4] Ybus blocks in registers, out[5] LDS layout keeps the factored DC matrix, out[6] dynamic LDS bytes per block,
 * out[7] topology-class launch. */
int gpf_get_plan(gpf_handle h, int32_t out[8]);
/* Raw device pointers + the stream, for zero-copy interop (grid2op_amd/engine.py: PowerFlowEngine.device_views wraps them as
 * torch tensors).  ptrs[0..21] = inj, topo, shunt_bus, out, topo_vect, line_status, status, chronics, rho, overflow_count, done,
 * episode, bus_vm, bus_va, shunt_bus_out, disc_round, then the trajectory buffers (NULL when not set): traj_rho, traj_status,
 * traj_out, traj_topo_vect, traj_shunt_bus, traj_line_status (rows are padded to gpf_lane_capacity lanes; trajectory buffers are
 * [cap][gpf_lane_capacity][row]); 22..27 = the environment dynamics (NULL while they are off): the action buffers redispatch
 * [lanes][n_gen], storage power [lanes][n_storage], curtailment [lanes][n_gen] (gpf_lane_actions_on_device), then target dispatch,
 * actual dispatch [lanes][n_gen] and state of charge [lanes][n_storage] (obs.target_dispatch / actual_dispatch / storage_charge);
 * 28..31 = the acting path of the topology actions (NULL until it is enabled): act_topo int32 [lanes][n_slot], sub_cooldown int32 [lanes][n_sub],
 * topo_flags uint8 [lanes][2], last_bus int32 [lanes][dim_topo] (gpf_upload_topo_actions); 32 = the engine-owned observation vectors
 * float32 [lanes][dim] (NULL until gpf_set_obs_spec; gpf_obs_vector with out_dev = NULL writes them); 33 = the engine-owned legality
 * masks uint8 [lanes][n_act] (NULL without an action table; gpf_topo_action_mask with out_dev = NULL writes them);
 * stream = hipStream_t */
#define GPF_N_DEVICE_POINTERS 34
int gpf_device_pointers(gpf_handle h, void** ptrs /* [GPF_N_DEVICE_POINTERS] */, void** stream);
/* The same with the length of the caller's array: entries beyond n_ptrs are not written, entries beyond the library's count are
 * NULL -- a caller built against an older / newer header cannot be overrun. */
int gpf_device_pointers_n(gpf_handle h, void** ptrs, int32_t n_ptrs, void** stream);

/* ---- grid-specialised step kernels (run-time compilation; grid2op_amd/csrc/gridpf_jit.hip) -------------------------------------
 * The shipped (ahead-of-time) kernels serve every grid: sizes, offsets of the static tables / result rows and the header of the
 * symbolic program reach them through a parameter block.  gpf_jit_enable() switches the engine's solver launches (gpf_step,
 * gpf_step_n, gpf_simulate_batch, gpf_runpf, gpf_solve_lane) to kernels compiled for THIS grid, in which those numbers are literals: at the first launch of
 * each kernel variant the library writes a header with the grid's numbers, compiles the unchanged kernel source of
 * <src_dir>/gridpf_sparse.hpp for that variant (hipcc --genco, about a second), loads the code object and launches it from then on;
 * code objects are cached in <cache_dir> by a hash of header + variant + sources, so a grid is compiled once per machine.
 * Results are BIT-IDENTICAL to the ahead-of-time kernels (same source, same arithmetic in the same order).  Nothing else changes: same
 * buffers, same calls.  The one-power-flow-per-lane kernels of gpf_runpf / gpf_solve_lane are specialised the same way.
 *   src_dir   directory with the kernel sources (NULL: "csrc" next to the library)
 *   cache_dir NULL: $GRIDPF_JIT_CACHE, else "_jit_cache" next to the library; when that is not writable or not private (owned by
 *             another user / group- or world-writable / a symbolic link): $XDG_CACHE_HOME/gridpf_jit, $HOME/.cache/gridpf_jit -- created 0700
 *             and held to the same rule.  Code objects are loaded without an integrity check: only private directories are trusted.
 * Code objects built ahead of time (grid2op_amd/_aot, made by __graft_entry__.build() for the grids of grid2op_amd/aot/) are used first
 * and need no compiler at run time.  The compiler is $GRIDPF_HIPCC, else /opt/rocm/bin/hipcc, else hipcc on PATH, started without a
 * shell; GPF_E_UNSUPPORTED when neither a compiler + cache nor ahead-of-time objects exist, when the sources are absent or the device
 * is not gfx950 -- the engine then simply keeps the ahead-of-time kernels.  A variant that fails to compile / load is reported on stderr and
 * in gpf_jit_info and runs ahead-of-time.  GRIDPF_JIT=1 in the environment enables it at gpf_create. */
int gpf_jit_enable(gpf_handle h, const char* src_dir, const char* cache_dir);
int gpf_jit_disable(gpf_handle h);
/* counts[6] = {enabled, variants compiled, variants loaded from the cache, variants failed, launches through specialised kernels,
 * variants loaded from the ahead-of-time directory ("_aot" next to the library)};
 * seconds = time spent compiling / loading; text = the variants loaded so far (+ the last error).  Any pointer may be NULL. */
int gpf_jit_info(gpf_handle h, int64_t* counts, double* seconds, char* text, size_t cap);
/* Launch features.  Beyond the grid, a step launch fixes which facilities of the engine it uses at all: cascade, auto-reset, warm start,
 * DC, line cooldowns, rebalancing, kept state, lane lists, outage tables, redispatch deltas, load jitter, the
 * observation trajectory, the DC factors' place in LDS, padding lanes.  With features on (the default of gpf_jit_enable) a step launch
 * first looks for a code object compiled for exactly its set of those answers (one 32-bit word, computed by the library for every launch;
 * it shows as the last template argument in gpf_jit_info's text), then for the grid-only object, then takes the shipped kernel.  A
 * missing feature object is no failure and is not reported.  At run time at most 4 words per kernel variant and engine are compiled or
 * taken from the disk cache; further words run on the grid-only object.  Ahead-of-time objects do not count.  Results are bit-identical
 * on every path.  on = 0: grid-only objects as before.
 * gpf_jit_feature_word: the word of a gpf_step_n launch of n_steps over all lanes with the options `opts`, on the engine as it stands plus
 * the optional inputs `have` (GPF_HAVE_*) says the launch will have; works on a header-only handle (how grid2op_amd/aot.py names the
 * ahead-of-time feature variants of a grid). */
#define GPF_HAVE_LANE_SCALE 1u  /* gpf_set_lane_chronics with lane_scale */
#define GPF_HAVE_OUTAGES 4u     /* gpf_upload_maintenance / gpf_upload_hazards */
#define GPF_HAVE_GEN_DELTA 8u   /* gpf_set_lane_redispatch */
#define GPF_HAVE_TRAJ_OBS 16u   /* gpf_set_trajectory(h, cap >= n_steps, GPF_TRAJ_OBS) */
int gpf_jit_features(gpf_handle h, int32_t on);
int gpf_jit_feature_word(gpf_handle h, int32_t n_steps, const gpf_step_opts* opts, uint32_t have, uint32_t* word);
/* the header the specialised kernels are compiled with (one grid's numbers as C literals); *need = bytes incl. the terminator */
int gpf_jit_source(gpf_handle h, char* text, size_t cap, size_t* need);

#ifdef __cplusplus
}
#endif
#endif /* GRIDPF_H */
