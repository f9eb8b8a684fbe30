"""Developer tool (outside bench.py): cost of the observation gather kernel against the same vector built with torch ops.

On the engine's stream, HIP events, after warm-up, for l2rpn_case14_sandbox x 4 096 lanes and l2rpn_wcci_2022_dev x 1 024 lanes:
  (a) `observation_vector()` for the complete spec (one gather kernel);
  (b) the same float32 rows assembled with torch.cat of casts from nothing but the tensors `device_views()` exposed before this feature
      (out, rho, line_status, overflow_count, topo_vect, sub_cooldown, the dispatch state ...; attributes with no buffer there and the
      const entries are filled once, outside the timed loop).
Prints medians and min / max over WINDOWS windows of CALLS calls, (a) as bytes moved / time against the 8 TB/s HBM peak and as a share of
a one-step launch of the same batch (timed here the same way), and writes profiles/obs_vector_bench.json.

    python tools/obs_vector_bench.py [--windows 7] [--calls 200]
"""
import argparse
import datetime as dt
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_vector_bench.json"))
    a = ap.parse_args()
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from grid2op_amd.obs_spec import KIND, ObsSpec
    gold = os.path.join(ROOT, "tests", "golden")
    res = {}
    for name, n in (("l2rpn_case14_sandbox", 4096), ("l2rpn_wcci_2022_dev", 1024)):
        m = GridModel.load_npz(os.path.join(gold, f"{name}.grid.npz"))
        ch = dict(np.load(os.path.join(gold, f"{name}.chronics.npz")))
        if "prod_v" not in ch:
            ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
        eng = PowerFlowEngine(m, n_lanes=n, device=0)
        eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
        eng.set_thermal_limits(ch["thermal_limits"])
        eng.set_lane_chronics(lane_offset=7 * np.arange(n))
        eng.set_obs_clock(dt.datetime(2019, 1, 6), 5, 2016)
        spec = ObsSpec.complete(m, fill=True)
        eng.set_obs_spec(spec)
        eng.step(1)
        v = eng.device_views()
        st = v["stream"]
        sl = eng.out_slices
        dev = v["out"].device

        # what a user does today: constants and the attributes without a buffer in the earlier views (calendar, line cooldowns, margins,
        # maintenance ...) are filled ONCE outside the loop; every buffer those views expose is cast per call
        earlier = {"rho": "rho", "line_status": "line_status", "timestep_overflow": "overflow_count",
                   "timestep_protection_engaged": "overflow_count", "topo_vect": "topo_vect", "time_before_cooldown_sub": "sub_cooldown",
                   "target_dispatch": "target_dispatch", "actual_dispatch": "actual_dispatch", "storage_charge": "storage_charge"}
        plan = []
        for nm, (kind, src, size, _, _) in zip(spec.names, spec.segments.tolist()):
            if kind == KIND["out"]:
                plan.append(("slice", v["out"][:, src:src + size]))
            elif nm == "current_step":
                plan.append(("cast", v["episode"][:, :1]))
            elif nm in earlier and v.get(earlier[nm]) is not None:
                plan.append(("slice" if v[earlier[nm]].dtype == torch.float32 else "cast", v[earlier[nm]]))
            elif kind == KIND["const"]:
                plan.append(("slice", torch.full((n, size), float(np.int32(src).view(np.float32)), dtype=torch.float32, device=dev)))
            else:
                plan.append(("slice", torch.zeros((n, size), dtype=torch.float32, device=dev)))

        def torch_vector():
            return torch.cat([x if how == "slice" else x.to(torch.float32) for how, x in plan], dim=1)

        def timed(fn):
            out = []
            with torch.cuda.stream(st):
                for _ in range(20):
                    fn()
                for _ in range(a.windows):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(a.calls):
                        fn()
                    e1.record(st)
                    e1.synchronize()
                    out.append(e0.elapsed_time(e1) * 1e3 / a.calls)
            return out
        assert torch_vector().shape == (n, spec.dim)
        ka = timed(lambda: eng.observation_vector())
        kb = timed(torch_vector)
        t = [0]

        def one_step():
            t[0] += 1
            eng.step(t[0])
        ks = timed(one_step)
        src_bytes = 4 * spec.dim                                 # (an upper bound of what a row reads: uint8 sources are smaller)
        moved = n * (src_bytes + 4 * spec.dim)
        stat = lambda x: {"median_us": float(np.median(x)), "min_us": float(min(x)), "max_us": float(max(x))}  # noqa: E731
        res[name] = {"lanes": n, "dim": spec.dim, "segments": int(len(spec.segments)), "windows": a.windows, "calls_per_window": a.calls,
                     "gather_kernel": stat(ka), "torch_cat_baseline": stat(kb), "one_step_launch": stat(ks),
                     "gather_below_baseline_in_every_window": bool(max(ka) < min(kb)),
                     "gather_bytes_moved": moved, "gather_tb_per_s": moved / (np.median(ka) * 1e-6) / 1e12,
                     "gather_share_of_hbm_peak_8tbs": moved / (np.median(ka) * 1e-6) / 8e12,
                     "gather_share_of_one_step_launch": float(np.median(ka) / np.median(ks))}
        eng.close()
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    bad = [k for k, r in res.items() if not r["gather_below_baseline_in_every_window"]]
    if bad:
        sys.exit(f"the gather kernel is not below the torch baseline in every window on {bad}")


if __name__ == "__main__":
    main()
