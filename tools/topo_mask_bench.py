"""Developer tool (outside bench.py): cost of the legality-mask kernel (`PowerFlowEngine.topo_action_mask`) next to a one-step launch.

On the engine's stream, HIP events, after warm-up, for l2rpn_case14_sandbox x 4 096 lanes and l2rpn_wcci_2022_dev (118 substations) x
1 024 lanes, each with tables of 64 and of 1 024 entries (the table of tests/topo_rules_ref.random_topo_table, repeated): the mask of all
lanes into the engine-owned buffer, and a one-step launch of the same engine in the same process -- what the mask precedes in an acting
loop.  Lane states carry cooldowns and open lines (tests/topo_mask_ref.hand_set_states), so that the rule arithmetic is not all zeros.
Prints medians and min / max over WINDOWS windows of CALLS calls and writes profiles/topo_mask_bench.json.

    python tools/topo_mask_bench.py [--windows 7] [--calls 200]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topo_mask_bench.json"))
    a = ap.parse_args()
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from topo_mask_ref import hand_set_states
    from topo_rules_ref import random_topo_table
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
        eng.set_topo_rules(1, 1, 3, 3)
        rng = np.random.default_rng(0)
        base = random_topo_table(m, rng)
        st = eng.device_views()["stream"]

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
        stat = lambda x: {"median_us": float(np.median(x)), "min_us": float(min(x)), "max_us": float(max(x))}  # noqa: E731
        t = [0]

        def one_step():
            t[0] += 1
            eng.step(t[0], nb_ts_reco=10)
        ks = timed(one_step)                                    # (before the states below: every lane on its reset topology, as in bench.py)
        topo, lcd, scd = hand_set_states(m, rng, n)
        eng.set_topology(topo)
        eng.set_cooldown(lcd)
        eng.set_sub_cooldown(scd)
        for n_act in (64, 1024):
            eng.upload_topo_actions((base * (n_act // len(base) + 1))[:n_act])
            km = timed(lambda: eng.topo_action_mask())
            mask = eng.topo_action_mask_host()
            res[f"{name}/{n_act}"] = {"lanes": n, "n_act": n_act, "windows": a.windows, "calls_per_window": a.calls, "mask_kernel": stat(km),
                                      "one_step_launch": stat(ks), "mask_share_of_one_step_launch": float(np.median(km) / np.median(ks)),
                                      "evaluations_per_us": n * n_act / float(np.median(km)), "share_of_entries_masked": float((mask != 0).mean())}
        eng.close()
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
