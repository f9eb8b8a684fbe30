"""Developer tool (outside bench.py): what one `lookahead` call costs, next to `simulate_batch` at the same shape.

256 environments x 16 candidates on l2rpn_case14_sandbox and on l2rpn_wcci_2022_dev (118 substations), engines of n_env (1 + K) lanes, a
1-step forecast, once with line-status candidates and once with bus-split candidates (every scratch lane of an environment then sits on
another topology class).  After warm-up, WINDOWS windows of CALLS calls in every setting, one call after the other on the engine's stream:

    la   lookahead(t, 1) with per-lane candidates in the device buffer, rotated on the device between the calls: with bus-split
         candidates every scratch lane changes its topology class at every call (the host re-keys each of them: the worst case)
    la_static   the same without the rotation: no scratch lane changes class after the first call
    sb   simulate_batch(t, range(n_env), the 16 table entries as ONE shared list, n_env, time_step=1): the nearest call the parent has

Reported per (grid, kind, setting): device time per call (HIP events around a window) and the wall time of the calls themselves (how long
the host is busy; `simulate_batch` builds its candidate rows there).  No ratio is an acceptance condition.  Writes
profiles/lookahead_bench.json.

    python tools/lookahead_bench.py [--windows 5] [--calls 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("l2rpn_case14_sandbox", 256, 16), ("l2rpn_wcci_2022_dev", 256, 16))


def tables(m, K):
    """K line-status entries, K bus-split entries (substations with at least four elements, every other element to busbar 2)"""
    pos_sub = np.zeros(m.dim_topo, np.int64)
    for pos, sub in ((m.line_or_pos_topo_vect, m.line_or_sub), (m.line_ex_pos_topo_vect, m.line_ex_sub), (m.gen_pos_topo_vect, m.gen_sub),
                     (m.load_pos_topo_vect, m.load_sub)):
        pos_sub[np.asarray(pos)] = np.asarray(sub)
    if m.n_storage:
        pos_sub[np.asarray(m.storage_pos_topo_vect)] = np.asarray(m.storage_sub)
    big = [s for s in range(m.n_sub) if (pos_sub == s).sum() >= 4]
    line = [{"set_line_status": [(int(l), -1)]} for l in (np.arange(K) * (m.n_line // K))]
    split = []
    for k in range(K):
        pos = np.flatnonzero(pos_sub == big[k % len(big)])
        shift = k // len(big)
        split.append({"set_bus": {int(p): (2 if (i + shift) % 2 else 1) for i, p in enumerate(pos)}})
    return {"line": line, "split": split}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookahead_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    gold = os.path.join(ROOT, "tests", "golden")
    res = {"calls_per_window": a.calls, "windows": a.windows, "settings": {}}
    for name, n_env, K in SHAPES:
        m = GridModel.load_npz(os.path.join(gold, f"{name}.grid.npz"))
        ch = dict(np.load(os.path.join(gold, f"{name}.chronics.npz")))
        if "prod_v" not in ch:
            ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
        n = n_env * (1 + K)
        for kind, table in tables(m, K).items():
            for setting in ("la", "la_static", "sb"):
                eng = PowerFlowEngine(m, n_lanes=n, device=0)
                tab = eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"])
                eng.upload_chronics(tab)
                eng.upload_forecasts((tab * np.float32(1.01))[None, :, None, :])
                eng.set_thermal_limits(ch["thermal_limits"])
                eng.set_lane_chronics(lane_offset=7 * np.arange(n))
                eng.set_topo_rules(max_sub_changed=1, max_line_status_changed=1)
                eng.upload_topo_actions(table)
                st = eng.device_views()["stream"]
                src = np.arange(n_env)
                if setting != "sb":
                    eng.set_lookahead(K, n_env)
                    cand = eng.lookahead_views()["cand"]
                    with torch.cuda.stream(st):
                        cand.copy_(((torch.arange(n_env * K, device=cand.device).reshape(n_env, K) * 5) % K).to(torch.int32))
                t, dev, host = [0], [], []

                def one_call():
                    t[0] += 1
                    if setting != "sb":
                        if setting == "la":
                            cand.copy_(cand.roll(1, dims=1))              # a policy's candidates differ from call to call
                        eng.lookahead(t[0] % 40, 1)
                    else:
                        eng.simulate_batch(t[0] % 40, src, table, n_env, time_step=1)
                with torch.cuda.stream(st):
                    for _ in range(5):
                        one_call()
                    eng.sync()
                    for _ in range(a.windows):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        w0 = time.perf_counter()
                        for _ in range(a.calls):
                            one_call()
                        w1 = time.perf_counter()
                        e1.record(st)
                        e1.synchronize()
                        dev.append(e0.elapsed_time(e1) * 1e3 / a.calls)
                        host.append((w1 - w0) * 1e6 / a.calls)
                extra = {}
                if setting != "sb":
                    got = eng.lookahead_values()
                    extra = {"playable_slots": int(got["n_playable"].sum()), "done_slots": int(got["n_done"].sum()),
                             "mean_best_value": float(got["best_value"][got["best"] >= 0].astype(np.float64).mean()) if (got["best"] >= 0).any() else None}
                eng.close()
                res["settings"][f"{name}/{kind}/{setting}"] = dict(
                    {"environments": n_env, "candidates": K, "call_us_median": float(np.median(dev)), "call_us_min": float(min(dev)), "call_us_max": float(max(dev)),
                     "host_us_median": float(np.median(host)), "simulations_per_sec": n_env * K / (float(np.median(dev)) * 1e-6)}, **extra)
                print(f"{name}/{kind}/{setting}: {np.median(dev):.1f} us per call, host {np.median(host):.1f} us", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["settings"], indent=1))


if __name__ == "__main__":
    main()
