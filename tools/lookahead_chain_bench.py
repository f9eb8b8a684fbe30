"""Developer tool (outside bench.py): what `lookahead_chain` costs, and that `lookahead(t, 1)` costs what it cost on the parent commit.

256 environments x 16 line-status candidates on l2rpn_case14_sandbox and on l2rpn_wcci_2022_dev (118 substations), engines of
n_env (1 + K) lanes, 12 forecast horizons.  The parent commit (a built checkout given with --parent) and this tree are measured in child
processes that alternate (parent, tree, parent, tree ...), so that both see the same box in the same minutes.  After warm-up, WINDOWS
windows of CALLS calls in every setting, one call after the other on the engine's stream, device time by HIP events around a window:

    la1        lookahead(t, 1), candidates in the device buffer (both commits)
    chain_H    lookahead_chain(t, H), H = 1, 4, 12 (this tree)
    steps_H    H one-step `step` launches of an engine of n_env K lanes (the parent): what the H power flows of a chain cost as launches

The bar: the median window of `la1` on this tree stays below the parent's slowest window plus 3 % (the box-to-box spread the README
states).  `chain_H` next to `steps_H` is reported without a bar.  --bench also runs `bench.py --gpus 1 --steps 20 --warmup 5` once in
each checkout (the chain off in it).  Writes profiles/lookahead_chain_bench.json.

    python tools/lookahead_chain_bench.py --parent /path/to/built/parent [--rounds 2] [--windows 5] [--calls 20] [--bench]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("l2rpn_case14_sandbox", 256, 16), ("l2rpn_wcci_2022_dev", 256, 16))
HORIZONS = (1, 4, 12)
FC_H = 12


def child(a):
    """one commit's settings, measured in this process; the result is the last line printed"""
    sys.path.insert(0, a.root)
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    gold = os.path.join(ROOT, "tests", "golden")
    res = {}

    def windows(st, eng, one_call):
        dev = []
        with torch.cuda.stream(st):
            for _ in range(5):
                one_call()
            eng.sync()
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.calls):
                    one_call()
                e1.record(st)
                e1.synchronize()
                dev.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        return dev

    for name, n_env, K in SHAPES:
        m = GridModel.load_npz(os.path.join(gold, f"{name}.grid.npz"))
        ch = dict(np.load(os.path.join(gold, f"{name}.chronics.npz")))
        if "prod_v" not in ch:
            ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
        table = [{"set_line_status": [(int(l), -1)]} for l in (np.arange(K) * (m.n_line // K))]

        def engine(n_lanes):
            eng = PowerFlowEngine(m, n_lanes=n_lanes, device=0)
            tab = eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"])[:96]
            eng.upload_chronics(tab)
            T = tab.shape[0]
            eng.upload_forecasts(np.stack([tab[(np.arange(T) + h + 1) % T] for h in range(FC_H)], axis=1)[None])
            eng.set_thermal_limits(ch["thermal_limits"])
            eng.set_lane_chronics(lane_offset=7 * np.arange(n_lanes))
            return eng
        # the look-ahead and the chain
        eng = engine(n_env * (1 + K))
        eng.set_topo_rules(max_sub_changed=1, max_line_status_changed=1)
        eng.upload_topo_actions(table)
        st = eng.device_views()["stream"]
        eng.set_lookahead(K, n_env)
        cand = eng.lookahead_views()["cand"]
        with torch.cuda.stream(st):
            cand.copy_(((torch.arange(n_env * K, device=cand.device).reshape(n_env, K) * 5) % K).to(torch.int32))
        t = [0]

        def la1():
            t[0] += 1
            eng.lookahead(t[0] % 40, 1)
        res[f"{name}/la1"] = windows(st, eng, la1)
        if a.kind == "tree":
            eng.set_lookahead_chain(FC_H)
            for H in HORIZONS:
                def chain():
                    t[0] += 1
                    eng.lookahead_chain(t[0] % 40, H)
                res[f"{name}/chain_{H}"] = windows(st, eng, chain)
            got, lc = eng.lookahead_values(), eng.lookahead_chain_values()
            res[f"{name}/chain_outcome"] = {"playable_slots": int(got["n_playable"].sum()), "done_slots": int(got["n_done"].sum()),
                                            "survived_mean": float(lc["survived"].mean())}
        eng.close()
        if a.kind == "parent":                                # H one-step launches of n_env K lanes
            eng = engine(n_env * K)
            st = eng.device_views()["stream"]
            for H in HORIZONS:
                def steps():
                    for _ in range(H):
                        t[0] += 1
                        eng.step(t[0] % 40)
                res[f"{name}/steps_{H}"] = windows(st, eng, steps)
            eng.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookahead_chain_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--kind", default="tree")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent or not os.path.exists(os.path.join(a.parent, "grid2op_amd", "libgridpf.so")):
        raise SystemExit("--parent must name a built checkout of the parent commit")
    raw = {}
    for r in range(a.rounds):
        for kind, root in (("parent", os.path.abspath(a.parent)), ("tree", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--kind", kind, "--windows", str(a.windows), "--calls", str(a.calls)]
            t0 = time.time()
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
            if p.returncode != 0:
                raise SystemExit(f"{kind} child failed ({p.returncode}):\n{p.stderr[-3000:]}")
            got = json.loads(p.stdout.strip().splitlines()[-1])
            print(f"round {r} {kind}: {time.time() - t0:.0f} s", flush=True)
            for key, v in got.items():
                if isinstance(v, list):
                    raw.setdefault(f"{kind}/{key}", []).extend(v)
                else:
                    raw[f"{kind}/{key}"] = v
    res = {"calls_per_window": a.calls, "windows_per_round": a.windows, "rounds": a.rounds, "settings": {}, "la1_bar": {}}
    for key, v in raw.items():
        res["settings"][key] = v if isinstance(v, dict) else {"call_us_median": float(np.median(v)), "call_us_min": float(min(v)), "call_us_max": float(max(v)), "windows": len(v)}
    for name, _, _ in SHAPES:
        par, tree = res["settings"][f"parent/{name}/la1"], res["settings"][f"tree/{name}/la1"]
        res["la1_bar"][name] = {"tree_median_us": tree["call_us_median"], "parent_slowest_window_us": par["call_us_max"], "bar_us": par["call_us_max"] * 1.03,
                                "within": bool(tree["call_us_median"] < par["call_us_max"] * 1.03)}
    if a.bench:
        res["bench"] = {}
        for kind, root in (("parent", os.path.abspath(a.parent)), ("tree", ROOT)):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True, timeout=900, cwd=root)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            res["bench"][kind] = json.loads(lines[-1]) if p.returncode == 0 and lines else {"failed": p.returncode, "stderr": p.stderr[-1000:]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if not all(v["within"] for v in res["la1_bar"].values()):
        raise SystemExit("lookahead(t, 1) on this tree is slower than the parent's slowest window plus 3 %")


if __name__ == "__main__":
    main()
