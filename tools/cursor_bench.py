"""Developer tool (outside bench.py): what cursor_prestep_kernel costs a one-step launch, and whether the launch with the feature off pays
for it.

HIP events on the engine's stream, after warm-up, for l2rpn_case14_sandbox x 4 096 lanes and l2rpn_wcci_2022_dev (118 substations) x
1 024 lanes, WINDOWS windows of CALLS one-step launches (auto-reset on) in every setting.  The chronics are cut into four tables:

    a   the parent commit (a built checkout of it: --parent PATH)         no chronics cursor exists
    b   this tree                                                         the feature off
    c   this tree, the cursor on (sampled, Philox), no episode limit      no episode ends: every lane returns early
    l   this tree, per-lane episode limits 9 .. 23, the cursor off        what d stands on: about one lane in sixteen ends per launch
    d   this tree, the same limits, the cursor on                         those lanes start a scenario at the next launch

Every setting runs in a child process of its own; a and b alternate, --runs times each, on the same machine, then c, l and d.  Per shape:

    unchanged path   median of b's windows  <=  slowest window of a  +  (slowest - fastest window of a)

c, l and d are reported next to b without a bar.  Writes profiles/cursor_bench.json.

    python tools/cursor_bench.py --parent /path/to/built/parent/checkout [--runs 2] [--windows 5] [--calls 100]
    python tools/cursor_bench.py                               # without a: no verdict on the unchanged path
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("l2rpn_case14_sandbox", 4096), ("l2rpn_wcci_2022_dev", 1024))
N_TABLES = 4


def worker(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    gold = os.path.join(ROOT, "tests", "golden")
    setting = a.worker
    res = {}
    for name, n in SHAPES:
        m = GridModel.load_npz(os.path.join(gold, f"{name}.grid.npz"))
        ch = dict(np.load(os.path.join(gold, f"{name}.chronics.npz")))
        if "prod_v" not in ch:
            ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
        eng = PowerFlowEngine(m, n_lanes=n, device=0)
        tab = eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"])
        T = tab.shape[0] // N_TABLES
        eng.upload_chronics(np.stack([tab[q * T:(q + 1) * T] for q in range(N_TABLES)]))
        eng.set_thermal_limits(ch["thermal_limits"])
        eng.set_lane_chronics(lane_offset=7 * np.arange(n))
        if setting in "ld":
            eng.set_episode_limit((9 + np.arange(n) % 15).astype(np.int32))
        if setting in "cd":
            eng.set_chronics_cursor(policy="sampled", seed=7, first_row=(7 * np.arange(n)) % T)     # (the rows b reads: the same work per launch)
        st, t, out = eng.device_views()["stream"], 0, []
        with torch.cuda.stream(st):
            for _ in range(10):
                t += 1
                eng.step(t, auto_reset=True)
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.calls):
                    t += 1
                    eng.step(t, auto_reset=True)
                e1.record(st)
                e1.synchronize()
                out.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        extra = {}
        if setting in "cd":
            cs = eng.chronics_cursor_state()
            extra = {"episodes_started": int(cs.n_started.sum()), "lanes_per_table": np.bincount(cs.table, minlength=N_TABLES).tolist()}
        if setting in "ld":
            extra["episodes_ended"] = int(eng.episode_stats()["n_episodes"].sum())
        eng.close()
        res[f"{name}/{setting}"] = dict({"one_step_launch_us": out}, **extra)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (setting a); without it no verdict on the unchanged path")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cursor_bench.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    raw = {}
    plan = ([("a", a.parent), ("b", ROOT)] if a.parent else [("b", ROOT)]) * a.runs + [("c", ROOT), ("l", ROOT), ("d", ROOT)] * a.runs
    for setting, tree in plan:                                  # one child at a time; any failure ends the run: nothing more is started
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", setting, "--tree", tree, "--windows", str(a.windows),
                            "--calls", str(a.calls)], capture_output=True, text=True, timeout=a.child_timeout)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"setting {setting} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        for key, v in json.loads(line[-1][7:]).items():
            slot = raw.setdefault(key, {"one_step_launch_us": []})
            slot["one_step_launch_us"].extend(v.pop("one_step_launch_us"))
            slot.update(v)
        print(f"setting {setting}: done", flush=True)
    res = {"calls_per_window": a.calls, "windows_per_run": a.windows, "runs": a.runs, "tables": N_TABLES, "settings": {}, "unchanged_path": {}}
    for key, v in sorted(raw.items()):
        x = v.pop("one_step_launch_us")
        res["settings"][key] = dict({"median_us": float(np.median(x)), "min_us": float(min(x)), "max_us": float(max(x)), "windows": len(x)}, **v)
    ok_all = True
    for name, _ in SHAPES:
        s = res["settings"]
        res.setdefault("cursor_on_minus_off_us", {})[name] = s[f"{name}/c"]["median_us"] - s[f"{name}/b"]["median_us"]
        res.setdefault("cursor_on_minus_off_with_limits_us", {})[name] = s[f"{name}/d"]["median_us"] - s[f"{name}/l"]["median_us"]
        if f"{name}/a" not in raw:
            continue
        pa, pb = s[f"{name}/a"], s[f"{name}/b"]
        bar = pa["max_us"] + (pa["max_us"] - pa["min_us"])
        ok = pb["median_us"] <= bar
        ok_all = ok_all and ok
        res["unchanged_path"][name] = {"parent_max_us": pa["max_us"], "parent_min_us": pa["min_us"], "bar_us": bar, "median_us": pb["median_us"], "ok": ok}
    if res["unchanged_path"]:
        res["unchanged_path_ok"] = ok_all
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if res["unchanged_path"] and not ok_all:
        sys.exit("the launch with the feature off is slower than the parent's (see the bars above)")


if __name__ == "__main__":
    main()
