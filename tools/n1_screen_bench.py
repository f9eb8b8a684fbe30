"""Developer tool (outside bench.py): what the N-1 screen costs a one-step launch, whether the launch without it pays for it, and what
the same screening costs through `simulate_batch(time_step=0)` with the K outages as candidates.

HIP events on the engine's stream, after warm-up, for l2rpn_case14_sandbox x 1 024 environments x 20 watched lines and l2rpn_wcci_2022_dev
(118 substations) x 256 environments x 16 watched lines; every engine has n_env (1 + K) lanes; WINDOWS windows of CALLS one-step launches
(auto-reset on) in every setting:

    a   the parent commit (a built checkout of it: --parent PATH)         no screen exists: all lanes are stepped
    b   this tree, screen off                                             all lanes are stepped
    c   this tree, screen on                                              n_env lanes stepped, n_env K contingency power flows
    s   this tree, screen off; after every launch simulate_batch(t, range(n_env), the K outages, n_env, time_step=0)

Every child process runs one of {a} / {b, c, s}; a and the others alternate, --runs times each, on the same machine.  Per shape:

    unchanged path    median of b's windows  <=  slowest window of a  +  (slowest - fastest window of a)
    screen vs today   every window of c lies below every window of s (reported, with what was measured, when it does not)

c also reports contingency power flows per second and the host's share of a launch (wall time of the calls of a window, which return
before the device has run them, over the window's device time).  Writes profiles/n1_screen_bench.json.

    python tools/n1_screen_bench.py --parent /path/to/built/parent/checkout [--runs 2] [--windows 10] [--calls 100]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("l2rpn_case14_sandbox", 1024, 20), ("l2rpn_wcci_2022_dev", 256, 16))


def worker(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    gold = os.path.join(ROOT, "tests", "golden")
    res = {}
    for name, n_env, K in SHAPES:
        m = GridModel.load_npz(os.path.join(gold, f"{name}.grid.npz"))
        ch = dict(np.load(os.path.join(gold, f"{name}.chronics.npz")))
        if "prod_v" not in ch:
            ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
        n = n_env * (1 + K)
        lines = (np.arange(K) * (m.n_line // K)).astype(np.int32)

        def timed(setting):
            eng = PowerFlowEngine(m, n_lanes=n, device=0)
            eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
            eng.set_thermal_limits(ch["thermal_limits"])
            eng.set_lane_chronics(lane_offset=7 * np.arange(n))
            if setting == "c":
                eng.set_n1_screen(lines, n_env)
            outages = [{"set_line_status": [(int(l), -1)]} for l in lines]
            src = np.arange(n_env)
            st, t, out, host = eng.device_views()["stream"], [0], [], []

            def one_step():
                t[0] += 1
                eng.step(t[0], auto_reset=True)
                if setting == "s":
                    eng.simulate_batch(t[0], src, outages, n_env, time_step=0)
            with torch.cuda.stream(st):
                for _ in range(10):
                    one_step()
                for _ in range(a.windows):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    w0 = time.perf_counter()
                    for _ in range(a.calls):
                        one_step()
                    w1 = time.perf_counter()
                    e1.record(st)
                    e1.synchronize()
                    out.append(e0.elapsed_time(e1) * 1e3 / a.calls)
                    host.append((w1 - w0) * 1e6 / a.calls)
            extra = {"host_us": host}
            if setting == "c":
                v = eng.n1_values()
                extra["mean_value"] = float(v[v > 0].astype(np.float64).mean())
                extra["diverged"] = int((v == -1).sum())
            eng.close()
            return dict({"one_step_launch_us": out}, **extra)
        for s in a.worker.split(","):
            res[f"{name}/{s}"] = timed(s)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (setting a); without it no verdict on the unchanged path")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--child-timeout", type=float, default=400.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "n1_screen_bench.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    raw = {}
    mine = "b,c,s"
    plan = ([("a", a.parent), (mine, ROOT)] if a.parent else [(mine, ROOT)]) * a.runs
    for settings, tree in plan:                                 # one child at a time; any failure ends the run: nothing more is started
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", settings, "--tree", tree, "--windows", str(a.windows),
                            "--calls", str(a.calls)], capture_output=True, text=True, timeout=a.child_timeout)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"setting {settings} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        for key, v in json.loads(line[-1][7:]).items():
            slot = raw.setdefault(key, {"one_step_launch_us": [], "host_us": []})
            slot["one_step_launch_us"].extend(v.pop("one_step_launch_us"))
            slot["host_us"].extend(v.pop("host_us"))
            slot.update(v)
        print(f"setting {settings}: done", flush=True)
    res = {"calls_per_window": a.calls, "windows_per_run": a.windows, "runs": a.runs, "settings": {}, "unchanged_path": {}, "screen_below_simulate_batch": {}}
    for key, v in sorted(raw.items()):
        x, h = v.pop("one_step_launch_us"), v.pop("host_us")
        res["settings"][key] = dict({"median_us": float(np.median(x)), "min_us": float(min(x)), "max_us": float(max(x)), "windows": len(x),
                                     "host_median_us": float(np.median(h)), "host_share": float(np.median(h) / np.median(x))}, **v)
    ok_all = True
    for name, n_env, K in SHAPES:
        s = res["settings"]
        c, sb = s[f"{name}/c"], s[f"{name}/s"]
        c["environments"], c["watched_lines"] = n_env, K
        c["contingency_power_flows_per_sec"] = n_env * K / (c["median_us"] * 1e-6)
        res["screen_below_simulate_batch"][name] = {"screen_max_us": c["max_us"], "simulate_batch_min_us": sb["min_us"], "ok": c["max_us"] < sb["min_us"]}
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
    print(json.dumps({"unchanged_path": res["unchanged_path"], "screen_below_simulate_batch": res["screen_below_simulate_batch"], "settings": res["settings"]}, indent=1))
    if res["unchanged_path"] and not ok_all:
        sys.exit("the launch without the screen is slower than the parent's (see the bars above)")


if __name__ == "__main__":
    main()
