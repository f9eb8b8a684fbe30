"""Developer tool (outside bench.py): what the two alert side kernels cost a one-step launch, and whether the launch without alerts pays
for them.

HIP events on the engine's stream, after warm-up, for l2rpn_case14_sandbox x 4 096 lanes and l2rpn_wcci_2022_dev (118 substations) x
1 024 lanes, WINDOWS windows of CALLS one-step launches (track_cooldown on, auto-reset on), l2rpn_idf_2023's multi-area Geometric
opponent (Philox source; its 22 lines in three areas on the large grid, the 20 lines of the small grid in three areas) in every setting:

    a  the parent commit (a built checkout of it: --parent PATH)          no alerts exist
    b  this tree                                                          alerts off
    c  this tree                                                          alerts on: the opponent's lines, ALERT_TIME_WINDOW = 12, masks on the device

Every setting runs in a child process of its own; a and b alternate (a b a b ...; c rides with b's process), --runs times each, on the
same machine.  The requirement on the unchanged path, per shape:

    median of b's windows  <=  slowest window of a  +  (slowest - fastest window of a)

c is reported next to the launch it rides on, without a bar.  Writes profiles/alert_bench.json.

    python tools/alert_bench.py --parent /path/to/built/parent/checkout [--runs 2] [--windows 10] [--calls 100]
    python tools/alert_bench.py                               # b and c alone: no verdict
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("l2rpn_case14_sandbox", 4096), ("l2rpn_wcci_2022_dev", 1024))
IDF_AREAS = [["26_31_106", "21_22_93", "17_18_88", "4_10_162", "12_14_68", "29_37_117"],
             ["62_58_180", "62_63_160", "48_50_136", "48_53_141", "41_48_131", "39_41_121", "43_44_125", "44_45_126", "34_35_110", "54_58_154"],
             ["74_117_81", "93_95_43", "88_91_33", "91_92_37", "99_105_62", "102_104_61"]]
# l2rpn_idf_2023: an attack every 32 h on average, 2 h long on average and 1 h at least, 5-minute steps, episodes of 2016 steps
GEOMETRIC = dict(kind=3, attack_hazard_rate=1.0 / 360.0, recovery_rate=1.0 / 12.0, recovery_minimum_duration=12, pmax_pmin_ratio=4.0,
                 episode_max_time=2016, schedule_cap=40, init_budget=1000.0, budget_per_ts=0.51, attack_duration=96, attack_cooldown=0)


def lines_and_areas(m):
    names = [str(x) for x in m.name_line]
    if all(x in names for area in IDF_AREAS for x in area):
        return [names.index(x) for area in IDF_AREAS for x in area], [a for a, area in enumerate(IDF_AREAS) for _ in area]
    lines = list(range(m.n_line))
    return lines, [3 * i // len(lines) for i in range(len(lines))]


def worker(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    gold = os.path.join(ROOT, "tests", "golden")
    res = {}
    for name, n in SHAPES:
        m = GridModel.load_npz(os.path.join(gold, f"{name}.grid.npz"))
        ch = dict(np.load(os.path.join(gold, f"{name}.chronics.npz")))
        if "prod_v" not in ch:
            ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
        lines, areas = lines_and_areas(m)

        def timed(alerts):
            eng = PowerFlowEngine(m, n_lanes=n, device=0)
            eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
            eng.set_thermal_limits(ch["thermal_limits"])
            eng.set_lane_chronics(lane_offset=7 * np.arange(n))
            eng.set_opponent(lines=lines, seed=1, **GEOMETRIC)
            eng.set_opponent_areas(areas)
            if alerts:
                eng.set_alerts(12)
            views = eng.device_views()
            st, t, out = views["stream"], [0], []
            if alerts:                                          # every third alertable line, as a policy's output would sit in the buffer
                with torch.cuda.stream(st):
                    views["act_alert"].fill_(sum(1 << i for i in range(0, len(lines), 3)))

            def one_step():
                t[0] += 1
                if alerts:
                    eng.alerts_on_device(True)
                eng.step(t[0], nb_ts_reco=10, auto_reset=True)
            with torch.cuda.stream(st):
                for _ in range(10):
                    one_step()
                for _ in range(a.windows):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(a.calls):
                        one_step()
                    e1.record(st)
                    e1.synchronize()
                    out.append(e0.elapsed_time(e1) * 1e3 / a.calls)
            extra = {"mean_total_number_of_alert": float(eng.alert_state()[:, 7 * len(lines)].mean())} if alerts else {}
            eng.close()
            return dict({"one_step_launch_us": out}, **extra)
        for s in a.worker.split(","):
            res[f"{name}/{s}"] = timed(s == "c")
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (setting a); without it no verdict")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alert_bench.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    raw = {}
    plan = ([("a", a.parent), ("b,c", ROOT)] if a.parent else [("b,c", ROOT)]) * a.runs
    for settings, tree in plan:                                 # one child at a time; any failure ends the run: nothing more is started
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", settings, "--tree", tree, "--windows", str(a.windows),
                            "--calls", str(a.calls)], capture_output=True, text=True, timeout=a.child_timeout)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"setting {settings} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        for key, v in json.loads(line[-1][7:]).items():
            slot = raw.setdefault(key, {"one_step_launch_us": []})
            slot["one_step_launch_us"].extend(v.pop("one_step_launch_us"))
            slot.update(v)
        print(f"setting {settings}: done", flush=True)
    res = {"calls_per_window": a.calls, "windows_per_run": a.windows, "runs": a.runs, "settings": {}, "unchanged_path": {}}
    for key, v in sorted(raw.items()):
        x = v.pop("one_step_launch_us")
        res["settings"][key] = dict({"median_us": float(np.median(x)), "min_us": float(min(x)), "max_us": float(max(x)), "windows": len(x)}, **v)
    ok_all = True
    for name, _ in SHAPES:
        if f"{name}/a" not in raw:
            continue
        pa, pb = res["settings"][f"{name}/a"], res["settings"][f"{name}/b"]
        bar = pa["max_us"] + (pa["max_us"] - pa["min_us"])
        ok = pb["median_us"] <= bar
        ok_all = ok_all and ok
        res["unchanged_path"][name] = {"parent_max_us": pa["max_us"], "parent_min_us": pa["min_us"], "bar_us": bar, "median_us": pb["median_us"], "ok": ok}
    if res["unchanged_path"]:
        res["unchanged_path_ok"] = ok_all
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"unchanged_path": res["unchanged_path"], "settings": res["settings"]}, indent=1))
    if res["unchanged_path"] and not ok_all:
        sys.exit("the launch without alerts is slower than the parent's (see the bars above)")


if __name__ == "__main__":
    main()
