"""Developer tool (outside bench.py): what reward_kernel costs a one-step launch, whether the launch without rewards pays for it, and what
the same rewards cost when a learner computes them with torch ops on the engine's device views.

HIP events on the engine's stream, after warm-up, for l2rpn_case14_sandbox x 4 096 lanes and l2rpn_wcci_2022_dev (118 substations) x
1 024 lanes, WINDOWS windows of CALLS one-step launches (auto-reset on) in every setting:

    a   the parent commit (a built checkout of it: --parent PATH)         no rewards exist
    b   this tree                                                         rewards off
    c5  this tree, rewards on                                             RedispReward, L2RPNReward, LinesCapacityReward, EconomicReward, GameplayReward
    c1  this tree, rewards on                                             RedispReward alone
    t5  this tree, rewards off; after every launch the five rewards       torch ops on device_views (float64 sums, float32 result),
    t1  ... and RedispReward alone                                        queued on the engine's stream

Every child process runs one of {a} / {b, c5, c1, t5, t1}; a and the others alternate, --runs times each, on the same machine.  Per shape:

    unchanged path   median of b's windows  <=  slowest window of a  +  (slowest - fastest window of a)
    kernel vs torch  every window of c5 (c1) lies below every window of t5 (t1)

Writes profiles/reward_bench.json.

    python tools/reward_bench.py --parent /path/to/built/parent/checkout [--runs 2] [--windows 10] [--calls 100]
    python tools/reward_bench.py                              # without a: no verdict on the unchanged path
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("l2rpn_case14_sandbox", 4096), ("l2rpn_wcci_2022_dev", 1024))
DTS = 300.0 / 3600.0


def torch_rewards(torch, v, sl, thermal, cost, p_redisp, p_econ, five):
    """the rewards a learner would write with torch ops on the views (no dynamics: no dispatch, no storage power)"""
    out = v["out"]
    failed = v["done"][:, 0] != 0
    gen_p, load_p = out[:, sl["gen_p"]].double(), out[:, sl["load_p"]].double()
    sg, sload = gen_p.sum(1), load_p.sum(1)
    mc = torch.where(gen_p > 0, cost, torch.full_like(cost, -1.0)).amax(1)
    regret = mc * p_redisp[4] * (sg - sload)
    redisp = torch.where(failed, torch.full_like(sg, p_redisp[2]), (p_redisp[1] - regret) / sload).float()
    if not five:
        return redisp[:, None]
    rel = torch.clamp(out[:, sl["a_or"]].double().abs() / (thermal.abs() + 0.1), max=1.0)
    l2 = torch.where(failed, torch.zeros_like(sg), torch.clamp(1.0 - rel * rel, min=0.0).sum(1)).float()
    ls = v["line_status"] != 0
    n = ls.sum(1).double()
    u = torch.minimum(torch.clamp(torch.where(ls, v["rho"].double(), torch.zeros((), dtype=torch.float64, device=out.device)).sum(1), min=0.0), n)
    cap = torch.where(failed, torch.zeros_like(sg), (n - u) / n).float()
    c = (gen_p * cost).sum(1) * p_econ[3]
    econ = torch.where(failed, torch.full_like(sg, p_econ[1]), p_econ[1] + (p_econ[2] - p_econ[1]) * torch.clamp(p_econ[0] - c, min=0.0, max=p_econ[0]) / p_econ[0]).float()
    game = torch.where(failed, torch.full_like(redisp, -1.0), torch.full_like(redisp, 1.0))
    return torch.stack([redisp, l2, cap, econ, game], 1)


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
        cost = np.linspace(10.0, 60.0, m.n_gen).astype(np.float32)
        pmax = np.full(m.n_gen, 200.0, np.float32)

        def timed(setting):
            eng = PowerFlowEngine(m, n_lanes=n, device=0)
            eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
            eng.set_thermal_limits(ch["thermal_limits"])
            eng.set_lane_chronics(lane_offset=7 * np.arange(n))
            five = setting.endswith("5")
            after = None
            if setting[0] in "ct":
                from grid2op_amd.engine import reward_config
                kw = dict(gen_cost_per_MW=cost, gen_pmax=pmax)
                rd, ec = reward_config("RedispReward", **kw), reward_config("EconomicReward", **kw)
                if setting[0] == "c":
                    eng.set_rewards([rd, reward_config("L2RPNReward"), reward_config("LinesCapacityReward"), ec, reward_config("GameplayReward")] if five else [rd], cost)
            views = eng.device_views()
            st, t, out = views["stream"], [0], []
            if setting[0] == "t":
                dev = views["out"].device
                th = torch.from_numpy(np.asarray(ch["thermal_limits"], np.float64)).to(dev)
                co = torch.from_numpy(cost.astype(np.float64)).to(dev)[None, :].expand(n, -1).contiguous()
                after = lambda: torch_rewards(torch, views, eng.out_slices, th, co, rd["p"], ec["p"], five)   # noqa: E731

            def one_step():
                t[0] += 1
                eng.step(t[0], auto_reset=True)
                return after() if after else None
            with torch.cuda.stream(st):
                for _ in range(10):
                    last = one_step()
                for _ in range(a.windows):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(a.calls):
                        last = one_step()
                    e1.record(st)
                    e1.synchronize()
                    out.append(e0.elapsed_time(e1) * 1e3 / a.calls)
            extra = {}
            if setting[0] == "c":
                extra["mean_reward"] = [float(x) for x in eng.rewards().astype(np.float64).mean(0)]
            if setting[0] == "t":
                extra["mean_reward"] = [float(x) for x in last.double().mean(0).cpu().numpy()]
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
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reward_bench.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    raw = {}
    mine = "b,c5,c1,t5,t1"
    plan = ([("a", a.parent), (mine, ROOT)] if a.parent else [(mine, ROOT)]) * a.runs
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
    res = {"calls_per_window": a.calls, "windows_per_run": a.windows, "runs": a.runs, "settings": {}, "unchanged_path": {}, "kernel_below_torch": {}}
    for key, v in sorted(raw.items()):
        x = v.pop("one_step_launch_us")
        res["settings"][key] = dict({"median_us": float(np.median(x)), "min_us": float(min(x)), "max_us": float(max(x)), "windows": len(x)}, **v)
    ok_all = True
    for name, _ in SHAPES:
        s = res["settings"]
        for k in ("5", "1"):
            res["kernel_below_torch"][f"{name}/{k}"] = {"kernel_max_us": s[f"{name}/c{k}"]["max_us"], "torch_min_us": s[f"{name}/t{k}"]["min_us"],
                                                        "ok": s[f"{name}/c{k}"]["max_us"] < s[f"{name}/t{k}"]["min_us"]}
        if f"{name}/a" not in raw:
            continue
        pa, pb = s[f"{name}/a"], s[f"{name}/b"]
        bar = pa["max_us"] + (pa["max_us"] - pa["min_us"])
        ok = pb["median_us"] <= bar
        ok_all = ok_all and ok
        res["unchanged_path"][name] = {"parent_max_us": pa["max_us"], "parent_min_us": pa["min_us"], "bar_us": bar, "median_us": pb["median_us"], "ok": ok}
    if res["unchanged_path"]:
        res["unchanged_path_ok"] = ok_all
    res["kernel_below_torch_ok"] = all(v["ok"] for v in res["kernel_below_torch"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"unchanged_path": res["unchanged_path"], "kernel_below_torch": res["kernel_below_torch"], "settings": res["settings"]}, indent=1))
    if res["unchanged_path"] and not ok_all:
        sys.exit("the launch without rewards is slower than the parent's (see the bars above)")
    if not res["kernel_below_torch_ok"]:
        sys.exit("a window of reward_kernel is not below every window of the torch baseline (see above)")


if __name__ == "__main__":
    main()
