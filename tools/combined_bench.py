"""Developer tool (outside bench.py): what combined topology + injection actions (gpf_set_combined_actions) cost a one-step launch, and
whether the launch with the mode off pays for them.

HIP events on the engine's stream, after warm-up, for educ_case14_storage (14 substations) x 4 096 lanes and l2rpn_wcci_2022_dev (118
substations) x 1 024 lanes, WINDOWS windows of CALLS one-step launches in every setting.  The dynamics and the acting path are on in all
of them (DefaultRules, no cooldowns, a table of one entry that puts every element of the largest substation on busbar 1), the chronics
are the rows of tests/golden/envdyn_*.npz:

    a   the parent commit (a built checkout of it: --parent PATH)    every launch carries a small redispatch pair (refilled from a device
    b   this tree, the mode off                                      tensor, up and down in turn) and storage powers; no topology action
    e   this tree, the mode on                                       the launches of b: what the side kernels cost by themselves (screen and
                                                                     settle; the cancel is queued only next to topology actions)
    t   this tree, the mode off                                      every lane plays the entry and no injection action: what the topology
                                                                     part costs by itself (its pre-step, and the read-back of moved lanes)
    c   this tree, the mode on                                       every lane acts in both parts: that injection action and the entry
    d   this tree, the mode on                                       the same, one lane in sixteen asks for more than a generator's ramp:
                                                                     the screen vetoes both its parts

The screen and the cancel rewrite the buffers of a vetoed lane, so c and d refill all three action buffers from device tensors before
every launch (two more small copies on the engine's stream than a and b, inside the timed window).  Every setting runs in a child
process of its own, under its own time limit; a and b alternate, --runs times each, on the same machine, then e, t, c and d; any failure
ends the run.  Per shape:

    unchanged path   median of b's windows  <=  slowest window of a  +  (slowest - fastest window of a)

e, t, c and d are reported next to b without a bar.  Writes profiles/combined_bench.json.

    python tools/combined_bench.py --parent /path/to/built/parent/checkout [--runs 2] [--windows 5] [--calls 100]
    python tools/combined_bench.py                               # without a: no verdict on the unchanged path
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("educ_case14_storage", 4096), ("l2rpn_wcci_2022_dev", 1024))


def worker(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from topo_rules_ref import topo_pos_sub
    gold = os.path.join(ROOT, "tests", "golden")
    setting = a.worker
    res = {}
    for name, n in SHAPES:
        m = GridModel.load_npz(os.path.join(gold, f"{name}.grid.npz"))
        fx = dict(np.load(os.path.join(gold, f"envdyn_{name}.npz")))
        eng = PowerFlowEngine(m, n_lanes=n, device=0)
        eng.upload_chronics(eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"]))
        eng.set_thermal_limits(fx["thermal_limit"])
        eng.set_gen_limits(fx["pmin"], fx["pmax"], fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], eps_poly=float(fx["eps_poly"]))
        eng.set_storage_params(fx["storage_Emax"], fx["storage_Emin"], fx["storage_loss"], fx["storage_charging_efficiency"],
                               fx["storage_discharging_efficiency"], fx["storage_charge0"], float(fx["delta_time_seconds"]), bool(fx["activate_storage_loss"]))
        eng.set_env_dynamics(True, tol_poly=float(fx["tol_poly"]))
        eng.set_gen_renewable(fx["renewable"])
        eng.set_lane_chronics(lane_offset=(np.arange(n) % 4).astype(np.int32))
        ps = topo_pos_sub(m)
        sub = max(range(m.n_sub), key=lambda s: (ps == s).sum())
        eng.set_topo_rules(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=0, cooldown_line=0)
        eng.upload_topo_actions([{"set_bus": {int(p): 1 for p in np.flatnonzero(ps == sub)}}])
        if setting in "cde":
            eng.set_combined_actions(True, check_values=True, storage_max_p_prod=fx["storage_max_p_prod"], storage_max_p_absorb=fx["storage_max_p_absorb"])
        disp = np.flatnonzero(fx["redispatchable"])
        red = np.zeros((n, m.n_gen), np.float32)
        amp = np.float32(0.02 * min(fx["ramp_up"][disp[0]], fx["ramp_down"][disp[1]]))
        red[:, disp[0]], red[:, disp[1]] = amp, -amp
        red[1::2] *= -1                                                       # (the targets of a lane stay near 0: no lane reaches pmax - pmin)
        if setting == "d":
            red[::16, disp[0]] = np.float32(1.5 * fx["ramp_up"][disp[0]])
        sto = (0.1 * np.minimum(fx["storage_max_p_prod"], fx["storage_max_p_absorb"]) * np.where(np.arange(m.n_storage) % 2, 1, -1)).astype(np.float32)
        v = eng.device_views()
        st = v["stream"]
        dev = v["act_redispatch"].device
        t_sto, t_ix = torch.from_numpy(np.tile(sto, (n, 1))).to(dev), torch.zeros((n, 1), dtype=torch.int32, device=dev)
        down = -red
        if setting == "d":
            down[::16, disp[0]] = red[::16, disp[0]]
        flip = [torch.from_numpy(down).to(dev), torch.from_numpy(red).to(dev)]  # launch by launch the pair goes up and down again
        t, out = 0, []

        def launch():
            nonlocal t
            t += 1
            v["act_redispatch"].copy_(flip[t % 2])                           # (in every setting: one small copy on the engine's stream)
            if setting in "cdt":
                v["act_storage"].copy_(t_sto)
                v["act_topo"].copy_(t_ix)
                eng.topo_actions_on_device(True)
            if setting != "t":
                eng.lane_actions_on_device(redispatch=True, storage_power=True)
            eng.step(abs(t % 30 - 15), nb_ts_reco=10, auto_reset=True)       # (rows 0 .. 15 and back: no jump a ramp cannot follow)
        with torch.cuda.stream(st):
            v["act_storage"].copy_(t_sto)
            for _ in range(10):
                launch()
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.calls):
                    launch()
                e1.record(st)
                e1.synchronize()
                out.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        extra = {"lanes_done": int(eng.episode()[0].sum())}
        if setting in "cde":
            fl = eng.action_flags()
            extra.update(vetoed_last_launch=int((fl["is_ambiguous"] | fl["is_illegal"]).sum()), cancelled_last_launch=int(fl["is_illegal_redisp"].sum()))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combined_bench.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    raw = {}
    plan = ([("a", a.parent), ("b", ROOT)] if a.parent else [("b", ROOT)]) * a.runs + [("e", ROOT), ("t", ROOT), ("c", ROOT), ("d", ROOT)] * a.runs
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
    res = {"calls_per_window": a.calls, "windows_per_run": a.windows, "runs": a.runs, "settings": {}, "unchanged_path": {}}
    for key, v in sorted(raw.items()):
        x = v.pop("one_step_launch_us")
        res["settings"][key] = dict({"median_us": float(np.median(x)), "min_us": float(min(x)), "max_us": float(max(x)), "windows": len(x)}, **v)
    ok_all = True
    for name, _ in SHAPES:
        s = res["settings"]
        res.setdefault("side_kernels_alone_us", {})[name] = s[f"{name}/e"]["median_us"] - s[f"{name}/b"]["median_us"]
        res.setdefault("both_parts_minus_off_us", {})[name] = s[f"{name}/c"]["median_us"] - s[f"{name}/b"]["median_us"]
        res.setdefault("one_in_sixteen_vetoed_minus_off_us", {})[name] = s[f"{name}/d"]["median_us"] - s[f"{name}/b"]["median_us"]
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
        sys.exit("the launch with the mode off is slower than the parent's (see the bars above)")


if __name__ == "__main__":
    main()
