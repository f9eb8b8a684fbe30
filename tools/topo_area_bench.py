"""Developer tool (outside bench.py): what rules by area and composite actions cost the topology kernels, and whether the default path
(no areas, one slot) pays for them.

HIP events on the engine's stream, after warm-up, for l2rpn_case14_sandbox x 4 096 lanes and l2rpn_wcci_2022_dev (118 substations) x
1 024 lanes, each with tables of 64 and of 1 024 entries, WINDOWS windows of CALLS calls, in four settings:

    a  the parent commit (a built checkout of it: --parent PATH)          no areas, one slot
    b  this tree                                                          no areas, one slot
    c  this tree                                                          3 areas,  one slot
    d  this tree                                                          3 areas,  3 slots (one entry per area)

Timed: the mask kernel (`topo_action_mask` of all lanes into the engine-owned buffer; lane states with cooldowns and open lines,
tests/topo_mask_ref.hand_set_states, rules 1 / 1 / 3 / 3), and the pre-step kernel as the difference between a one-step launch that carries
topology actions (indices resident in ``act_topo``, `topo_actions_on_device`) and a one-step launch of the same engine that carries none.
That difference holds the pre-step kernel, the action branch of the post-step kernel and the compact read-back of moved lanes (one
4-byte copy and a stream synchronisation, the table holding bus items); the pre-step kernel cannot be launched alone from Python.  The
table keeps the lanes where they are, so that every call of a window does the same work: entry e sets every element of one substation to
busbar 1 (even e) or sets the status of an in-service line to +1 (odd e) -- one substation or one line affected, legal under limits
1 / 1, applied in full (steps 1-4 of the pre-step), nothing moves; cooldowns 0 / 0 keep it legal at the next call.

Every setting runs in a child process of its own; a and b alternate (a b a b ...; c and d ride with b's process), --runs times each, on
the same machine.  The requirement on the default path, per shape, table and kernel:

    median of b's windows  <=  slowest window of a  +  (slowest - fastest window of a)

c and d are reported next to the one-step launch, without a bar.  Writes profiles/topo_area_bench.json.

    python tools/topo_area_bench.py --parent /path/to/built/parent/checkout [--runs 2] [--windows 5] [--calls 100]
    python tools/topo_area_bench.py                      # b, c, d alone: no verdict
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("l2rpn_case14_sandbox", 4096), ("l2rpn_wcci_2022_dev", 1024))
TABLES = (64, 1024)
N_AREA, N_SLOT = 3, 3


def stationary_table(m, pos_sub, n_act):
    """entry e -> (dict, substation whose area it acts in); see the module docstring"""
    lo = np.asarray(m.line_or_pos_topo_vect)
    table, subs = [], []
    for e in range(n_act):
        if e % 2 == 0:
            s = (e // 2) % m.n_sub
            table.append({"set_bus": {int(p): 1 for p in np.flatnonzero(pos_sub == s)}})
        else:
            l = (e // 2) % m.n_line
            s = int(pos_sub[lo[l]])                                 # (a line counts in the area of its origin substation)
            table.append({"set_line_status": [(int(l), 1)]})
        subs.append(s)
    return table, np.asarray(subs)


def worker(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))              # (the pure-Python helpers of this tree, whichever library is timed)
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from topo_mask_ref import hand_set_states
    from topo_rules_ref import topo_pos_sub
    gold = os.path.join(ROOT, "tests", "golden")
    settings = a.worker.split(",")
    res = {}
    for name, n in SHAPES:
        m = GridModel.load_npz(os.path.join(gold, f"{name}.grid.npz"))
        ch = dict(np.load(os.path.join(gold, f"{name}.chronics.npz")))
        if "prod_v" not in ch:
            ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
        pos_sub = np.asarray(topo_pos_sub(m))
        sub_area = (np.arange(m.n_sub) * N_AREA // m.n_sub).astype(np.int32)
        rng = np.random.default_rng(0)
        states = hand_set_states(m, rng, n)

        def engine():
            eng = PowerFlowEngine(m, n_lanes=n, device=0)
            eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
            eng.set_thermal_limits(ch["thermal_limits"])
            eng.set_lane_chronics(lane_offset=7 * np.arange(n))
            return eng, eng.device_views()["stream"]

        def timed(st, fn):
            out = []
            with torch.cuda.stream(st):
                for _ in range(10):
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

        for n_act in TABLES:
            table, ent_sub = stationary_table(m, pos_sub, n_act)
            by_area = [np.flatnonzero(sub_area[ent_sub] == k) for k in range(N_AREA)]
            for s in settings:
                areas, n_slot = s in "cd", N_SLOT if s == "d" else 1
                # the pre-step: lanes on their reset topology, which the table leaves alone
                eng, st = engine()
                t = [0]
                eng.upload_topo_actions(table)
                eng.set_topo_rules(1, 1, 0, 0)
                if areas:
                    eng.set_topo_areas(sub_area)
                if n_slot > 1:
                    eng.set_topo_slots(n_slot)
                if n_slot == 1:
                    idx = rng.integers(0, n_act, size=(n, 1))
                else:                                            # one entry per area and slot
                    idx = np.stack([by_area[k][rng.integers(0, len(by_area[k]), size=n)] for k in range(n_slot)], axis=1)
                act = eng.device_views()["act_topo"]
                with torch.cuda.stream(st):
                    act.copy_(torch.as_tensor(idx.astype(np.int32)).reshape(act.shape), non_blocking=False)

                def one_step():
                    t[0] += 1
                    eng.step(t[0], nb_ts_reco=10)

                def acting_step():
                    eng.topo_actions_on_device()
                    one_step()
                before = eng.get_topology()[0].copy()
                plain = timed(st, one_step)
                acting = timed(st, acting_step)
                ill, amb = eng.topo_action_flags()
                assert not np.asarray(ill).any() and not np.asarray(amb).any(), "the stationary table must stay legal"
                assert np.array_equal(eng.get_topology()[0], before), "the stationary table moved a lane"
                eng.close()
                # the mask: hand-set lane states with cooldowns and open lines
                eng, st = engine()
                eng.upload_topo_actions(table)
                eng.set_topo_rules(1, 1, 3, 3)
                if areas:
                    eng.set_topo_areas(sub_area)
                if n_slot > 1:
                    eng.set_topo_slots(n_slot)
                eng.set_topology(states[0])
                eng.set_cooldown(states[1])
                eng.set_sub_cooldown(states[2])
                mask = timed(st, lambda: eng.topo_action_mask())
                share = float((eng.topo_action_mask_host() != 0).mean())
                eng.close()
                res[f"{name}/{n_act}/{s}"] = {"one_step_launch_us": plain, "acting_one_step_launch_us": acting, "mask_kernel_us": mask,
                                              "share_of_entries_masked": share}
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (setting a); without it no verdict")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--child-timeout", type=float, default=420.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topo_area_bench.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    raw = {}
    plan = ([("a", a.parent), ("b,c,d", ROOT)] if a.parent else [("b,c,d", ROOT)]) * a.runs
    for settings, tree in plan:                                 # one child at a time; any failure ends the run: nothing more is started
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", settings, "--tree", tree, "--windows", str(a.windows),
                            "--calls", str(a.calls)], capture_output=True, text=True, timeout=a.child_timeout)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"setting {settings} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        for key, v in json.loads(line[-1][7:]).items():
            slot = raw.setdefault(key, {})
            for k, w in v.items():                              # (windows of all runs of a setting side by side)
                if isinstance(w, list):
                    slot.setdefault(k, []).extend(w)
                else:
                    slot[k] = w
        print(f"setting {settings}: done", flush=True)
    stat = lambda x: {"median_us": float(np.median(x)), "min_us": float(min(x)), "max_us": float(max(x)), "windows": len(x)}  # noqa: E731
    res = {"calls_per_window": a.calls, "windows_per_run": a.windows, "runs": a.runs, "settings": {}, "default_path": {}}
    for key, v in sorted(raw.items()):
        pre = [x - float(np.median(v["one_step_launch_us"])) for x in v["acting_one_step_launch_us"]]
        res["settings"][key] = {"prestep_us": stat(pre), "mask_kernel_us": stat(v["mask_kernel_us"]), "one_step_launch_us": stat(v["one_step_launch_us"]),
                                "acting_one_step_launch_us": stat(v["acting_one_step_launch_us"]), "share_of_entries_masked": v["share_of_entries_masked"]}
    ok_all = True
    for key in sorted(k[:-2] for k in raw if k.endswith("/b") and k[:-2] + "/a" in raw):
        pa, pb = res["settings"][key + "/a"], res["settings"][key + "/b"]
        for kern in ("prestep_us", "mask_kernel_us"):
            bar = pa[kern]["max_us"] + (pa[kern]["max_us"] - pa[kern]["min_us"])
            ok = pb[kern]["median_us"] <= bar
            ok_all = ok_all and ok
            res["default_path"][f"{key}/{kern}"] = {"parent_min_us": pa[kern]["min_us"], "parent_max_us": pa[kern]["max_us"], "bar_us": bar,
                                                    "this_tree_median_us": pb[kern]["median_us"], "within": bool(ok)}
    res["verdict"] = ("default path within the parent's spread" if ok_all else "default path ABOVE the parent's spread") if res["default_path"] \
        else "not evaluated (no --parent)"
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
