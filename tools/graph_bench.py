"""Developer tool (outside bench.py): what one `graph_observation` call costs, with and without the dense planes, beside `observation_vector`
(the complete observation, the yardstick for a read-only gather here) on the same lanes.

HIP events on the engine's stream around WINDOWS windows of CALLS calls each, after warm-up, into caller-owned tensors (no allocation in
the windows), for l2rpn_case14_sandbox x 4 096 lanes and l2rpn_wcci_2022_dev (118 substations) x 2 048 lanes.  The lanes hold the
recorded topologies of tests/golden/graph_*.npz in turn (split substations, open lines) after one power flow.  Per setting: microseconds
per call (median, fastest and slowest window) and the bytes a call writes.  GRIDPF_GRAPH_STAGE=0 in the environment times the kernel
without its LDS copies of the lanes' rows (--out then names another file).  Writes profiles/graph_bench.json.

    python tools/graph_bench.py [--windows 10] [--calls 1000]
"""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("l2rpn_case14_sandbox", "graph_case14.npz", 6, 4096), ("l2rpn_wcci_2022_dev", "graph_wcci118.npz", 4, 2048))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    from grid2op_amd.obs_spec import ObsSpec
    gold = os.path.join(ROOT, "tests", "golden")
    record = {"windows": a.windows, "calls": a.calls, "GRIDPF_GRAPH_STAGE": os.environ.get("GRIDPF_GRAPH_STAGE", "1"), "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, fixture, n_topo, n in SHAPES:
        m = GridModel.load_npz(os.path.join(gold, name + ".grid.npz"))
        fx = np.load(os.path.join(gold, fixture))
        eng = PowerFlowEngine(m, n_lanes=n, device=0)
        eng.set_topology(fx["topo_vect"][np.arange(n) % n_topo], fx["shunt_bus"][np.arange(n) % n_topo])
        eng.runpf()
        assert eng.results().converged.all()
        spec = ObsSpec.complete(m, fill=True)
        eng.set_obs_clock(datetime.datetime(2019, 1, 6), 5, 2016)
        eng.set_obs_spec(spec)
        eng.set_graph_obs(True)
        lay = eng.graph_layout()
        dev = torch.device("cuda", 0)
        obs = torch.empty((n, spec.dim), dtype=torch.float32, device=dev)
        idx = torch.empty((n, lay["width"]), dtype=torch.int32, device=dev)
        feat = torch.empty((n, lay["NB"], 4), dtype=torch.float32, device=dev)
        dense = torch.empty((n, 3, lay["NB"], lay["NB"]), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        stream = eng.device_views()["stream"]
        settings = {
            "observation_vector": (lambda: eng.observation_vector(out=obs), obs.numel() * 4),
            "graph_observation": (lambda: eng.graph_observation(out_index=idx, out_features=feat), (idx.numel() + feat.numel()) * 4),
            "graph_observation_dense": (lambda: eng.graph_observation(out_index=idx, out_features=feat, out_dense=dense),
                                        (idx.numel() + feat.numel() + dense.numel()) * 4),     # (the planes' zero fill; the few entries stored on top are not counted)
        }
        times = {k: [] for k in settings}
        for k, (call, _) in settings.items():
            for _ in range(5):
                call()
        eng.sync()
        for _ in range(a.windows):                        # the settings alternate window by window
            for k, (call, _) in settings.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.calls):
                    call()
                e1.record(stream)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
        shape = {"lanes": n, "NB": lay["NB"], "obs_dim": spec.dim, "index_width": lay["width"]}
        for k, (_, nbytes) in settings.items():
            t = np.asarray(times[k])
            shape[k] = {"us_per_call_median": float(np.median(t)), "us_fastest_window": float(t.min()), "us_slowest_window": float(t.max()),
                        "bytes_written": int(nbytes), "gb_per_s_median": float(nbytes / np.median(t) / 1e3)}
            print(name, n, k, json.dumps(shape[k]), flush=True)
        record["shapes"][name] = shape
        eng.close()
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
