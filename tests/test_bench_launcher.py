"""``bench.py --gpus N`` on CPU: the launcher must really start N ranks (one process per GPU in production; here gloo +
the arithmetic-free stub engine), shard the global batch, and print ONE JSON line that says so.  Also: a request for
more GPUs than are visible must fail loudly instead of silently measuring fewer, and `ShardedEngine` (the single-process
form) must route global lane ranges to the right per-device engine."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _run(argv, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + argv, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


def test_gpus_2_launches_two_ranks_and_reports_them():
    p = _run(["--gpus", "2", "--steps", "7", "--warmup", "2", "--windows", "3", "--stub-engine", "--dist-backend", "gloo",
              "--no-cpu-baseline"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout                           # rank 0 only
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 7 and res["warmup"] == 2
    assert res["config"]["lanes_per_gpu"] == 4096 and res["config"]["total_lanes"] == 8192
    assert res["scaling"] == "weak" and res["windows"]["n"] == 3
    # value = the units ALL ranks processed / the (max over ranks) time of the median window
    assert res["value"] == pytest.approx(8192 * 7 / (res["ms_per_step"] * 7 * 1e-3), rel=1e-9)
    assert "STUB" in res["data"]


def test_gpus_mismatch_with_world_size_fails_loudly():
    p = _run(["--gpus", "2", "--stub-engine", "--dist-backend", "gloo"], env_extra={"WORLD_SIZE": "1", "RANK": "0"})
    assert p.returncode != 0
    assert "WORLD_SIZE" in p.stderr


def test_more_gpus_than_visible_is_refused():
    """No silent 1-GPU measurement: in this container no HIP device is visible at all."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    p = _run(["--gpus", "2", "--steps", "2", "--warmup", "1"])
    assert p.returncode != 0
    assert "refusing" in p.stderr and not [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_sharded_engine_routes_global_lanes(load_model):
    from grid2op_amd.sharding import ShardedEngine, lane_range
    from stub_engine import StubEngine
    m = load_model("rte_case5_example")
    made = []

    def factory(model, n, dev, nbb):
        e = StubEngine(model, n_lanes=n, device=dev, n_busbar=nbb)
        made.append(e)
        return e
    se = ShardedEngine(m, 37, devices=[0, 1, 2], engine_factory=factory)
    assert [e.n_lanes for e in made] == [lane_range(37, 3, r)[1] for r in range(3)] and [e.device for e in made] == [0, 1, 2]
    se.set_lane_chronics(lane_offset=np.arange(37))
    r = se.results()
    assert np.array_equal(r.out[:, 0], np.arange(37))                         # global lane order
    r = se.results(10, 20)
    assert np.array_equal(r.out[:, 0], np.arange(10, 30))                     # a range spanning all three shards
    inj = np.arange(37 * se.n_inj, dtype=float).reshape(37, -1)
    se.set_injections(inj[5:30], lane0=5)
    assert np.array_equal(se.get_injections(5, 25), inj[5:30])
    topo = np.tile(m.initial_topo_vect(), (4, 1))
    topo[:, 0] = 2
    se.set_topology(topo, lane0=11)                                           # crosses the shard boundary at lane 13
    assert (se.results(11, 4).topo_vect[:, 0] == 2).all() and se.results(10, 1).topo_vect[0, 0] == 1
    se.step(0)
    se.runpf(12, 2)
    assert [e.n_steps for e in made] == [1, 1, 1] and [e.n_runpf for e in made] == [1, 1, 0]
    eng, l0 = se.owner(36)
    assert eng is made[2] and l0 == made[2].n_lanes - 1
    with pytest.raises(ValueError):
        se.results(30, 10)
    se.close()


def test_plain_run_times_exactly_steps_and_dumps_the_last_step(tmp_path):
    """A plain run times ONE window of exactly --steps steps and measures nothing else; --dump-outputs writes the result arrays of the
    last timed step (the stub engine's first result column is the lane's chronics offset), identical from run to run."""
    dumps = []
    for k in range(2):
        d = tmp_path / f"out{k}"
        p = _run(["--gpus", "1", "--steps", "7", "--warmup", "2", "--batch", "64", "--stub-engine", "--dump-outputs", str(d)],
                 env_extra={"GRIDPF_BENCH_FULL": str(tmp_path / "full.json")})
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout
        res = json.loads(lines[0])
        assert res["steps"] == 7 and res["windows"]["n"] == 1 and res["ms_per_step"] > 0
        assert res["cpu_baseline"] is None and res["configs"] == {} and "parity" not in res
        with open(tmp_path / "full.json") as f:
            full = json.load(f)
        assert len(full["windows"]["elapsed_ms"]) == 1 and "shipped_kernels" not in full
        files = sorted(os.listdir(d))
        assert {"p_or", "rho", "bus_vm", "topo_vect", "status"} <= {f[:-4] for f in files} and "lanes.npy" not in files
        arrs = {f[:-4]: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and a.shape[0] == 64 and a.size > 0 and np.isfinite(a).all() for a in arrs.values())
        assert "storage_p" not in arrs                                          # l2rpn_case14_sandbox has no storage unit: no empty file
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        dumps.append(arrs)
    assert dumps[0].keys() == dumps[1].keys()
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


def test_dump_outputs_samples_lanes_beyond_64_mb(tmp_path):
    import bench
    from grid2op_amd.engine import LaneResults
    n = 70000
    out = np.arange(n, dtype=np.float32)[:, None] * np.ones((1, 300), np.float32)          # 84 MB of float32 rows
    r = LaneResults(out=out, topo_vect=np.ones((n, 4), np.int32), shunt_bus=np.zeros((n, 1), np.int32), line_status=np.ones((n, 2), bool),
                    status=np.zeros((n, 4), np.int32), bus_vm=None, bus_va=None, _slices={"a": slice(0, 100), "b": slice(100, 300)})
    for k in range(2):
        bench.dump_outputs(r, str(tmp_path / f"d{k}"))
    a = {f[:-4]: np.load(tmp_path / "d0" / f) for f in os.listdir(tmp_path / "d0")}
    assert sorted(a) == ["a", "b", "lanes", "line_status", "shunt_bus", "status", "topo_vect"]
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    lanes = a["lanes"].astype(np.int64)
    assert 0 < lanes.size < n and np.all(np.diff(lanes) > 0)
    assert np.array_equal(a["a"][:, 0], lanes.astype(np.float32)) and a["b"].shape == (lanes.size, 200)
    for f in os.listdir(tmp_path / "d0"):
        assert np.array_equal(np.load(tmp_path / "d0" / f), np.load(tmp_path / "d1" / f)), f


def test_dump_outputs_writes_missing_values_as_flagged_zeros(tmp_path):
    """Unused buses (NaN voltages) and failed lanes (NaN rows) are written as 0 and flagged by bus_active / status: every file is finite,
    nothing else is touched."""
    import bench
    from grid2op_amd.engine import LaneResults
    n, nb = 4, 6
    out = np.arange(n * 5, dtype=np.float32).reshape(n, 5)
    out[2] = np.nan                                                              # lane 2 failed: no results
    vm = np.linspace(0.9, 1.1, n * nb).reshape(n, nb)
    vm[:, 3:] = np.nan                                                           # buses 3.. unused
    vm[2] = np.nan
    va = np.where(np.isnan(vm), np.nan, -vm)
    st = np.zeros((n, 4), np.int32)
    st[2, 0] = 3
    r = LaneResults(out=out, topo_vect=np.ones((n, 4), np.int32), shunt_bus=np.zeros((n, 1), np.int32), line_status=np.ones((n, 2), bool),
                    status=st, bus_vm=vm, bus_va=va, _slices={"a": slice(0, 2), "b": slice(2, 5), "c": slice(5, 5)})
    rho = np.ones((n, 2), np.float32)
    rho[2] = np.nan
    bench.dump_outputs(r, str(tmp_path), (rho, np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)))
    a = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(np.isfinite(v).all() and v.size > 0 for v in a.values()) and "c" not in a          # a field without elements: no file
    assert np.array_equal(a["bus_active"], np.isfinite(vm).astype(np.float32))
    assert np.array_equal(a["bus_vm"], np.nan_to_num(vm)) and np.array_equal(a["bus_va"], np.nan_to_num(va))
    assert np.array_equal(a["a"][[0, 1, 3]], out[[0, 1, 3], :2]) and not a["a"][2].any() and not a["rho"][2].any()
    assert a["status"][2, 0] == 3
