"""GPU test of the register-resident item ADDRESSES of the flat LU program and of the Jacobian that is only written for an evaluation
that is factorised (gridpf_sparse.hpp: FlatWords, LATE_J): the run-time specialised instance-group kernels built by default against the
same kernels built with -DGPF_NO_WORDS_RES, the developer switch that selects the untouched streaming sweeps and the Newton loop that
writes where it computes.  The flag is read when the library starts, so each build runs in a fresh child process (this file, as a
script); every array a launch leaves behind must agree byte for byte.

Cases: the 14-substation grid (two instances per wavefront) and the 5-substation grid (four), 64 lanes, one 3-step launch with load
jitter, rebalancing and the observation trajectory on; the same with lines out on some lanes (lane 1 shares its wavefront with the
intact lane 0); and a launch with a loose tolerance (found by bisection), where the instances of one wavefront converge in different iterations -- the
decision "this evaluation is factorised" is per wavefront, so one group is done while its neighbour iterates."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
B, N = 64, 3
CASES = [("l2rpn_case14_sandbox", "plain"), ("rte_case5_example", "plain"), ("l2rpn_case14_sandbox", "lines_out"),
         ("rte_case5_example", "lines_out"), ("l2rpn_case14_sandbox", "loose"), ("rte_case5_example", "loose")]
LINES_OUT = {1: 3, 5: 2, 20: 3}            # lane -> line


def _arrays(eng, tag, out):
    r = eng.results()
    rho, ovc, dr = eng.step_outputs()
    out.update({f"{tag}.out": r.out, f"{tag}.status": r.status, f"{tag}.topo_vect": r.topo_vect, f"{tag}.line_status": r.line_status,
                f"{tag}.shunt_bus": r.shunt_bus, f"{tag}.bus_vm": r.bus_vm, f"{tag}.bus_va": r.bus_va, f"{tag}.rho": rho,
                f"{tag}.overflow_count": ovc, f"{tag}.disc_round": dr})
    t_rho, t_st = eng.trajectory(N)
    out.update({f"{tag}.traj_rho": t_rho, f"{tag}.traj_status": t_st})
    for s, o in enumerate(eng.trajectory_obs(N)):
        out.update({f"{tag}.traj{s}_out": o.out, f"{tag}.traj{s}_topo": o.topo_vect, f"{tag}.traj{s}_lstat": o.line_status,
                    f"{tag}.traj{s}_shb": o.shunt_bus})


def _split_tolerance(eng):
    """A tolerance (MVA) at which the instances of some wavefront stop after different numbers of iterations: bisection between a loose
    and a tight one on "every lane still takes the loose count".  The lanes' mismatches after an iteration are a few percent apart, so a
    fixed list of tolerances hits the gap only by luck."""
    ipw = eng.plan()["instances_per_wavefront"]

    def iters(tol):
        eng.step(0, n_steps=N, rebalance=1.02, tol_mva=tol)
        return eng.results().status[:, 1].copy()
    hi, lo = 10.0, 1e-6
    it_hi = iters(hi)
    assert not (iters(lo) == it_hi).all()
    for _ in range(60):
        mid = float(np.sqrt(hi * lo))
        it = iters(mid).reshape(-1, ipw)
        if (it.min(axis=1) != it.max(axis=1)).any():
            return mid
        if (it.reshape(-1) == it_hi).all():
            hi = mid
        else:
            lo = mid
    raise AssertionError("no tolerance splits a wavefront")


def _child(outfile, cache):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from grid2op_amd.grid_model import GridModel
    from test_gpu_multistep import _setup
    gold = os.path.join(ROOT, "tests", "golden")
    load_model = lambda name: GridModel.load_npz(os.path.join(gold, f"{name}.grid.npz"))  # noqa: E731
    load_npz = lambda fname: dict(np.load(os.path.join(gold, fname)))  # noqa: E731
    out = {}
    for name, case in CASES:
        m, ch, eng, tab, off, scale = _setup(load_model, load_npz, name, B)
        info = eng.specialize(True, cache_dir=cache, verify=False)
        assert info["enabled"], info
        eng.set_trajectory(N, eng.TRAJ_OBS)
        if case in ("lines_out", "loose"):
            for lane, line in LINES_OUT.items():
                eng.disconnect_line(lane, line % m.n_line)
        if case == "loose":        # the instances of a wavefront carry different loads: their mismatches pass a tolerance in different iterations
            ipw = eng.plan()["instances_per_wavefront"]
            heavier = (1.0 + 0.12 * (np.arange(B) % ipw)).astype(np.float32)[:, None]
            eng.set_lane_chronics(lane_offset=off, lane_scale=scale * heavier)
        tol = 1e-8
        if case == "loose":
            tol = _split_tolerance(eng)
            out[f"{name}.{case}.tol"] = np.asarray(tol)
        eng.step(0, n_steps=N, rebalance=1.02, tol_mva=tol)
        _arrays(eng, f"{name}.{case}.0", out)
        info = eng.specialization()
        assert info["failed"] == 0 and info["launches"] >= 1, info
        out[f"{name}.{case}.ipw"] = np.asarray(eng.plan()["instances_per_wavefront"])
        eng.close()
    np.savez(outfile, **out)


@pytest.fixture(scope="module")
def both_builds(tmp_path_factory):
    """{key: array} of the default build and of the -DGPF_NO_WORDS_RES build: one child process each, every case in it."""
    got = []
    for tag, flags in (("default", None), ("streaming", "-DGPF_NO_WORDS_RES")):
        d = tmp_path_factory.mktemp(tag)
        env = dict(os.environ)
        env.pop("GRIDPF_JIT_FLAGS", None)
        if flags:
            env["GRIDPF_JIT_FLAGS"] = flags
        env["GRIDPF_JIT_CACHE"] = str(d / "cache")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(d / "out.npz"), str(d / "cache")], env=env, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, (tag, p.stdout[-2000:], p.stderr[-4000:])
        got.append(dict(np.load(d / "out.npz")))
    return got


@pytest.mark.parametrize("name,case", CASES)
def test_resident_addresses_and_late_jacobian_reproduce_the_streaming_build(name, case, both_builds):
    new, ref = both_builds
    keys = sorted(k for k in new if k.startswith(f"{name}.{case}."))
    assert keys and keys == sorted(k for k in ref if k.startswith(f"{name}.{case}.")), keys[:4]
    assert int(new[f"{name}.{case}.ipw"]) == (2 if name == "l2rpn_case14_sandbox" else 4)
    for k in keys:
        x, y = new[k], ref[k]
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
    st = new[f"{name}.{case}.0.status"]
    if case == "plain":
        assert (st[:, 0] == 0).all() and (st[:, 1] >= 2).all(), st[:4]
    if case == "lines_out":
        ls = new[f"{name}.{case}.0.line_status"]
        n_line = ls.shape[1]
        for lane, line in LINES_OUT.items():
            assert not ls[lane, line % n_line] and ls[lane - 1].all(), (lane, line)
    if case == "loose":
        ipw = int(new[f"{name}.{case}.ipw"])
        assert float(new[f"{name}.{case}.tol"]) == float(ref[f"{name}.{case}.tol"])
        it = st[:, 1].reshape(-1, ipw)
        split = int((it.min(axis=1) != it.max(axis=1)).sum())
        print(f"{name}: tolerance {float(new[f'{name}.{case}.tol']):.4g} MVA, {split} wavefronts whose instances took different iteration counts")
        assert split > 0, "no wavefront had one group done while its neighbour iterated: the case checks nothing"


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
