"""GPU test of the launch features of the grid-specialised step kernels (gridpf_common.hpp: FEAT_*, gridpf_host.hpp: gpf_step_features):
a code object compiled for one launch-feature word is only ever launched with that word.  Two engines of the same grid run the same
sequence of launches -- A on the shipped kernels, B with features on -- through launches whose words differ (cascade, an outage table with
an outage inside the window, auto-reset, a one-step launch on the kept state, trajectory off), and after EVERY launch every buffer the
step kernel writes must agree byte for byte.  The object of the first launch would ignore the outage of the third."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_multistep import _setup  # noqa: E402

N_A = 5          # steps of the multi-step launches


def _buffers(eng, n_steps, traj, cool):
    r = eng.results()
    rho, ovc, dr = eng.step_outputs()
    topo, sb = eng.get_topology()
    got = dict(out=r.out, status=r.status, topo_vect=r.topo_vect, line_status=r.line_status, shunt_bus=r.shunt_bus, bus_vm=r.bus_vm,
               rho=rho, overflow_count=ovc, disc_round=dr, topo_rows=topo, shunt_rows=sb, inj=eng.get_injections())
    for k, x in zip(("done", "ep_steps", "ep_resets"), eng.episode()):
        got[k] = np.asarray(x)
    if cool:
        got["cooldown"] = eng.cooldown()
    if traj:
        t_rho, t_st = eng.trajectory(n_steps)
        got.update(traj_rho=t_rho, traj_status=t_st)
        for s, o in enumerate(eng.trajectory_obs(n_steps)):
            got.update({f"traj{s}_out": o.out, f"traj{s}_topo": o.topo_vect, f"traj{s}_lstat": o.line_status, f"traj{s}_shb": o.shunt_bus})
        if cool:
            got["traj_cool"] = eng.trajectory_cooldown(n_steps)
    return got


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


@pytest.mark.parametrize("name,B", [("l2rpn_case14_sandbox", 64),          # two instances per wavefront
                                    ("rte_case5_example", 64),             # four per wavefront
                                    ("l2rpn_neurips_2020_track1", 16)])    # one per wavefront
def test_feature_objects_reproduce_the_shipped_kernels_through_changing_launch_features(name, B, load_model, load_npz, tmp_path, monkeypatch):
    monkeypatch.setenv("GRIDPF_JIT_CACHE", str(tmp_path))
    m, ch, e_a, tab, off, scale = _setup(load_model, load_npz, name, B)
    _, _, e_b, _, _, _ = _setup(load_model, load_npz, name, B)
    T = tab.shape[0]
    info = e_b.specialize(True, verify=False, features=True)
    assert info["enabled"]
    maint = np.zeros((T, m.n_line), np.uint8)
    maint[(np.arange(T) % 7 == 3) | (np.arange(T) % 7 == 4), 1] = 1         # line 1 out for two rows in every seven: inside the window of most lanes
    t = [0]
    launches = [0]

    def both(what, n_steps, traj=True, cool=False, **kw):
        for e in (e_a, e_b):
            e.step(t[0], n_steps=n_steps, **kw)
        launches[0] += 1
        _same(_buffers(e_a, n_steps, traj, cool), _buffers(e_b, n_steps, traj, cool), (name, what))
        t[0] += n_steps

    for e in (e_a, e_b):
        e.set_trajectory(N_A, e.TRAJ_OBS)
    both("(a) trajectory, rebalance", N_A, rebalance=1.02)
    if "thermal_limits" in ch:
        for e in (e_a, e_b):
            e.set_thermal_limits(np.asarray(ch["thermal_limits"]) * 0.85)
    both("(b) cascade", N_A, cool=True, rebalance=1.02, cascade=True)
    for e in (e_a, e_b):
        e.upload_maintenance(maint)
    both("(c) outage table", 3, cool=True, rebalance=1.02)
    assert (_buffers(e_b, 3, True, True)["topo_rows"][:, m.line_or_pos_topo_vect[1]] == -1).any(), "no lane met the outage: the case checks nothing"
    both("(d) auto-reset", N_A, cool=True, rebalance=1.02, auto_reset=True)
    both("(e) one step, kept state", 1, cool=True, rebalance=1.02)
    for e in (e_a, e_b):
        e.set_trajectory(0)
    both("(f) trajectory off", N_A, traj=False, cool=True, rebalance=1.02)
    for e in (e_a, e_b):
        e.upload_maintenance(None)
        e.reset()
        e.set_trajectory(N_A, e.TRAJ_OBS)
    both("(g) as (a)", N_A, rebalance=1.02)

    info = e_b.specialization()
    words = {v.split(">")[0].split(",")[8] for v in info["variants"].split(" | ")[0].split() if re.match(r"^<([^,>]+,){8}\d+>", v)}
    assert len(words) >= 2, info
    assert info["failed"] == 0 and info["launches"] == launches[0] == 7, info
    assert e_a.specialization()["launches"] == 0
    e_a.close()
    e_b.close()
