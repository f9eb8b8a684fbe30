"""Engine teardown and reuse: an engine with every optional resource allocated (environment dynamics, topology actions, an observation
trajectory, the pinned result block, a simulate batch and a PTDF batch) runs its workload and is destroyed; a second, identical engine
built right after it -- on the memory the first one freed -- must give bit-identical results.  Exercises the owners that free the
engine's device buffers, pinned host blocks, events and stream (gridpf_engine.hpp)."""
import numpy as np
import pytest

from test_gpu_envdyn import _engine

pytestmark = pytest.mark.gpu

NAME = "educ_case14_storage"


def _workload(m, fx):
    B = 8
    eng = _engine(m, fx, B)                       # environment dynamics on (generator limits, storage parameters)
    eng.set_trajectory(2, eng.TRAJ_OBS)
    eng.upload_topo_actions([{}, {"set_line_status": [(3, -1)]}, {"set_line_status": [(5, -1)]}])
    eng.set_topo_rules(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=2, cooldown_line=2)
    disp = np.nonzero(fx["redispatchable"])[0]
    red = np.zeros((B, m.n_gen), np.float32)
    red[0, disp[0]], red[0, disp[1]] = 2.0, -2.0
    sto = np.zeros((B, m.n_storage), np.float32)
    sto[1] = 1.5
    eng.set_lane_actions(red, sto)                # the pinned action block
    eng.step(1, n_steps=2, nb_ts_reco=2)
    eng.set_lane_topo_actions(np.array([1, 2, -1, 0, 1, 2, -1, 0], np.int32))
    eng.step(3, nb_ts_reco=2)
    r = eng.results(pinned=True)                  # aliases the engine's pinned block: copied below
    got = {"out": r.out.copy(), "status": r.status.copy(), "topo": r.topo_vect.copy(), "scd": eng.sub_cooldown(), "cd": eng.cooldown()}
    got.update({f"env_{k}": v for k, v in eng.env_state().items()})
    got["traj_out"] = eng.trajectory_obs(1)[0].out
    eng.simulate_batch(3, [0, 1], [{}, {"set_line_status": [(3, -1)]}], dst_lane0=4, time_step=0)
    got["sim_out"] = eng.results(4, 4).out
    info = eng.ptdf_build_batch(with_lodf=True)
    got["ptdf_class"] = info["lane_class"]
    got["ptdf_status"] = info["class_status"]
    got["ptdf_flows"] = eng.ptdf_flows()
    got["lodf_worst"] = eng.lodf_screen()
    eng.close()                                   # gpf_destroy: every buffer, pinned block, event and the stream
    return got


def test_second_engine_after_destroy_is_bit_identical(load_model, load_npz):
    m = load_model(NAME)
    fx = load_npz(f"envdyn_{NAME}.npz")
    a = _workload(m, fx)
    b = _workload(m, fx)
    assert (a["cd"] > 0).any()                    # the topology actions were played
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
