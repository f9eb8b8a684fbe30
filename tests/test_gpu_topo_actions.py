"""Topology actions in the batched step (include/gridpf.h: gpf_upload_topo_actions): the device path against a twin engine that gets the
same post-action rows through set_topology from the Python restatement (tests/topo_rules_ref.py), host vs device hand-over, the
multi-step decrement of the substation cooldowns and the refusals.

No maintenance is uploaded in this file: no outage is under way at any one-step launch, so the shared reference-topology state of
one-step launches (GRIDPF_KEEP) is on throughout (the keep path agents use).
"""
import numpy as np
import pytest

from conftest import golden_path
from topo_rules_ref import TopoRules, random_topo_table

pytestmark = pytest.mark.gpu

STEP = dict(cascade=True, nb_ts_reco=10)
# The twin comparison steps without the protections: a line the step kernel trips on the device leaves the lane's planning class as it
# was on BOTH launch paths of this engine (the host is told at its next gpf_set_topology), while the twin re-sends every row -- a
# different, equally valid bus-level program whose last bits differ.  Line status changes then come from the agents alone.
TWIN = dict(cascade=False, nb_ts_reco=10)
RULES = dict(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=3)


def _engine(name, n, offsets):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path(f"{name}.grid.npz"))
    ch = dict(np.load(golden_path(f"{name}.chronics.npz")))
    if "prod_v" not in ch:                         # (fixtures without voltage set-points: the grid's own)
        ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    eng.set_lane_chronics(lane_offset=offsets)
    if "thermal_limits" in ch:                     # (rte_case5_example has none)
        eng.set_thermal_limits(ch["thermal_limits"])
    return m, eng


def _state(eng):
    r = eng.results()
    ill, amb = eng.topo_action_flags()
    return dict(out=r.out, topo=eng.get_topology()[0], status=r.status, cd=eng.cooldown(), scd=eng.sub_cooldown(), lb=eng.last_bus(),
                ill=ill, amb=amb, done=eng.episode()[0])


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name,n,steps", [("l2rpn_case14_sandbox", 4096, 32), ("l2rpn_wcci_2022_dev", 1024, 32)])
def test_device_path_equals_host_restatement_twin(name, n, steps):
    rng = np.random.default_rng(7)
    offsets = 5 * np.arange(n)
    m, a = _engine(name, n, offsets)
    _, b = _engine(name, n, offsets)
    acts = random_topo_table(m, rng)
    amb = a.upload_topo_actions(acts)
    a.set_topo_rules(**RULES)
    off, items = a.pack_actions(acts)
    ref = TopoRules(m, off, items, True, 1, 1, 3, 3)
    assert np.array_equal(amb, ref.ambiguous) and amb.any()
    line_cd = np.zeros((n, m.n_line), np.int64)
    sub_cd = np.zeros((n, m.n_sub), np.int64)
    last = np.maximum(np.tile(a.last_bus(0, 1)[0], (n, 1)), 1)
    topo = b.get_topology()[0]
    n_ill = n_amb = 0
    for t in range(1, steps + 1):
        idx = rng.integers(-1, len(acts), size=n).astype(np.int32)
        rows, aff_l, aff_s, ill, am = [], [], [], np.zeros(n, bool), np.zeros(n, bool)
        for k in range(n):
            r_, ill[k], am[k], al, as_ = ref.pre(topo[k], line_cd[k], sub_cd[k], last[k], int(idx[k]))
            rows.append(r_); aff_l.append(al); aff_s.append(as_)
        b.set_topology(np.asarray(rows, np.int32))
        a.set_lane_topo_actions(idx)
        a.step(t, **TWIN)
        b.step(t, **TWIN)
        sa = _state(a)
        topo = b.get_topology()[0]
        dn = b.episode()[0]
        lcd = b.cooldown()
        for k in range(n):
            if dn[k]:
                continue
            lcd[k], sub_cd[k], last[k] = ref.post(topo[k], lcd[k], sub_cd[k], last[k], aff_l[k], aff_s[k])
        b.set_cooldown(lcd)
        line_cd = lcd.astype(np.int64)
        assert np.array_equal(sa["ill"], ill) and np.array_equal(sa["amb"], am), t
        n_ill += int(ill.sum()); n_amb += int(am.sum())
        assert np.array_equal(sa["topo"], topo), t
        assert np.array_equal(sa["out"], b.results().out, equal_nan=True), t
        assert np.array_equal(sa["cd"], lcd) and np.array_equal(sa["scd"], sub_cd) and np.array_equal(sa["lb"], last), t
        assert np.array_equal(sa["done"], dn), t
    assert n_ill > 0 and n_amb > 0
    a.close(); b.close()


def test_host_and_device_handover_bit_identical():
    import torch
    n = 512
    rng = np.random.default_rng(3)
    m, a = _engine("l2rpn_case14_sandbox", n, 3 * np.arange(n))
    _, d = _engine("l2rpn_case14_sandbox", n, 3 * np.arange(n))
    acts = random_topo_table(m, rng)
    for e in (a, d):
        e.upload_topo_actions(acts)
        e.set_topo_rules(**RULES)
    views = d.device_views()
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    for t in range(1, 17):
        with torch.cuda.stream(views["stream"]):
            idx = torch.randint(-1, len(acts) + 2, (n,), generator=gen, device="cuda:0", dtype=torch.int32)   # (+2: out of the table)
            views["act_topo"][:, 0].copy_(idx)
        d.topo_actions_on_device()
        d.step(t, **STEP)
        a.set_lane_topo_actions(idx.cpu().numpy())
        a.step(t, **STEP)
        _same(_state(a), _state(d), ("out", "topo", "status", "cd", "scd", "lb", "ill", "amb", "done"))
        if t == 1:
            assert _state(d)["amb"][idx.cpu().numpy() >= len(acts)].all()       # an index outside the table counts as ambiguous
    a.close(); d.close()


def test_multistep_decrement_equals_one_step_launches():
    n = 256
    rng = np.random.default_rng(5)
    m, a = _engine("l2rpn_case14_sandbox", n, 2 * np.arange(n))
    _, b = _engine("l2rpn_case14_sandbox", n, 2 * np.arange(n))
    acts = random_topo_table(m, rng)
    idx = rng.integers(0, len(acts), size=n).astype(np.int32)
    for e in (a, b):
        e.upload_topo_actions(acts)
        e.set_topo_rules(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=5, cooldown_line=3)
        e.set_lane_topo_actions(idx)
        e.step(1, nb_ts_reco=10)
    assert a.sub_cooldown().max() == 5
    a.step(2, n_steps=3, nb_ts_reco=10)
    for t in (2, 3, 4):
        b.step(t, nb_ts_reco=10)
    _same(_state(a), _state(b), ("out", "topo", "scd", "lb", "done"))
    assert a.sub_cooldown().max() == 2
    a.reset()
    assert not a.sub_cooldown().any() and (a.last_bus() >= 1).all()
    a.close(); b.close()


def test_refusals():
    from grid2op_amd._capi import GridPFError
    n = 64
    m, a = _engine("l2rpn_case14_sandbox", n, np.arange(n))
    a.upload_topo_actions([{"set_line_status": [(0, -1)]}])
    a.set_topo_rules(**RULES)
    a.set_lane_topo_actions(np.zeros(n, np.int32))
    with pytest.raises(GridPFError):
        a.step(1, n_steps=2, nb_ts_reco=10)        # topology actions need a one-step launch
    with pytest.raises(GridPFError):
        a.step(1, nb_ts_reco=-1)                   # cooldown_line > 0: the line cooldowns must be maintained by the launch
    a.step(1, nb_ts_reco=10)                       # the actions are still pending: taken by this one
    ill, amb = a.topo_action_flags()
    assert not ill.any() and not amb.any()
    assert (a.get_topology()[0][:, m.line_or_pos_topo_vect[0]] == -1).all()
    assert (a.cooldown()[:, 0] == 3).all()
    a.step(2, n_steps=4, nb_ts_reco=10)            # without actions: multi-step is fine, the agents' line cooldowns count down
    assert (a.cooldown()[:, 0] == 0).all()
    a.close()


def test_out_of_range_index_is_an_ambiguous_do_nothing():
    n = 64
    m, a = _engine("l2rpn_case14_sandbox", n, np.arange(n))
    a.upload_topo_actions([{"set_line_status": [(0, -1)]}])
    a.set_topo_rules(**RULES)
    before = a.get_topology()[0]
    idx = np.full(n, 1, np.int32)
    idx[::2] = -7
    a.set_lane_topo_actions(idx)
    a.step(1, nb_ts_reco=10)
    ill, amb = a.topo_action_flags()
    assert amb.all() and not ill.any()
    assert np.array_equal(a.get_topology()[0], before) and not a.sub_cooldown().any() and not a.cooldown().any()
    a.close()


def test_combined_topology_and_injection_actions_refused(load_model, load_npz):
    from grid2op_amd._capi import GridPFError
    from grid2op_amd.engine import PowerFlowEngine
    m, fx = load_model("educ_case14_storage"), load_npz("envdyn_educ_case14_storage.npz")
    n = 16
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(fx["ch_load_p"], fx["ch_load_q"], fx["ch_prod_p"], fx["ch_prod_v"]))
    eng.set_thermal_limits(fx["thermal_limit"])
    eng.set_gen_limits(fx["pmin"], fx["pmax"], fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], eps_poly=float(fx["eps_poly"]))
    eng.set_storage_params(fx["storage_Emax"], fx["storage_Emin"], fx["storage_loss"], fx["storage_charging_efficiency"],
                           fx["storage_discharging_efficiency"], fx["storage_charge0"], float(fx["delta_time_seconds"]),
                           bool(fx["activate_storage_loss"]))
    eng.set_env_dynamics(True, tol_poly=float(fx["tol_poly"]))
    eng.upload_topo_actions([{"set_line_status": [(0, -1)]}])
    eng.set_topo_rules(1, 1, 3, 0)
    eng.set_lane_topo_actions(np.zeros(n, np.int32))
    eng.set_lane_actions(redispatch=np.zeros((n, m.n_gen), np.float32))
    with pytest.raises(GridPFError, match="combined"):
        eng.step(1)
    eng.set_lane_topo_actions(None)                # the injection action alone goes through
    eng.step(1)
    eng.close()


def _split_then_isolate_table(m):
    """entry 0..k-1: splits of the largest substations; then entries that put one load alone on busbar 2 (the lane's episode ends)"""
    from topo_rules_ref import topo_pos_sub
    ps = topo_pos_sub(m)
    big = [int(s) for s in np.argsort(-np.bincount(ps, minlength=m.n_sub))[:4]]
    acts = []
    for s in big[:2]:
        pos = np.flatnonzero(ps == s)
        acts.append({"set_bus": {int(p): (2 if i % 2 else 1) for i, p in enumerate(pos)}})
    for s in big[2:]:
        loads = np.flatnonzero(np.asarray(m.load_sub) == s)
        acts.append({"set_bus": {int(m.load_pos_topo_vect[loads[0]]): 2}})
    return acts


def test_auto_reset_of_a_lane_an_action_moved_is_rekeyed_and_cleared():
    """Step 1: every lane splits a substation (another topology class).  Step 2: half of them put a load alone on busbar 2 of another
    substation, which ends their episode: auto-reset back to the rows last sent (the unsplit topology).  Step 3 (do nothing) must then
    run every lane on the class of the rows it really has: bit-identical to a twin engine that got those rows through set_topology."""
    n = 256
    offs = 3 * np.arange(n)
    m, a = _engine("l2rpn_case14_sandbox", n, offs)
    _, b = _engine("l2rpn_case14_sandbox", n, offs)
    acts = _split_then_isolate_table(m)
    a.upload_topo_actions(acts)
    a.set_topo_rules(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=0)
    a.set_lane_topo_actions((np.arange(n) % 2).astype(np.int32))
    a.step(1, auto_reset=True)
    idx = np.full(n, -1, np.int32)
    idx[::2] = 2 + (np.arange(n)[::2] // 2) % 2
    a.set_lane_topo_actions(idx)
    a.step(2, auto_reset=True)
    _, _, resets = a.episode()
    hit = resets > 0
    assert hit.sum() >= n // 4, resets
    init = np.asarray(m.initial_topo_vect())
    assert (a.get_topology()[0][hit] == init).all()
    assert not a.sub_cooldown()[hit].any() and (a.last_bus()[hit] == np.maximum(init, 1)).all()   # env.reset(): cleared
    assert a.sub_cooldown()[~hit].max() >= 2
    b.set_topology(a.get_topology()[0])
    a.step(3, auto_reset=True)
    b.step(3, auto_reset=True)
    ra, rb = a.results(), b.results()
    assert np.array_equal(ra.out, rb.out, equal_nan=True) and np.array_equal(ra.status, rb.status)
    with pytest.raises(Exception):
        a.step(4, n_steps=2, auto_reset=True)      # lanes still on a moved class: a reset inside a multi-step launch is refused
    a.close(); b.close()


def test_copy_lanes_and_fanout_n1_carry_the_acting_state_and_the_moved_mark():
    """Lane 1 splits substation 3 (another topology class, a substation cooldown, a last known busbar 2), lane 2 plays an index outside
    the table (ambiguous).  copy_lanes and fanout_n1 give their destinations the sources' substation cooldowns, last known busbars and
    flags.  Lane 4, the copy of lane 1, is then the only lane an action holds on another class than its reset topology's (lane 1 is
    reset; the contingency lanes have the split rows as their reset topology): a multi-step auto-reset launch is refused for it alone,
    and when its episode ends the auto-reset re-keys it -- the next step is bit-identical to a twin engine that got the rows through
    set_topology -- and clears the mark."""
    from grid2op_amd._capi import GridPFError
    n = 8
    offs = 3 * np.arange(n)
    m, a = _engine("rte_case5_example", n, offs)
    _, b = _engine("rte_case5_example", n, offs)
    p_ex6, p_or7, p_load2 = int(m.line_ex_pos_topo_vect[6]), int(m.line_or_pos_topo_vect[7]), int(m.load_pos_topo_vect[2])
    a.upload_topo_actions([{"set_bus": {p_ex6: 2, p_or7: 2}},        # 0: lines 6 and 7 on busbar 2 of substation 3
                           {"set_bus": {p_load2: 2}}])               # 1: a load alone on busbar 2 of substation 4: the episode ends
    a.set_topo_rules(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=0)
    acting = ("topo", "scd", "lb", "ill", "amb")
    a.set_lane_topo_actions(np.array([-1, 0, 7, -1, -1, -1, -1, -1], np.int32))
    a.step(1, auto_reset=True)
    s = _state(a)
    assert s["scd"][1, 3] == 3 and s["lb"][1, p_ex6] == 2 and s["topo"][1, p_or7] == 2 and s["amb"][2] and not s["amb"][1] and not s["ill"].any()
    assert not s["scd"][[0, 2]].any() and not s["done"].any()
    a.copy_lanes(1, 4, 2)                              # lanes 4, 5 := lanes 1, 2
    a.fanout_n1(1, 6, [-1, 0])                         # lanes 6, 7 := lane 1, lane 7 with line 0 out
    c = _state(a)
    for k in acting:
        assert np.array_equal(c[k][4:6], s[k][1:3]) and np.array_equal(c[k][:4], s[k][:4]), k
    for k in ("scd", "lb", "ill", "amb"):
        assert np.array_equal(c[k][6], s[k][1]) and np.array_equal(c[k][7], s[k][1]), k
    out0 = s["topo"][1].copy()
    out0[[m.line_or_pos_topo_vect[0], m.line_ex_pos_topo_vect[0]]] = -1
    assert np.array_equal(c["topo"][6], s["topo"][1]) and np.array_equal(c["topo"][7], out0)
    a.reset(1, 1)
    with pytest.raises(GridPFError, match="another topology class"):
        a.step(2, n_steps=2, auto_reset=True)          # lane 4 took lane 1's mark with its rows
    a.set_lane_topo_actions(np.array([-1, -1, -1, -1, 1, -1, 1, -1], np.int32))
    a.step(2, auto_reset=True)
    e = _state(a)
    init = np.asarray(m.initial_topo_vect())
    assert np.array_equal(a.episode()[2], [0, 0, 0, 0, 1, 0, 1, 0])
    assert np.array_equal(e["topo"][4], init) and np.array_equal(e["topo"][6], s["topo"][1])      # each back on its own reset topology
    assert not e["scd"][[4, 6]].any() and np.array_equal(e["lb"][4], np.maximum(init, 1)) and np.array_equal(e["lb"][6], s["topo"][1])
    assert (e["scd"][[5, 7], 3] == [0, 2]).all()       # (lane 5 is lane 2, which applied nothing; lane 7 counts lane 1's cooldown down)
    b.set_topology(e["topo"])
    a.step(3, auto_reset=True)
    b.step(3, auto_reset=True)
    ra, rb = a.results(), b.results()
    assert np.array_equal(ra.out, rb.out, equal_nan=True) and np.array_equal(ra.status, rb.status) and ra.converged.all()
    a.step(4, n_steps=2, auto_reset=True)              # no lane is on a moved class any more
    a.close(); b.close()


def test_keep_on_and_off_bit_identical(monkeypatch):
    """GRIDPF_KEEP on and off (the shared reference-topology state of one-step launches): lanes leave the reference topology through
    splits and come back through merges; no maintenance uploaded (no outage under way at any launch)."""
    n = 512
    rng = np.random.default_rng(9)
    m, on = _engine("l2rpn_case14_sandbox", n, 4 * np.arange(n))
    monkeypatch.setenv("GRIDPF_KEEP", "0")
    _, off = _engine("l2rpn_case14_sandbox", n, 4 * np.arange(n))
    monkeypatch.delenv("GRIDPF_KEEP")
    acts = random_topo_table(m, rng)
    for e in (on, off):
        e.upload_topo_actions(acts)
        e.set_topo_rules(**RULES)
    back = 0
    for t in range(1, 25):
        idx = rng.integers(-1, len(acts), size=n).astype(np.int32)
        for e in (on, off):
            e.set_lane_topo_actions(idx)
            e.step(t, **STEP)
        s_on, s_off = _state(on), _state(off)
        _same(s_on, s_off, ("out", "topo", "status", "cd", "scd", "lb", "ill", "amb", "done"))
        back += int((s_on["topo"] == np.asarray(m.initial_topo_vect())).all(axis=1).sum())
    assert back > 0
    on.close(); off.close()
