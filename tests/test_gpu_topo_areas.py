"""Rules by area and composite actions on the device (include/gridpf.h: gpf_set_topo_areas / gpf_set_topo_slots; kernels:
grid2op_amd/csrc/gridpf_topo.hpp topo_prestep_kernel<true>, gridpf_topo_mask.hpp topo_mask_kernel) against the episode recorded from the
reference environment under ``RulesByArea`` (tests/golden/topo_area_*.npz), a twin engine whose table holds the concatenated entries, the
legality masks and the factorisation guarantee.  Shapes: 14 substations x 64 lanes, 118 substations x 32 lanes.

The lanes step without the protections (no line leaves by itself, as in the recording); a lane whose power flow fails books nothing, in
the reference as here, and is compared on its flags alone."""
import numpy as np
import pytest

from conftest import golden_path
import topo_area_ref as A
import topo_mask_ref as R

pytestmark = pytest.mark.gpu

RULES = dict(max_sub_changed=1, max_line_status_changed=1, cooldown_sub=3, cooldown_line=3)
STEP = dict(cascade=False, nb_ts_reco=10)
LANES = {"case14": 64, "wcci118": 32}
TAGS = sorted(A.FIXTURES)


def _engine(name, n):
    from grid2op_amd.engine import PowerFlowEngine
    from grid2op_amd.grid_model import GridModel
    m = GridModel.load_npz(golden_path(f"{name}.grid.npz"))
    ch = dict(np.load(golden_path(f"{name}.chronics.npz")))
    if "prod_v" not in ch:
        ch["prod_v"] = np.tile((m.gen_vm0 * m.sub_vn_kv[m.gen_sub]).astype(np.float32), (ch["prod_p"].shape[0], 1))
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    eng.upload_chronics(eng.pack_chronics(ch["load_p"], ch["load_q"], ch["prod_p"], ch["prod_v"]))
    eng.set_lane_chronics(lane_offset=np.zeros(n, dtype=np.int64))
    eng.set_thermal_limits(ch["thermal_limits"])
    return m, eng


def _area_engine(tag, n_slot=3, table=None):
    fix = A.load_fixture(tag)
    m, eng = _engine(A.FIXTURES[tag], LANES[tag])
    eng.upload_topo_actions(R.unpack_actions(fix["off"], fix["items"]) if table is None else table)
    eng.set_topo_rules(**RULES)
    eng.set_topo_areas(fix["sub_area"])
    eng.set_topo_slots(n_slot)
    return fix, m, eng


def _set_recorded(eng, fix, src, lane0=0):
    """lanes lane0.. take the recorded states `src` (fresh lanes: an earlier failed step is forgotten)"""
    eng.reset(lane0, len(src))
    eng.set_topology(fix["topo_vect"][src], lane0=lane0)
    eng.set_cooldown(fix["cooldown_line"][src], lane0=lane0)
    eng.set_sub_cooldown(fix["cooldown_sub"][src], lane0=lane0)
    eng.set_last_bus(np.maximum(fix["last_bus"][src], 1), lane0=lane0)


def _state(eng):
    ill, amb = eng.topo_action_flags()
    return dict(topo=eng.get_topology()[0], cd=eng.cooldown(), scd=eng.sub_cooldown(), lb=eng.last_bus(), ill=ill, amb=amb, done=eng.episode()[0],
                out=eng.results().out)


def _merged(acts, comp):
    out = {}
    for a in comp:
        if a < 0:
            continue
        out.setdefault("set_line_status", []).extend(acts[a].get("set_line_status", ()))
        out.setdefault("change_line_status", []).extend(acts[a].get("change_line_status", ()))
        out.setdefault("set_bus", {}).update(acts[a].get("set_bus", {}))
        out.setdefault("change_bus", []).extend(acts[a].get("change_bus", ()))
    return out


def _longest(fix, set_only=False):
    """the longest table entry that is not ambiguous (set_only: of set_bus / set_line_status items alone)"""
    off, kinds = fix["off"], np.asarray(fix["items"]).reshape(-1, 3)[:, 0]
    ok = [a for a in range(len(off) - 1) if not fix["ambiguous"][0, a] and not (set_only and (kinds[off[a]:off[a + 1]] >= 2).any())]
    return max(ok, key=lambda a: off[a + 1] - off[a])


@pytest.mark.parametrize("tag", TAGS)
def test_replay_of_the_recorded_episode(tag):
    """lane 0 lives through the recorded episode (re-seated where the reference environment was reset), the other lanes start every launch
    from random recorded states and play what was played there: flags and rows after every one-step launch are the recording's"""
    fix, m, eng = _area_engine(tag)
    n, T = LANES[tag], len(fix["played"])
    rng = np.random.default_rng(17)
    assert np.array_equal(eng.get_topology(0, 1)[0][0], fix["topo_vect"][0])
    n_cmp = n_ill = n_lane0 = 0
    reseat = True
    for j in range(T):
        src = np.concatenate([[j], rng.integers(0, T, n - 1)])
        if reseat:
            _set_recorded(eng, fix, src[:1], 0)
        _set_recorded(eng, fix, src[1:], 1)
        eng.set_lane_topo_actions(fix["comps"][fix["played"][src]])
        eng.step(j + 1, **STEP)
        s = _state(eng)
        assert np.array_equal(s["ill"], fix["is_illegal"][src]) and np.array_equal(s["amb"], fix["is_ambiguous"][src]), j
        ok = ~fix["done"][src] & ~s["done"]
        assert np.array_equal(s["topo"][ok], fix["topo_after"][src][ok]), j
        assert np.array_equal(s["cd"][ok], fix["cooldown_line_after"][src][ok]) and np.array_equal(s["scd"][ok], fix["cooldown_sub_after"][src][ok]), j
        assert np.array_equal(s["lb"][ok], np.maximum(fix["last_bus_after"][src][ok], 1)), j
        n_cmp += int(ok.sum()); n_ill += int(s["ill"].sum()); n_lane0 += int(ok[0])
        reseat = not ok[0]
    assert n_cmp >= 0.6 * n * T and n_lane0 >= 0.6 * T and n_ill > 0
    eng.close()


@pytest.mark.parametrize("tag", TAGS)
def test_composite_equals_the_concatenated_entry(tag):
    """slots (a, b, c) of one engine against ONE entry holding the concatenated item list in a twin: flags, rows, cooldowns, last known
    busbars and results, over steps in which the host re-keys lanes to new topology classes and lanes auto-reset.  One index may sit in
    several slots: the first three composites hold the table's longest entry three times, twice next to another entry, and an entry
    around an empty slot, and lanes 0-2 play them at every step"""
    fix = A.load_fixture(tag)
    acts = R.unpack_actions(fix["off"], fix["items"])
    rng = np.random.default_rng(23)
    lg = _longest(fix)
    other = int(fix["comps"][0, 0])
    assert other != lg and other >= 0 and not fix["ambiguous"][0, other]
    dup = np.array([[lg, lg, lg], [lg, lg, other], [other, -1, other]], np.int32)
    comps = np.concatenate([dup, fix["comps"], rng.integers(-1, len(acts), size=(40, 3)).astype(np.int32)])
    _, m, a = _area_engine(tag)
    _, _, b = _area_engine(tag, n_slot=1, table=[_merged(acts, c) for c in comps])
    n = LANES[tag]
    # the part of a lane's topology class key the rows show: the busbar of every line end, an open end counting as busbar 1.  A lane whose
    # key differs from the launch before was re-keyed by the host: moved by its action, or put back by an auto-reset
    ends = np.concatenate([np.asarray(m.line_or_pos_topo_vect), np.asarray(m.line_ex_pos_topo_vect)])
    key = lambda topo: np.where(topo[:, ends] >= 2, topo[:, ends], 1)  # noqa: E731
    prev, ep_prev = key(a.get_topology()[0]), a.episode()[2]
    key0 = prev.copy()
    moved = resets = resets_of_moved = 0
    for t in range(1, 9):
        pick = rng.integers(-1, len(comps), size=n)
        pick[:3] = np.arange(3)
        a.set_lane_topo_actions(np.where(pick[:, None] >= 0, comps[np.maximum(pick, 0)], -1).astype(np.int32))
        b.set_lane_topo_actions(pick.astype(np.int32))
        for e in (a, b):
            e.step(t, cascade=True, nb_ts_reco=10, auto_reset=True)
        sa, sb = _state(a), _state(b)
        for k in ("ill", "amb", "topo", "cd", "scd", "lb", "done"):
            assert np.array_equal(sa[k], sb[k]), (t, k)
        assert np.array_equal(sa["out"], sb["out"], equal_nan=True), t
        assert np.array_equal(a.episode()[2], b.episode()[2]), t
        assert not sa["amb"][0] and not sa["amb"][2], t          # (an entry that is not ambiguous, repeated: not ambiguous)
        now, ep = key(sa["topo"]), a.episode()[2]
        reset = ep > ep_prev
        moved += int(((now != prev).any(1) & ~reset & ~sa["ill"] & ~sa["amb"] & (pick >= 0)).sum())
        resets += int(reset.sum()); resets_of_moved += int((reset & (prev != key0).any(1)).sum())
        prev, ep_prev = now, ep
        print(tag, "step", t, "lanes re-keyed by their action", moved, "auto-resets", resets, "of lanes on another class", resets_of_moved)
    assert moved > 0 and resets > 0 and resets_of_moved > 0
    a.close(); b.close()


def test_one_entry_table_played_in_both_slots():
    """the gathered list holds n_slot times the longest entry: a table of ONE entry played as (0, 0) is the entry itself, not ambiguous"""
    tag = "case14"
    fix = A.load_fixture(tag)
    acts = R.unpack_actions(fix["off"], fix["items"])
    k = _longest(fix, set_only=True)                          # (set_bus / set_line_status: playing it twice is playing it once)
    _, m, a = _area_engine(tag, n_slot=2, table=[acts[k]])
    _, _, b = _area_engine(tag, n_slot=1, table=[acts[k]])
    n = LANES[tag]
    a.set_lane_topo_actions(np.zeros((n, 2), np.int32))
    b.set_lane_topo_actions(np.zeros(n, np.int32))
    for e in (a, b):
        e.step(1, **STEP)
    sa, sb = _state(a), _state(b)
    assert not sa["amb"].any()
    for key in ("ill", "amb", "topo", "cd", "scd", "lb", "done"):
        assert np.array_equal(sa[key], sb[key]), key
    a.close(); b.close()


@pytest.mark.parametrize("tag", TAGS)
def test_mask_bytes_under_areas_equal_playing_every_entry_alone(tag):
    fix, m, eng = _area_engine(tag)
    n, T = LANES[tag], len(fix["played"])
    n_act = len(fix["off"]) - 1
    # the recorded states: the device mask gives the reference's verdicts and the emulator's bytes
    _set_recorded(eng, fix, np.arange(T))
    mask = eng.topo_action_mask_host(0, T)
    A.check_against_reference(fix, mask)
    emu = A.emul(m, fix["off"], fix["items"], fix["sub_area"], fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"])
    assert np.array_equal(mask, emu["mask"])
    assert np.array_equal(eng.topo_action_areas(), emu["areas"])
    # every entry played alone (in a random slot) from two source states with cooldowns and open lines
    rng = np.random.default_rng(5)
    seen = 0
    for s in (T - 1, T // 2):
        for a0 in range(0, n_act, n):
            ent = np.arange(a0, min(a0 + n, n_act))
            src = np.full(n, s)
            _set_recorded(eng, fix, src)
            idx = np.full((n, 3), -1, np.int32)
            idx[np.arange(len(ent)), rng.integers(0, 3, len(ent))] = ent
            eng.set_lane_topo_actions(idx)
            eng.step(1, **STEP)
            ill, amb = eng.topo_action_flags()
            byte = mask[s, ent]
            assert np.array_equal(ill[:len(ent)], (byte & 0x0F) != 0) and np.array_equal(amb[:len(ent)], (byte & 0x10) != 0), (s, a0)
            assert not ill[len(ent):].any() and not amb[len(ent):].any()
            seen |= int(np.bitwise_or.reduce(byte))
    assert seen & 0x10 and seen & 0x0F
    eng.close()


@pytest.mark.parametrize("tag", TAGS)
def test_factorisation_guarantee(tag):
    """entries with pairwise disjoint area sets in the slots: applied exactly when every entry's mask byte is 0"""
    fix, m, eng = _area_engine(tag)
    n, T = LANES[tag], len(fix["played"])
    areas = eng.topo_action_areas()
    n_area = int(fix["sub_area"].max()) + 1
    rng = np.random.default_rng(31)
    n_masked = n_applied = n_draws = 0
    for rep in range(3):
        src = rng.integers(0, T, n)
        _set_recorded(eng, fix, src)
        mask = eng.topo_action_mask_host()
        idx = np.full((n, 3), -1, np.int32)
        for k in range(n):
            while True:
                c = rng.choice(len(areas), size=min(3, n_area), replace=False)
                if all(areas[c] != 0) and all((areas[c[i]] & areas[c[j]]) == 0 for i in range(len(c)) for j in range(i)):
                    break
            idx[k, :len(c)] = c
        eng.set_lane_topo_actions(idx)
        eng.step(1, **STEP)
        ill, amb = eng.topo_action_flags()
        each = np.where(idx >= 0, mask[np.arange(n)[:, None], np.maximum(idx, 0)], 0)
        assert np.array_equal(~ill & ~amb, (each == 0).all(1)), rep
        n_masked += int((each != 0).any(1).sum()); n_applied += int((~ill & ~amb).sum()); n_draws += n
    assert 4 * n_masked >= n_draws and n_applied > 0
    eng.close()


@pytest.mark.parametrize("tag", sorted(R.FIXTURES))
def test_no_areas_and_one_slot_is_the_single_entry_path(tag):
    """an engine brought back to no areas and one slot against an untouched one, on the whole-grid recordings of the legality masks"""
    fix = R.load_fixture(tag)
    n = LANES[tag]
    T = fix["topo_vect"].shape[0]
    m, a = _engine(R.FIXTURES[tag], n)
    _, b = _engine(R.FIXTURES[tag], n)
    acts = R.unpack_actions(fix["off"], fix["items"])
    for e in (a, b):
        e.upload_topo_actions(acts)
        e.set_topo_rules(**RULES)
    b.set_topo_areas(np.arange(m.n_sub) % 2)
    b.set_topo_slots(3)
    b.set_topo_areas(None)
    b.set_topo_slots(1)
    src = np.arange(n) % T
    for e in (a, b):
        e.set_topology(fix["topo_vect"][src]); e.set_cooldown(fix["cooldown_line"][src]); e.set_sub_cooldown(fix["cooldown_sub"][src])
    ma, mb = a.topo_action_mask_host(), b.topo_action_mask_host()
    assert np.array_equal(ma, mb)
    R.check_against_reference(fix, mb[:T])
    rng = np.random.default_rng(3)
    for t in range(1, 4):
        idx = rng.integers(-1, len(acts), size=n).astype(np.int32)
        a.set_lane_topo_actions(idx)
        b.set_lane_topo_actions(idx[:, None])
        for e in (a, b):
            e.step(t, **STEP)
        sa, sb = _state(a), _state(b)
        for k in ("ill", "amb", "topo", "cd", "scd", "lb", "done"):
            assert np.array_equal(sa[k], sb[k]), (t, k)
        assert np.array_equal(sa["out"], sb["out"], equal_nan=True), t
    assert tuple(b.device_views()["act_topo"].shape) == (n, 1)
    a.close(); b.close()


def test_three_slots_written_on_the_device():
    import torch
    tag = "case14"
    fix, m, d = _area_engine(tag)
    _, _, h = _area_engine(tag)
    n, n_act = LANES[tag], len(fix["off"]) - 1
    views = d.device_views()
    assert tuple(views["act_topo"].shape) == (n, 3) and views["act_topo"].dtype == torch.int32
    gen = torch.Generator(device="cuda:0").manual_seed(9)
    for t in range(1, 5):
        with torch.cuda.stream(views["stream"]):
            idx = torch.randint(-1, n_act + 1, (n, 3), generator=gen, device="cuda:0", dtype=torch.int32)       # (+1: outside the table)
            views["act_topo"].copy_(idx)
        d.topo_actions_on_device()
        d.step(t, **STEP)
        hi = idx.cpu().numpy()
        h.set_lane_topo_actions(hi)
        h.step(t, **STEP)
        sd, sh = _state(d), _state(h)
        for k in ("ill", "amb", "topo", "cd", "scd", "lb", "done"):
            assert np.array_equal(sd[k], sh[k]), (t, k)
        assert sd["amb"][(hi >= n_act).any(1)].all()              # an index outside the table in any slot: ambiguous
    d.close(); h.close()
