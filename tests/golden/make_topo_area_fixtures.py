#!/usr/bin/env python
"""Record the reference environment's verdicts under ``RulesByArea`` on single table entries and on composite actions (build container
only, never on a GPU box).

    python tests/golden/make_topo_area_fixtures.py /path/to/reference      # writes tests/golden/topo_area_{case14,wcci118}.npz

The UNMODIFIED reference Environment runs on `OracleHipBackend` (tests/conformance_backend.py) with ``gamerules_class=RulesByArea(areas)``,
MAX_SUB_CHANGED = MAX_LINE_STATUS_CHANGED = 1, NB_TIMESTEP_COOLDOWN_SUB = NB_TIMESTEP_COOLDOWN_LINE = 3 and NO_OVERFLOW_DISCONNECTION (the
line status then changes through the agent alone, which the recorder asserts), over a scripted 30-step episode.  At every step, BEFORE
acting, for every entry of the table and for every composite (two or three entries built as ONE reference action from the merged dict):
``is_ambiguous()[0]`` and the ``(legal, reason)`` of ``rules._lookparam_byarea`` and of ``PreventReconnection`` called separately (reason
bits 0x01 / 0x02 / 0x04 / 0x08 of include/gridpf.h GPF_MASK_*), and whole-grid ``LookParam`` on the composites.  For the composite
played: ``info["is_illegal"]``, ``info["is_ambiguous"]`` and the state after the step.  Written as the few arrays of
tests/topo_area_ref.pack (one verdict byte per question, the rows side by side), read back through its ``unpack`` and compared.  Data
only; tests/test_topo_area_cpu.py and tests/test_gpu_topo_areas.py read it through ``topo_area_ref.load_fixture``."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
N_STEPS = 30
N_SLOT = 3
PARAMS = dict(MAX_SUB_CHANGED=1, MAX_LINE_STATUS_CHANGED=1, NB_TIMESTEP_COOLDOWN_SUB=3, NB_TIMESTEP_COOLDOWN_LINE=3)
# output tag -> (environment, seed, first substation of every area)
GRIDS = {"case14": ("l2rpn_case14_sandbox", 3, (0, 7)), "wcci118": ("l2rpn_wcci_2022_dev", 5, (0, 40, 80))}
BIT_OF_MESSAGE = (("line status affected by the action in one area", 0x01), ("substation affected by the action in one area", 0x02),
                  ("line status affected", 0x01), ("substation affected", 0x02), ("Powerline with ids", 0x04), ("Substation with ids", 0x08))


def verdict(call, action, env):
    legal, reason = call(action, env)
    if legal:
        return True, 0
    bits = [b for msg, b in BIT_OF_MESSAGE if msg in str(reason)]
    assert bits, str(reason)
    return False, bits[0]


def merged(table, comp):
    """ONE action dict from the entries of a composite, in slot order (a later set_bus of a position replaces an earlier one)"""
    out = {}
    for a in comp:
        if a < 0:
            continue
        act = table[a]
        out.setdefault("set_line_status", []).extend(act.get("set_line_status", ()))
        out.setdefault("change_line_status", []).extend(act.get("change_line_status", ()))
        out.setdefault("set_bus", {}).update(act.get("set_bus", {}))
        out.setdefault("change_bus", []).extend(act.get("change_bus", ()))
    return out


def build_table_and_composites(model, sub_area, rng):
    """the table of make_topo_mask_fixtures.build_table + per-area line actions + tie-line entries; about 40 composites: one entry per
    area, pairs in the same area, tie lines with a line of either side, conflicts across entries, triples"""
    from make_topo_mask_fixtures import build_table
    from topo_rules_ref import topo_pos_sub
    table = build_table(model, rng)
    ps = topo_pos_sub(model)
    lo, le = np.asarray(model.line_or_pos_topo_vect), np.asarray(model.line_ex_pos_topo_vect)
    a_or, a_ex = sub_area[ps[lo]], sub_area[ps[le]]
    n_area = int(sub_area.max()) + 1
    inner = [[int(l) for l in np.flatnonzero((a_or == k) & (a_ex == k))] for k in range(n_area)]
    ties = [int(l) for l in np.flatnonzero(a_or != a_ex)]
    assert ties and all(len(x) >= 2 for x in inner)
    line_off, line_chg, sub_act = {}, {}, {}
    for k in range(n_area):                                 # two line entries and one substation entry per area
        for l in rng.choice(inner[k], size=2, replace=False):
            line_off[(k, int(l))] = len(table); table.append({"set_line_status": [(int(l), -1)]})
            line_chg[(k, int(l))] = len(table); table.append({"change_line_status": [int(l)]})
        subs = [s for s in np.flatnonzero(sub_area == k) if (ps == s).sum() >= 4]
        s = int(rng.choice(subs))
        pos = np.flatnonzero(ps == s)
        sub_act[k] = len(table); table.append({"set_bus": {int(pos[0]): 2, int(pos[1]): 2}})
    tie_ent = []
    for l in rng.choice(ties, size=min(3, len(ties)), replace=False):
        l = int(l)
        tie_ent.append((l, len(table))); table.append({"set_line_status": [(l, -1)]})
        tie_ent.append((l, len(table))); table.append({"set_bus": {int(le[l]): 2}})
    comps = []
    by_area = lambda d, k: [v for (kk, _), v in d.items() if kk == k]  # noqa: E731
    for k in range(n_area):
        k2 = (k + 1) % n_area
        comps.append((by_area(line_off, k)[0], by_area(line_off, k2)[0]))            # one line per area
        comps.append((by_area(line_chg, k)[1], by_area(line_off, k2)[1]))
        comps.append((sub_act[k], sub_act[k2]))                                     # one substation per area
        comps.append((sub_act[k], by_area(line_off, k2)[0]))
        comps.append((by_area(line_off, k)[0], by_area(line_off, k)[1]))             # two lines of one area
        comps.append((by_area(line_off, k)[0], by_area(line_chg, k)[1]))
        comps.append((sub_act[k], by_area(line_off, k)[0]))                          # a substation and a line of one area: legal
    for l, ent in tie_ent:                                  # a tie line counts in the area of its ORIGIN substation
        comps.append((ent, by_area(line_off, int(a_ex[l]))[0]))
        comps.append((ent, by_area(line_off, int(a_or[l]))[0]))
        comps.append((ent, sub_act[int(a_ex[l])]))
    comps.append((tie_ent[0][1], tie_ent[1][1]))             # a line disconnected in one entry, its end assigned in the other: ambiguous
    l0 = next(l for (k, l) in line_off if k == 0)
    comps.append((line_off[(0, l0)], line_chg[(0, l0)]))       # set and change of one line status across entries: ambiguous
    n_base = len(comps)
    while len(comps) < n_base + 8:                            # seeded random pairs / triples of the whole table
        comps.append(tuple(int(x) for x in rng.choice(len(table), size=int(rng.integers(2, N_SLOT + 1)), replace=False)))
    if n_area >= 3:
        comps.append((by_area(line_off, 0)[0], by_area(line_off, 1)[0], by_area(line_off, 2)[0]))
        comps.append((sub_act[0], sub_act[1], sub_act[2]))
        comps.append((sub_act[0], by_area(line_off, 1)[0], by_area(line_off, 1)[1]))
    comps.append((-1, by_area(line_off, 0)[0], -1))         # empty slots around one entry
    arr = np.full((len(comps), N_SLOT), -1, np.int32)
    for i, c in enumerate(comps):
        arr[i, :len(c)] = c
    return table, arr


def record(tag, env_name, seed, starts, out_dir):
    import grid2op
    from grid2op.Parameters import Parameters
    from grid2op.Rules import LookParam, PreventReconnection
    from grid2op.Rules.rulesByArea import RulesByArea
    from conformance_backend import OracleHipBackend
    from grid2op_amd.grid_model import GridModel
    from make_topo_mask_fixtures import to_reference
    from topo_area_ref import pack, unpack
    from topo_rules_ref import pack_actions

    model = GridModel.load_npz(os.path.join(HERE, env_name + ".grid.npz"))
    bounds = list(starts) + [model.n_sub]
    areas = [list(range(bounds[k], bounds[k + 1])) for k in range(len(starts))]
    sub_area = np.zeros(model.n_sub, np.int32)
    for k, subs in enumerate(areas):
        sub_area[subs] = k
    p = Parameters()
    for k, v in PARAMS.items():
        setattr(p, k, v)
    p.NO_OVERFLOW_DISCONNECTION = True
    env = grid2op.make(env_name, test=True, backend=OracleHipBackend(), param=p, gamerules_class=RulesByArea(areas))
    cls = type(env)
    rules = env._game_rules.legal_action
    assert isinstance(rules, RulesByArea)
    assert np.array_equal(cls.line_or_pos_topo_vect, model.line_or_pos_topo_vect) and np.array_equal(cls.line_ex_pos_topo_vect, model.line_ex_pos_topo_vect)
    rng = np.random.default_rng(seed)
    table, comps = build_table_and_composites(model, sub_area, rng)
    off, items = pack_actions(table)
    order = rng.permutation(len(comps))
    look, prev = LookParam(), PreventReconnection()
    env.seed(seed)
    obs = env.reset()
    keys = ("topo_vect", "cooldown_line", "cooldown_sub", "last_bus", "ambiguous", "area_legal", "area_bit", "prevent_legal", "prevent_bit",
            "comp_ambiguous", "comp_area_legal", "comp_area_bit", "comp_prevent_legal", "comp_prevent_bit", "comp_look_legal", "played",
            "is_illegal", "is_ambiguous", "done", "topo_after", "cooldown_line_after", "cooldown_sub_after", "last_bus_after")
    rec = {k: [] for k in keys}
    mk = lambda a: to_reference(env.action_space, a, cls.dim_topo)  # noqa: E731
    state = lambda: (np.asarray(obs.topo_vect, np.int32).copy(), np.asarray(obs.time_before_cooldown_line, np.int32).copy(),  # noqa: E731
                     np.asarray(obs.time_before_cooldown_sub, np.int32).copy(),
                     np.asarray(env._backend_action.last_topo_registered.values, np.int32).copy())
    for t in range(N_STEPS):
        assert np.array_equal(env.get_current_line_status(), (obs.topo_vect[cls.line_or_pos_topo_vect] > 0) & (obs.topo_vect[cls.line_ex_pos_topo_vect] > 0))
        for k, v in zip(("topo_vect", "cooldown_line", "cooldown_sub", "last_bus"), state()):
            rec[k].append(v)
        # fresh action objects for every question: is_ambiguous() caches "checked" on the object
        rec["ambiguous"].append([bool(mk(a).is_ambiguous()[0]) for a in table])
        av = [verdict(rules._lookparam_byarea, mk(a), env) for a in table]
        pv = [verdict(prev, mk(a), env) for a in table]
        rec["area_legal"].append([v[0] for v in av]); rec["area_bit"].append([v[1] for v in av])
        rec["prevent_legal"].append([v[0] for v in pv]); rec["prevent_bit"].append([v[1] for v in pv])
        cd = [merged(table, c) for c in comps]
        rec["comp_ambiguous"].append([bool(mk(a).is_ambiguous()[0]) for a in cd])
        av = [verdict(rules._lookparam_byarea, mk(a), env) for a in cd]
        pv = [verdict(prev, mk(a), env) for a in cd]
        rec["comp_area_legal"].append([v[0] for v in av]); rec["comp_area_bit"].append([v[1] for v in av])
        rec["comp_prevent_legal"].append([v[0] for v in pv]); rec["comp_prevent_bit"].append([v[1] for v in pv])
        rec["comp_look_legal"].append([verdict(look, mk(a), env)[0] for a in cd])
        k = int(order[t % len(comps)])
        rec["played"].append(k)
        before = env.get_current_line_status().copy()
        act = mk(cd[k])
        obs, _, done, info = env.step(act)
        rec["is_illegal"].append(bool(info["is_illegal"])); rec["is_ambiguous"].append(bool(info["is_ambiguous"])); rec["done"].append(bool(done))
        if not done:                                        # the line status changes through the agent alone
            named = np.zeros(cls.n_line, bool)
            d = cd[k]
            named[[l for l, _ in d.get("set_line_status", ())] + list(d.get("change_line_status", ()))] = True
            for pos in list(d.get("set_bus", {})) + list(d.get("change_bus", ())):
                named |= (cls.line_or_pos_topo_vect == pos) | (cls.line_ex_pos_topo_vect == pos)
            after = (obs.topo_vect[cls.line_or_pos_topo_vect] > 0) & (obs.topo_vect[cls.line_ex_pos_topo_vect] > 0)
            assert not ((before != after) & ~named).any(), "a line changed its status by itself"
        for k2, v in zip(("topo_after", "cooldown_line_after", "cooldown_sub_after", "last_bus_after"), state()):
            rec[k2].append(v)
        if done:
            obs = env.reset()
    env.close()
    out = {"off": off, "items": items, "comps": comps, "sub_area": sub_area, "grid": np.array(env_name),
           "params": np.array([PARAMS["MAX_SUB_CHANGED"], PARAMS["MAX_LINE_STATUS_CHANGED"], PARAMS["NB_TIMESTEP_COOLDOWN_SUB"],
                               PARAMS["NB_TIMESTEP_COOLDOWN_LINE"]], np.int32)}
    for k, v in rec.items():
        v = np.asarray(v)
        small = k.endswith("_bit") or k.split("_after")[0] in ("topo_vect", "topo", "cooldown_line", "cooldown_sub", "last_bus")
        assert not small or (np.abs(v) < 128).all()
        out[k] = v if v.dtype == bool else v.astype(np.int8 if small else np.int32)       # (busbars, cooldowns, reason bits: one byte each)
    path = os.path.join(out_dir, f"topo_area_{tag}.npz")
    np.savez_compressed(path, **pack(out))
    back = unpack(dict(np.load(path)))
    assert sorted(back) == sorted(out) and all(np.array_equal(back[k], out[k]) and back[k].dtype == out[k].dtype for k in out)
    # the condition on the fixture: the per-area rules differ from the whole-grid ones, in both directions, on the recorded composites
    n_all = out["comp_area_legal"].size
    n_free = int((out["comp_area_legal"] & ~out["comp_look_legal"]).sum())
    n_ill = int((~out["comp_area_legal"]).sum())
    print(f"{tag}: {len(table)} entries, {len(comps)} composites x {N_STEPS} steps; composite verdicts: {n_all}, legal by area but illegal "
          f"whole-grid {n_free}, illegal by area {n_ill}, ambiguous {int(out['comp_ambiguous'].sum())}; played: illegal "
          f"{int(out['is_illegal'].sum())}, ambiguous {int(out['is_ambiguous'].sum())}, done {int(out['done'].sum())}; {os.path.getsize(path)} bytes")
    assert 10 * n_free >= n_all and 10 * n_ill >= n_all


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    reference = os.path.abspath(sys.argv[1])
    for q in (ROOT, os.path.join(ROOT, "tests"), HERE, reference, os.path.join(ROOT, "tests", "_refshim")):
        if q not in sys.path:
            sys.path.insert(0, q)
    os.environ.setdefault("_GRID2OP_FORCE_TEST", "1")
    warnings.filterwarnings("ignore")
    for tag, (env_name, seed, starts) in GRIDS.items():
        if len(sys.argv) > 2 and tag not in sys.argv[2:]:
            continue
        record(tag, env_name, seed, starts, HERE)


if __name__ == "__main__":
    main()
