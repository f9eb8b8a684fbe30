"""Combined topology + injection actions (include/gridpf.h gpf_set_combined_actions) without a GPU: the recordings of the unmodified
reference environment (tests/golden/combined_*.npz, made by tests/golden/make_combined_fixtures.py), the restatement
(tests/combined_ref.py on tests/topo_rules_ref.py and the dynamics oracle) and the library's rule core compiled with g++
(tests/native/combined_emul.cpp) held together -- flags, topology rows and cooldowns exactly, dispatch targets and charge within the
1e-4 MW / MWh of tests/test_gpu_envdyn.py --, the per-entry storage words against the table, and for every coverage case of the
recordings the state a path WITHOUT the coupling would have left, which must differ from the recorded one."""
import subprocess

import numpy as np
import pytest

import combined_ref as CR
from conftest import golden_path
from test_oracle_envdyn import dyn_from_fixture
from topo_rules_ref import SET_BUS, TopoRules

TAGS = ("case14_storage", "wcci118")
_cache = {}


def _fixture(tag):
    if tag not in _cache:
        from grid2op_amd.grid_model import GridModel
        fx = dict(np.load(golden_path(f"combined_{tag}.npz")))
        m = GridModel.load_npz(golden_path(f"{fx['grid']}.grid.npz"))
        p = [int(x) for x in fx["params"]]
        rules = TopoRules(m, fx["off"], fx["items"].reshape(-1, 3), legal_rules=True, max_sub=p[0], max_line=p[1], cd_sub=p[2], cd_line=p[3])
        lim = CR.Limits(fx["ramp_up"], fx["ramp_down"], fx["redispatchable"], fx["renewable"], fx["storage_max_p_prod"], fx["storage_max_p_absorb"],
                        m.storage_pos_topo_vect)
        _cache[tag] = (fx, m, rules, CR.CombinedLane(rules, lim), lim)
    return _cache[tag]


def test_the_rule_core_under_sanitizers():
    """tests/native/combined_emul.cpp as a stand-alone program with its own main, built with the address and undefined-behaviour sanitizers"""
    r = subprocess.run([CR.sanitized_program()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("tag", TAGS)
def test_storage_words_of_the_table(tag):
    fx, m, rules, lane, lim = _fixture(tag)
    words = CR.entry_words(fx["off"], fx["items"], m.storage_pos_topo_vect)
    assert np.array_equal(words, CR.emul_words(fx["off"], fx["items"], m.storage_pos_topo_vect))
    pos = {int(p): k for k, p in enumerate(m.storage_pos_topo_vect)}
    items = fx["items"].reshape(-1, 3)
    hit = 0
    for a in range(len(fx["off"]) - 1):
        bits = {pos[int(i)] for kind, i, v in items[fx["off"][a]:fx["off"][a + 1]] if int(i) in pos and kind in (SET_BUS, 2) and (kind == 2 or v > 0)}
        assert int(words[a]) == sum(1 << k for k in bits), a
        hit += bool(bits)
    p0 = int(m.storage_pos_topo_vect[0])
    single = {int(items[fx["off"][a]][2]): a for a in range(len(fx["off"]) - 1)
              if fx["off"][a + 1] - fx["off"][a] == 1 and tuple(items[fx["off"][a]][:2]) == (SET_BUS, p0)}
    assert hit >= 1 and words[single[1]] == 1 and words[single[-1]] == 0       # the entry that reconnects unit 0; the one that disconnects it has no bit


def test_emulator_equals_restatement_on_seeded_rows():
    """the screen, the cancel and the merge on rows drawn at and around every threshold, 1 / 6 / 62 / 64 generators, 0 / 2 / 7 / 64 storage units"""
    rng = np.random.default_rng(17)
    reasons = set()
    for n_gen, n_sto in ((1, 0), (6, 2), (62, 7), (64, 64)):
        ru, rd = rng.uniform(1, 20, n_gen).astype(np.float32).astype(np.float64), rng.uniform(1, 20, n_gen).astype(np.float32).astype(np.float64)
        can, ren = rng.random(n_gen) < 0.6, rng.random(n_gen) < 0.4
        mp, ma = rng.uniform(1, 10, n_sto).astype(np.float32), rng.uniform(1, 10, n_sto).astype(np.float32)
        pos = np.arange(n_sto) + n_gen
        lim = CR.Limits(ru, rd, can, ren, mp if n_sto else None, ma if n_sto else None, pos)
        tab_amb = np.array([0, 0, 1], np.uint8)
        tab_word = np.array([0, (1 << n_sto) - 1 if n_sto else 0, 0], np.uint64)
        for trial in range(300):
            red = np.where(can, rng.uniform(-1, 1, n_gen) * np.where(rng.random(n_gen) < 0.5, ru, rd), 0).astype(np.float32)
            sto = (rng.uniform(-1, 1, n_sto) * np.minimum(mp, ma)).astype(np.float32) if n_sto else np.zeros(0, np.float32)
            cur = np.where(ren & (rng.random(n_gen) < 0.3), rng.uniform(0, 1, n_gen), -1).astype(np.float32)
            row = np.ones(n_gen + n_sto, np.int32)
            kind = trial % 10
            g = int(rng.integers(n_gen))
            if kind == 1:
                red[g] = np.nextafter(np.float32(ru[g]), np.float32(np.inf)) if can[g] else np.float32(1e-6)
            elif kind == 2:
                red[g] = -np.nextafter(np.float32(rd[g]), np.float32(np.inf)) if can[g] else np.float32(-1e-7)
            elif kind == 3 and n_sto:
                u = int(rng.integers(n_sto))
                sto[u] = np.nextafter(ma[u], np.float32(np.inf)) if trial % 20 < 10 else -np.nextafter(mp[u], np.float32(np.inf))
            elif kind == 4:
                cur[g] = rng.choice([1.0000001, -1e-3, 0.5, np.float32(-1) + np.float32(1e-6)])
            elif kind == 5 and n_sto:
                row[pos[int(rng.integers(n_sto))]] = -1
            elif kind == 6 and n_sto:
                row[pos] = -1
                sto[int(rng.integers(n_sto))] = np.nan
            slot = int(rng.choice([-1, 0, 1, 2, 7, -5]))
            parts = [red if trial % 7 else None, sto if n_sto and trial % 5 else None, cur if trial % 3 else None]
            for check, rules_on in ((1, 1), (0, 1), (1, 0)):
                touched = int(tab_word[slot]) if 0 <= slot < 3 else 0
                want = CR.screen(lim, *parts, row, touched, bool(check), bool(rules_on))
                got, slots = CR.emul_pre(lim, ru, rd, *parts, row, [slot], tab_amb, tab_word, check, rules_on)
                assert got == want, (n_gen, n_sto, trial, check, rules_on, got, want)
                static_amb = slot < -1 or slot >= 3 or slot == 2
                assert slots[0] == (-1 if (want[0] or want[1]) and not static_amb else slot)
                reasons.add(want[2])
                for t_ill, t_amb in ((0, 0), (1, 0), (0, 1)):
                    void = t_ill or t_amb or want[0] or want[1]
                    r_, s_, c_ = CR.emul_cancel(n_gen, n_sto, (t_ill, t_amb), want, *parts)
                    for x, y, fill in ((parts[0], r_, 0.0), (parts[1], s_, 0.0), (parts[2], c_, -1.0)):
                        assert (x is None) == (y is None) and (x is None or np.array_equal(y, np.full_like(x, fill) if void else x, equal_nan=True))
                    for ir in (0, 1):
                        assert np.array_equal(CR.emul_merge(t_ill, t_amb, want, ir), CR.merge(t_ill, t_amb, want, ir))
    assert reasons >= set(CR.VALUE_RULES) | {CR.NONE, CR.DISCO_STORAGE}


@pytest.mark.parametrize("tag", TAGS)
def test_recording_restatement_and_emulator(tag):
    fx, m, rules, lane, lim = _fixture(tag)
    names = [str(c) for c in fx["cases"]]
    n = len(fx["done"])
    seen = {c: 0 for c in names}
    differs = {c: 0 for c in names}
    topo = line_cd = sub_cd = last = dyn = None
    for i in range(n):
        if fx["is_reset"][i]:
            topo = fx["topo_vect"][i].astype(np.int64)
            line_cd, sub_cd, last = np.zeros(m.n_line, np.int64), np.zeros(m.n_sub, np.int64), np.maximum(topo, 1)
            dyn = dyn_from_fixture(fx)
            dyn.prev_p[:] = fx["ch_prod_p"][fx["row"][i]]
            continue
        a, red, sto, cur = int(fx["played"][i]), fx["act_redisp"][i], fx["act_storage"][i], fx["act_curtail"][i]
        pre = lane.pre(topo, line_cd, sub_cd, last, a, red, sto, cur)
        # the emulator: the same verdict, the same slot, the same surviving rows
        got, slots = CR.emul_pre(lim, fx["ramp_up"], fx["ramp_down"], red, sto, cur, topo, [a], rules.ambiguous, lane.words, 1, 1)
        assert got == pre["screen"] and slots[0] == pre["played"], (tag, i)
        surv = CR.emul_cancel(m.n_gen, m.n_storage, pre["topo_flags"], pre["screen"], red, sto, cur)
        assert all(np.array_equal(x, pre[k]) for x, k in zip(surv, ("redisp", "storage", "curtail"))), (tag, i)
        ghost = _copy_dyn(dyn)
        ok, _, _ = dyn.step(fx["ch_prod_p"][fx["row"][i]], pre["redisp"], pre["storage"], pre["curtail"])
        done = not ok
        cd_step = np.maximum(line_cd - 1, 0)                                        # (no trips, no outages in these recordings)
        line_after, sub_after, last_after, flags = lane.post(pre, pre["row"], cd_step, sub_cd, last, done, dyn.illegal)
        assert np.array_equal(flags, CR.emul_merge(*pre["topo_flags"], pre["screen"], dyn.illegal)), (tag, i)
        # the recording
        assert done == bool(fx["done"][i]), (tag, i)
        assert (bool(flags[0]), bool(flags[1])) == (bool(fx["is_illegal"][i]), bool(fx["is_ambiguous"][i])), (tag, i, flags)
        assert not fx["is_illegal_reco"][i]
        c = names[fx["case"][i]] if fx["case"][i] >= 0 else None
        if done:
            assert fx["failed_redisp"][i] and c == "game_over"
            seen[c] += 1
            differs[c] += int((pre["row"] != topo).any())                           # the step carried an applied topology action
            continue
        assert bool(flags[2]) == bool(fx["failed_redisp"][i]), (tag, i)
        assert np.array_equal(pre["row"], fx["topo_vect"][i]), (tag, i, c)
        assert np.array_equal(line_after, fx["cooldown_line"][i]) and np.array_equal(sub_after, fx["cooldown_sub"][i]), (tag, i, c)
        assert np.abs(dyn.target - fx["target_dispatch"][i]).max() < 1e-4 and np.abs(dyn.charge - fx["storage_charge"][i]).max() < 1e-4, (tag, i, c)
        assert np.abs(dyn.limit - fx["limit_curtailment"][i]).max() < 1e-6, (tag, i, c)
        if c is not None:
            # what a path that ignored the coupling would have left: it must not be the recorded state
            seen[c] += 1
            loose_row, l_ill, l_amb, l_al, l_as = rules.pre(topo, line_cd, sub_cd, last, a)
            ghost.step(fx["ch_prod_p"][fx["row"][i]], red, sto, cur)
            inj_differs = np.abs(ghost.target - fx["target_dispatch"][i]).max() > 1e-3 or np.abs(ghost.charge - fx["storage_charge"][i]).max() > 1e-3
            if c in ("reconnection", "look_param", "topo_ambiguous"):                # (a): the injection part applied all the same
                differs[c] += int(inj_differs)
            elif c in CR_VALUE_CASES or c == "disco_storage":                        # (b): the topology part applied all the same
                differs[c] += int((loose_row != fx["topo_vect"][i]).any())
            elif c == "disco_reconnects":                                            # without the entry's word the storage rule fires
                differs[c] += int(CR.screen(lim, red, sto, cur, topo, 0)[1] and not pre["screen"][1])
            elif c == "illegal_redisp":                                              # (c): the action's cooldowns booked all the same
                l2, s2, _ = rules.post(pre["row"], cd_step, sub_cd, last, pre["aff_lines"], pre["aff_subs"])
                differs[c] += int(not np.array_equal(l2, fx["cooldown_line"][i]) or not np.array_equal(s2, fx["cooldown_sub"][i]))
                assert (pre["row"] != topo).any()                                    # ... and the topology IS applied
            elif c == "both_legal":
                differs[c] += int((pre["row"] != topo).any() and np.abs(dyn.target).max() > 0)
        topo, line_cd, sub_cd, last = pre["row"], line_after, sub_after, last_after
    assert all(seen[c] >= 2 and differs[c] >= 2 for c in names), (seen, differs)


CR_VALUE_CASES = ("fixed_gen", "ramp_up", "ramp_down", "storage_power", "curtail_range", "curtail_fixed")


def _copy_dyn(dyn):
    import copy
    return copy.deepcopy(dyn)
