"""Legality masks of the topology action table (include/gridpf.h: gpf_topo_action_mask), the parts that need no GPU: the library's rule
core and summary builder (grid2op_amd/csrc/gridpf_topo_mask.hpp), compiled with g++ into a host emulator, give the verdicts the reference
environment recorded (tests/golden/topo_mask_*.npz); so does the Python restatement; the fixture is not degenerate; ShardedEngine routes
the two calls; the public surface is declared."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_path
from grid2op_amd.grid_model import GridModel
from grid2op_amd.sharding import ShardedEngine
from stub_engine import StubEngine
from topo_rules_ref import pack_actions, random_topo_table
import topo_mask_ref as R


@pytest.fixture(scope="module", params=sorted(R.FIXTURES))
def recorded(request, load_model):
    fix = R.load_fixture(request.param)
    assert str(fix["grid"]) == R.FIXTURES[request.param]
    return load_model(R.FIXTURES[request.param]), fix


def test_emulator_gives_the_reference_verdicts(recorded):
    m, fix = recorded
    max_sub, max_line = int(fix["params"][0]), int(fix["params"][1])
    mask, amb = R.emul_mask(m, fix["off"], fix["items"], fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], True, max_sub, max_line)
    R.check_against_reference(fix, mask)
    assert np.array_equal(amb, fix["ambiguous"][0])
    # AlwaysLegal: the ambiguous bit alone; a line-cooldown buffer that does not exist reads as zeros
    free, _ = R.emul_mask(m, fix["off"], fix["items"], fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], False, max_sub, max_line)
    assert np.array_equal(free, np.where(fix["ambiguous"], R.AMBIGUOUS, 0))
    nocd, _ = R.emul_mask(m, fix["off"], fix["items"], fix["topo_vect"], None, fix["cooldown_sub"], True, max_sub, max_line)
    zero, _ = R.emul_mask(m, fix["off"], fix["items"], fix["topo_vect"], 0 * fix["cooldown_line"], fix["cooldown_sub"], True, max_sub, max_line)
    assert np.array_equal(nocd, zero) and not (nocd & R.LINE_COOLDOWN).any()


def test_restatement_gives_the_reference_verdicts_and_the_emulators_bytes(recorded):
    m, fix = recorded
    rules = R.MaskRules(m, fix["off"], fix["items"], True, int(fix["params"][0]), int(fix["params"][1]), int(fix["params"][2]), int(fix["params"][3]))
    assert np.array_equal(rules.ambiguous, fix["ambiguous"][0])
    mask = rules.masks(fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"])
    R.check_against_reference(fix, mask)
    emu, _ = R.emul_mask(m, fix["off"], fix["items"], fix["topo_vect"], fix["cooldown_line"], fix["cooldown_sub"], True, int(fix["params"][0]),
                         int(fix["params"][1]))
    assert np.array_equal(mask, emu)


def test_fixture_covers_every_reason_and_has_legal_entries_at_every_step(recorded):
    _, fix = recorded
    assert list(fix["params"]) == [1, 1, 3, 3]
    n_steps, n_act = fix["ambiguous"].shape
    assert n_steps >= 25 and n_act >= 35 and fix["topo_vect"].shape[0] == n_steps
    seen = fix["look_bit"] | fix["prevent_bit"]
    for bit in (R.TOO_MANY_LINES, R.TOO_MANY_SUBS, R.LINE_COOLDOWN, R.SUB_COOLDOWN):
        assert (seen == bit).any(), bit
    assert fix["ambiguous"].any() and (fix["ambiguous"] == fix["ambiguous"][0]).all()
    legal = ~fix["ambiguous"] & fix["look_legal"] & fix["prevent_legal"]
    assert legal.any(axis=1).all()
    assert np.array_equal(fix["look_bit"] != 0, ~fix["look_legal"]) and np.array_equal(fix["prevent_bit"] != 0, ~fix["prevent_legal"])
    assert (fix["cooldown_line"] > 0).any() and (fix["cooldown_sub"] > 0).any() and (fix["topo_vect"] < 0).any()      # the states are not all alike


def test_emulator_on_a_random_table_equals_the_restatement(load_model):
    """a larger table (repeated past 64 and 256 entries) on states with many cooldowns and open lines, the two limits unequal too: bytes equal"""
    m = load_model("l2rpn_wcci_2022_dev")
    rng = np.random.default_rng(5)
    acts = random_topo_table(m, rng)
    acts = (acts * 10)[:300]
    off, items = pack_actions(acts)
    n = 6
    topo = np.tile(m.initial_topo_vect(), (n, 1)).astype(np.int32)
    lo, le = np.asarray(m.line_or_pos_topo_vect), np.asarray(m.line_ex_pos_topo_vect)
    for k in range(n):
        for l in rng.choice(m.n_line, size=12, replace=False):
            topo[k, lo[l]] = topo[k, le[l]] = -1
    lcd = (rng.random((n, m.n_line)) < 0.2) * rng.integers(1, 4, (n, m.n_line))
    scd = (rng.random((n, m.n_sub)) < 0.2) * rng.integers(1, 4, (n, m.n_sub))
    for max_sub, max_line in ((1, 1), (2, 1), (1, 2), (0, 0)):
        emu, amb = R.emul_mask(m, off, items, topo, lcd, scd, True, max_sub, max_line)
        rules = R.MaskRules(m, off, items, True, max_sub, max_line, 3, 3)
        assert np.array_equal(amb, rules.ambiguous)
        assert np.array_equal(emu, rules.masks(topo, lcd, scd))
    assert len(set(np.unique(emu))) > 4


def test_sanitized_stand_alone_emulator_runs_clean():
    """the emulator file with its own main under the address and undefined-behaviour sanitizers (a plain program: the summary builder and the
    rule core on random tables of a grid with more than 64 lines and substations, against a dense evaluation)"""
    p = subprocess.run([R.sanitized_program()], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert " 0 mismatches" in p.stdout


class _MaskStub(StubEngine):
    N_ACT = 7

    def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
        super().__init__(model, n_lanes, device, n_busbar)
        self.mask_calls = []

    def topo_action_mask(self, lane0=0, n=None, out=None):
        n = self.n_lanes - lane0 if n is None else n
        self.mask_calls.append((lane0, n, out))
        return np.full((n, self.N_ACT), self.device, np.uint8) if out is None else out

    def topo_action_mask_host(self, lane0=0, n=None):
        n = self.n_lanes - lane0 if n is None else n
        return np.full((n, self.N_ACT), self.device, np.uint8) + (np.arange(lane0, lane0 + n, dtype=np.uint8) * 16)[:, None]


def test_sharded_engine_routes_the_mask_calls_by_lane_range():
    m = GridModel.load_npz(golden_path("l2rpn_case14_sandbox.grid.npz"))
    se = ShardedEngine(m, 37, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: _MaskStub(mm, n, dev, nbb))
    parts = se.topo_action_mask()
    assert [p.shape for p in parts] == [(bn, 7) for _, bn in se.blocks] and [int(p[0, 0]) for p in parts] == [0, 1, 2]
    b1 = se.blocks[1][0]
    parts = se.topo_action_mask(b1 - 2, 5)                        # crosses the first block boundary
    assert [p.shape[0] for p in parts] == [2, 3]
    assert se.engines[0].mask_calls[-1][:2] == (b1 - 2, 2) and se.engines[1].mask_calls[-1][:2] == (0, 3) and len(se.engines[2].mask_calls) == 1
    outs = ["a", "b"]
    assert se.topo_action_mask(b1 - 2, 5, out=outs) == outs and se.engines[1].mask_calls[-1][2] == "b"
    with pytest.raises(ValueError, match="2 shards intersect"):
        se.topo_action_mask(b1 - 2, 5, out=["a"])
    host = se.topo_action_mask_host(b1 - 2, 5)
    assert host.shape == (5, 7) and list(host[:, 0] & 0x0F) == [0, 0, 1, 1, 1]
    assert list(host[:, 0] >> 4) == [(b1 - 2) % 16, (b1 - 1) % 16, 0, 1, 2]       # local lane numbers of each shard
    assert se.topo_action_mask_host().shape == (37, 7)


def test_public_surface_is_declared():
    from grid2op_amd import _capi, engine
    hdr = open(os.path.join(ROOT, "include", "gridpf.h")).read()
    assert "#define GPF_ABI_VERSION 326" in hdr and "#define GPF_N_DEVICE_POINTERS 34" in hdr
    assert _capi.ABI_VERSION == 326 and _capi.N_DEVICE_POINTERS == 34
    assert re.search(r"int gpf_topo_action_mask\(gpf_handle h, int32_t lane0, int32_t n, uint8_t\* out_dev, int64_t row_stride\);", hdr)
    assert re.search(r"int gpf_get_topo_action_mask\(gpf_handle h, int32_t lane0, int32_t n, uint8_t\* host_out\);", hdr)
    for name in ("gpf_topo_action_mask", "gpf_get_topo_action_mask"):
        assert name in _capi.EXPORTED_SYMBOLS
    for name, bit in (("TOO_MANY_LINES", 0x01), ("TOO_MANY_SUBS", 0x02), ("LINE_COOLDOWN", 0x04), ("SUB_COOLDOWN", 0x08), ("AMBIGUOUS", 0x10)):
        assert re.search(r"#define GPF_MASK_%s 0x%02x\b" % (name, bit), hdr)
        assert getattr(engine, "MASK_" + name) == bit == getattr(R, name)
    for cite in ("Rules/LookParam.py:28-53", "Rules/PreventReconnection.py:23-60", "Action/baseAction.py:1782-2020"):
        assert cite in hdr[hdr.index("legality masks of the action table"):hdr.index("int gpf_topo_action_mask(")]
    core = open(os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_topo_mask.hpp")).read()
    assert len(re.findall(r"inline unsigned topo_mask_eval\(", core)) == 1 and core.count("topo_mask_eval(") == 2      # defined once, called by the kernel
