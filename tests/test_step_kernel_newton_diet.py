"""Fewer instructions per Newton iteration in the instance-group step kernel (gridpf_sparse.hpp: FlatWords, LATE_J): the lane's item
ADDRESSES of the flat LU program are resident in registers, so no pass decodes a word; "this lane has an item in pass k" and "the
destination is a matrix block" are read off the destination address where they are used instead of being reloaded from spilled lane
masks; and the Jacobian blocks are only written for an evaluation that is factorised.

CPU checks on the ISA of the headline feature variant (14 substations, two instances per wavefront), compiled once per session with the
command line and the helpers of tests/test_step_kernel_features.py, against constants measured on the parent commit with the counters of
this file.

WHAT IS COUNTED.  `newton_loop_lines` (tests/test_step_kernel_words_resident.py) takes the blocks the compiler ANNOTATES as belonging to
the loop around the back-edge marker.  In the parent's layout the pair phase is entered from the loop's last block by a branch to a
block in front of the annotated header, which the compiler annotates with the step loop only: that set misses about 60 instructions the
parent executes in every iteration, and it contains them in this tree, where the loop has one entry.  `newton_cycle_lines` below follows
the branches instead: every block laid out behind the entry marker that lies on a path from the back-edge marker's block to itself.
The annotated set is printed beside it.

REACHED.  The iteration went from 760 to 696 instructions, 64 fewer (on the annotated blocks 704 -> 696, although that set gained the pair
phase).  Gone are the 22 address decodes (v_add_u32_sdwa 22 -> 0) and the 22 reloads of the eleven per-pass lane masks (v_readlane +
v_writelane 40 -> 18); the verdict of the mismatch phase is two group reductions on the mismatch itself and mask arithmetic, without a
branch per test; the fill blocks are zeroed by one predicated store where their count is a literal no larger than the group.  The compiler
gave some back: one v_cmp per predicate at its point of use, an s_nop behind some of them, and a second exec region for the pair and the
bus lanes, whose Jacobian writes sit behind the exit test.  The lane moves that are left carry the high halves of pi / 2 pi / the sincos
constants through scalar spill slots, not group-uniform flags; holding pi in a register of the lane made the loop longer and was dropped."""
import re

import pytest

from test_step_kernel_features import _compile, headline_feature_variant
from test_step_kernel_words_resident import SCRATCH, VMEM_LOAD, _blocks, newton_loop_lines

INSTR = re.compile(r"^\s+[a-z]")
LANE_MOVE = re.compile(r"^\s+v_(readlane|writelane)_b32")
SDWA_ADD = re.compile(r"^\s+v_add_u32_sdwa")
BRANCH = re.compile(r"^\s+s_c?branch\S*\s+\.L(BB\d+_\d+)")

# parent commit e78be07, headline feature variant, the counters of this file
PARENT_CYCLE_INSTR = 760         # instructions of newton_cycle_lines
PARENT_CYCLE_LANE_MOVES = 40     # v_readlane_b32 + v_writelane_b32 in it
PARENT_CYCLE_SDWA_ADD = 22       # v_add_u32_sdwa in it
PARENT_ANNOTATED_INSTR = 704     # instructions of newton_loop_lines (without the parent's pair phase, see above)
PARENT_ANNOTATED_LANE_MOVES = 40
PARENT_ANNOTATED_SDWA_ADD = 22


def newton_cycle_lines(asm):
    """Instruction lines of every block that is laid out behind the block of the entry marker and lies on a cycle through the block of the
    back-edge marker (branch targets and fall-through; the step loop around it closes in front of the entry marker, so it adds nothing)."""
    blocks = _blocks(asm)
    begin = [i for i, b in enumerate(blocks) if any("GPF_NEWTON_NWR_BEGIN" in l for l in b[2])]
    back = [i for i, b in enumerate(blocks) if any("GPF_NEWTON_NWR_BACKEDGE" in l for l in b[2])]
    assert len(begin) == 1 and len(back) == 1
    index = {b[0]: i for i, b in enumerate(blocks) if b[0]}
    succ = {}
    for i in range(begin[0] + 1, len(blocks)):
        ins = [l for l in blocks[i][2] if INSTR.match(l)]
        s = {index[m.group(1)] for l in ins for m in [BRANCH.match(l)] if m}
        if not (ins and re.match(r"^\s+(s_branch|s_endpgm)\b", ins[-1])) and i + 1 < len(blocks):
            s.add(i + 1)
        succ[i] = {j for j in s if j > begin[0]}

    def reach(start, edges):
        seen, todo = set(), [start]
        while todo:
            for j in edges.get(todo.pop(), ()):
                if j not in seen:
                    seen.add(j)
                    todo.append(j)
        return seen
    pred = {}
    for i, s in succ.items():
        for j in s:
            pred.setdefault(j, set()).add(i)
    cycle = reach(back[0], succ) & reach(back[0], pred)
    assert back[0] in cycle, "the back-edge marker is not on a cycle"
    return [l for i in sorted(cycle) for l in blocks[i][2]]


def _counts(lines):
    ins = [l for l in lines if INSTR.match(l)]
    return len(ins), sum(bool(LANE_MOVE.match(l)) for l in ins), sum(bool(SDWA_ADD.match(l)) for l in ins)


@pytest.fixture(scope="session")
def headline_asm(tmp_path_factory):
    hdr, variant = headline_feature_variant()
    d = tmp_path_factory.mktemp("diet")
    jobs = [_compile(d, hdr, variant, "feat"), _compile(d, hdr, variant.rsplit(",", 1)[0], "grid")]
    asm = []
    for p, out in jobs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-2000:]
        asm.append(out.read_text())
    return asm


def test_cycle_finder_on_a_two_entry_loop():
    """A hand-written listing with the parent's shape: the loop's last block branches to a block in front of the annotated header."""
    asm = "\n".join([
        "\t; GPF_NEWTON_NWR_BEGIN",
        "\ts_mov_b32 s0, 0",
        ".LBB0_1:                                ;   in Loop: Header=BB0_9 Depth=1",
        "\tv_readlane_b32 s1, v0, 1",
        ".LBB0_2:                                ;   Parent Loop BB0_9 Depth=1",
        "                                        ; =>  This Loop Header: Depth=2",
        "\tv_add_u32_sdwa v1, v2, v3",
        "\ts_cbranch_vccnz .LBB0_4",
        ".LBB0_3:                                ;   in Loop: Header=BB0_2 Depth=2",
        "\t; GPF_NEWTON_NWR_BACKEDGE",
        "\ts_cbranch_execnz .LBB0_1",
        "\ts_branch .LBB0_2",
        ".LBB0_4:",
        "\tv_writelane_b32 v0, s1, 1",
    ])
    assert _counts(newton_loop_lines(asm)) == (4, 0, 1)          # the annotated set: without BB0_1
    assert _counts(newton_cycle_lines(asm)) == (5, 1, 1)


def test_newton_loop_of_the_headline_kernel_is_at_least_60_instructions_shorter(headline_asm):
    feat, _ = headline_asm
    n, moves, sdwa = _counts(newton_cycle_lines(feat))
    n_a, moves_a, sdwa_a = _counts(newton_loop_lines(feat))
    print(f"Newton iteration (cycle through the back edge): instructions {PARENT_CYCLE_INSTR} -> {n}, v_readlane + v_writelane "
          f"{PARENT_CYCLE_LANE_MOVES} -> {moves}, v_add_u32_sdwa {PARENT_CYCLE_SDWA_ADD} -> {sdwa}")
    print(f"annotated loop blocks (newton_loop_lines): instructions {PARENT_ANNOTATED_INSTR} -> {n_a}, v_readlane + v_writelane "
          f"{PARENT_ANNOTATED_LANE_MOVES} -> {moves_a}, v_add_u32_sdwa {PARENT_ANNOTATED_SDWA_ADD} -> {sdwa_a}")
    assert n >= n_a
    assert 2 * moves <= PARENT_CYCLE_LANE_MOVES and 2 * moves_a <= PARENT_ANNOTATED_LANE_MOVES, (moves, moves_a)
    assert n <= PARENT_CYCLE_INSTR - 60, (PARENT_CYCLE_INSTR, n)


def test_no_pass_of_the_lu_decodes_an_address(headline_asm):
    """Between the entry of a pass (the phase boundary in front of it) and its first ds_read_b128 there is no v_add_u32_sdwa: in the parent
    every pass started with the four "base + 16-bit field" adds of its item words."""
    feat, _ = headline_asm
    lines = [l for l in newton_cycle_lines(feat) if INSTR.match(l) or "wave barrier" in l]
    n_pass, head = 0, None                                        # head: the instructions since the last phase boundary, up to the first read
    for l in lines:
        if "wave barrier" in l:
            head = []
        elif head is not None and re.match(r"^\s+ds_read_b128", l):
            assert not [x for x in head if SDWA_ADD.match(x)], head
            n_pass += 1
            head = None
        elif head is not None:
            head.append(l)
    assert n_pass >= 6, n_pass                                    # 5 forward passes + 1 back pass on this grid
    assert not [l for l in lines if SDWA_ADD.match(l)]


def test_no_spill_no_scratch_and_the_loop_is_still_the_newton_loop(headline_asm):
    feat, grid = headline_asm
    num = lambda key, a: int(re.search(r"\.%s:\s*(\d+)" % key, a).group(1))  # noqa: E731
    for a in (feat, grid):
        assert num("vgpr_spill_count", a) == 0 and num("private_segment_fixed_size", a) == 0 and num("vgpr_count", a) <= 256
        assert not [l for l in a.split("\n") if SCRATCH.match(l)]
        assert a.count("; GPF_NEWTON_NWR_BEGIN") == 1 and a.count("; GPF_NEWTON_NWR_BACKEDGE") == 1
    assert num("vgpr_count", feat) <= num("vgpr_count", grid), (num("vgpr_count", feat), num("vgpr_count", grid))
    print(f"VGPRs: feature build {num('vgpr_count', feat)}, grid-only build {num('vgpr_count', grid)}; SGPR spills {num('sgpr_spill_count', feat)}")
    loop = newton_loop_lines(feat)
    assert sum("ds_add_f64" in l for l in loop) >= 12 and any("v_rndne_f64" in l for l in loop)
    assert len([l for l in loop if INSTR.match(l)]) > 300
    assert not [l.strip() for l in loop if VMEM_LOAD.match(l)]
