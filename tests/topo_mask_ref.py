"""Test helpers of the legality masks (include/gridpf.h: gpf_topo_action_mask): the host emulator built from the library's own rule core
(tests/native/topo_mask_emul.cpp), the restatement with reason bits (a subclass of tests/topo_rules_ref.TopoRules) and the checks of a
mask against the verdicts recorded from the reference environment (tests/golden/topo_mask_*.npz, made by
tests/golden/make_topo_mask_fixtures.py).  Test helper only: the engine never imports it."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT, golden_path
from topo_rules_ref import TopoRules, topo_pos_sub

TOO_MANY_LINES, TOO_MANY_SUBS, LINE_COOLDOWN, SUB_COOLDOWN, AMBIGUOUS = 0x01, 0x02, 0x04, 0x08, 0x10
FIXTURES = {"case14": "l2rpn_case14_sandbox", "wcci118": "l2rpn_wcci_2022_dev"}

_SRC = os.path.join(ROOT, "tests", "native", "topo_mask_emul.cpp")
_HDR = os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_topo_mask.hpp")
_BUILD = os.path.join(ROOT, "tests", "native", "_build")
_lib = None


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in (_SRC, _HDR))


def emulator():
    """the emulator as a shared library, built with g++ (no HIP header involved)"""
    global _lib
    so = os.path.join(_BUILD, "libtopomaskemul.so")
    if _lib is None or _stale(so):
        if _stale(so):
            os.makedirs(_BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", _SRC, "-o", so])
        _lib = C.CDLL(so)
        _lib.topo_mask_emul.restype = C.c_int
    return _lib


def sanitized_program():
    """the same file with its own main, built with the address and undefined-behaviour sanitizers: a stand-alone program"""
    exe = os.path.join(_BUILD, "topo_mask_emul_san")
    if _stale(exe):
        os.makedirs(_BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-DTOPO_MASK_EMUL_MAIN", _SRC, "-o", exe])
    return exe


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def emul_mask(model, off, items, topo, line_cd, sub_cd, legal_rules=True, max_sub=1, max_line=1):
    """-> (mask uint8 [n, n_act], static ambiguity bool [n_act]) of lanes with rows topo / line_cd (None: no buffer) / sub_cd"""
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    off, items, topo, sub_cd = i32(off), i32(items).reshape(-1, 3), i32(topo).reshape(-1, model.dim_topo), i32(sub_cd).reshape(-1, model.n_sub)
    lcd = None if line_cd is None else i32(line_cd).reshape(-1, model.n_line)
    lo, le, ps = i32(model.line_or_pos_topo_vect), i32(model.line_ex_pos_topo_vect), i32(topo_pos_sub(model))
    n, n_act = topo.shape[0], len(off) - 1
    mask = np.full((n, n_act), 0xEE, np.uint8)
    amb = np.zeros(max(n_act, 1), np.uint8)
    u8 = C.POINTER(C.c_uint8)
    rc = emulator().topo_mask_emul(model.dim_topo, model.n_line, model.n_sub, _ip(lo), _ip(le), _ip(ps), n_act, _ip(off), _ip(items),
                                   int(bool(legal_rules)), int(max_line), int(max_sub), n, _ip(topo), None if lcd is None else _ip(lcd), _ip(sub_cd),
                                   mask.ctypes.data_as(u8), amb.ctypes.data_as(u8))
    assert rc == 0
    return mask, amb[:n_act].astype(bool)


class MaskRules(TopoRules):
    """the restatement with every reason kept: `TopoRules.pre` up to the legality decision, as reason bits"""

    def mask(self, row, line_cd, sub_cd, a):
        if self.ambiguous[a]:
            return AMBIGUOUS
        if not self.on:
            return 0
        # (the impact arithmetic of TopoRules.pre)
        setv, chg, setl, swl = self._dense(self._items(a))
        lo, le = self.lo, self.le
        status = (np.asarray(row)[lo] > 0) & (np.asarray(row)[le] > 0)
        notc = ~status
        imp = swl | (setl != 0)
        eff = chg | (setv != 0)
        clr = imp & notc
        hit = ((setv[lo] > 0) & notc) | ((setv[le] > 0) & notc) | ((setv[lo] < 0) & status) | ((setv[le] < 0) & status)
        imp = imp | hit
        clr = clr | hit
        eff[lo[clr]] = False
        eff[le[clr]] = False
        subs = np.zeros(self.m.n_sub, bool)
        subs[self.pos_sub[eff]] = True
        m = (TOO_MANY_LINES if imp.sum() > self.max_line else 0) | (TOO_MANY_SUBS if subs.sum() > self.max_sub else 0)
        m |= LINE_COOLDOWN if (np.asarray(line_cd)[imp] > 0).any() else 0
        m |= SUB_COOLDOWN if (np.asarray(sub_cd)[subs] > 0).any() else 0
        # ... and its verdict is the one `pre` gives
        _, ill, amb, _, _ = self.pre(row, line_cd, sub_cd, None, a)
        assert ill == (m != 0) and not amb
        return m

    def masks(self, topo, line_cd, sub_cd):
        return np.array([[self.mask(topo[k], line_cd[k], sub_cd[k], a) for a in range(self.n_act)] for k in range(len(topo))], np.uint8)


def unpack_actions(off, items):
    """the {kind, id, value} encoding -> the dicts `PowerFlowEngine.upload_topo_actions` takes (packed again they give the same items)"""
    acts = []
    for a in range(len(off) - 1):
        d = {}
        for kind, i, v in np.asarray(items).reshape(-1, 3)[off[a]:off[a + 1]]:
            if kind == 0:
                d.setdefault("set_bus", {})[int(i)] = int(v)
            elif kind == 1:
                d.setdefault("set_line_status", []).append((int(i), int(v)))
            elif kind == 2:
                d.setdefault("change_bus", []).append(int(i))
            elif kind == 3:
                d.setdefault("change_line_status", []).append(int(i))
        acts.append(d)
    return acts


def hand_set_states(model, rng, n):
    """n lane states with cooldowns and open lines, lane 0 untouched: (topo, line cooldowns, substation cooldowns), int32"""
    topo = np.tile(model.initial_topo_vect(), (n, 1)).astype(np.int32)
    lo, le = np.asarray(model.line_or_pos_topo_vect), np.asarray(model.line_ex_pos_topo_vect)
    lcd = ((rng.random((n, model.n_line)) < 0.3) * rng.integers(1, 4, (n, model.n_line))).astype(np.int32)
    scd = ((rng.random((n, model.n_sub)) < 0.3) * rng.integers(1, 4, (n, model.n_sub))).astype(np.int32)
    for k in range(1, n):
        if k % 3 == 1:                                        # cooldowns only
            continue
        for l in rng.choice(model.n_line, size=max(2, model.n_line // (2 if k % 3 == 2 else 5)), replace=False):
            topo[k, lo[l]] = topo[k, le[l]] = -1
        if k % 3 == 2:                                        # open lines only
            lcd[k] = 0
            scd[k] = 0
    lcd[0] = 0
    scd[0] = 0
    return topo, lcd, scd


_fix = {}


def load_fixture(tag):
    if tag not in _fix:
        _fix[tag] = dict(np.load(golden_path(f"topo_mask_{tag}.npz")))
    return _fix[tag]


def check_against_reference(fix, mask):
    """`mask` [steps, n_act] against the reference's recorded verdicts at every (step, entry)"""
    amb, ll, lb, pl, pb = (fix[k] for k in ("ambiguous", "look_legal", "look_bit", "prevent_legal", "prevent_bit"))
    assert mask.shape == amb.shape
    assert np.array_equal(mask == 0, ~amb & ll & pl)                         # playable <=> not ambiguous and both rules say legal
    assert np.array_equal((mask & AMBIGUOUS) != 0, amb)
    assert (mask[amb] == AMBIGUOUS).all()                                    # an ambiguous entry carries that bit alone
    ok = ~amb
    assert ((mask & lb)[ok] == lb[ok]).all() and ((mask & pb)[ok] == pb[ok]).all()      # each rule's first reason is among the mask's
    assert np.array_equal(((mask & (TOO_MANY_LINES | TOO_MANY_SUBS)) != 0)[ok], ~ll[ok])        # the mask's bits are those two rules' and nobody else's
    assert np.array_equal(((mask & (LINE_COOLDOWN | SUB_COOLDOWN)) != 0)[ok], ~pl[ok])
