"""Test helpers of the rules by area and the composite actions (include/gridpf.h: gpf_set_topo_areas / gpf_set_topo_slots): the host
emulator built from the library's own rule core (tests/native/topo_area_emul.cpp), a Python restatement of ``RulesByArea._lookparam_byarea``
(Rules/rulesByArea.py:120-140 of the reference) on a composite's concatenated item list, and the checks against the verdicts recorded
from the reference environment (tests/golden/topo_area_*.npz, made by tests/golden/make_topo_area_fixtures.py).  Test helper only."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT, golden_path
from topo_rules_ref import TopoRules, topo_pos_sub

TOO_MANY_LINES, TOO_MANY_SUBS, LINE_COOLDOWN, SUB_COOLDOWN, AMBIGUOUS = 0x01, 0x02, 0x04, 0x08, 0x10
FIXTURES = {"case14": "l2rpn_case14_sandbox", "wcci118": "l2rpn_wcci_2022_dev"}

_SRC = os.path.join(ROOT, "tests", "native", "topo_area_emul.cpp")
_HDR = os.path.join(ROOT, "grid2op_amd", "csrc", "gridpf_topo_mask.hpp")
_BUILD = os.path.join(ROOT, "tests", "native", "_build")
_lib = None


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in (_SRC, _HDR))


def emulator():
    global _lib
    so = os.path.join(_BUILD, "libtopoareaemul.so")
    if _lib is None or _stale(so):
        if _stale(so):
            os.makedirs(_BUILD, exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", _SRC, "-o", so])
        _lib = C.CDLL(so)
        _lib.topo_area_emul.restype = C.c_int
    return _lib


def sanitized_program():
    """the same file with its own main, built with the address and undefined-behaviour sanitizers: a stand-alone program"""
    exe = os.path.join(_BUILD, "topo_area_emul_san")
    if _stale(exe):
        os.makedirs(_BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-DTOPO_AREA_EMUL_MAIN", _SRC, "-o", exe])
    return exe


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def emul(model, off, items, sub_area, topo, line_cd, sub_cd, comps=None, legal_rules=True, max_sub=1, max_line=1):
    """-> dict(mask [n, n_act], ambiguous [n_act], areas uint32 [n_act], comp_mask [n, n_comp], comp_ambiguous [n_comp])"""
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    off, items, topo, sub_cd = i32(off), i32(items).reshape(-1, 3), i32(topo).reshape(-1, model.dim_topo), i32(sub_cd).reshape(-1, model.n_sub)
    lcd = None if line_cd is None else i32(line_cd).reshape(-1, model.n_line)
    sa = None if sub_area is None else i32(sub_area)
    lo, le, ps = i32(model.line_or_pos_topo_vect), i32(model.line_ex_pos_topo_vect), i32(topo_pos_sub(model))
    n, n_act = topo.shape[0], len(off) - 1
    cp = None if comps is None else i32(comps)
    n_comp, n_slot = (0, 0) if cp is None else cp.shape
    mask, amb, areas = np.full((n, n_act), 0xEE, np.uint8), np.zeros(max(n_act, 1), np.uint8), np.zeros(max(n_act, 1), np.uint32)
    cmask, camb = np.full((n, max(n_comp, 1)), 0xEE, np.uint8), np.zeros(max(n_comp, 1), np.uint8)
    u8 = C.POINTER(C.c_uint8)
    rc = emulator().topo_area_emul(model.dim_topo, model.n_line, model.n_sub, _ip(lo), _ip(le), _ip(ps), n_act, _ip(off), _ip(items), _ip(sa),
                                   int(bool(legal_rules)), int(max_line), int(max_sub), n, _ip(topo), _ip(lcd), _ip(sub_cd), mask.ctypes.data_as(u8),
                                   amb.ctypes.data_as(u8), areas.ctypes.data_as(C.POINTER(C.c_uint32)), n_comp, n_slot, _ip(cp),
                                   cmask.ctypes.data_as(u8), camb.ctypes.data_as(u8))
    assert rc == 0
    return dict(mask=mask, ambiguous=amb[:n_act].astype(bool), areas=areas[:n_act], comp_mask=cmask[:, :n_comp], comp_ambiguous=camb[:n_comp].astype(bool))


class AreaRules(TopoRules):
    """the restatement: a composite's item list is the concatenation of its slots' lists; the limits hold per area, a line counting in
    the area of its origin substation"""

    def __init__(self, model, off, items, sub_area, max_sub=1, max_line=1):
        super().__init__(model, off, items, True, max_sub, max_line, 3, 3)
        self.sub_area = np.asarray(sub_area)
        self.n_area = int(self.sub_area.max()) + 1
        self.line_area = self.sub_area[np.asarray(model.line_or_sub)]

    def concat(self, comp):
        comp = [int(a) for a in np.atleast_1d(comp)]
        if any(a < -1 or a >= self.n_act for a in comp):
            return None
        its = [self._items(a) for a in comp if a >= 0]
        return np.concatenate(its) if its else np.zeros((0, 3), np.int64)

    def impact(self, row, its):
        setv, chg, setl, swl = self._dense(its)
        lo, le = self.lo, self.le
        status = (np.asarray(row)[lo] > 0) & (np.asarray(row)[le] > 0)
        notc = ~status
        imp = swl | (setl != 0)
        for kind, i, v in its:                                # (a line-status item with a value != 0 marks its line for good)
            if kind == 1 and v != 0:
                imp[i] = True
        eff = chg | (setv != 0)
        clr = imp & notc
        hit = ((setv[lo] > 0) & notc) | ((setv[le] > 0) & notc) | ((setv[lo] < 0) & status) | ((setv[le] < 0) & status)
        imp = imp | hit
        clr = clr | hit
        eff[lo[clr]] = False
        eff[le[clr]] = False
        subs = np.zeros(self.m.n_sub, bool)
        subs[self.pos_sub[eff]] = True
        return imp, subs

    def mask(self, row, line_cd, sub_cd, comp):
        its = self.concat(comp)
        if its is None or self._ambiguous(its):
            return AMBIGUOUS
        imp, subs = self.impact(row, its)
        m = 0
        for k in range(self.n_area):
            m |= TOO_MANY_LINES if imp[self.line_area == k].sum() > self.max_line else 0
            m |= TOO_MANY_SUBS if subs[self.sub_area == k].sum() > self.max_sub else 0
        m |= LINE_COOLDOWN if (np.asarray(line_cd)[imp] > 0).any() else 0
        m |= SUB_COOLDOWN if (np.asarray(sub_cd)[subs] > 0).any() else 0
        return m

    def masks(self, topo, line_cd, sub_cd, comps):
        return np.array([[self.mask(topo[k], line_cd[k], sub_cd[k], c) for c in comps] for k in range(len(topo))], np.uint8)

    def action_areas(self):
        m = self.m
        lo, le = self.lo, self.le
        line_of = np.full(m.dim_topo, -1)
        line_of[lo] = np.arange(m.n_line)
        line_of[le] = np.arange(m.n_line)
        out = np.zeros(self.n_act, np.uint32)
        for a in range(self.n_act):
            for kind, i, _ in self._items(a):
                subs = [self.pos_sub[i]] if kind in (0, 2) else []
                l = line_of[i] if kind in (0, 2) else i
                if l >= 0:
                    subs += [m.line_or_sub[l], m.line_ex_sub[l]]
                for s in subs:
                    out[a] |= np.uint32(1 << int(self.sub_area[s]))
        return out


_STATE = ("topo_vect", "last_bus", "cooldown_line", "cooldown_sub")            # columns of `state`, before ([:, 0]) and after ([:, 1]) the step
_AFTER = ("topo_after", "last_bus_after", "cooldown_line_after", "cooldown_sub_after")
_STEP = (("played", np.int32), ("is_illegal", bool), ("is_ambiguous", bool), ("done", bool))


def pack(rec):
    """the recorder's arrays -> the few arrays of the file (a zip member costs more than these small arrays do): per (step, entry) and per
    (step, composite) ONE byte = ambiguous << 4 | reason bit of _lookparam_byarea | reason bit of PreventReconnection (a rule's reason bit
    is 0 exactly when it says legal) | for composites "illegal under whole-grid LookParam" << 5; the four per-step scalars in `step`; the
    rows before / after the step side by side in `state`; dim_topo and n_line appended to `params`"""
    for p in ("", "comp_"):
        assert np.array_equal(rec[p + "area_legal"], rec[p + "area_bit"] == 0) and np.array_equal(rec[p + "prevent_legal"], rec[p + "prevent_bit"] == 0)
    bits = lambda p: (rec[p + "ambiguous"].astype(np.uint8) << 4) | rec[p + "area_bit"].astype(np.uint8) | rec[p + "prevent_bit"].astype(np.uint8)  # noqa: E731
    out = {k: rec[k] for k in ("off", "items", "comps", "sub_area", "grid")}
    out["params"] = np.concatenate([rec["params"], [rec["topo_vect"].shape[1], rec["cooldown_line"].shape[1]]]).astype(np.int32)
    out["verdict"] = bits("")
    out["comp_verdict"] = bits("comp_") | ((~rec["comp_look_legal"]).astype(np.uint8) << 5)
    out["step"] = np.stack([rec[k].astype(np.int16) for k, _ in _STEP], axis=1)
    out["state"] = np.stack([np.concatenate([rec[k] for k in _STATE], axis=1), np.concatenate([rec[k] for k in _AFTER], axis=1)], axis=1).astype(np.int8)
    return out


def unpack(f):
    """the arrays of the file -> the recorder's arrays (the inverse of `pack`)"""
    out = {k: f[k] for k in ("off", "items", "comps", "sub_area", "grid")}
    out["params"] = f["params"][:4]
    D, L = (int(v) for v in f["params"][4:6])
    S = len(f["sub_area"])
    for p, v in (("", f["verdict"]), ("comp_", f["comp_verdict"])):
        out[p + "ambiguous"] = (v & AMBIGUOUS) != 0
        out[p + "area_bit"] = (v & (TOO_MANY_LINES | TOO_MANY_SUBS)).astype(np.int8)
        out[p + "prevent_bit"] = (v & (LINE_COOLDOWN | SUB_COOLDOWN)).astype(np.int8)
        out[p + "area_legal"] = out[p + "area_bit"] == 0
        out[p + "prevent_legal"] = out[p + "prevent_bit"] == 0
    out["comp_look_legal"] = (f["comp_verdict"] & 0x20) == 0
    for i, (k, dt) in enumerate(_STEP):
        out[k] = f["step"][:, i].astype(dt)
    cuts = np.cumsum([D, D, L])
    assert f["state"].shape[2] == 2 * D + L + S
    for side, keys in enumerate((_STATE, _AFTER)):
        for k, v in zip(keys, np.split(f["state"][:, side], cuts, axis=1)):
            out[k] = np.ascontiguousarray(v)
    return out


_fix = {}


def load_fixture(tag):
    if tag not in _fix:
        _fix[tag] = unpack(dict(np.load(golden_path(f"topo_area_{tag}.npz"))))
    return _fix[tag]


def check_against_reference(fix, mask, prefix=""):
    """`mask` [steps, n] against the recorded verdicts of the entries (prefix "") or the composites (prefix "comp_")"""
    amb, al, ab, pl, pb = (fix[prefix + k] for k in ("ambiguous", "area_legal", "area_bit", "prevent_legal", "prevent_bit"))
    assert mask.shape == amb.shape
    assert np.array_equal(mask == 0, ~amb & al & pl)
    assert np.array_equal((mask & AMBIGUOUS) != 0, amb) and (mask[amb] == AMBIGUOUS).all()
    ok = ~amb
    assert ((mask & ab)[ok] == ab[ok]).all() and ((mask & pb)[ok] == pb[ok]).all()          # each rule's first reason is among the mask's
    assert np.array_equal(((mask & (TOO_MANY_LINES | TOO_MANY_SUBS)) != 0)[ok], ~al[ok])
    assert np.array_equal(((mask & (LINE_COOLDOWN | SUB_COOLDOWN)) != 0)[ok], ~pl[ok])
