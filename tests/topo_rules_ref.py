"""Python restatement of the topology acting path of the batched step (include/gridpf.h: gpf_upload_topo_actions), one lane at a time.

What BaseEnv.step does for the topology part of an action (paths relative to the reference checkout):
  1. ambiguity   BaseAction._check_for_ambiguity (Action/baseAction.py:3668-3760, topology kinds)
  2. impact      BaseAction.get_topological_impact (Action/baseAction.py:1782-2020) with the line status before the step
  3. legality    Rules/LookParam.py:28-53 + Rules/PreventReconnection.py:23-60
  4. application _BackendAction.__iadd__ (Action/_backendAction.py:836-919)
  5. bookkeeping Environment/baseEnv.py:3346-3395 + _BackendAction.update_state (Action/_backendAction.py:1533-1555)
Test helper only: the engine never imports it.
"""
from __future__ import annotations

import numpy as np

SET_BUS, SET_LINE_STATUS, CHANGE_BUS, CHANGE_LINE_STATUS, SET_SHUNT_BUS = 0, 1, 2, 3, 4


def pack_actions(actions):
    """the {kind, id, value} encoding of gpf_simulate_batch / gpf_upload_topo_actions for the keys set_bus (dict position -> bus),
    change_bus (positions), set_line_status ((line, +-1) pairs) and change_line_status (lines)"""
    off, items = [0], []
    for act in actions:
        items += [(SET_LINE_STATUS, int(l), int(v)) for l, v in act.get("set_line_status", ())]
        items += [(CHANGE_LINE_STATUS, int(l), 0) for l in act.get("change_line_status", ())]
        items += [(SET_BUS, int(p), int(v)) for p, v in dict(act.get("set_bus", {})).items()]
        items += [(CHANGE_BUS, int(p), 0) for p in act.get("change_bus", ())]
        off.append(len(items))
    return np.asarray(off, np.int32), np.asarray(items, np.int32).reshape(-1, 3)


def topo_pos_sub(model) -> np.ndarray:
    """substation of every topo_vect position"""
    ps = np.zeros(model.dim_topo, dtype=np.int64)
    ps[model.line_or_pos_topo_vect] = model.line_or_sub
    ps[model.line_ex_pos_topo_vect] = model.line_ex_sub
    ps[model.gen_pos_topo_vect] = model.gen_sub
    ps[model.load_pos_topo_vect] = model.load_sub
    if model.n_storage:
        ps[model.storage_pos_topo_vect] = model.storage_sub
    return ps


class TopoRules:
    def __init__(self, model, off, items, legal_rules=True, max_sub=1, max_line=1, cd_sub=0, cd_line=0):
        self.m = model
        self.off = np.asarray(off)
        self.items = np.asarray(items).reshape(-1, 3)
        self.on, self.max_sub, self.max_line, self.cd_sub, self.cd_line = legal_rules, max_sub, max_line, cd_sub, cd_line
        self.pos_sub = topo_pos_sub(model)
        self.lo, self.le = np.asarray(model.line_or_pos_topo_vect), np.asarray(model.line_ex_pos_topo_vect)
        self.n_act = len(self.off) - 1
        self.ambiguous = np.array([self._ambiguous(self._items(k)) for k in range(self.n_act)], dtype=bool)

    def _items(self, k):
        return self.items[self.off[k]:self.off[k + 1]]

    def _dense(self, its):
        m = self.m
        setv = np.zeros(m.dim_topo, dtype=np.int64)
        chg = np.zeros(m.dim_topo, dtype=bool)
        setl = np.zeros(m.n_line, dtype=np.int64)
        swl = np.zeros(m.n_line, dtype=bool)
        for kind, i, v in its:
            if kind == SET_BUS:
                setv[i] = v
            elif kind == CHANGE_BUS:
                chg[i] = True
            elif kind == SET_LINE_STATUS:
                setl[i] = v
            elif kind == CHANGE_LINE_STATUS:
                swl[i] = True
        return setv, chg, setl, swl

    def _ambiguous(self, its) -> bool:
        setv, chg, setl, swl = self._dense(its)
        lo, le = self.lo, self.le
        if (chg & (setv != 0)).any() or (swl & (setl != 0)).any():
            return True
        if ((setv[lo] == -1) & (setv[le] > 0)).any() or ((setv[le] == -1) & (setv[lo] > 0)).any():
            return True
        d, r = setl == -1, setl == 1
        if (d & ((setv[lo] > 0) | (setv[le] > 0) | chg[lo] | chg[le])).any():
            return True
        if (r & ((setv[lo] == -1) | (setv[le] == -1) | chg[lo] | chg[le])).any():
            return True
        return False

    # ---- 4. application: _BackendAction.__iadd__ restricted to topology ---------------------------------------------------------
    def apply(self, row, last, its, sb=None):
        row = np.array(row, dtype=np.int64)
        lo, le = self.lo, self.le
        old = lambda p: int(last[p]) if last is not None and last[p] >= 1 else 1  # noqa: E731

        def reco(l):
            if row[lo[l]] < 0:
                row[lo[l]] = old(lo[l])
            if row[le[l]] < 0:
                row[le[l]] = old(le[l])

        def disco(l):
            row[lo[l]] = -1
            row[le[l]] = -1
        for kind, l, v in its:
            if kind == CHANGE_LINE_STATUS:
                if row[lo[l]] > 0 or row[le[l]] > 0:
                    disco(l)
                else:
                    reco(l)
        for kind, l, v in its:
            if kind == SET_LINE_STATUS:
                if v < 0:
                    disco(l)
                elif v > 0:
                    reco(l)
        any_bus = any(k == CHANGE_BUS or (k == SET_BUS and v != 0) for k, _, v in its)
        ob, eb = row[lo].copy(), row[le].copy()
        for kind, p, v in its:
            if kind == CHANGE_BUS and row[p] > 0:
                row[p] = (1 - row[p]) + 2
        for kind, p, v in its:
            if kind == SET_BUS and v != 0:
                row[p] = v
        if any_bus:
            for l in range(self.m.n_line):
                o_, x_ = row[lo[l]], row[le[l]]
                d_now = ob[l] == -1 or o_ == -1 or eb[l] == -1 or x_ == -1
                r_now = ob[l] == -1 and (o_ >= 1 or x_ >= 1)
                if r_now:
                    reco(l)
                elif d_now:
                    disco(l)
        if sb is not None:
            sb = np.array(sb, dtype=np.int64)
            for kind, i, v in its:
                if kind == SET_SHUNT_BUS and v != 0:
                    sb[i] = v
        return row, sb

    # ---- 1-4 --------------------------------------------------------------------------------------------------------------------
    def pre(self, row, line_cd, sub_cd, last, a):
        """-> (new row, is_illegal, is_ambiguous, aff_lines, aff_subs) for action index `a` (-1: do nothing)"""
        m = self.m
        none = (np.zeros(m.n_line, bool), np.zeros(m.n_sub, bool))
        if a == -1:
            return np.array(row), False, False, *none
        if a < -1 or a >= self.n_act or self.ambiguous[a]:
            return np.array(row), False, True, *none
        its = self._items(a)
        setv, chg, setl, swl = self._dense(its)
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
        subs = np.zeros(m.n_sub, bool)
        subs[self.pos_sub[eff]] = True
        if self.on and (imp.sum() > self.max_line or subs.sum() > self.max_sub or (np.asarray(line_cd)[imp] > 0).any()
                        or (np.asarray(sub_cd)[subs] > 0).any()):
            return np.array(row), True, False, *none
        new, _ = self.apply(row, last, its)
        return new, False, False, imp, subs

    # ---- 5 -----------------------------------------------------------------------------------------------------------------------
    def post(self, topo_after, line_cd, sub_cd, last, aff_lines, aff_subs):
        """bookkeeping after a converged step: line_cd = the cooldowns after the step's own update (trips, outages)"""
        line_cd, sub_cd, last = np.array(line_cd), np.array(sub_cd), np.array(last)
        if self.cd_line > 0:
            c = aff_lines & (line_cd < self.cd_line)
            line_cd[c] = self.cd_line
        if self.cd_sub > 0:
            sub_cd = np.maximum(sub_cd - 1, 0)
            sub_cd[aff_subs] = self.cd_sub
        conn = np.asarray(topo_after) >= 1
        last[conn] = np.asarray(topo_after)[conn]
        return line_cd, sub_cd, last


def random_topo_table(model, rng, n_split=10, n_merge=4, n_change=4, n_line_act=10, n_busbar=2):
    """A split-heavy action table (dicts as PowerFlowEngine.pack_actions takes them) over the substations with >= 4 elements."""
    ps = topo_pos_sub(model)
    subs = [s for s in range(model.n_sub) if (ps == s).sum() >= 4]
    acts = []

    def split(s):
        pos = np.flatnonzero(ps == s)
        while True:
            b = rng.integers(1, n_busbar + 1, size=len(pos))
            if (b == 1).sum() >= 2 and (b == 2).sum() >= 2:
                return {int(p): int(v) for p, v in zip(pos, b)}
    for _ in range(n_split):
        acts.append({"set_bus": split(int(rng.choice(subs)))})
    for _ in range(n_merge):
        s = int(rng.choice(subs))
        acts.append({"set_bus": {int(p): 1 for p in np.flatnonzero(ps == s)}})
    for _ in range(n_change):
        s = int(rng.choice(subs))
        acts.append({"change_bus": [int(p) for p in rng.choice(np.flatnonzero(ps == s), size=2, replace=False)]})
    for k in range(n_line_act):
        l = int(rng.integers(model.n_line))
        acts.append({"set_line_status": [(l, -1 if k % 3 == 0 else 1)]} if k % 3 != 2 else {"change_line_status": [l]})
    s1, s2 = rng.choice(subs, size=2, replace=False)
    two = split(int(s1))
    two.update(split(int(s2)))
    acts.append({"set_bus": two})                                            # two substations at once
    p = int(np.flatnonzero(ps == subs[0])[0])
    acts.append({"set_bus": {p: 2}, "change_bus": [p]})                      # ambiguous
    return acts
