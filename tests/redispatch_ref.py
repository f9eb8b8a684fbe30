"""TEST INFRASTRUCTURE -- closed-form reference of the redispatch program that `gpf_redispatch` solves (gridpf_redispatch.hpp).

The program of `oracle.redispatch_oracle.qp_terms` is separable with one coupling constraint:

    x_i(lambda) = clip(t_i - lambda / (2 w_i), lo_i, hi_i)   for i in M,        sum_M x_i(lambda) is piecewise linear and non-increasing,

the generators of G \\ M sit at hi (lambda < 0) or at lo (lambda > 0), and when lambda = 0 they share what is left in proportion to
1 / w_i, clipped: x_i = clip(alpha / w_i, lo_i, hi_i), piecewise linear and non-decreasing in alpha.  Bounds are widened by eps_poly / 2.
Both roots are found WITHOUT iteration: the breakpoints of the piecewise-linear sum are sorted, the sum is evaluated at each, the segment
that contains the wanted value is located, and the root is interpolated inside it (written as the linear equation of the segment's active
set, which is the same point and is exact when the wanted value is exactly 0).  Everything is `np.longdouble`; float64 comes out.

It shares no root-finding code with the device kernels nor with `solve_exact` of the oracle (a bisection), and does not import it."""
import numpy as np

from oracle.redispatch_oracle import qp_terms

L = np.longdouble


def _root_of_clipped_sum(slope, offset, lo, hi, want):
    """v with sum_i clip(offset_i + slope_i * v, lo_i, hi_i) = want, slope_i > 0 (non-decreasing sum), all longdouble.
    -> (v, x); `want` must lie within [sum lo, sum hi].  On a flat segment every v gives the same x: the left end is returned."""
    bp = np.unique(np.concatenate([(lo - offset) / slope, (hi - offset) / slope]))          # sorted
    val = np.clip(offset[None, :] + slope[None, :] * bp[:, None], lo[None, :], hi[None, :]).sum(axis=1)
    if want <= val[0]:
        j = 0
    elif want >= val[-1]:
        j = len(bp) - 1
    else:
        j = int(np.searchsorted(val, want, side="right")) - 1                                  # val[j] <= want < val[j + 1]
    if j == len(bp) - 1 or val[j + 1] == val[j]:
        v = bp[j]
    else:
        mid = L(0.5) * (bp[j] + bp[j + 1])                                                     # the active set of the open segment
        u = offset + slope * mid
        inside = (u > lo) & (u < hi)
        fixed = np.where(u >= hi, hi, lo)[~inside].sum()
        v = (want - fixed - offset[inside].sum()) / slope[inside].sum()
        v = min(max(v, bp[j]), bp[j + 1])
    return v, np.clip(offset + slope * v, lo, hi)


def solve_closed_form(q, eps_poly):
    """Exact minimiser of the program `q` = qp_terms(...).  -> (x [participating] float64, info) with info["branch"] in
    {"empty", "up", "down", "share", "nofree"}, info["lam"] (longdouble) and the widened bounds info["lo"], info["hi"] (float64)."""
    lo, hi = q["lo"].astype(L) - L(eps_poly) / 2, q["hi"].astype(L) + L(eps_poly) / 2
    w, tv, mod, rhs = q["w"].astype(L), q["tv"].astype(L), q["mod"].astype(bool), L(q["rhs"])
    info = dict(lo=lo.astype(np.float64), hi=hi.astype(np.float64), lam=L(0))
    if len(lo) == 0:
        return np.zeros(0), dict(info, branch="empty")
    free = ~mod
    x = np.zeros(len(lo), dtype=L)
    s0 = np.clip(tv[mod], lo[mod], hi[mod]).sum()
    f_lo, f_hi = lo[free].sum(), hi[free].sum()
    info.update(s0=s0, f_lo=f_lo, f_hi=f_hi)
    if rhs - s0 > f_hi or rhs - s0 < f_lo:
        up = rhs - s0 > f_hi
        # sum_M x_i(lambda) is non-increasing in lambda: solve in v = -lambda, slope 1 / (2 w_i)
        v, xm = _root_of_clipped_sum(1 / (2 * w[mod]), tv[mod], lo[mod], hi[mod], rhs - (f_hi if up else f_lo))
        x[mod] = xm
        x[free] = hi[free] if up else lo[free]
        info.update(branch="up" if up else "down", lam=-v)
    else:
        x[mod] = np.clip(tv[mod], lo[mod], hi[mod])
        if free.any():
            _, xf = _root_of_clipped_sum(1 / w[free], np.zeros(int(free.sum()), dtype=L), lo[free], hi[free], rhs - s0)
            x[free] = xf
        info["branch"] = "share" if free.any() else "nofree"
    return x.astype(np.float64), info


def feasibility_terms(new_p, prev_p, actual, target, rhs, lim):
    """The sums the two refusals compare (longdouble): sum_move, s_up, s_down (unwidened availability) and s_lo, s_hi (widened bounds)."""
    pmin, pmax, ru, rd = (lim[k].astype(L) for k in ("pmin", "pmax", "ramp_up", "ramp_down"))
    np_, pv, a = new_p.astype(L), prev_p.astype(L), actual.astype(L)
    part = ((new_p > 0.0) | (np.abs(actual) >= 1e-7) | (target != actual)) & lim["redispatchable"].astype(bool)
    incr = np_ - (pv - a)
    add = L(lim["eps_poly"]) / 2
    lo = np.maximum(pmin - (np_ + a), -rd - incr) - add
    hi = np.minimum(pmax - (np_ + a), ru - incr) + add
    return dict(part=part, sum_move=incr[part].sum() + L(rhs), s_up=np.minimum(pmax - pv, ru)[part].sum(),
                s_down=np.maximum(pmin - pv, -rd)[part].sum(), s_lo=lo[part].sum(), s_hi=hi[part].sum())


def dispatch_ref(new_p, prev_p, actual, target, modified, rhs, lim, with_info=False):
    """One call of the automaton on float64 rows [n_gen].  -> (ok, actual_dispatch after, float64): `actual` unchanged on both refusals
    (sum_move outside [s_down, s_up]; rhs outside [s_lo, s_hi]) and for the generators outside G."""
    new_p, prev_p, actual, target = (np.asarray(a, dtype=np.float64) for a in (new_p, prev_p, actual, target))
    lim = dict(lim, redispatchable=np.asarray(lim["redispatchable"]).astype(bool))
    q = qp_terms(new_p, prev_p, actual, target, np.asarray(modified).astype(bool), float(rhs), 0.0, 0.0, lim)
    if q is None:
        return (False, actual.copy(), None, None) if with_info else (False, actual.copy())
    f = feasibility_terms(new_p, prev_p, actual, target, rhs, lim)
    if L(rhs) < f["s_lo"] or L(rhs) > f["s_hi"]:
        return (False, actual.copy(), q, None) if with_info else (False, actual.copy())
    x, info = solve_closed_form(q, lim["eps_poly"])
    out = actual.copy()
    out[q["part"]] = (actual[q["part"]].astype(L) + x.astype(L)).astype(np.float64)
    return (True, out, q, dict(info, x=x)) if with_info else (True, out)


def spacing32(ref):
    """The GPU tolerance: one float32 spacing at the magnitude of float32(ref)."""
    return np.spacing(np.abs(np.float32(ref))).astype(np.float64)
