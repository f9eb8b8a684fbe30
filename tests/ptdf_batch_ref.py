"""Plain float64 numpy statement of the tables `gpf_ptdf_build_batch` forms per topology class, built from oracle/pf_oracle.py alone:

  PTDF  T = `ptdf(m, state)`                                      [n_line, n_sub * n_busbar]
  H[:, k] = T[:, f_k] - T[:, t_k]                                 (f_k, t_k: global buses of the ends of line k)
  LODF  L[:, k] = H[:, k] / (1 - H_kk),  L[k, k] = -1             [n_line, n_line]

with the special columns classified by what the ORACLE does with line k forced off (`solve(..., is_dc=True)`), never by a threshold on
1 - H_kk and never by counting elements per bus:

  * line k out of service (or both ends on one bus): its outage changes nothing, the column is zero;
  * the DC power flow of the contingency fails (the outage islands an active bus): the WHOLE column is NaN, rows of out-of-service lines
    included;
  * the DC power flow of the contingency converges on FEWER active buses than the base topology has: the outage removed a bus that
    carried nothing but this line end (a stub).  Such a bus has no injection, so the line carries exactly 0 for every injection and its
    outage leaves every other flow as it was: the WHOLE column is zero (diagonal included: L[k, k] f_k = 0 whatever L[k, k] is, and a
    zero column is what "nothing changes" means).  Here 1 - H_kk = 0 up to rounding, so the quotient is not formed;
  * otherwise the contingency converges on the same buses: line k lies on a cycle, 1 - H_kk > 0, the quotient above.

Nothing of the kernels under test is in this file."""
import numpy as np

from oracle.pf_oracle import LaneState, element_buses, ptdf, solve

PTDF_BAR = 1e-9                        # absolute bar on PTDF entries (tests/test_gpu_ptdf_batch.py)
F32_EPS = 2.0 ** -23


def state_of(m, topo, shunt_bus=None):
    st = LaneState.from_model(m)
    st.topo = np.asarray(topo).copy()
    if shunt_bus is not None and m.n_shunt:
        st.shunt_bus = np.asarray(shunt_bus).copy()
    return st


def active_buses(m, state, n_busbar=2):
    """bool [n_sub * n_busbar]: buses that carry an in-service element (`_BackendAction._get_active_bus`, as oracle `solve`)."""
    parts = element_buses(m, state)
    act = np.zeros(m.n_sub * n_busbar, dtype=bool)
    for i in (0, 1, 3, 4, 5, 6):
        a = np.asarray(parts[i])
        act[a[a >= 0]] = True
    return act


def reference_buses(m, state, n_busbar=2):
    gbus = np.asarray(element_buses(m, state)[3])
    ref = np.zeros(m.n_sub * n_busbar, dtype=bool)
    ref[gbus[(gbus >= 0) & np.asarray(m.gen_slack, dtype=bool)]] = True
    return ref


def reduced_dim(m, state):
    """Active non-reference buses: the dimension of the reduced B' (`class_n`)."""
    return int((active_buses(m, state) & ~reference_buses(m, state)).sum())


def verdict(m, state):
    """Status the builder must report for the topology, from the oracle's DC power flow: 0 converged, 2 islanded, 3 no slack."""
    r = solve(m, state, is_dc=True)
    if r.converged:
        return 0
    if r.reason == "no in-service slack generator":
        return 3
    assert r.reason == "islanded grid", r.reason
    return 2


def without_line(state, m, k):
    s2 = state.copy()
    s2.topo[m.line_or_pos_topo_vect[k]] = -1
    s2.topo[m.line_ex_pos_topo_vect[k]] = -1
    return s2


def lodf_parts(m, state):
    """dict: T (PTDF), H, L (LODF), inv_den [n_line] (1 / (1 - H_kk) of the quotient columns, NaN elsewhere) and kind [n_line]:
    'off' | 'nan' | 'stub' | 'live'."""
    T = ptdf(m, state)
    lor, lex, status = element_buses(m, state)[:3]
    nl = m.n_line
    H = np.zeros((nl, nl))
    L = np.zeros((nl, nl))
    inv_den = np.full(nl, np.nan)
    kind = np.empty(nl, dtype=object)
    n_act = int(active_buses(m, state).sum())
    for k in range(nl):
        if not status[k] or lor[k] == lex[k]:
            kind[k] = "off"
            continue
        H[:, k] = T[:, lor[k]] - T[:, lex[k]]
        s2 = without_line(state, m, k)
        if not solve(m, s2, is_dc=True).converged:
            kind[k] = "nan"
            L[:, k] = np.nan
        elif int(active_buses(m, s2).sum()) < n_act:
            kind[k] = "stub"
        else:
            kind[k] = "live"
            inv_den[k] = 1.0 / (1.0 - H[k, k])
            L[:, k] = H[:, k] * inv_den[k]
            L[k, k] = -1.0
    return dict(T=T, H=H, L=L, inv_den=inv_den, kind=kind)


def lodf_reference(m, state):
    """float64 [n_line, n_line], see the module docstring."""
    return lodf_parts(m, state)["L"]


def lodf_tolerance(ref, inv_den):
    """[n_line, n_line] bound on |stored float32 LODF - ref|: float32 rounding of the stored value + an error of H of at most twice the
    PTDF bar (H is a difference of two PTDF entries) pushed through the quotient H / (1 - H_kk): d(H_mk / den) <= |dH| / |den| +
    |H_mk| |dH| / den^2 = |dH| / |den| (1 + |L_mk|), with dH <= 2 PTDF_BAR in the numerator and in the denominator (factor 2 x 2 = 4).
    Both terms from the reference.  NaN where the column is no quotient (those entries must match exactly)."""
    ref = np.asarray(ref, dtype=np.float64)
    return F32_EPS * np.abs(ref) + 4.0 * PTDF_BAR * np.abs(np.asarray(inv_den, dtype=np.float64))[None, :] * (1.0 + np.abs(ref))


def reduced_matrix(m, state):
    """B' over the active non-reference buses (the bus order of `ptdf`), and those buses."""
    lor, lex, status = element_buses(m, state)[:3]
    nb = len(active_buses(m, state))
    B = np.zeros((nb, nb))
    for l in np.nonzero(status)[0]:
        f, t = lor[l], lex[l]
        if f == t:
            continue
        b = m.br_bdc[l]
        B[f, f] += b
        B[t, t] += b
        B[f, t] -= b
        B[t, f] -= b
    free = np.nonzero(active_buses(m, state) & ~reference_buses(m, state))[0]
    return B[np.ix_(free, free)], free


def gauss_jordan_inverse(A):
    """In-place Gauss-Jordan WITHOUT pivoting, float64: the algorithm of the kernels stripped of tiles and matrix cores."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    for p in range(n):
        rp = 1.0 / A[p, p]
        col = A[:, p].copy()
        row = A[p, :] * rp
        A -= np.outer(col, row)
        A[p, :] = row
        A[:, p] = -col * rp
        A[p, p] = rp
    return A


def ptdf_by_gauss_jordan(m, state):
    """`ptdf(m, state)` with the inverse of B' from `gauss_jordan_inverse` instead of `np.linalg.inv`."""
    Bp, free = reduced_matrix(m, state)
    lor, lex, status = element_buses(m, state)[:3]
    nb = len(active_buses(m, state))
    X = np.zeros((nb, nb))
    X[np.ix_(free, free)] = gauss_jordan_inverse(Bp)
    out = np.zeros((m.n_line, nb))
    for l in np.nonzero(status)[0]:
        if lor[l] != lex[l]:
            out[l] = m.br_bdc[l] * (X[lor[l]] - X[lex[l]])
    return out
