"""The redispatching automaton (grid2op/Environment/baseEnv.py:2211-2470).

CPU: the oracle restatement (oracle/redispatch_oracle.py, scipy SLSQP like the reference) reproduces the calls recorded inside
unmodified reference environments (tests/golden/redispatch_cases.npz).  GPU: the device kernel behind ``gpf_redispatch`` solves the
same quadratic program exactly (the program is separable: one multiplier); it must satisfy the constraints, reach the optimum
of the objective (never worse than SLSQP's approximate minimiser), land on the recorded dispatch wherever the minimiser is
unique, and equal the closed-form reference (tests/redispatch_ref.py) to one float32 spacing.  What `apply=True` installs is
checked in tests/test_gpu_redispatch.py."""
import numpy as np
import pytest

from conftest import golden_path

ENVS = ["l2rpn_case14_sandbox", "l2rpn_wcci_2022_dev", "educ_case14_storage"]


def _cases(env):
    d = dict(np.load(golden_path("redispatch_cases.npz")))
    tag = env + "__"
    c = {k[len(tag):]: v for k, v in d.items() if k.startswith(tag)}
    lim = {k: c[k] for k in ("pmin", "pmax", "ramp_up", "ramp_down", "redispatchable")}
    lim["eps_poly"], lim["tol_poly"] = float(c["eps_poly"]), float(c["tol_poly"])
    return c, lim


@pytest.mark.parametrize("env", ENVS)
def test_oracle_reproduces_the_reference_automaton(env):
    from oracle.redispatch_oracle import compute_dispatch
    c, lim = _cases(env)
    n = len(c["ok"])
    assert n >= 60
    worst = 0.0
    for k in range(n):
        ok, after = compute_dispatch(c["new_p"][k], c["prev_p"][k], c["actual"][k], c["target"][k], c["modified"][k], float(c["storage"][k]),
                                     float(c["curtail"][k]), float(c["detached"][k]), lim, first=bool(c["first"][k]))
        assert ok == bool(c["ok"][k]), k
        worst = max(worst, float(np.abs(after - c["actual_after"][k]).max()))
    assert worst < 1e-5, worst                  # same solver, same formulation: float32 storage of the recording is the only gap
    assert np.abs(c["actual_after"]).max() > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS)
def test_device_redispatch_solves_the_same_program(env, load_model):
    from grid2op_amd.engine import PowerFlowEngine
    from oracle.redispatch_oracle import objective_mw, qp_terms
    from redispatch_ref import dispatch_ref, spacing32
    m = load_model(env)
    c, lim = _cases(env)
    n = len(c["ok"])
    eng = PowerFlowEngine(m, n_lanes=n, device=0)
    eng.set_gen_limits(lim["pmin"], lim["pmax"], lim["ramp_up"], lim["ramp_down"], lim["redispatchable"], eps_poly=lim["eps_poly"])
    prev = np.where(c["first"][:, None], c["new_p"], c["prev_p"])
    rhs = c["storage"] - c["curtail"] + c["detached"]
    ok, after = eng.redispatch(c["new_p"], prev, c["actual"], c["target"], c["modified"], rhs)
    assert np.array_equal(ok, c["ok"])
    n_unique = 0
    worst = gap = dev = 0.0
    for k in range(n):
        # the exact reference on the recorded inputs: the final cast to float32 is the only rounding that counts (one spacing, no more)
        ok_ref, after_ref = dispatch_ref(c["new_p"][k], prev[k], c["actual"][k], c["target"][k], c["modified"][k], rhs[k], lim)
        assert ok_ref == bool(ok[k]), k
        d = np.abs(after[k].astype(np.float64) - np.float32(after_ref).astype(np.float64)) / spacing32(after_ref)
        assert (d <= 1.0).all(), (k, float(d.max()), int(d.argmax()), after[k][d.argmax()], after_ref[d.argmax()])
        dev = max(dev, float(d.max()))
        q = qp_terms(c["new_p"][k], c["prev_p"][k], c["actual"][k], c["target"][k], c["modified"][k], float(c["storage"][k]),
                     float(c["curtail"][k]), float(c["detached"][k]), lim, first=bool(c["first"][k]))
        part = q["part"]
        x = (after[k] - c["actual"][k])[part].astype(np.float64)
        x_ref = (c["actual_after"][k] - c["actual"][k])[part]
        assert np.array_equal(after[k][~part], c["actual"][k][~part].astype(np.float32)), k       # untouched outside G
        tol = 2e-3                                                           # MW; float32 state, tol_poly of the reference is 1e-2
        assert abs(x.sum() - q["rhs"]) < tol, (k, x.sum(), q["rhs"])
        assert (x >= q["lo"] - 0.5 * lim["eps_poly"] - tol).all() and (x <= q["hi"] + 0.5 * lim["eps_poly"] + tol).all(), k
        assert objective_mw(q, x) <= objective_mw(q, x_ref) + 1e-4, (k, objective_mw(q, x), objective_mw(q, x_ref))
        # SLSQP stops at ftol = 1e-6 on a scaled objective whose weights are ~1/n_gen: its minimiser is approximate -- the recorded x
        # sit up to ~0.4 MW from the exact optimum (whole groups of identical generators shifted together) at an objective that is
        # never lower than the device's.  The distance is therefore only a sanity bound; optimality is the criterion above.
        assert np.abs(x - x_ref)[q["mod"]].max() < 1.0, (k, np.abs(x - x_ref).max())
        n_unique += int(q["mod"].all())
        gap = max(gap, objective_mw(q, x_ref) - objective_mw(q, x))
        worst = max(worst, float(np.abs(x - x_ref)[q["mod"]].max()))
    assert n_unique >= 5
    print(f"{env}: {n} programs, worst |x - x_SLSQP| on the modified generators {worst:.3f} MW, SLSQP objective above the exact "
          f"optimum by up to {gap:.2e} MW^2; worst distance to the closed-form reference {dev:.2f} float32 spacings")
    eng.close()
