#!/usr/bin/env python
"""Record which scenario every ``env.reset()`` of the unmodified reference environment starts (build container only, never on a GPU box).

    python tests/golden/make_cursor_fixtures.py /path/to/reference        # -> tests/golden/chronics_cursor_case14.npz

l2rpn_case14_sandbox (``test=True``: the scenarios 0000 / 0001 / 0002) with short episodes (``max step`` 2 - 4), do-nothing steps, in
three phases a replay can configure once each:

  phase 0   plain resets (``next_chronics``: the order wraps), one after ``env.set_id``, one that ends in a game over (the agent opens
            the first line whose loss ends the episode, as make_episode_limit_fixtures.py does), one more plain reset behind it
  phase 1   seeded ``sample_next_chronics(p)`` resets with a non-uniform p; the uniform each one consumed is recovered from a copy of
            ``space_prng``'s state taken before the call
  phase 2   ``env.reset(options={"init ts": 2})``

Per row (the reset observation is a row): phase, scenario index, table row, how the episode began, ``gen_p`` / ``load_p`` / ``rho`` /
``line_status`` and the six calendar attributes of the observation.  Also each scenario's start and the first rows of the three
scenarios' chronics.  The recorder asserts that tests/cursor_ref.py reproduces every recorded scenario.  Data only."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
CALENDAR = ("year", "month", "day", "hour_of_day", "minute_of_hour", "day_of_week")
PLAIN, SET_ID, SAMPLED, INIT_TS = 0, 1, 2, 3
PROBABILITIES = (0.2, 0.5, 0.3)
MAX_BYTES = 64 * 1024


def record(reference, seed=11):
    import grid2op
    from grid2op.Exceptions import AmbiguousAction, IllegalAction
    from grid2op.Parameters import Parameters
    from conformance_backend import OracleHipBackend
    from grid2op_amd.chronics import load_chronics_multifolder
    from grid2op_amd.grid_model import GridModel
    import cursor_ref as CR
    env_name = "l2rpn_case14_sandbox"
    model = GridModel.load_npz(os.path.join(HERE, env_name + ".grid.npz"))
    p = Parameters()
    p.NO_OVERFLOW_DISCONNECTION = True
    env = grid2op.make(env_name, test=True, backend=OracleHipBackend(), param=p)
    cls = type(env)
    env.seed(seed)
    mf = env.chronics_handler.real_data
    pr, thermal = env.parameters, env.get_thermal_limit().astype(np.float32)
    names = [os.path.basename(x) for x in mf.subpaths]
    assert names == ["0000", "0001", "0002"] and list(mf._order) == [0, 1, 2]
    keys = ("phase", "is_reset", "how", "set_id", "uniform", "scenario", "row", "max_step", "done", "terminated", "truncated", "agent_line",
            "gen_p", "load_p", "rho", "line_status") + CALENDAR
    rec = {k: [] for k in keys}
    starts = {}

    def note(obs, phase, is_reset, how, set_id, u, N, done, failed, agent_line):
        sc = names.index(os.path.basename(env.chronics_handler.get_id()))
        now = int((np.datetime64(env.time_stamp) - np.datetime64("1970-01-01T00:00")) / np.timedelta64(1, "m"))
        if is_reset and how != INIT_TS:
            starts[sc] = now                        # (every scenario is started plainly before "init ts" starts one further in)
        at = (now - starts[sc]) // 5                # the table row from the clock: nb_time_step restarts at 0 after "init ts"
        row = dict(phase=phase, is_reset=int(is_reset), how=how, set_id=set_id, uniform=u, scenario=sc, row=at, max_step=N,
                   done=int(done), terminated=int(failed), truncated=int(done and not failed), agent_line=agent_line,
                   gen_p=obs.gen_p.astype(np.float32), load_p=obs.load_p.astype(np.float32), rho=obs.rho.astype(np.float32),
                   line_status=obs.line_status.copy())
        for k in CALENDAR:
            row[k] = int(getattr(obs, k))
        for k in keys:
            rec[k].append(row[k])

    def killer(obs):
        for l in range(cls.n_line):                 # the first line whose loss ends the episode right now
            if obs.line_status[l] and obs.time_before_cooldown_line[l] == 0:
                sim_env = env.copy()
                _, _, d_, i_ = sim_env.step(env.action_space({"set_line_status": [(l, -1)]}))
                sim_env.close()
                if d_ and any(not isinstance(e, (AmbiguousAction, IllegalAction)) for e in i_.get("exception", []) or []):
                    return l
        raise AssertionError("no line ends the episode")

    def episode(phase, how, N, set_id=-1, kill_at=0, init_ts=0):
        u = np.nan
        if how == SET_ID:
            env.set_id(set_id)
        if how == SAMPLED:
            twin = np.random.RandomState()
            twin.set_state(mf.space_prng.get_state())
            u = float(twin.random_sample())
            env.chronics_handler.sample_next_chronics(list(PROBABILITIES))
        opts = {"max step": N}
        if how == INIT_TS:
            opts["init ts"] = init_ts
        obs = env.reset(options=opts)
        note(obs, phase, True, how, set_id, u, N, False, False, -1)
        for t in range(1, N + 1):
            line = killer(obs) if t == kill_at else -1
            act = env.action_space({"set_line_status": [(line, -1)]} if line >= 0 else {})
            obs, _, done, info = env.step(act)
            failed = bool(done) and bool(info.get("exception"))
            note(obs, phase, False, how, set_id, u, N, done, failed, line)
            assert done == (t == N or t == kill_at) and failed == (t == kill_at), (how, t, done, info.get("exception"))
            if done:
                break

    for i, N in enumerate((2, 3, 4, 2, 3, 2)):      # six plain resets: 0001 0002 0000 0001 0002 0000 (make() took 0000)
        episode(0, PLAIN, N)
    episode(0, SET_ID, 2, set_id=2)
    episode(0, PLAIN, 4, kill_at=2)                 # the game over, and the reset after it
    episode(0, PLAIN, 2)
    for i in range(7):
        episode(1, SAMPLED, 2 + i % 2)
    episode(2, INIT_TS, 3, init_ts=2)
    env.close()

    out = {k: np.asarray(rec[k], dtype=np.float32 if k in ("gen_p", "load_p", "rho") else bool if k == "line_status" else np.float64 if k == "uniform"
                         else np.int32) for k in keys}
    n_rows = int(out["row"].max()) + 2
    chron_dir = os.path.join(reference, "grid2op", "data", env_name, "chronics")
    charac = os.path.join(reference, "grid2op", "data", env_name, "prods_charac.csv")
    names2, ch = load_chronics_multifolder(chron_dir, model, prods_charac=charac, max_rows=n_rows, truncate=True)
    assert names2 == names
    for k, v in ch.items():
        if k in ("load_p", "load_q", "prod_p", "prod_v"):
            out["chron_" + k] = v.astype(np.float32)
        elif k in ("maintenance", "hazards"):
            assert not v[:, :n_rows].any(), "an outage in the recorded window"
    out.update(grid=np.array(env_name), start_minutes=np.array([starts[s] for s in range(3)], np.int64), thermal_limit=thermal,
               probabilities=np.array(PROBABILITIES, np.float64), seed=np.int32(seed),
               params=np.array([pr.MAX_SUB_CHANGED, pr.MAX_LINE_STATUS_CHANGED, pr.NB_TIMESTEP_COOLDOWN_SUB, pr.NB_TIMESTEP_COOLDOWN_LINE,
                                pr.NB_TIMESTEP_RECONNECTION], np.int32))

    # the restatement reproduces every recorded scenario from the recorded uniforms; the sequence wraps; the sampled resets differ
    starts_at = np.flatnonzero(out["is_reset"])
    for phase in (0, 1, 2):
        idx = [i for i in starts_at if out["phase"][i] == phase]
        sampled = phase == 1
        ref = CR.CursorRef(1, [0, 1, 2], n_rows, CR.SAMPLED if sampled else CR.SEQUENTIAL, CR.cdf_of(PROBABILITIES) if sampled else None,
                           first_row=int(out["row"][idx[0]]), next_pos=-1 if sampled else int(out["scenario"][idx[0]]),
                           draws=out["uniform"][idx][None] if sampled else None)
        for i in idx:
            if out["how"][i] == SET_ID:
                ref.next_pos[0] = out["set_id"][i]
            ref.start(0, 0)
            assert ref.table[0] == out["scenario"][i] and ref.offset[0] == out["row"][i], (phase, i, ref.table[0], out["scenario"][i])
    plain = [int(out["scenario"][i]) for i in starts_at if out["phase"][i] == 0 and out["how"][i] == PLAIN][:6]
    assert plain == [1, 2, 0, 1, 2, 0], plain
    assert len({int(out["scenario"][i]) for i in starts_at if out["how"][i] == SAMPLED}) >= 2
    assert sum(out["how"][starts_at] == SAMPLED) >= 6 and out["terminated"].sum() == 1 and (out["row"][out["how"] == INIT_TS][0] == 2)
    path = os.path.join(HERE, "chronics_cursor_case14.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"chronics_cursor_case14: {len(out['done'])} rows, {len(starts_at)} episodes, scenarios {[int(out['scenario'][i]) for i in starts_at]}, {size} bytes")
    assert size <= MAX_BYTES, "cut steps"


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    reference = os.path.abspath(sys.argv[1])
    for q in (ROOT, os.path.join(ROOT, "tests"), HERE, reference, os.path.join(ROOT, "tests", "_refshim")):
        if q not in sys.path:
            sys.path.insert(0, q)
    os.environ.setdefault("_GRID2OP_FORCE_TEST", "1")
    warnings.filterwarnings("ignore")
    record(reference)


if __name__ == "__main__":
    main()
