"""The opponent of the batched acting path (include/gridpf.h gpf_set_opponent), the parts that need no GPU: the Python restatement
(tests/opponent_ref.py) and the library's rule core compiled with g++ into a host emulator (tests/native/opponent_emul.cpp) reproduce
the episodes recorded from the unmodified reference (tests/golden/opponent_*.npz) exactly; Philox known answers; the draw-to-value table
at its edges; descriptor validation through a header-only handle; ShardedEngine forwarding on the stub engine."""
import subprocess

import numpy as np
import pytest

import opponent_ref as R
from conftest import golden_path
from stub_engine import StubEngine

TAGS = ("neurips36", "wcci118", "case14")
STATE_KEYS = ("budget_is_f32", "attack_duration", "attack_cooldown", "attack_line", "previous_fails", "next_attack_time", "attack_counter")
COLS = {"budget_is_f32": 0, "attack_duration": 1, "attack_cooldown": 2, "attack_line": 3, "previous_fails": 4, "next_attack_time": 5,
        "attack_counter": 6, "n_draws": 8, "info_line": 11, "info_duration": 12}


def fixture_config(fx):
    """the keyword arguments of PowerFlowEngine.set_opponent / OpponentRef / Emulator of a recorded episode (table source)"""
    cfg = dict(kind=int(fx["kind"]), lines=fx["lines"], init_budget=float(fx["space"][0]), budget_per_ts=float(fx["space"][1]),
               attack_duration=int(fx["space_int"][0]), attack_cooldown=int(fx["space_int"][1]), draw_source=R.TABLE)
    if cfg["kind"] == R.WEIGHTED_RANDOM:
        cfg.update(rho_normalization=fx["rho_normalization"], attack_period=int(fx["attack_period"]))
    if cfg["kind"] == R.GEOMETRIC:
        cfg.update(attack_hazard_rate=float(fx["geometric"][0]), recovery_rate=float(fx["geometric"][1]), pmax_pmin_ratio=float(fx["geometric"][2]),
                   recovery_minimum_duration=int(fx["geometric_int"][0]), episode_max_time=int(fx["geometric_int"][1]),
                   schedule_cap=int(fx["schedule"].shape[1]))
    return cfg


@pytest.fixture(scope="module", params=TAGS)
def recorded(request):
    return dict(np.load(golden_path(f"opponent_{request.param}.npz")))


def test_fixtures_leave_the_main_branch():
    fxs = [dict(np.load(golden_path(f"opponent_{t}.npz"))) for t in TAGS]
    assert sorted(int(f["kind"]) for f in fxs) == [1, 2, 3]
    starts = sum(int(((f["info_line"][1:] >= 0) & (f["info_line"][:-1] != f["info_line"][1:])).sum()) for f in fxs)
    assert starts >= 20
    assert sum(int(f["previous_fails"].sum()) for f in fxs) >= 3                    # attacks refused for budget
    assert any(f["done"].any() and f["is_reset"][1:].any() for f in fxs)            # a game over with env.reset()
    assert any((f["budget_is_f32"] == 0).any() and (f["budget_is_f32"][1:] == 1).any() for f in fxs)
    assert any((f["agent_value"] == 1).any() for f in fxs) and any(f["is_illegal"].any() for f in fxs)


def test_restatement_reproduces_the_recorded_episodes(recorded):
    fx = recorded
    cfg = fixture_config(fx)
    ref = R.OpponentRef(draws=fx["draws"], **cfg)
    resets = 0
    for i in range(len(fx["is_reset"])):
        if fx["is_reset"][i]:
            if cfg["kind"] == R.GEOMETRIC:
                n = int(fx["schedule_count"][resets])
                ref.waits, ref.durs = [int(x) for x in fx["schedule"][resets, :n, 0]], [int(x) for x in fx["schedule"][resets, :n, 1]]
            resets += 1
            got = ref.prestep(0, False, None, None)
        else:
            got = ref.prestep(1, False, fx["rho"][i - 1], fx["line_status"][i - 1])
        assert got == (int(fx["info_line"][i]), int(fx["info_duration"][i])), i
        row = ref.row()
        for k in STATE_KEYS + ("n_draws",):
            assert row[COLS[k]] == int(fx[k][i]), (i, k, row[COLS[k]], int(fx[k][i]))
        assert float(ref.budget) == float(fx["budget"][i]), i
    assert ref.flags == 0 and ref.cursor == len(fx["draws"]) and ref.margin >= 1e-4


def test_emulator_reproduces_the_recorded_episodes(recorded, load_model):
    """the library's rule core on 3 lanes, with the recorded effects on the line cooldowns: obs.time_before_cooldown_line of the next
    observation is max(attack duration, cooldown before) - 1 on the attacked line"""
    fx = recorded
    m = load_model(str(fx["grid"]))
    cfg = fixture_config(fx)
    n = 3
    emu = R.Emulator(n, m.n_line, m.line_or_pos_topo_vect, m.line_ex_pos_topo_vect, draws=np.tile(fx["draws"], (n, 1)), **cfg)
    resets = 0
    for i in range(len(fx["is_reset"])):
        reset = bool(fx["is_reset"][i])
        if reset and cfg["kind"] == R.GEOMETRIC:
            k = int(fx["schedule_count"][resets])
            emu.sched[:, :k] = fx["schedule"][resets, :k]
            emu.state[:, 7] = k
        resets += int(reset)
        j = max(i - 1, 0)
        topo = np.tile(fx["topo_vect"][j].astype(np.int32), (n, 1))
        cool = np.tile(fx["cooldown_line"][j].astype(np.int32), (n, 1))
        emu.prestep(np.full(n, 0 if reset else 1), np.zeros(n), np.tile(fx["rho"][j], (n, 1)), np.tile(fx["line_status"][j], (n, 1)), topo, cool)
        for lane in range(n):
            for k in STATE_KEYS + ("n_draws", "info_line", "info_duration"):
                assert emu.state[lane, COLS[k]] == int(fx[k][i]), (i, k)
            assert emu.budget[lane] == float(fx["budget"][i]), i
        line = int(fx["info_line"][i])
        if line >= 0:
            assert topo[0, m.line_or_pos_topo_vect[line]] == -1 and topo[0, m.line_ex_pos_topo_vect[line]] == -1
            if not fx["done"][i]:
                assert not fx["line_status"][i][line] and fx["cooldown_line"][i][line] == cool[0, line] - 1, i
    assert (emu.state[:, 10] == 0).all()


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    assert R.philox4x32_10(ctr, key) == want
    out, u = R.emul_philox(ctr, key)
    assert out == want and u == R.philox_u(want[0], want[1]) and 0.0 <= u < 1.0
    assert R.philox_u(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53 and R.philox_u(0, 0) == 0.0


def _one_step(kind, lines, rho, status, draws, state=None, **kw):
    """one launch of restatement and emulator from a fresh (or given) state on a 4-line grid"""
    n_line = 4
    orp, exp_ = np.arange(n_line) * 2, np.arange(n_line) * 2 + 1
    base = dict(init_budget=10.0, budget_per_ts=0.0, attack_duration=2, attack_cooldown=0, draw_source=R.TABLE)
    base.update(kw)
    ref = R.OpponentRef(kind, lines, draws=draws, **base)
    emu = R.Emulator(1, n_line, orp, exp_, kind, lines, draws=np.asarray(draws)[None], **base)
    ref.prestep(0, False, None, None)
    topo, cool = np.ones((1, 2 * n_line), np.int32), np.zeros((1, n_line), np.int32)
    emu.prestep([0], [0], np.zeros((1, n_line)), np.ones((1, n_line)), topo, cool)
    if state is not None:
        state(ref, emu)
    got = ref.prestep(1, False, np.asarray(rho, np.float32), np.asarray(status, bool))
    emu.prestep([1], [0], np.asarray(rho, np.float32)[None], np.asarray(status, np.uint8)[None], topo, cool)
    assert (int(emu.state[0, 11]), int(emu.state[0, 12])) == got
    assert list(emu.state[0, :13]) == ref.row()[:13] and emu.budget[0] == float(ref.budget)
    return got, ref


def test_draw_to_value_table_at_its_edges():
    below_one = 1.0 - 2.0 ** -53
    # RandomLine among the 3 connected of 4 attackable lines (list order 3, 1, 0, 2; line 0 is out)
    for u, line in ((0.0, 3), (below_one, 2), (0.33, 3), (1.0 / 3.0, 1), (2.0 / 3.0, 2), (0.34, 1)):    # (1/3 * 3 rounds to 1.0)
        assert _one_step(R.RANDOM_LINE, [3, 1, 0, 2], [0.5] * 4, [0, 1, 1, 1], [u])[0] == (line, 2)
    # WeightedRandom: _next_attack_time = 1 + floor(u * attack_period)
    for u, nxt in ((0.0, 0), (below_one, 4), (0.2, 1), (0.39, 1)):        # (0.2 * 5 rounds to 1.0: floor 1; stored after the decrement)
        got, ref = _one_step(R.WEIGHTED_RANDOM, [0, 1, 2], [0.25, 0.25, 0.5, 0.0], [1, 1, 1, 1], [u, 0.1], attack_period=5)
        assert ref.next_time == nxt and (got[0] >= 0) == (nxt == 0)
    # ... and the cdf search: cumulative weights 0.25, 0.5, 1 are exact; a u ON a boundary belongs to the next line (side="right")
    for u, line in ((0.0, 0), (0.25, 1), (0.5, 2), (below_one, 2), (0.2499999, 0)):
        assert _one_step(R.WEIGHTED_RANDOM, [0, 1, 2], [0.25, 0.25, 0.5, 0.0], [1, 1, 1, 1], [0.0, u], attack_period=5)[0] == (line, 2)
    # a disconnected line and a line without flow are never chosen; a sum of 0 is no attack and no draw
    assert _one_step(R.WEIGHTED_RANDOM, [0, 1, 2], [0.0, 0.3, 0.3, 0.0], [1, 0, 1, 1], [0.0, 0.0], attack_period=5)[0] == (2, 2)
    got, ref = _one_step(R.WEIGHTED_RANDOM, [0, 1, 2], [0.0, 0.0, 0.0, 0.0], [1, 1, 1, 1], [0.0, 0.5], attack_period=5)
    assert got == (-1, 0) and ref.cursor == 1
    # Geometric: ranks 0..2 by rho, weights 1, 2, 4 (ratio 4): cumulative 1/7, 3/7, 1 in the order of the list
    sched = dict(attack_hazard_rate=0.5, recovery_rate=0.5, recovery_minimum_duration=1, episode_max_time=50, schedule_cap=4, attack_duration=5)

    def with_schedule(ref, emu):                    # the waiting time of the first attack has run down to its last step
        ref.waits, ref.durs, ref.next_time = [1, 2], [2, 3], 1
        emu.sched[0, :2] = [[1, 2], [2, 3]]
        emu.state[0, 7], emu.state[0, 5] = 2, 1
    for u, line in ((0.0, 1), (0.14, 1), (0.15, 2), (0.42, 2), (0.43, 0), (below_one, 0)):
        got, _ = _one_step(R.GEOMETRIC, [1, 2, 0], [0.9, 0.1, 0.5, 0.0], [1, 1, 1, 1], [u], state=with_schedule, **sched)
        assert got == (line, 2)
    # `~status.all()`: ANY attackable line out gives the attack up, though the counter has moved
    got, ref = _one_step(R.GEOMETRIC, [1, 2, 0], [0.9, 0.1, 0.5, 0.0], [1, 1, 0, 1], [0.5], state=with_schedule, **sched)
    assert got == (-1, 0) and ref.counter == 1 and ref.cursor == 0
    # one attackable line in total: taken without a draw
    got, ref = _one_step(R.GEOMETRIC, [3], [0.9, 0.1, 0.5, 0.2], [1, 1, 1, 1], [], state=with_schedule, **sched)
    assert got == (3, 2) and ref.cursor == 0 and ref.flags == 0
    # a table that has run out: no attack, sticky flag
    got, ref = _one_step(R.RANDOM_LINE, [0, 1], [0.5] * 4, [1, 1, 1, 1], [])
    assert got == (-1, 0) and ref.flags == R.FLAG_DRAWS_EXHAUSTED
    # the schedule's inversion: max(1, ceil(log1p(-u) / log1p(-p)))
    assert [R.geometric(u, 0.25) for u in (0.0, 0.2, 0.25, 0.26, below_one)] == [1, 1, 1, 2, 128]


def test_budget_arithmetic_is_numpys():
    """float32 until the first paid attack step, float64 from then on, float32 again after a reset"""
    got, ref = _one_step(R.RANDOM_LINE, [0], [0.5] * 4, [1, 1, 1, 1], [0.5], init_budget=2.3, budget_per_ts=0.1)
    assert got == (0, 2) and ref.budget.dtype == np.float64 and float(ref.budget) == float(np.float32(2.3) + np.float32(0.1)) - 1.0
    ref.prestep(1, False, np.zeros(4, np.float32), np.ones(4, bool))
    assert float(ref.budget) == float(np.float64(np.float32(2.3) + np.float32(0.1)) - 1.0 + np.float32(0.1) - 1.0)
    ref.prestep(0, False, None, None)
    assert ref.budget.dtype == np.float32 and ref.episode == 2


def test_sanitized_stand_alone_emulator_runs_clean():
    p = subprocess.run([R.sanitized_program()], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK") and not p.stderr, (p.stdout, p.stderr[-2000:])


GOOD = dict(kind=R.GEOMETRIC, lines=[0, 1, 2], init_budget=1.0, budget_per_ts=0.1, attack_duration=3, attack_cooldown=2, attack_hazard_rate=0.1,
            recovery_rate=0.2, recovery_minimum_duration=1, pmax_pmin_ratio=4.0, episode_max_time=100, schedule_cap=8, draw_source=R.PHILOX)
BAD = [(dict(kind=7), "unknown opponent kind"), (dict(lines=[]), "no attackable line"), (dict(lines=[0, 99]), r"outside \[0, n_line"),
       (dict(lines=[0, -1]), r"outside \[0, n_line"), (dict(lines=[1, 1]), "listed twice"), (dict(init_budget=-0.5), "positive \\(or null\\) budget"),
       (dict(budget_per_ts=float("nan")), "budget_per_ts"), (dict(attack_duration=-1), "must not be negative"),
       (dict(attack_cooldown=-1), "must not be negative"), (dict(draw_source=5), "unknown draw source"), (dict(lane_base=-1), "lane_base"),
       (dict(kind=R.WEIGHTED_RANDOM, attack_period=0), "attack_period needs to be > 0"),
       (dict(kind=R.WEIGHTED_RANDOM, rho_normalization=[1.0, 0.0, 1.0]), r"rho_normalization\[1\]"),
       (dict(recovery_rate=0.0), "recovery_rate"), (dict(recovery_rate=1.5), "recovery_rate"), (dict(attack_hazard_rate=-1.0), "attack_hazard_rate"),
       (dict(recovery_minimum_duration=-1), "recovery_minimum_duration"), (dict(pmax_pmin_ratio=0.0), "pmax_pmin_ratio"),
       (dict(episode_max_time=0), "finite episode duration"), (dict(episode_max_time=2 ** 31 - 1), "finite episode duration"),
       (dict(schedule_cap=0), "schedule_cap")]


def test_descriptor_validation_before_the_device_is_touched(load_model):
    """every bad field is refused with its reason on a header-only handle; a good descriptor gets as far as the missing device"""
    from grid2op_amd.engine import GridPFError, PowerFlowEngine
    eng = PowerFlowEngine(load_model("l2rpn_case14_sandbox"), n_lanes=4, device=-1)
    for change, reason in BAD:
        with pytest.raises(GridPFError, match=reason):
            eng.set_opponent(**dict(GOOD, **change))
    for kind in (R.RANDOM_LINE, R.WEIGHTED_RANDOM, R.GEOMETRIC):
        with pytest.raises(GridPFError, match="no HIP device"):
            eng.set_opponent(**dict(GOOD, kind=kind))
    eng.set_opponent(None)                                                          # off needs no device
    with pytest.raises(GridPFError, match="no opponent"):
        eng.opponent_state()
    with pytest.raises(ValueError, match="one entry per attackable line"):
        eng.set_opponent(**dict(GOOD, kind=R.WEIGHTED_RANDOM, rho_normalization=[1.0]))
    eng.close()


def test_opponent_config_from_a_reference_style_configuration(load_model):
    from grid2op_amd.engine import OPP_GEOMETRIC, OPP_WEIGHTED_RANDOM, opponent_config
    m = load_model("l2rpn_wcci_2022_dev")
    names = [str(m.name_line[i]) for i in (106, 93, 88)]
    c = opponent_config(m, "GeometricOpponent", dict(lines_attacked=names, attack_every_xxx_hour=24, average_attack_duration_hour=4,
                                                      minimum_attack_duration_hour=1), 144.0, 0.17, 96, 12, max_episode_duration=2016, seed=5)
    assert c["kind"] == OPP_GEOMETRIC and c["lines"] == [106, 93, 88] and c["recovery_minimum_duration"] == 12
    assert c["attack_hazard_rate"] == 1.0 / (12.0 * 20) and c["recovery_rate"] == 1.0 / (12.0 * 3) and c["episode_max_time"] == 2016
    assert c["schedule_cap"] >= 4 * 2016 / 240 and c["attack_duration"] == 96 and c["attack_cooldown"] == 12

    class WeightedRandomOpponent:                                                   # the class itself works like its name
        pass
    w = opponent_config(m, WeightedRandomOpponent, dict(lines_attacked=names, rho_normalization=[0.4, 0.5, 0.6], attack_period=288), 144.0, 0.16667, 48, 288)
    assert w["kind"] == OPP_WEIGHTED_RANDOM and w["rho_normalization"] == [0.4, 0.5, 0.6] and w["attack_period"] == 288
    for kw, reason in ((dict(average_attack_duration_hour=1, minimum_attack_duration_hour=2), "cannot be lower"),
                       (dict(average_attack_duration_hour=2, minimum_attack_duration_hour=2), "not supported"),
                       (dict(attack_every_xxx_hour=3, average_attack_duration_hour=4), "attack_every_xxx_hour <= average"),
                       (dict(lines_attacked=["nope"]), "unable to find the powerline")):
        with pytest.raises(ValueError, match=reason):
            opponent_config(m, "GeometricOpponent", dict(dict(lines_attacked=names), **kw), max_episode_duration=100)
    with pytest.raises(ValueError, match="finite episode duration"):
        opponent_config(m, "GeometricOpponent", dict(lines_attacked=names))
    with pytest.raises(ValueError, match="single-area line opponents"):
        opponent_config(m, "GeometricOpponentMultiArea", dict(lines_attacked=names))


class _OppStub(StubEngine):
    def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
        super().__init__(model, n_lanes, device, n_busbar)
        self.calls, self.n_lanes_ = [], n_lanes

    def set_opponent(self, kind=0, lines=(), **kw):
        self.calls.append(("set", kind, tuple(lines), kw))

    def upload_opponent_draws(self, draws):
        self.calls.append(("draws", np.array(draws)))

    def upload_opponent_schedule(self, schedule, count):
        self.calls.append(("schedule", np.array(schedule), np.array(count)))

    def opponent_state(self, lane0=0, n=None):
        from grid2op_amd.engine import OPP_STATE_INTS, OpponentState
        n = self.n_lanes_ - lane0 if n is None else n
        rows = np.zeros((n, OPP_STATE_INTS), np.int32)
        rows[:, 8] = 1000 * self.device + lane0 + np.arange(n)
        return OpponentState.from_rows(np.full(n, float(self.device)), rows)

    def set_opponent_state(self, state, lane0=0):
        self.calls.append(("state", lane0, state.budget.copy(), state.rows()))


def test_sharded_engine_forwards_the_opponent(load_model):
    from grid2op_amd.engine import OPP_STATE_INTS, OpponentState
    from grid2op_amd.sharding import ShardedEngine
    m = load_model("l2rpn_case14_sandbox")
    se = ShardedEngine(m, 10, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: _OppStub(mm, n, dev, nbb))
    bases = [b0 for b0, _ in se.blocks]
    se.set_opponent(2, [1, 2], seed=9, attack_period=4)
    assert [e.calls[-1] for e in se.engines] == [("set", 2, (1, 2), dict(seed=9, attack_period=4, lane_base=b)) for b in bases]
    se.set_opponent(2, [1, 2], lane_base=100)
    assert [e.calls[-1][3]["lane_base"] for e in se.engines] == [100 + b for b in bases]
    draws = np.arange(30.0).reshape(10, 3)
    se.upload_opponent_draws(draws)
    sch, cnt = np.arange(10 * 2 * 2).reshape(10, 2, 2), np.arange(10)
    se.upload_opponent_schedule(sch, cnt)
    for e, (b0, bn) in zip(se.engines, se.blocks):
        assert np.array_equal(e.calls[-2][1], draws[b0:b0 + bn])
        assert np.array_equal(e.calls[-1][1], sch[b0:b0 + bn]) and np.array_equal(e.calls[-1][2], cnt[b0:b0 + bn])
    st = se.opponent_state(2, 7)
    want = np.concatenate([1000 * e.device + np.arange(bn) for e, (_, bn) in zip(se.engines, se.blocks)])[2:9]
    assert np.array_equal(st.cursor, want) and len(st.budget) == 7
    rows = np.zeros((10, OPP_STATE_INTS), np.int32)
    rows[:, 1] = np.arange(10)
    se.set_opponent_state(OpponentState.from_rows(np.arange(10.0), rows))
    for e, (b0, bn) in zip(se.engines, se.blocks):
        tag, lane0, bud, r = e.calls[-1]
        assert tag == "state" and lane0 == 0 and np.array_equal(bud, np.arange(10.0)[b0:b0 + bn]) and np.array_equal(r[:, 1], np.arange(b0, b0 + bn))
    se.set_opponent(None)
    assert all(e.calls[-1][:2] == ("set", None) for e in se.engines)


@pytest.mark.parametrize("kind", [R.RANDOM_LINE, R.WEIGHTED_RANDOM, R.GEOMETRIC])
@pytest.mark.parametrize("n_att", [1, 70])
def test_emulator_on_random_observations_equals_the_restatement(kind, n_att):
    """Philox source, schedules sampled by the rule core itself, random rho / outages / game overs on 9 lanes x 120 launches of a
    75-line grid (more than one stride of 64 attackable lines)"""
    rng = np.random.default_rng(17 + kind)
    n, n_line, steps = 9, 75, 120
    orp, exp_ = np.arange(n_line) * 2, np.arange(n_line) * 2 + 1
    lines = rng.permutation(n_line)[:n_att]
    cfg = dict(init_budget=3.0, budget_per_ts=0.5, attack_duration=3, attack_cooldown=4, attack_period=3, attack_hazard_rate=0.3, recovery_rate=0.5,
               recovery_minimum_duration=1, pmax_pmin_ratio=4.0, episode_max_time=40, schedule_cap=5, draw_source=R.PHILOX, seed=0xABCDEF0123456789,
               rho_normalization=0.5 + rng.random(n_att))
    emu = R.Emulator(n, n_line, orp, exp_, kind, lines, lane_base=500, **cfg)
    refs = [R.OpponentRef(kind, lines, global_lane=500 + k, **cfg) for k in range(n)]
    topo, cool = np.ones((n, 2 * n_line), np.int32), np.zeros((n, n_line), np.int32)
    survived, attacked = np.zeros(n, np.int32), 0
    for t in range(steps):
        status = (topo[:, orp] > 0) & (topo[:, exp_] > 0)
        rho = np.where(status, rng.random((n, n_line)), 0.0).astype(np.float32)
        done = (rng.random(n) < 0.02) & (survived > 0)
        want_topo, want_cool = topo.copy(), cool.copy()
        for k in range(n):
            line, dur = refs[k].prestep(int(survived[k]), bool(done[k]), rho[k], status[k])
            if survived[k] > 0 and not done[k]:
                R.apply_attack(line, dur, want_topo[k], want_cool[k], orp, exp_)
                attacked += int(line >= 0)
        emu.prestep(survived, done, rho, status, topo, cool)
        assert np.array_equal(emu.state[:, :13], np.array([r.row()[:13] for r in refs])), t
        assert np.array_equal(emu.budget, np.array([float(r.budget) for r in refs])), t
        assert np.array_equal(topo, want_topo) and np.array_equal(cool, want_cool), t
        cool[:] = np.maximum(cool - 1, 0)
        back = (cool == 0) & ~((topo[:, orp] > 0) & (topo[:, exp_] > 0)) & (rng.random((n, n_line)) < 0.7)
        topo[:, orp] = np.where(back, 1, topo[:, orp])
        topo[:, exp_] = np.where(back, 1, topo[:, exp_])
        survived = np.where(rng.random(n) < 0.03, 0, survived + 1).astype(np.int32)
    assert min(r.margin for r in refs) > 1e-9 and attacked >= 3 * n
    if kind == R.GEOMETRIC:
        assert any(r.flags & R.FLAG_SCHEDULE_CAPPED for r in refs)
