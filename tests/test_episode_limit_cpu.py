"""Episode time limits of the batched acting path (include/gridpf.h gpf_set_episode_limit), the parts that need no GPU: the numpy
restatement (tests/episode_ref.py) against the episodes recorded from the unmodified reference (tests/golden/episode_limit_*.npz) -- flags
and lengths exactly, rewards within the bounds of tests/reward_ref.py, EpisodeDurationReward at one float32 spacing, the alert bonus
exactly --, the library's rules compiled with g++ (tests/native/episode_emul.cpp) against the restatement, the defaulted `truncated`
parameter against the six-argument call, every refusal through a header-only handle, the exported symbols and the routing of
`ShardedEngine`."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import alert_ref as AR
import episode_ref as E
import reward_ref as R
from conftest import golden_path

TAGS = ("case14", "storage")
SLOTS = [(R.REDISP, [5.0, 1.0e5, -10.0, 0.25, 300.0 / 3600.0]), (R.L2RPN, []), (R.LINES_CAPACITY, []),
         (R.ECONOMIC, [5.0e4, -0.5, 1.5, 300.0 / 3600.0]), (R.GAMEPLAY, [-1.0, 1.0])]


@pytest.fixture(scope="module", params=TAGS)
def recorded(request):
    return dict(np.load(golden_path(f"episode_limit_{request.param}.npz")))


@pytest.fixture(scope="module")
def recorded_alert():
    return dict(np.load(golden_path("episode_limit_alert_case14.npz")))


def _steps(fx):
    return [i for i in range(len(fx["done"])) if not fx["is_reset"][i]]


def _episodes(fx):
    """(step rows of one episode) lists: an episode ends at a done row"""
    out, cur = [], []
    for i in _steps(fx):
        cur.append(i)
        if fx["done"][i]:
            out.append(cur)
            cur = []
    assert not cur
    return out


def test_fixtures_cover_the_cases():
    c, s, a = (dict(np.load(golden_path(f"episode_limit_{k}.npz"))) for k in ("case14", "storage", "alert_case14"))
    tr, te = c["truncated"].astype(bool), c["terminated"].astype(bool)
    ill, amb = c["is_illegal"].astype(bool), c["is_ambiguous"].astype(bool)
    assert (tr & ~ill & ~amb).sum() >= 1 and (tr & ill).sum() >= 1 and (tr & amb).sum() >= 1
    assert (te & (c["nb_time_step"] == c["max_step"])).sum() >= 1 and (te & (c["nb_time_step"] < c["max_step"])).sum() >= 1
    assert set(int(x) for x in c["max_step"]) == {1, 2, 5, 12} and (tr & (c["max_step"] == 1)).sum() >= 1
    assert not (tr & te).any() and np.array_equal(tr | te, c["done"].astype(bool))
    assert s["truncated"].sum() == 2 and not s["terminated"].any() and set(int(x) for x in s["max_step"]) == {6}
    n = len(s["done"]) // 2
    assert np.array_equal(s["row"][:n], s["row"][n:]) and np.abs(s["actual_dispatch"][n - 1]).sum() > 0
    # the second episode restarts: its first step's dispatch is its own action's, not the first episode's last
    assert np.abs(s["target_dispatch"][n] - s["act_redisp"][n]).max() < 1e-5 and np.abs(s["target_dispatch"][n - 1] - s["act_redisp"][n - 1]).max() > 1e-3
    assert a["truncated"].sum() == 2 and a["terminated"].sum() == 1
    W = int(a["time_window"])
    since = a["env_time_since_last_attack"][a["truncated"].astype(bool)].astype(int)
    in_window = [bool(((r >= 0) & (r <= W)).any()) for r in since]
    assert sorted(in_window) == [False, True]


def test_restatement_flags_lengths_and_duration_reward(recorded):
    """the restatement driven by the recorded failures alone gives the recorded truncated flag, nb_time_step and EpisodeDurationReward"""
    fx = recorded
    for ep in _episodes(fx):
        ref = E.EpisodeRef()
        N = int(fx["max_step"][ep[0]])
        for t, i in enumerate(ep, 1):
            failed = bool(fx["terminated"][i])
            ref.poststep(t - 1 if failed else t, N, failed)
            assert ref.terminated == failed and ref.truncated == bool(fx["truncated"][i]), i
            assert ref.length == (int(fx["nb_time_step"][i]) if fx["done"][i] else 0), i
            got = np.float32(fx["reward_episode_duration"][i])
            assert abs(float(got) - float(ref.duration_reward)) <= float(np.spacing(np.float32(abs(ref.duration_reward)))), (i, got, ref.duration_reward)
            assert (ref.duration_reward != 0) == bool(fx["done"][i])
        assert ref.n_episodes == 1 and ref.length_last == int(fx["nb_time_step"][ep[-1]])


def test_restatement_rewards_against_the_recorded_reference(recorded):
    """every step, every slot, with is_done = failed or truncated where the reference reads it; the constant branches are exact"""
    fx = recorded
    slots = R.fixture_slots(fx)
    n_cmp = n_trunc_const = 0
    for i in _steps(fx):
        row, tr, got = E.fixture_row(fx, i), bool(fx["truncated"][i]), R.fixture_rewards(fx, i)
        for s, (kind, p) in enumerate(slots):
            want = E.value(kind, p, trunc=tr, **row)
            if E.constant_branch(kind, row["failed"], row["illegal"], row["ambiguous"], tr):
                assert want.tobytes() == got[s].tobytes(), (i, s, want, got[s])
                n_trunc_const += int(tr)
            else:
                b = R.bound(kind, p, **row)
                assert abs(float(got[s]) - float(want)) <= b, (i, s, float(got[s]), float(want), b)
                n_cmp += 1
    assert n_cmp >= 20 and n_trunc_const >= 2
    if str(fx["grid"]) == "l2rpn_case14_sandbox":            # the flag matters: without it the truncated steps miss the recording
        miss = 0
        for i in _steps(fx):
            if fx["truncated"][i]:
                row, got = E.fixture_row(fx, i), R.fixture_rewards(fx, i)
                miss += int(abs(float(R.value(R.L2RPN, [], **row)) - float(got[1])) > 1.0)
        assert miss >= 3


def _check_emulator(slots, row, trunc):
    got, want = E.emul_reward_lane(slots, trunc, **row), E.lane_values(slots, trunc=trunc, **row)
    assert R.spacing_ok(got, want).all(), (got, want)
    for s, (kind, _) in enumerate(slots):
        if E.constant_branch(kind, row["failed"], row["illegal"], row["ambiguous"], trunc):
            assert got[s].tobytes() == want[s].tobytes(), (s, got[s], want[s])


def test_emulator_equals_the_restatement_on_the_recorded_episodes(recorded):
    fx = recorded
    slots = R.fixture_slots(fx)
    for i in _steps(fx):
        _check_emulator(slots, E.fixture_row(fx, i), bool(fx["truncated"][i]))


def test_emulator_default_is_the_six_argument_call(recorded):
    """reward_value(..., truncated = false) and the call without the parameter: bit for bit on every recorded row, and the six-argument
    emulator of the rewards' own tests gives the same bits"""
    fx = recorded
    slots = R.fixture_slots(fx)
    for i in _steps(fx):
        row = E.fixture_row(fx, i)
        six, seven, old = E.emul_reward_lane(slots, None, **row), E.emul_reward_lane(slots, False, **row), R.emul_lane(slots, **row)
        assert six.tobytes() == seven.tobytes() == old.tobytes(), i


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_emulator_equals_the_restatement_on_seeded_rows(n):
    from test_reward_cpu import synthetic_row
    rng = np.random.default_rng(900 + n)
    for rep in range(4):
        row = synthetic_row(rng, n, n_sto=n if rep % 2 else 0, dispatch=rep % 3 != 0)
        for f in range(16):
            _check_emulator(SLOTS, dict(row, failed=bool(f & 1), illegal=bool(f & 2), ambiguous=bool(f & 4)), bool(f & 8))


@pytest.mark.parametrize("n_slot", [1, 8])
def test_emulator_returns_are_a_sequential_float64_sum(n_slot):
    """lanes with limits 0 .. 6, failures every 7th launch: the emulator's flags, lengths and duration rewards equal the restatement's, its
    returns equal the restatement's and a plain sequential numpy float64 sum of the float32 rewards, bit for bit"""
    rng = np.random.default_rng(40 + n_slot)
    for limit in range(7):
        st, ref = E.Stats(), E.EpisodeRef(n_slot, per_timestep=0.5)
        acc, steps, last = np.zeros(n_slot, np.float64), 0, None
        for t in range(1, 60):
            failed = t % 7 == 0
            steps = steps if failed else steps + 1
            rw = (rng.uniform(-1e3, 1e3, n_slot) * 10.0 ** rng.integers(-6, 3, n_slot)).astype(np.float32)
            for s in range(n_slot):
                acc[s] = acc[s] + np.float64(rw[s])
            after = 0 if failed else steps                     # (auto_reset: a failed lane restarts inside the launch)
            fresh, lane = E.emul_poststep(st, after, limit, failed, 0.5, rw)
            assert fresh == ref.poststep(after, limit, failed, rw)
            assert (lane.terminated, lane.truncated, lane.length) == (int(ref.terminated), int(ref.truncated), ref.length), (limit, t)
            assert np.float32(lane.duration_reward).tobytes() == ref.duration_reward.tobytes()
            assert E.emul_truncated(after, limit, failed) == ref.truncated == E.truncated(after, limit, failed)
            if fresh:
                last, acc = acc.copy(), np.zeros(n_slot, np.float64)
                if not failed:                                 # (auto_reset: a truncated lane restarts too)
                    steps = st.steps_prev = ref.steps_prev = 0
            assert np.array(st.running[:n_slot]).tobytes() == acc.tobytes() == ref.running.tobytes(), (limit, t)
            if last is not None:
                assert np.array(st.last[:n_slot]).tobytes() == last.tobytes() == ref.last.tobytes(), (limit, t)
            assert st.n_episodes == ref.n_episodes and st.length_last == ref.length_last
        assert ref.n_episodes >= 8


def test_a_truncated_lane_left_alone_reflags_and_rolls_over_once():
    st, ref = E.Stats(), E.EpisodeRef(1)
    for t in range(1, 8):
        fresh, lane = E.emul_poststep(st, t, 3, False, 1.0, np.ones(1, np.float32))
        assert fresh == ref.poststep(t, 3, False, np.ones(1, np.float32)) == (t == 3)
        assert lane.truncated == int(t >= 3) and lane.length == (t if t >= 3 else 0)
    assert st.n_episodes == 1 and st.length_last == 3 and st.last[0] == 3.0 and st.running[0] == 4.0


class _AlertLane:
    """one lane of the library's alert rules with an episode limit (tests/native/episode_emul.cpp)"""

    def __init__(self, A, W, consts, bonus):
        self.A, self.W, self.bonus = A, W, float(bonus)
        self.c = (C.c_float * 4)(*[float(x) for x in consts])
        self.ob, self.ax = np.zeros(6 * A + 1, np.int32), np.zeros(3 + 2 * (W + 2), np.uint64)

    def launch(self, steps_before, raise_mask, att_mask, limit, failed):
        return np.float32(E.emul_lib().episode_emul_alert_poststep(
            C.c_int(self.A), C.c_int(self.W), self.c, self.ob.ctypes.data_as(C.c_void_p), self.ax.ctypes.data_as(C.c_void_p), C.c_int(steps_before),
            C.c_int(0), C.c_uint64(raise_mask), C.c_uint64(att_mask), C.c_int(limit), C.c_int(int(failed)), C.c_float(self.bonus)))

    def obs(self):
        A, o = self.A, self.ob
        return dict(active_alert=o[:A], time_since_last_alert=o[A:2 * A], alert_duration=o[2 * A:3 * A], time_since_last_attack=o[3 * A:4 * A],
                    attack_under_alert=o[4 * A:5 * A], was_alert_used_after_attack=o[5 * A:6 * A], total_number_of_alert=o[6 * A:])


def test_alert_bonus_and_attributes_of_a_truncated_step(recorded_alert):
    """The recorded alert scenario launch by launch through the library's rules: the reward equals the recording exactly -- the configured
    reward_end_episode_bonus on the two truncated steps --, and so do the seven alert attributes of every observation but a game over's.
    The reset observation takes a launch here (the opponent and the alerts expect one), so the limit is max step + 1."""
    fx = recorded_alert
    lines = [int(x) for x in fx["lines"]]
    A, W = len(lines), int(fx["time_window"])
    bonus = float(fx["reward_end_episode_bonus"])
    lane = _AlertLane(A, W, fx["reward_constants"], bonus)
    steps, n_trunc, kept = 0, 0, 0
    for i in range(len(fx["is_reset"])):
        if fx["is_reset"][i]:
            steps = 0
        limit = int(fx["max_step"][i]) + 1
        failed = bool(fx["terminated"][i])
        r = lane.launch(steps, AR.mask_of(fx["alert_mask"][i]), AR.mask_of(fx["info_lines"][i][lines]), limit, failed)
        steps = steps if failed else steps + 1
        trunc = E.truncated(steps, limit, failed)
        assert trunc == bool(fx["truncated"][i]), i
        assert r.tobytes() == np.float32(fx["alert_reward"][i]).tobytes(), (i, r, fx["alert_reward"][i])
        if trunc:
            assert float(r) == bonus
            n_trunc += 1
            kept += int(np.any(fx["obs_was_alert_used_after_attack"][i] != 0))
        if not failed:
            for k, v in lane.obs().items():
                assert np.array_equal(v, np.asarray(fx["obs_" + k][i]).reshape(-1).astype(np.int32)), (i, k, v, fx["obs_" + k][i])
    assert n_trunc == 2 and kept >= 1


def test_every_refusal_on_a_header_only_handle(load_model):
    from grid2op_amd import _capi
    from grid2op_amd.engine import GridPFError, PowerFlowEngine
    m = load_model("l2rpn_case14_sandbox")
    eng = PowerFlowEngine(m, n_lanes=4, device=-1)
    for fn in (eng.episode_ends, eng.episode_stats, eng.episode_views):
        with pytest.raises(GridPFError, match="episode limits are off"):
            fn()
    L = eng._lib
    for rc in (L.gpf_get_episode_ends(eng._h, 0, 1, None, None, None, None), L.gpf_get_episode_stats(eng._h, 0, 1, None, None, None, None),
               L.gpf_episode_device_pointers(eng._h, (C.c_void_p * _capi.N_EPISODE_POINTERS)(), _capi.N_EPISODE_POINTERS)):
        assert rc != 0 and b"episode limits are off" in L.gpf_last_error()
    with pytest.raises(GridPFError, match="negative max_steps"):
        eng.set_episode_limit(-1)
    with pytest.raises(GridPFError, match="lane 2: negative limit"):
        eng.set_episode_limit([3, 0, -4, 1])
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        with pytest.raises(GridPFError, match="per_timestep must be finite and positive"):
            eng.set_episode_limit(5, per_timestep=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(GridPFError, match="alert_end_bonus is not finite"):
            eng.set_episode_limit(5, alert_end_bonus=bad)
    eng.set_episode_limit(None)                                           # off is always possible
    eng.set_episode_limit(0)
    opts = _capi.GpfStepOpts(max_iter=10, tol_mva=1e-4)
    assert L.gpf_step_n(eng._h, 0, 3, C.byref(opts)) != 0 and b"episode limit" not in L.gpf_last_error()     # off: another refusal (no chronics)
    with pytest.raises(GridPFError, match="no HIP device"):               # a good call gets as far as the missing device
        eng.set_episode_limit(5, per_timestep=2.0, alert_end_bonus=1.0)
    with pytest.raises(GridPFError, match="no HIP device"):
        eng.set_episode_limit([1, 0, 2, 3])
    with pytest.raises(GridPFError, match="episode limits are off"):      # ... and leaves the getters refusing
        eng.episode_ends()
    # a multi-step launch while a limit is set: the message has the opponent's form
    assert L.gpf_step_n(eng._h, 0, 3, C.byref(opts)) != 0
    msg = L.gpf_last_error().decode()
    assert msg.startswith("gpf_step_n: with an episode limit set (gpf_set_episode_limit) a launch must be a one-step launch") and msg.endswith("use n_steps = 1")
    eng.set_episode_limit(None)
    assert L.gpf_step_n(eng._h, 0, 3, C.byref(opts)) != 0 and b"episode limit" not in L.gpf_last_error()
    eng.close()


def test_exported_symbols_and_constants():
    from grid2op_amd import _capi, engine
    names = ("gpf_set_episode_limit", "gpf_get_episode_ends", "gpf_get_episode_stats", "gpf_episode_device_pointers")
    assert all(n in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), n) for n in names)
    assert _capi.ABI_VERSION == 326 and _capi.N_DEVICE_POINTERS == 34 and _capi.N_EPISODE_POINTERS == 8 and engine.REWARD_MAX_SLOTS == E.MAX_SLOTS == 8
    assert C.sizeof(_capi.GpfEpisodeDesc) == 24 and _capi.GpfEpisodeDesc.lane_max_steps.offset == 8 and _capi.GpfEpisodeDesc.alert_end_bonus.offset == 20
    hdr = open(golden_path("../../include/gridpf.h")).read()
    assert "#define GPF_N_EPISODE_POINTERS 8" in hdr and "#define GPF_ABI_VERSION 326" in hdr
    assert engine.alert_end_bonus() == 1.0 and engine.alert_end_bonus(type("R", (), {"reward_end_episode_bonus": np.float32(2.5)})()) == 2.5


def test_sharded_engine_forwards_the_episode_limits(load_model):
    from stub_engine import StubEngine
    from grid2op_amd.sharding import ShardedEngine

    class Stub(StubEngine):
        def __init__(self, model, n_lanes=1, device=0, n_busbar=2):
            super().__init__(model, n_lanes, device, n_busbar)
            self.calls, self.n_lanes_ = [], n_lanes

        def set_episode_limit(self, max_steps, per_timestep=1.0, alert_end_bonus=0.0):
            self.calls.append((max_steps, per_timestep, alert_end_bonus))

        def _ids(self, lane0, n):
            n = self.n_lanes_ - lane0 if n is None else n
            return 1000 * self.device + lane0 + np.arange(n)

        def episode_ends(self, lane0=0, n=None):
            ids = self._ids(lane0, n)
            return dict(terminated=ids % 2 == 0, truncated=ids % 2 == 1, length=ids.astype(np.int32), duration_reward=ids.astype(np.float32))

        def episode_stats(self, lane0=0, n=None):
            ids = self._ids(lane0, n)
            return dict(return_running=np.tile(ids[:, None], (1, 2)).astype(np.float64), return_last=np.tile(-ids[:, None], (1, 2)).astype(np.float64),
                        length_last=ids.astype(np.int32), n_episodes=(ids + 1).astype(np.int32))

        def episode_views(self):
            return {"limit": self.device}

    m = load_model("l2rpn_case14_sandbox")
    se = ShardedEngine(m, 10, devices=[0, 1, 2], engine_factory=lambda mm, n, dev, nbb: Stub(mm, n, dev, nbb))
    se.set_episode_limit(7, 2.0, 1.5)
    assert all(e.calls[-1] == (7, 2.0, 1.5) for e in se.engines)
    se.set_episode_limit(None)
    assert all(e.calls[-1][0] is None for e in se.engines)
    lim = np.arange(10) + 3
    se.set_episode_limit(lim, alert_end_bonus=1.0)
    for e, (b0, bn) in zip(se.engines, se.blocks):                        # per-lane limits are cut by lane
        assert np.array_equal(e.calls[-1][0], lim[b0:b0 + bn]) and e.calls[-1][1:] == (1.0, 1.0)
    want = np.concatenate([1000 * e.device + np.arange(bn) for e, (_, bn) in zip(se.engines, se.blocks)])
    ends, stats = se.episode_ends(2, 7), se.episode_stats(2, 7)
    assert np.array_equal(ends["length"], want[2:9]) and np.array_equal(ends["truncated"], want[2:9] % 2 == 1) and ends["duration_reward"].dtype == np.float32
    assert np.array_equal(stats["return_last"][:, 1], -want[2:9]) and np.array_equal(stats["n_episodes"], want[2:9] + 1)
    assert se.episode_stats()["return_running"].shape == (10, 2)
    assert se.episode_views() == [{"limit": e.device} for e in se.engines]


def test_sanitized_stand_alone_episode_emulator_runs_clean():
    p = subprocess.run([E.sanitized_program()], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK") and not p.stderr, (p.stdout, p.stderr[-2000:])
