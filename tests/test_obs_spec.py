"""CPU checks of the observation-vector layout (grid2op_amd/obs_spec.py) and of its numpy restatement (tests/obs_ref.py) against
the vectors the reference recorded on rte_case5_example (tests/golden/obsvec_runner_case5.npz, made by make_obsvec_fixtures.py)."""
import datetime as dt
import json

import numpy as np
import pytest

import obs_ref
from conftest import golden_path
from grid2op_amd.obs_spec import ATTR_TABLE, KIND, ObsSpec, check_segments, out_offsets

# rte_case5_example/prods_charac.csv: Pmin, Pmax, max_ramp_up, max_ramp_down; gen_0_0 is a wind farm
CASE5_LIMITS = ([0.0, 0.0], [10.0, 30.0], [0.0, 10.0], [0.0, 10.0])
CASE5_RENEWABLE = [True, False]


def _fixture():
    return np.load(golden_path("obsvec_runner_case5.npz"))


def test_complete_spec_has_the_width_of_the_recorded_vectors(load_model):
    m = load_model("rte_case5_example")
    spec = ObsSpec.complete(m, fill=True)
    fx = _fixture()
    assert spec.dim == fx["vectors"].shape[1] == 192
    assert len(spec.segments) <= 64 and spec.segments.dtype == np.int32 and spec.segments.shape[1] == 5
    assert spec.subtract.shape == spec.divide.shape == (192,) and spec.subtract.dtype == np.float32
    assert not spec.subtract.any() and (spec.divide == 1).all()
    for grid in ("l2rpn_case14_sandbox", "l2rpn_wcci_2022_dev", "l2rpn_neurips_2020_track1"):
        ObsSpec.complete(load_model(grid), fill=True)            # every grid's layout fits the segment table


def test_offsets_follow_the_committed_name_list(load_model):
    m = load_model("rte_case5_example")
    with open(golden_path("obs_attr_list.json")) as f:
        doc = json.load(f)
    listed = [(d["name"], d["size"], d["dtype"], d["fill"]) for d in doc["attr_list_vect"]]
    assert listed == [tuple(a) for a in ATTR_TABLE]
    assert len(listed) == 67 and listed[0][0] == "year" and listed[-1][0] == "timestep_protection_engaged"
    sizes = dict(one=1, n_gen=m.n_gen, n_load=m.n_load, n_line=m.n_line, n_sub=m.n_sub, dim_topo=m.dim_topo, n_storage=m.n_storage,
                 n_shunt=m.n_shunt)
    spec = ObsSpec.complete(m, fill=False)
    pos = 0
    for name, rule, _, fill in listed:
        if fill is None and sizes.get(rule, 0):
            assert spec.offsets[name] == slice(pos, pos + sizes[rule]), name
            pos += sizes[rule]
    assert spec.dim == pos
    full = ObsSpec.complete(m, fill=True)
    pos = 0
    for name, rule, _, fill in listed:                          # the engine's attributes sit where the reference has them
        if fill is None and sizes.get(rule, 0):
            assert full.offsets[name].start == pos, name
        pos += sizes.get(rule, 0)
    assert pos == 192


def test_custom_order_and_affine_broadcasting(load_model):
    m = load_model("l2rpn_case14_sandbox")
    scale = np.linspace(1.0, 2.0, m.n_line).astype(np.float32)
    spec = ObsSpec(m, ["rho", ("const", 3, 2.5), "gen_p", "thermal_limit", "hour_of_day"], subtract={"gen_p": 10.0, "const0": 0.5},
                   divide={"rho": scale, "gen_p": 100})
    assert spec.names == ["rho", "const0", "gen_p", "thermal_limit", "hour_of_day"]
    assert spec.dim == 2 * m.n_line + 3 + m.n_gen + 1
    assert spec.offsets["gen_p"] == slice(m.n_line + 3, m.n_line + 3 + m.n_gen)
    assert np.array_equal(spec.divide[spec.offsets["rho"]], scale) and (spec.divide[spec.offsets["gen_p"]] == 100).all()
    assert (spec.subtract[spec.offsets["gen_p"]] == 10).all() and (spec.subtract[spec.offsets["const0"]] == 0.5).all()
    kinds = spec.segments[:, 0].tolist()
    assert kinds == [KIND["rho"], KIND["const"], KIND["out"], KIND["thermal_limit"], KIND["calendar"]]
    assert spec.segments[2, 1] == out_offsets(m)["gen_p"] and spec.segments[4, 1] == 3
    assert np.int32(spec.segments[1, 1]).view(np.float32) == np.float32(2.5)
    st = {"done": np.array([False, True]), "rho": np.tile(scale, (2, 1)), "gen_p": np.full((2, m.n_gen), 60.0),
          "thermal_limit": np.ones((2, m.n_line)), "hour_of_day": np.array([[7], [7]])}
    v = obs_ref.compose(spec, st)
    assert np.array_equal(v[0, spec.offsets["rho"]], np.ones(m.n_line, np.float32))
    assert np.array_equal(v[0, spec.offsets["gen_p"]], np.full(m.n_gen, np.float32(0.5)))
    assert np.array_equal(v[0, spec.offsets["const0"]], np.full(3, np.float32(2.0)))
    assert np.array_equal(v[1, spec.offsets["gen_p"]], np.full(m.n_gen, np.float32(-0.1)))     # game over: (0 - 10) / 100
    assert v[1, spec.offsets["hour_of_day"]] == 7 and (v[1, spec.offsets["thermal_limit"]] == 1).all()


def test_refusals(load_model):
    m = load_model("rte_case5_example")
    with pytest.raises(ValueError, match=r"'curtailment'.*const"):
        ObsSpec(m, ["rho", "curtailment"])
    with pytest.raises(ValueError, match=r"'not_an_attribute'.*const"):
        ObsSpec(m, ["not_an_attribute"])
    with pytest.raises(ValueError, match="twice"):
        ObsSpec(m, ["rho", "rho"])
    with pytest.raises(ValueError, match="no element"):
        ObsSpec(m, ["storage_charge"])                          # rte_case5_example has no storage unit
    with pytest.raises(ValueError, match="divide is zero"):
        ObsSpec(m, ["rho", "gen_p"], divide={"gen_p": [1.0, 0.0]})
    with pytest.raises(ValueError, match="8 values"):
        ObsSpec(m, ["rho"], subtract={"rho": [1.0, 2.0]})
    with pytest.raises(ValueError, match="not an attribute of this spec"):
        ObsSpec(m, ["rho"], subtract={"gen_p": 1.0})
    seg = ObsSpec(m, ["rho", "gen_p"]).segments.copy()
    seg[1, 3] -= 1
    with pytest.raises(ValueError, match="overlap"):
        check_segments(seg, 10)
    seg[1, 3] += 2
    with pytest.raises(ValueError, match="outside"):
        check_segments(seg, 10)
    with pytest.raises(ValueError, match="gap"):
        check_segments(seg, 11)


def test_maintenance_lookahead_is_the_reference_definition():
    """The docstring examples of GridValue.get_maintenance_time_1d / get_maintenance_duration_1d (Chronics/gridValue.py:296-315, 371-390)
    and the columns the reference recorded on the 36-substation grid (simulate_maintenance_neurips36.npz carries the table window they
    came from: rows row0 .. of the episode)."""
    one = np.array([0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0])[:, None]
    nxt, dur = obs_ref.maintenance_lookahead(one)
    assert nxt[:, 0].tolist() == [5, 4, 3, 2, 1, 0, 0, 0, 4, 3, 2, 1, 0, 0, -1, -1, -1]
    assert dur[:, 0].tolist() == [3, 3, 3, 3, 3, 3, 2, 1, 2, 2, 2, 2, 2, 1, 0, 0, 0]
    nxt, dur = obs_ref.maintenance_lookahead(np.zeros((10, 2)))
    assert (nxt == -1).all() and (dur == 0).all()
    fx = np.load(golden_path("simulate_maintenance_neurips36.npz"))
    nxt, dur = obs_ref.maintenance_lookahead(fx["maintenance"])
    rows = fx["row"] - int(fx["row0"])
    inside = (rows >= 0) & (rows < fx["maintenance"].shape[0])
    assert inside.sum() >= 4
    checked = 0
    for k in np.nonzero(inside)[0]:
        # the time of the next outage is fully known inside the window; an outage the window cuts looks shorter than recorded
        ref_n, ref_d = fx["time_next_maintenance"][k], fx["duration_next_maintenance"][k]
        left = fx["maintenance"].shape[0] - rows[k]
        seen = (ref_n >= 0) & (ref_n < left)                    # the outage starts inside the window
        assert np.array_equal(nxt[rows[k]][seen], ref_n[seen]) and (nxt[rows[k]][~seen] == -1).all()
        cut = seen & (ref_n + ref_d >= left)
        assert np.array_equal(dur[rows[k]][seen & ~cut], ref_d[seen & ~cut])
        assert np.array_equal(dur[rows[k]][cut], left - ref_n[cut]) and (dur[rows[k]][~seen] == 0).all()
        checked += int(seen.sum())
    assert checked >= 8


def test_compose_reproduces_every_recorded_row(load_model):
    """`compose` fed with the attributes cut out of the recorded vectors (calendar, margins and game over restated from their definitions,
    not copied) gives the recorded vectors back: the layout, the const values and the game-over vector are the reference's."""
    m = load_model("rte_case5_example")
    spec = ObsSpec.complete(m, fill=True)
    fx = _fixture()
    vec, ep = fx["vectors"], fx["episode"]
    assert len(vec) >= 5
    n_over = 0
    for e in range(len(fx["played"])):
        rows = vec[ep == e]
        played = int(fx["played"][e])
        start = dt.datetime(*[int(x) for x in fx["start"][e]])
        assert len(rows) in (played + 1, played + 2) or played == 100
        for k, row in enumerate(rows):
            over = k == played + 1 or (k == played and len(rows) == played + 1 and not np.any(row[spec.offsets["line_status"]]))
            st = {"done": np.array([over])}
            for name in spec.names:
                if not name.startswith("const"):
                    st[name] = row[spec.offsets[name]][None, :]
            cal = obs_ref.calendar(start, 5, [k])
            for i, name in enumerate(obs_ref.CALENDAR):
                st[name] = cal[:, i:i + 1]
            st["current_step"], st["max_step"], st["delta_time"] = np.array([[k]]), np.array([[100]]), np.array([[5]])
            st["gen_margin_up"], st["gen_margin_down"] = obs_ref.margins(st["gen_p"], *CASE5_LIMITS, CASE5_RENEWABLE)
            setp = st["gen_p"] - st["gen_p_delta"]
            st["gen_p_before_curtail"] = np.where(np.array(CASE5_RENEWABLE)[None, :], setp, np.float32(0))
            if over:                                             # what a failed lane holds: NaN results; the fill must not depend on it
                for name in ("gen_p", "rho", "p_or", "gen_margin_up", "target_dispatch"):
                    st[name] = np.full_like(np.asarray(st[name], dtype=np.float32), np.nan)
                st["topo_vect"] = np.zeros((1, m.dim_topo))
                n_over += 1
            got = obs_ref.compose(spec, st)[0]
            exact = np.ones(192, dtype=bool)
            for name in ("gen_margin_up", "gen_margin_down", "gen_p_before_curtail"):     # float32 arithmetic on recorded float32: 1 ulp of 30 MW
                exact[spec.offsets[name]] = False
            assert np.array_equal(got[exact], row[exact]), (fx["names"][e], k, np.nonzero(got != row)[0])
            assert np.allclose(got[~exact], row[~exact], rtol=0, atol=4e-6), (fx["names"][e], k)
    assert n_over >= 2
    # 1.11.0 alone: 3 played rows + 2 game-over rows that keep the calendar (minute 5 and 10)
    first = vec[ep <= 1]
    assert len(first) == 5 and first[[1, 4], 4].tolist() == [5.0, 10.0] and (first[[1, 4], 6:8] == 0).all()
