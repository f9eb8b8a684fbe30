"""The batched chronics loader against the REFERENCE's own readers (grid2op.Chronics.GridStateFromFile / Multifolder /
GridStateFromFileWithForecasts) and against the committed fixtures.  The input files are the reference's chronics folders, copied
under tests/golden/chronics_data; what the reference's readers decode from them is recorded in
tests/golden/chronics_reference_readers.json (scenario order, lengths, sha256 of every table), both by
tests/golden/make_chronics_fixtures.py."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import golden_path

DATA = golden_path("chronics_data")


@pytest.fixture(scope="module")
def readers():
    with open(golden_path("chronics_reference_readers.json")) as f:
        return json.load(f)


def _digest(a, dtype):
    """as make_chronics_fixtures.digest: sha256 of the table as `dtype`, C order, prefixed with its shape"""
    a = np.ascontiguousarray(np.asarray(a), dtype=dtype)
    return hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()


@pytest.mark.parametrize("env,scen", [("l2rpn_case14_sandbox", "0000"), ("rte_case5_example", "00"),
                                       ("l2rpn_neurips_2020_track1", "Scenario_august_dummy"),
                                       ("l2rpn_wcci_2022_dev", "2050-02-14_0")])
def test_loader_matches_fixture(env, scen, load_model, load_npz):
    from grid2op_amd.chronics import chronics_table, load_chronics_folder
    m = load_model(env)
    base = os.path.join(DATA, env)
    ch = load_chronics_folder(os.path.join(base, "chronics", scen), m, prods_charac=os.path.join(base, "prods_charac.csv"),
                              max_rows=600)
    fx = load_npz(f"{env}.chronics.npz")
    for k in ("load_p", "load_q", "prod_p"):
        assert np.array_equal(ch[k], fx[k]), k
    if "prod_v" in fx:
        assert np.array_equal(ch["prod_v"], fx["prod_v"])
    else:
        assert ch["prod_v"].shape == ch["prod_p"].shape and (ch["prod_v"] > 0).all()
    tab = chronics_table(ch)
    assert tab.dtype == np.float32 and tab.shape[1] == 2 * m.n_load + 2 * m.n_gen


def test_name_mapping(load_model):
    """names_chronics_to_backend (environment.py:431-437): file columns renamed before matching."""
    from grid2op_amd.chronics import load_chronics_folder
    m = load_model("l2rpn_case14_sandbox")
    folder = os.path.join(DATA, "l2rpn_case14_sandbox", "chronics", "0000")
    ident = {"loads": {str(n): str(n) for n in m.name_load}, "prods": {str(n): str(n) for n in m.name_gen}}
    a = load_chronics_folder(folder, m, max_rows=10)
    b = load_chronics_folder(folder, m, names_chronics_to_backend=ident, max_rows=10)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(KeyError):
        load_chronics_folder(folder, m, names_chronics_to_backend={"loads": {str(m.name_load[0]): "nope"}}, max_rows=3)


@pytest.mark.parametrize("env", ["l2rpn_case14_sandbox", "l2rpn_neurips_2020_track1", "l2rpn_wcci_2022_dev", "rte_case5_example",
                                 "educ_case14_storage"])
def test_multifolder_equals_the_reference_readers(env, load_model, readers):
    """Scenario order, every row of load_p / load_q / prod_p / prod_v and the maintenance / hazards tables, as
    ``Multifolder`` + ``GridStateFromFile`` (grid2op/Chronics/multiFolder.py, gridStateFromFile.py) decode them."""
    from grid2op_amd.chronics import chronics_table, load_chronics_multifolder
    m = load_model(env)
    base = os.path.join(DATA, env)
    names, ch = load_chronics_multifolder(os.path.join(base, "chronics"), m, prods_charac=os.path.join(base, "prods_charac.csv"),
                                          truncate=True)
    ref = readers["multifolder"][env]
    assert names == ref["scenarios"]                                            # sorted scenario order
    T = ch["load_p"].shape[1]
    assert T == ref["T"]
    for k, name in enumerate(names):
        d = ref["tables"][k]
        for key in ("load_p", "load_q", "prod_p"):
            assert _digest(ch[key][k], np.float32) == d[key], (name, key)
        if d["prod_v"] is not None:
            assert _digest(ch["prod_v"][k], np.float32) == d["prod_v"], name
        for key in ("maintenance", "hazards"):
            r = d[key]
            if r is not None and key in ch:
                assert _digest(ch[key][k].astype(bool), np.bool_) == r["sha256"], (name, key)
            elif r is not None:
                assert not r["any"]
    tab = chronics_table(ch)
    assert tab.shape == (len(names), T, 2 * m.n_load + 2 * m.n_gen) and tab.dtype == np.float32
    if env == "l2rpn_neurips_2020_track1":
        assert "maintenance" in ch and ch["maintenance"].sum() > 0


def test_forecast_tables_equal_the_reference_reader(load_model, readers):
    """``GridStateFromFileWithForecasts`` (grid2op/Chronics/gridStateFromFileWithForecasts.py): the *_forecasted tables that
    ``obs.simulate`` injects."""
    from grid2op_amd.chronics import load_chronics_folder
    ref = readers["forecasts"]
    env, scen = ref["env"], ref["scenario"]
    m = load_model(env)
    folder = os.path.join(DATA, env, "chronics", scen)
    ch = load_chronics_folder(folder, m, forecasts=True)
    for key, attr in (("load_p_forecasted", "load_p_forecast"), ("load_q_forecasted", "load_q_forecast"),
                      ("prod_p_forecasted", "prod_p_forecast"), ("prod_v_forecasted", "prod_v_forecast")):
        assert _digest(ch[key], np.float32) == ref["tables"][attr], key
