"""CPU tests of the cross-entropy planner's host side (ndivplanning_amd/evaluation.py: CemSettings, cem_normal_floats,
the `mpc.cem` mapping of a config) and of the arguments ndp_plan_cem_update and ndp_normal_noise refuse before they
launch anything (the library loads without a GPU)."""
import pytest

import plan_common as C
from ndivplanning_amd import evaluation as E
from ndivplanning_amd.utils.file import DotMap


def test_defaults_are_the_documented_hyperparameters():
    s = E.CemSettings()
    assert (s.iterations, s.elites, s.momentum, s.min_std, s.proposal) == (3, None, 0.1, 0.05, "generator")
    assert s.low == (-1.0,) * 4 and s.high == (1.0,) * 4
    assert [s.elite_count(r) for r in (2, 3, 4, 8, 32, 256)] == [1, 1, 1, 2, 8, 64]
    assert E.CemSettings(elites=5).elite_count(5) == 5
    assert E.CemSettings(low=[-1, -2, -3, -4], high=2).low == (-1.0, -2.0, -3.0, -4.0)


@pytest.mark.parametrize("kwargs", [
    {"iterations": -1}, {"iterations": 1.5}, {"iterations": True}, {"elites": 0}, {"elites": 257}, {"elites": 2.5},
    {"momentum": 1.0}, {"momentum": -0.1}, {"momentum": float("nan")}, {"min_std": -1e-3}, {"min_std": float("inf")},
    {"min_std": float("nan")}, {"proposal": "gaussian"}, {"low": 0.5, "high": 0.25}, {"low": [0, 0, 0]},
    {"high": [1, 1, 1, float("nan")]}, {"low": [-1, -1, 2, -1], "high": [1, 1, 1, 1]}, {"low": float("-inf")}])
def test_settings_are_validated(kwargs):
    with pytest.raises(ValueError):
        E.CemSettings(**kwargs)


def test_elites_and_rollouts_must_fit():
    with pytest.raises(ValueError):
        E.CemSettings(elites=6).elite_count(5)
    for r in (1, 257):
        with pytest.raises(ValueError):
            E.CemSettings().elite_count(r)
    with pytest.raises(ValueError):
        E._cem_check(E.CemSettings(), 8, 33)
    with pytest.raises(TypeError):
        E._cem_check({"iterations": 2}, 8, 3)


def test_normal_floats_against_a_hand_count():
    # plan_step: I x Th x B x R x 4
    assert E.cem_normal_floats(2, 8, 3, 2) == 2 * 3 * 2 * 8 * 4
    assert E.cem_normal_floats(1, 5, 4, 0) == 0
    # mpc_plan, T = 6, Th = 3: planning steps of 3, 3, 3, 2, 1 horizon steps = 12; B = 2, R = 8, I = 2
    assert E.cem_normal_floats(2, 8, 3, 2, seq_length=6) == 12 * 2 * 2 * 8 * 4
    # T = 3, Th = 5: 2 + 1 horizon steps
    assert E.cem_normal_floats(1, 4, 5, 3, seq_length=3) == 3 * 3 * 1 * 4 * 4


def _config(cem=None, **mpc):
    block = dict({"rollouts": 8, "time_horizon": 3}, **mpc)
    if cem is not None:
        block["cem"] = cem
    return DotMap({"random_seed": 3, "mpc": block})


def test_the_config_mapping():
    assert E.cem_from_config(_config()) is None                       # absent: off
    assert E.cem_from_config(DotMap({"random_seed": 3})) is None
    s = E.cem_from_config(_config({"iterations": 2, "elites": 3, "proposal": "uniform", "low": [-1, -1, 0, -1], "high": 1}))
    assert (s.iterations, s.elites, s.proposal, s.low, s.high) == (2, 3, "uniform", (-1.0, -1.0, 0.0, -1.0), (1.0,) * 4)


@pytest.mark.parametrize("cem", [{"iters": 2}, {"iterations": -1}, {"elites": 9}, {"proposal": "noise"}, [1, 2], 3,
                                 {"momentum": 1.0}])
def test_a_bad_config_mapping_raises(cem):
    with pytest.raises(ValueError):
        E.cem_from_config(_config(cem))


def test_a_config_whose_planner_does_not_fit_raises():
    with pytest.raises(ValueError):
        E.cem_from_config(_config({"iterations": 1}, time_horizon=33))
    with pytest.raises(ValueError):
        E.cem_from_config(_config({"iterations": 1}, rollouts=1))


# ------------------------------------------------------------------------------- refused before anything is launched
@pytest.fixture(scope="module")
def lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


@pytest.mark.parametrize("over", C.REFUSED, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_refused_arguments(lib, over):
    assert C.refused_call(lib, **over) == 1                                    # NDP_E_ARG
    assert b"ndp_plan_cem_update" in lib.ndp_last_error()


def test_normal_noise_refuses_bad_arguments(lib):
    assert lib.ndp_normal_noise(None, 8, 1, None, None) == 1
    assert lib.ndp_normal_noise(0x1000, 0, 1, None, None) == 1
    assert b"ndp_normal_noise" in lib.ndp_last_error()
