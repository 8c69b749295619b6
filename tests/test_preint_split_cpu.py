"""Preintegration::evaluate with its trigonometric part split out, without a GPU (oracle-backed build of the host layer):
correctionQuaternion / earthRateQuaternion + evaluateGiven is evaluate(), in every bit of the residual and the four Jacobian blocks, for both
variants at the four kinds of evaluation point; and evaluateGiven really uses the quaternion it is given."""
import ctypes as C

import numpy as np
import pytest

import preint_split_data as sd
from ctypes_util import bits

LENS = {0: [41, 17], 1: [2, 41]}  # Earth: intervals of 2 and of 41 samples (1 and 40 rows of pn)


@pytest.fixture(scope="module")
def lib():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


@pytest.fixture(scope="module", params=[0, 1])
def case(request, lib):
    variant = request.param
    imus, states = sd.intervals(LENS[variant])
    cur = sd.current_states(lib, variant, imus, states)
    return variant, imus, states, cur


@pytest.mark.parametrize("kind", sd.POINT_KINDS)
def test_evaluate_given_is_evaluate_in_every_bit(lib, case, kind):
    variant, imus, states, cur = case
    points = [sd.eval_point(kind, states[i], cur[i]) for i in range(len(imus))]
    o = sd.eval_split(lib, variant, imus, states, points)
    assert np.all(o["ok"] == 1)
    assert np.array_equal(bits(o["r_given"]), bits(o["r_eval"]))
    assert np.array_equal(bits(o["J_given"]), bits(o["J_eval"]))
    # the evaluation is not trivial: finite, non-zero rows for the 17- and 41-sample intervals (the 2-sample interval's information is not
    # positive definite: NaN in every entry, on both paths)
    for i, n in enumerate(LENS[variant]):
        if n > 2:
            assert np.all(np.isfinite(o["r_eval"][i])) and np.all(np.isfinite(o["J_eval"][i])) and np.abs(o["J_eval"][i]).max() > 1.0, i
        else:
            assert np.all(np.isnan(o["r_eval"][i]))
    # the quaternions: unit, the correction the identity exactly where bg0 == delta.bg, the Earth one the identity for the Normal variant
    assert np.allclose(np.linalg.norm(o["q_corr"], axis=1), 1.0, atol=1e-15) and np.allclose(np.linalg.norm(o["q_nn"], axis=1), 1.0, atol=1e-15)
    ident = np.array([0.0, 0.0, 0.0, 1.0])
    for i in range(len(imus)):
        assert np.array_equal(o["q_corr"][i], ident) == (kind in ("end_state", "bias_equal")), (i, o["q_corr"][i])
        assert np.array_equal(o["q_nn"][i], ident) == (variant == 0), (i, o["q_nn"][i])
    if kind == "large_bias_step":
        dbg = o["points"][:, 10:13] - o["delta"][:, 10:13]
        assert np.all(np.abs(np.linalg.norm(dbg, axis=1) - 0.1) < 0.01)


def test_the_given_quaternion_is_used(lib, case):
    """the identity in place of q_corr at a point with a bias step changes residual and Jacobians"""
    variant, imus, states, cur = case
    points = [sd.eval_point("large_bias_step", states[i], cur[i]) for i in range(len(imus))]
    wrong = np.tile([0.0, 0.0, 0.0, 1.0], (len(imus), 1))
    o = sd.eval_split(lib, variant, imus, states, points, q_corr_in=wrong)
    i = LENS[variant].index(41)
    assert np.all(o["ok"] == 1)
    assert not np.array_equal(o["q_corr"][i], wrong[i])
    assert not np.array_equal(bits(o["r_given"][i]), bits(o["r_eval"][i]))
    assert not np.array_equal(bits(o["J_given"][i]), bits(o["J_eval"][i]))
    assert np.abs(o["r_given"][i] - o["r_eval"][i]).max() > 1e-3  # (a correction of about 0.02 rad is missing, not an ulp)


def test_entry_returns_what_the_resident_set_takes(lib, case):
    variant, imus, states, cur = case
    points = [sd.eval_point("perturbed", states[i], cur[i]) for i in range(len(imus))]
    o = sd.eval_split(lib, variant, imus, states, points)
    n = len(imus)
    assert list(np.diff(o["pn_off"])) == [len(m) - 1 for m in imus] and o["pn"].shape == (sum(len(m) - 1 for m in imus), 4)
    assert np.all(o["dt"] > 0) and np.allclose(o["dt"], [0.005 * (len(m) - 1) for m in imus])
    assert np.all(o["env"][:, 0] == 9.8)
    for i in range(n):
        assert np.array_equal(o["delta"][i, 10:16], states[i][10:16])  # delta.bg / delta.ba are the start state's
        assert np.abs(o["jac"][i]).max() >= 1.0
        if len(imus[i]) > 2:
            assert np.all(np.isfinite(o["sqrt_info"][i])) and np.abs(o["sqrt_info"][i]).max() > 1.0
    if variant == 1:
        assert np.all(o["pn"][:, 0] == 0.005)
