"""PreintegrationOdo::evaluate with its trigonometric part split out, without a GPU (oracle-backed build of the host layer), on the
integration results of the reference golden (tests/golden/preint_odo_ref_golden.npz: every case, both variants):
correctionQuaternion / earthRateQuaternion + evaluateGiven is evaluate(), in every bit of the residual and the four Jacobian blocks, at the
five kinds of evaluation point; evaluateGiven really uses the quaternions it is given; and the intervals evaluate() refuses or answers
with NaN (one sample: zero covariance; two and three samples: an information matrix that is not positive definite) behave the same way on
both sides of the split.  evaluate() itself is pinned against the reference by tests/test_preint_odo_host.py."""
import ctypes as C

import numpy as np
import pytest

import preint_odo_data as od
import preint_odo_split_data as sd
from ctypes_util import bits

IDENT = np.array([0.0, 0.0, 0.0, 1.0])
NAN_CASES = ("two_samples", "three_samples")


@pytest.fixture(scope="module")
def lib():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


@pytest.fixture(scope="module")
def golden():
    res = od.golden()
    assert len(res) == 14 and {g["variant"] for g in res} == set(od.VARIANTS)
    return res


def _points(kind, results):
    return [sd.eval_point(kind, g["delta"], g["cur"], g["s0"]) for g in results]


@pytest.mark.parametrize("kind", sd.POINT_KINDS)
def test_evaluate_given_is_evaluate_in_every_bit(lib, golden, kind):
    o = sd.eval_split(lib, golden, _points(kind, golden))
    assert np.all(o["ok"] == 1)
    assert np.array_equal(bits(o["r_given"]), bits(o["r_eval"]))
    assert np.array_equal(bits(o["J_given"]), bits(o["J_eval"]))
    for i, g in enumerate(golden):
        if g["case"] in NAN_CASES:  # as today: NaN wherever the reference has NaN, on both paths
            assert np.isnan(o["r_eval"][i]).any() and np.isnan(g["r"]).any(), g["case"]
        else:
            assert np.all(np.isfinite(o["r_eval"][i])) and np.all(np.isfinite(o["J_eval"][i])) and np.abs(o["J_eval"][i]).max() > 1.0, g["case"]
        # the quaternions: unit; the correction the identity exactly where bg0 == delta.bg; the Earth one the identity for the Odo variant
        assert abs(np.linalg.norm(o["q_corr"][i]) - 1) < 1e-15 and abs(np.linalg.norm(o["q_nn"][i]) - 1) < 1e-15
        assert np.array_equal(o["q_corr"][i], IDENT) == (kind in ("end_state", "bias_equal")), (i, o["q_corr"][i])
        assert np.array_equal(o["q_nn"][i], IDENT) == (g["variant"] == od.ODO), (i, o["q_nn"][i])
    J0, J1, J2, J3 = sd.j_blocks(o["J_eval"])
    fin = [i for i, g in enumerate(golden) if g["case"] not in NAN_CASES]
    assert not J0[fin][:, :, 6].any() and not J2[fin][:, :, 6].any()  # the seventh pose columns
    pts, delta = o["points"], o["delta"]
    if kind == "large_bias_step":
        assert np.all(np.abs(np.linalg.norm(pts[:, 10:13] - delta[:, 10:13], axis=1) - 0.1) < 0.01)
    if kind == "sodo_equal":
        assert np.array_equal(pts[:, 16], delta[:, 19]) and np.all(pts[:, 33] != pts[:, 16])
    else:
        assert (kind == "end_state") == bool(np.array_equal(pts[:, 16], delta[:, 19]))


def test_the_given_correction_quaternion_is_used(lib, golden):
    """the identity in place of q_corr at a point with a bias step changes residual and Jacobians"""
    wrong = np.tile(IDENT, (len(golden), 1))
    o = sd.eval_split(lib, golden, _points("large_bias_step", golden), q_corr_in=wrong)
    assert np.all(o["ok"] == 1)
    for i, g in enumerate(golden):
        if g["case"] in NAN_CASES:
            continue
        assert not np.array_equal(o["q_corr"][i], IDENT)
        assert not np.array_equal(bits(o["r_given"][i]), bits(o["r_eval"][i]))
        assert not np.array_equal(bits(o["J_given"][i]), bits(o["J_eval"][i]))
    i = next(i for i, g in enumerate(golden) if g["case"] == "plain")
    assert np.abs(o["r_given"][i] - o["r_eval"][i]).max() > 1e-3  # (a correction of about 0.02 rad is missing, not an ulp)


def test_the_given_earth_rate_quaternion_is_used_by_earth_odo_only(lib, golden):
    wrong = np.tile(IDENT, (len(golden), 1))
    o = sd.eval_split(lib, golden, _points("perturbed", golden), q_nn_in=wrong)
    assert np.all(o["ok"] == 1)
    seen = set()
    for i, g in enumerate(golden):
        if g["case"] in NAN_CASES:
            continue
        same = np.array_equal(bits(o["r_given"][i]), bits(o["r_eval"][i])) and np.array_equal(bits(o["J_given"][i]), bits(o["J_eval"][i]))
        assert same == (g["variant"] == od.ODO), (g["case"], g["variant"])
        seen.add(g["variant"])
    assert seen == set(od.VARIANTS)


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_one_sample_interval_is_refused_on_both_sides(lib, variant):
    """an interval of one IMU sample has a zero covariance: evaluate() and evaluateGiven() both refuse (zero rows, zero sqrt_info)"""
    imu, s0, par25, abv = od.cases()["one_sample"]
    ld = od.integrate_ld(variant, imu, s0, par25, dtype=np.float64)
    assert not ld["cov"].any() and len(ld["pn"]) == 0
    res = dict(ld, variant=variant, iewn=par25[6:9])
    o = sd.eval_split(lib, [res], [sd.eval_point("perturbed", ld["delta"], ld["cur"], s0)])
    assert list(o["ok"]) == [0]
    assert not o["r_eval"].any() and not o["J_eval"].any() and not o["r_given"].any() and not o["J_given"].any() and not o["sqrt_info"].any()


def test_entry_returns_what_the_resident_set_takes(lib, golden):
    o = sd.eval_split(lib, golden, _points("perturbed", golden))
    assert np.all(o["env"][:, 0] == 9.8)
    for i, g in enumerate(golden):
        assert np.array_equal(o["env"][i, 1:], g["iewn"])
        assert len(o["pn_rows"][i]) == (len(g["imu"]) - 1 if g["variant"] == od.EARTH_ODO else 0)
        if g["case"] not in NAN_CASES:
            S = o["sqrt_info"][i].reshape(19, 19)
            assert np.all(np.isfinite(S)) and np.all(np.tril(S, -1) == 0) and np.all(np.diag(S) > 0)


def test_invalid_variant_is_refused(lib, golden):
    from ctypes_util import ErrBuf, f64, i32, ptr
    g = golden[0]
    err = ErrBuf()
    z = lambda *s: np.zeros(s)
    rc = lib.icgh_backend_preint_odo_eval_split(1, ptr(i32([1])), ptr(f64(od.params19(od.params25(), od.ABV))), ptr(f64(g["delta"])), ptr(f64(g["jac"])),
                                                ptr(f64(g["cov"])), ptr(f64([g["dt"]])), None, None, ptr(f64(g["iewn"])), ptr(z(34)), None, None, ptr(z(19)),
                                                ptr(z(646)), ptr(z(19)), ptr(z(646)), ptr(z(4)), ptr(z(4)), ptr(z(361)), ptr(z(4)), ptr(i32([0])), *err.args)
    assert rc == -1 and "variant 1 is neither 2 (Odo) nor 3 (EarthOdo)" in err.text()
