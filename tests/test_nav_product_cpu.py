"""The navigation factors as product classes (host/nav_factors.h) through icgh_backend_nav_eval, on the oracle-backed host build.

Kinds 0..3 (the 48 cases of nav_utils.factor_cases()) are held to the reference golden tests/golden/nav_ref_golden.npz within 1e-12 relative,
the bound tests/test_host_nav_cpu.py holds the tools entry to, and equal icgh_nav_factor bit for bit.  Kinds 4 and 5 (ImuErrorFactor 7 x 10,
ImuMixPriorFactor 10 x 10) are compared with a numpy restatement bit for bit: every entry is one IEEE division (or a subtraction and a
division) of the inputs.  A reference golden for these two is not added: the recipe under oracle/ that produces the golden does not change.
The corrector entries are compared with ResidualBlockInfo::Evaluate (through the same entry) and a numpy restatement in its operation order."""
import ctypes as C

import numpy as np
import pytest

import nav_product_data as nd
import nav_utils as nu
from ctypes_util import bits, ptr


@pytest.fixture(scope="module")
def host():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


@pytest.fixture(scope="module")
def base(host):
    cases = nu.factor_cases()
    return cases, nd.host_eval(host, cases)


def test_product_classes_meet_reference_golden_and_tools_bits(host, base):
    cases, got = base
    assert len(cases) == 48
    exp = np.load(nu.GOLDEN)
    for i, (kind, aux, x) in enumerate(cases):
        nr, nc = nd.SHAPES[kind]
        assert tuple(got["shape"][i]) == (kind, nr, nc)
        r = got["r"][got["r_off"][i]:got["r_off"][i + 1]]
        J = got["J"][got["j_off"][i]:got["j_off"][i + 1]].reshape(nr, nc)
        for name, g in (("r", r), ("J", J)):
            e = exp[f"factor_{i}_{name}"]
            err = float(np.abs(g - e).max()) / max(1.0, float(np.abs(e).max()))
            assert err < 1e-12, (i, kind, name, err)
        rt, Jt = np.zeros(nr), np.zeros((nr, nc))
        a, xx = np.ascontiguousarray(aux, np.float64), np.ascontiguousarray(x, np.float64)
        assert host.icgh_nav_factor(kind, ptr(a), ptr(xx), ptr(rt), ptr(Jt)) == 0
        assert np.array_equal(bits(r), bits(rt)) and np.array_equal(bits(J), bits(Jt)), (i, kind)
        assert got["sq"][i] == sum_sq(r)
        if nc == 7:
            assert np.array_equal(bits(J[:, 6]), np.zeros(nr, np.uint64))  # the seventh pose column is +0.0


def sum_sq(r):
    s = np.float64(0.0)
    for v in r:
        s = s + v * v
    return s


def test_odometer_widths_equal_numpy_restatement(host):
    cases = nd.odo_cases()
    got = nd.host_eval(host, cases)
    assert {c[0] for c in cases} == {4, 5}
    for i, (kind, aux, x) in enumerate(cases):
        nr, nc = nd.SHAPES[kind]
        assert tuple(got["shape"][i]) == (kind, nr, nc)
        r = got["r"][got["r_off"][i]:got["r_off"][i + 1]]
        J = got["J"][got["j_off"][i]:got["j_off"][i + 1]].reshape(nr, nc)
        re, Je = np.zeros(nr), np.zeros((nr, nc))
        if kind == 4:
            re[0:3], re[3:6], re[6] = x[3:6] / nd.GRY_BIAS_STD, x[6:9] / nd.ACC_BIAS_STD, x[9] / nd.ODO_SCALE_STD
            for k in range(3):
                Je[k, k + 3], Je[k + 3, k + 6] = 1.0 / nd.GRY_BIAS_STD, 1.0 / nd.ACC_BIAS_STD
            Je[6, 9] = 1.0 / nd.ODO_SCALE_STD
        else:
            re[:] = (x - aux[:10]) / aux[10:]
            Je[np.arange(10), np.arange(10)] = 1.0 / aux[10:]
        assert np.array_equal(bits(r), bits(re)) and np.array_equal(bits(J), bits(Je)), (i, kind)
        assert got["sq"][i] == sum_sq(r)


def test_nine_wide_defaults_are_the_first_columns_of_the_odometer_forms(host):
    """kind 1 and kind 4 share their first six rows, kind 3 and kind 5 their first nine: the same divisions"""
    odo = nd.odo_cases()
    e10, m10 = odo[0], odo[1]
    nine = [(1, np.zeros(1), e10[2][:9]), (3, np.concatenate([m10[1][:9], m10[1][10:19]]), m10[2][:9])]
    a, b = nd.host_eval(host, nine), nd.host_eval(host, [e10, m10])
    assert np.array_equal(bits(a["r"][:6]), bits(b["r"][:6]))
    assert np.array_equal(bits(a["r"][6:15]), bits(b["r"][7:16]))


def test_corrector_equals_residual_block_info_inside_and_outside(host):
    cases = nd.mixed_set() + nu.factor_cases()[:8]
    n = len(cases)
    huber = np.where(np.arange(n) % 3 == 0, 1.0, np.where(np.arange(n) % 3 == 1, 1e6, 0.0))
    huber[6] = 1.0  # the zero-lever GNSS member, outside
    plain = nd.host_eval(host, cases)
    loss = nd.host_eval(host, cases, huber=huber)
    assert np.array_equal(bits(plain["r"]), bits(loss["r"])) and np.array_equal(bits(plain["J"]), bits(loss["J"]))
    inside = outside = 0
    for i, (kind, _, _) in enumerate(cases):
        nr, nc = nd.SHAPES[kind]
        rs, js = slice(loss["r_off"][i], loss["r_off"][i + 1]), slice(loss["j_off"][i], loss["j_off"][i + 1])
        s1, a, scale = loss["corr"][i]
        if huber[i] == 0.0:
            assert (s1, a, scale) == (1.0, 0.0, 1.0)
            assert np.array_equal(bits(loss["r_corr"][rs]), bits(loss["r"][rs])) and np.array_equal(bits(loss["J_corr"][js]), bits(loss["J"][js]))
            continue
        assert a == 0.0  # Huber: rho'' <= 0 everywhere
        if loss["sq"][i] > huber[i] ** 2:
            outside += 1
            assert s1 < 1.0 and scale == s1
        else:
            inside += 1
            assert s1 == 1.0 and scale == 1.0
        re, Je = nd.corrected_numpy(loss["r"][rs], loss["J"][js].reshape(nr, nc), s1, a, scale)
        assert np.array_equal(bits(loss["r_corr"][rs]), bits(re)) and np.array_equal(bits(loss["J_corr"][js]), bits(Je)), (i, kind)
    assert inside >= 3 and outside >= 3
    # the given-scalars form fed the loss's own scalars is the loss form
    given = nd.host_eval(host, cases, huber=huber, corr_in=loss["corr"])
    for k in ("r", "J", "r_corr", "J_corr", "corr"):
        assert np.array_equal(bits(given[k]), bits(loss[k])), k


def test_given_scalars_with_alpha_equal_numpy_restatement(host):
    cases = nd.mixed_set()
    n = len(cases)
    rng = np.random.RandomState(3)
    corr = np.stack([rng.uniform(0.3, 1.0, n), rng.uniform(-0.2, 0.2, n) / 50.0, rng.uniform(0.3, 1.2, n)], axis=1)
    mark = np.ones(n)
    mark[2] = 0.0
    got = nd.host_eval(host, cases, huber=mark, corr_in=corr)
    for i, (kind, _, _) in enumerate(cases):
        nr, nc = nd.SHAPES[kind]
        rs, js = slice(got["r_off"][i], got["r_off"][i + 1]), slice(got["j_off"][i], got["j_off"][i + 1])
        if mark[i] == 0.0:
            assert np.array_equal(bits(got["r_corr"][rs]), bits(got["r"][rs])) and np.array_equal(bits(got["J_corr"][js]), bits(got["J"][js]))
            continue
        re, Je = nd.corrected_numpy(got["r"][rs], got["J"][js].reshape(nr, nc), *corr[i])
        assert np.array_equal(bits(got["r_corr"][rs]), bits(re)) and np.array_equal(bits(got["J_corr"][js]), bits(Je)), (i, kind)
        assert not np.array_equal(bits(got["J_corr"][js]), bits(got["J"][js]))


def test_unknown_kind_is_refused(host):
    from ctypes_util import ErrBuf, f64, i32
    err = ErrBuf()
    kind, aux_off, aux, pts, off = i32([6]), i32([0, 0]), f64(np.zeros(1)), f64(np.zeros(10)), i32([0])
    rc = host.icgh_backend_nav_eval(1, ptr(kind), ptr(aux_off), ptr(aux), ptr(pts), ptr(off), None, None, None, None, None, None, None, None, None,
                                    *err.args)
    assert rc == -1 and "outside 0..5" in err.text()
