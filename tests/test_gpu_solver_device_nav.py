"""WindowSolverBatch::setDeviceNavFactors on the GPU: the navigation factors resident on the device give the host's solve in every bit.  The
five windows of prior_solve_data (2 to 8 states, one window without a prior, one with a constant state — its GNSS factor has a cost and no
host block —, one far start, which rejects steps at most variants) through icgh_backend_solve_nav_batch with the product's factors (ImuPosePriorFactor,
ImuMixPriorFactor, ImuErrorFactor, a GnssFactor on every state), at the variants 0, 1 (mix blocks of 9) and 2, 3 (mix blocks of 10), without a
loss on the GNSS factors and with HuberLoss(1.0) (the fixes put members inside and outside its kernel): modes 2, 3, 4 and 5 with the switch on
against mode 0.  States, inverse depths, summaries and prior costs are compared on bit patterns."""
import ctypes as C

import numpy as np
import pytest

import nav_solve_data as nsd
import preint_odo_solve_data as os_
import preint_solve_data as psd
import prior_solve_data as ps
from ctypes_util import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import harness
    return C.CDLL(harness.HOST_LIB)


@pytest.fixture(scope="module")
def five(oracle):
    """per variant: (windows, starts, priors, state_const, integration results or None)"""
    import icgvins
    w9, w10 = ps.five_windows(oracle), os_.five_windows(oracle)
    ctx = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    out = {0: (*w9, None), 1: (*w9, None)}
    for v in (2, 3):
        out[v] = (*w10, os_.integrate_on_device(ctx, v, w10[0], w10[1]))
    ctx.close()
    return out


def _solve(lib, five, variant, mode, n=None, **kw):
    wins, starts, priors, const, results = five[variant]
    if n is not None:
        k = sum(len(w["offsets"]) - 1 for w in wins[:n])
        wins, starts, priors, const, results = wins[:n], starts[:n], priors[:n], const[:n], None if results is None else results[:k]
    return nsd.solve_nav_batch(lib, wins, starts, priors, mode, variant=variant, results=results, state_const=const, **kw)


@pytest.fixture(scope="module", params=[(v, h) for v in (0, 1, 2, 3) for h in (0.0, 1.0)], ids=lambda p: f"variant{p[0]}-huber{p[1]}")
def host_solve(request, lib, five):
    """mode 0 at one variant and one GNSS loss: what every device mode has to reproduce"""
    v, h = request.param
    out = _solve(lib, five, v, 0, gnss_huber=h)
    assert out[0] == 0 and out[6] == 0, out[1]
    summ = out[4]
    assert (summ[:, 2] > 0).all() and (summ[:, 1] < summ[:, 0]).all(), summ  # every window takes a successful step
    return v, h, out


def _same(a, b, n_windows):
    for w in range(n_windows):
        assert np.array_equal(bits(a[2][w]), bits(b[2][w])), ("states", w)
        assert np.array_equal(bits(a[3][w]), bits(b[3][w])), ("inverse depths", w)
    assert np.array_equal(bits(a[4]), bits(b[4])), ("summaries", a[4], b[4])
    assert np.array_equal(bits(a[5]), bits(b[5])), ("prior costs", a[5], b[5])


@pytest.mark.parametrize("mode", [2, 3, 4, 5])
def test_device_nav_equals_the_host_solve_bit_for_bit(lib, five, host_solve, mode):
    variant, huber, ref = host_solve
    out = _solve(lib, five, variant, mode, device_nav=1, gnss_huber=huber)
    assert out[0] == 0, out[1]
    _same(out, ref, 5)
    assert out[6] == nsd.nav_factor_count(five[variant][0]), out[6]  # every navigation factor of the batch, the one on the constant state included


def test_the_huber_loss_is_in_the_device_solve(lib, five):
    a = _solve(lib, five, 2, 5, n=2, device_nav=1, gnss_huber=0.0)
    b = _solve(lib, five, 2, 5, n=2, device_nav=1, gnss_huber=1.0)
    assert a[0] == 0 and b[0] == 0, (a[1], b[1])
    assert a[6] == b[6] == nsd.nav_factor_count(five[2][0][:2])
    assert not np.array_equal(bits(a[2][0]), bits(b[2][0]))


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5])
def test_without_the_switch_the_results_are_the_older_entries(lib, five, mode):
    """device_nav off, the stand-in priors: the bits of icgh_backend_solve_preint_batch / icgh_backend_solve_preint_odo_batch on the same windows"""
    for variant in (1, 3):
        wins, starts, priors, const, results = five[variant]
        x = _solve(lib, five, variant, mode, nav_factors=0)
        if variant == 1:
            y = psd.solve_preint_batch(lib, wins, starts, priors, mode, variant=variant, state_const=const)
        else:
            y = os_.solve_preint_odo_batch(lib, wins, starts, results, priors, mode, variant=variant, state_const=const)
        assert x[0] == 0 and y[0] == 0 and x[6] == 0, (x[1], y[1])
        _same(x, y, 5)


def test_device_nav_off_keeps_the_factors_on_the_pool(lib, five, host_solve):
    variant, huber, ref = host_solve
    out = _solve(lib, five, variant, 5, device_nav=0, gnss_huber=huber)
    assert out[0] == 0 and out[6] == 0, out[1]
    _same(out, ref, 5)


def test_the_switch_without_the_host_part_is_refused(lib, five):
    wins, starts = five[0][0], five[0][1]
    rc, msg, st, _, summ, _, _ = _solve(lib, five, 0, 1, n=2, device_nav=1 + 16)
    assert rc == -3 and "setDeviceNavFactors(true) needs setDeviceHostPart(true)" in msg, (rc, msg)
    assert not summ.any() and np.array_equal(st[0], starts[0][0])
    rc, msg, _, _, summ, _, _ = _solve(lib, five, 0, 0, n=2, device_nav=1)
    assert rc == -3 and "setDeviceNavFactors(true) needs setDeviceHostPart(true)" in msg and not summ.any(), (rc, msg)
