"""WindowSolverBatch::setDevicePreintegration with odometer factors on the GPU: PreintegrationOdoFactors resident on the device give the
host's solve in every bit.  The five windows of prior_solve_data (2 to 8 states, one window without a prior, one with a constant state, one
far start with rejected steps) with 17-wide states and 10-wide mix blocks through icgh_backend_solve_preint_odo_batch, the integration results
from ONE icg_preint_odo_batch call per variant, in modes 0 (host), 2 (device reduced solve and host part), 3 (and device prior), 4 (mode 2
and device preintegration) and 5 (mode 3 and device preintegration), at the Odo and at the EarthOdo variant: states, inverse depths, summaries
and prior costs are compared on bit patterns."""
import ctypes as C

import numpy as np
import pytest

import preint_odo_data as od
import preint_odo_solve_data as os_
import prior_solve_data as ps
from ctypes_util import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import harness
    return C.CDLL(harness.HOST_LIB)


@pytest.fixture(scope="module")
def five(oracle):
    return os_.five_windows(oracle)


@pytest.fixture(scope="module")
def results(five):
    import icgvins
    wins, starts, _, _ = five
    ctx = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    out = {v: os_.integrate_on_device(ctx, v, wins, starts) for v in od.VARIANTS}
    ctx.close()
    return out


@pytest.fixture(scope="module", params=list(od.VARIANTS))
def host_solve(request, lib, five, results):
    """mode 0 at one variant: what every device mode has to reproduce"""
    wins, starts, priors, const = five
    v = request.param
    out = os_.solve_preint_odo_batch(lib, wins, starts, results[v], priors, 0, variant=v, state_const=const)
    assert out[0] == 0 and out[6] == 0, out[1]
    ps.check_conditions(out[4], out[5], priors)
    return v, out


def _same(a, b, n_windows):
    for w in range(n_windows):
        assert np.array_equal(bits(a[2][w]), bits(b[2][w])), ("states", w)
        assert np.array_equal(bits(a[3][w]), bits(b[3][w])), ("inverse depths", w)
    assert np.array_equal(bits(a[4]), bits(b[4])), ("summaries", a[4], b[4])
    assert np.array_equal(bits(a[5]), bits(b[5])), ("prior costs", a[5], b[5])


@pytest.mark.parametrize("mode", [2, 3, 4, 5])
def test_device_modes_equal_the_host_solve_bit_for_bit(lib, five, results, host_solve, mode):
    wins, starts, priors, const = five
    variant, ref = host_solve
    out = os_.solve_preint_odo_batch(lib, wins, starts, results[variant], priors, mode, variant=variant, state_const=const)
    assert out[0] == 0, out[1]
    _same(out, ref, len(wins))
    # every odometer factor with a free block is resident in modes 4 and 5 (all of them here: no window is constant throughout)
    assert out[6] == (sum(len(w["offsets"]) - 1 for w in wins) if mode >= 4 else 0), out[6]


def test_the_earth_odo_variant_is_another_solve(lib, five, results):
    wins, starts, priors, _ = five
    a = os_.solve_preint_odo_batch(lib, wins[:2], starts[:2], results[od.ODO][:3], priors[:2], 4, variant=od.ODO)
    b = os_.solve_preint_odo_batch(lib, wins[:2], starts[:2], results[od.EARTH_ODO][:3], priors[:2], 4, variant=od.EARTH_ODO)
    assert a[0] == 0 and b[0] == 0, (a[1], b[1])
    assert a[6] == 3 and b[6] == 3  # (windows of 2 and 3 states: 3 intervals)
    assert not np.array_equal(bits(a[2][0]), bits(b[2][0]))


def test_preintegration_switch_without_the_host_part_is_refused(lib, five, results):
    wins, starts, priors, _ = five
    rc, msg, st, _, summ, _, _ = os_.solve_preint_odo_batch(lib, wins[:2], starts[:2], results[od.ODO][:3], priors[:2], 4 + 16)
    assert rc == -3 and "setDevicePreintegration(true) needs setDeviceHostPart(true)" in msg, (rc, msg)
    assert not summ.any() and np.array_equal(st[0], os_.odo_window(wins[0], starts[0])[1])


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_a_robustified_factor_stays_on_the_pool(lib, five, results, variant):
    """window 1's odometer factors carry a Huber loss: they are not resident, the others are, and mode 5 is still mode 0"""
    wins, starts, priors, const = five
    rob = [0.0, 0.5, 0.0, 0.0, 0.0]
    ref = os_.solve_preint_odo_batch(lib, wins, starts, results[variant], priors, 0, variant=variant, state_const=const, preint_robust=rob)
    out = os_.solve_preint_odo_batch(lib, wins, starts, results[variant], priors, 5, variant=variant, state_const=const, preint_robust=rob)
    assert ref[0] == 0 and out[0] == 0, (ref[1], out[1])
    _same(out, ref, len(wins))
    assert out[6] == sum(len(w["offsets"]) - 1 for k, w in enumerate(wins) if k != 1), out[6]
    plain = os_.solve_preint_odo_batch(lib, wins, starts, results[variant], priors, 0, variant=variant, state_const=const)
    assert not np.array_equal(bits(plain[2][1]), bits(ref[2][1]))  # (the loss is in window 1's solve)
    assert np.array_equal(bits(plain[2][0]), bits(ref[2][0]))
