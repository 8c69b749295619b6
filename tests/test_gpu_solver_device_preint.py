"""WindowSolverBatch::setDevicePreintegration on the GPU: the preintegration factors resident on the device give the host's solve in every
bit.  prior_solve_data.five_windows (2 to 8 states, one window without a prior, one with a constant state, one far start with rejected
steps: trial evaluations and re-damping are exercised) through icgh_backend_solve_preint_batch in modes 0 (host), 2 (device reduced solve and
host part), 3 (and device prior), 4 (mode 2 and device preintegration) and 5 (mode 3 and device preintegration), at the Normal and at the
Earth variant: states, inverse depths, summaries and prior costs are compared on bit patterns."""
import ctypes as C

import numpy as np
import pytest

import preint_solve_data as qs
import prior_solve_data as ps
from ctypes_util import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import harness
    return C.CDLL(harness.HOST_LIB)


@pytest.fixture(scope="module")
def five(oracle):
    return ps.five_windows(oracle)


@pytest.fixture(scope="module", params=[0, 1])
def host_solve(request, lib, five):
    """mode 0 at one variant: what every device mode has to reproduce"""
    wins, starts, priors, const = five
    out = qs.solve_preint_batch(lib, wins, starts, priors, 0, variant=request.param, state_const=const)
    assert out[0] == 0, out[1]
    ps.check_conditions(out[4], out[5], priors)
    return request.param, out


def _same(a, b, n_windows):
    for w in range(n_windows):
        assert np.array_equal(bits(a[2][w]), bits(b[2][w])), ("states", w)
        assert np.array_equal(bits(a[3][w]), bits(b[3][w])), ("inverse depths", w)
    assert np.array_equal(bits(a[4]), bits(b[4])), ("summaries", a[4], b[4])
    assert np.array_equal(bits(a[5]), bits(b[5])), ("prior costs", a[5], b[5])


@pytest.mark.parametrize("mode", [2, 3, 4, 5])
def test_device_modes_equal_the_host_solve_bit_for_bit(lib, five, host_solve, mode):
    wins, starts, priors, const = five
    variant, ref = host_solve
    out = qs.solve_preint_batch(lib, wins, starts, priors, mode, variant=variant, state_const=const)
    assert out[0] == 0, out[1]
    _same(out, ref, len(wins))
    # every preintegration factor with a free block is resident in modes 4 and 5 (all of them here: no window is constant throughout)
    assert out[6] == (sum(len(w["offsets"]) - 1 for w in wins) if mode >= 4 else 0), out[6]


def test_the_earth_variant_is_another_solve(lib, five):
    wins, starts, priors, const = five
    a = qs.solve_preint_batch(lib, wins[:2], starts[:2], priors[:2], 4, variant=0)
    b = qs.solve_preint_batch(lib, wins[:2], starts[:2], priors[:2], 4, variant=1)
    assert a[0] == 0 and b[0] == 0, (a[1], b[1])
    assert not np.array_equal(bits(a[2][0]), bits(b[2][0]))


def test_preintegration_switch_without_the_host_part_is_refused(lib, five):
    wins, starts, priors, _ = five
    rc, msg, st, _, summ, _, _ = qs.solve_preint_batch(lib, wins[:2], starts[:2], priors[:2], 4 + 16)
    assert rc == -3 and "setDevicePreintegration(true) needs setDeviceHostPart(true)" in msg, (rc, msg)
    assert not summ.any() and np.array_equal(st[0], starts[0][0])


@pytest.mark.parametrize("variant", [0, 1])
def test_a_robustified_factor_stays_on_the_pool(lib, five, variant):
    """window 1's preintegration factors carry a Huber loss: they are not resident, the others are, and mode 5 is still mode 0"""
    wins, starts, priors, const = five
    rob = [0.0, 0.5, 0.0, 0.0, 0.0]
    ref = qs.solve_preint_batch(lib, wins, starts, priors, 0, variant=variant, state_const=const, preint_robust=rob)
    out = qs.solve_preint_batch(lib, wins, starts, priors, 5, variant=variant, state_const=const, preint_robust=rob)
    assert ref[0] == 0 and out[0] == 0, (ref[1], out[1])
    _same(out, ref, len(wins))
    assert out[6] == sum(len(w["offsets"]) - 1 for k, w in enumerate(wins) if k != 1), out[6]
    plain = qs.solve_preint_batch(lib, wins, starts, priors, 0, variant=variant, state_const=const)
    assert not np.array_equal(bits(plain[2][1]), bits(ref[2][1]))  # (the loss is in window 1's solve)
    assert np.array_equal(bits(plain[2][0]), bits(ref[2][0]))
