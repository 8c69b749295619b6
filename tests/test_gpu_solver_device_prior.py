"""WindowSolverBatch with every window's marginalization prior resident on the device (setDevicePrior) against the host pool: states, inverse
depths and summaries are the same bits in mode 0 (host), 1 (device reduced solve), 2 (and device host part) and 3 (and device prior), on
visual-inertial windows with a prior given as arrays (icgh_backend_solve_prior_batch)."""
import ctypes as C

import numpy as np
import pytest

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


def test_four_modes_give_identical_bits(lib, five):
    wins, starts, priors, const = five
    assert [len(w["states"]) for w in wins] == [2, 3, 4, 8, 8] and all(w["obs"].shape[1] > 0 for w in wins)
    res = {}
    for mode in (0, 1, 2, 3):
        rc, msg, st, inv, summ, pcost = ps.solve_prior_batch(lib, wins, starts, priors, mode, state_const=const)
        assert rc == 0, (mode, msg)
        res[mode] = (st, inv, summ, pcost)
    st0, inv0, summ0, pcost0 = res[0]
    ps.check_conditions(summ0, pcost0, priors)
    for mode in (1, 2, 3):
        st, inv, summ, pcost = res[mode]
        assert np.array_equal(bits(summ), bits(summ0)), (mode, summ, summ0)
        assert np.array_equal(bits(pcost), bits(pcost0)), (mode, pcost, pcost0)
        for w in range(len(wins)):
            assert np.array_equal(bits(st[w]), bits(st0[w])) and np.array_equal(bits(inv[w]), bits(inv0[w])), (mode, w)


def test_robust_prior_and_constant_prior_stay_bit_equal(lib, five):
    """a robustified prior stays on the pool, a prior whose states are all constant has a cost but no block: mode 3 is mode 0 on both"""
    wins, starts, priors, _ = five
    sel = [0, 2, 4]
    w3, s3, p3 = [wins[k] for k in sel], [starts[k] for k in sel], [priors[k] for k in sel]
    p3[2] = ps.make_prior(wins[4], [0, 3], 36)
    const = [None, None, [1, 0, 0, 1, 0, 0, 0, 0]]
    out = {}
    for mode in (0, 3):
        rc, msg, st, inv, summ, pcost = ps.solve_prior_batch(lib, w3, s3, p3, mode, state_const=const, robust=[0.5, 0.0, 0.0])
        assert rc == 0, (mode, msg)
        out[mode] = (st, inv, summ, pcost)
    assert (out[0][2][:, 2] > 0).all() and (out[0][3][:, 0] > 0).all(), out[0][2:]
    assert out[0][3][2, 0] == out[0][3][2, 1]  # the constant prior's cost does not move
    assert np.array_equal(bits(out[3][2]), bits(out[0][2])), (out[3][2], out[0][2])
    for w in range(3):
        assert np.array_equal(bits(out[3][0][w]), bits(out[0][0][w])) and np.array_equal(bits(out[3][1][w]), bits(out[0][1][w])), w


def test_prior_switch_needs_the_host_part_switch(lib, five):
    wins, starts, priors, _ = five
    rc, msg, st, _, _, _ = ps.solve_prior_batch(lib, wins[:1], starts[:1], priors[:1], 3 + 16)
    assert rc == -3 and "setDeviceHostPart" in msg, (rc, msg)
