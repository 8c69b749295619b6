"""icgh_backend_solve_nav_batch without a GPU, on the oracle-backed build of the host layer: the five windows of prior_solve_data (2 to 8
states, one without a prior, one with a constant state, one far start) with the product's navigation factors (ImuPosePriorFactor and
ImuMixPriorFactor on state 0, an ImuErrorFactor on the last state, a GnssFactor on every state) at variant 0 (mix blocks of 9) and variant 2
(mix blocks of 10, the integration results of preint_odo_data.integrate_ld in float64).  Mode 0 solves them with and without a Huber loss on
the GNSS factors, the Huber problem is another problem, the device switch says which entry the build lacks, invalid modes are refused, and
with the stand-in priors the entry gives the bits of the entries whose windows it shares."""
import ctypes as C

import numpy as np
import pytest

import nav_solve_data as nsd
import preint_odo_solve_data as os_
import preint_solve_data as psd
import prior_solve_data as ps
from ctypes_util import bits


@pytest.fixture(scope="module")
def lib():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


@pytest.fixture(scope="module")
def five(oracle):
    """per variant: (windows, starts, priors, state_const, integration results or None)"""
    w9 = ps.five_windows(oracle)
    w10 = os_.five_windows(oracle)
    return {0: (*w9, None), 2: (*w10, os_.integrate_on_host(2, w10[0], w10[1]))}


def _solve(lib, five, variant, mode=0, n=None, **kw):
    wins, starts, priors, const, results = five[variant]
    if n is not None:
        k = sum(len(w["offsets"]) - 1 for w in wins[:n])
        wins, starts, priors, const, results = wins[:n], starts[:n], priors[:n], const[:n], None if results is None else results[:k]
    return nsd.solve_nav_batch(lib, wins, starts, priors, mode, variant=variant, results=results, state_const=const, **kw)


@pytest.fixture(scope="module")
def solved(lib, five):
    return {(v, h): _solve(lib, five, v, gnss_huber=h) for v in (0, 2) for h in (0.0, 1.0)}


@pytest.mark.parametrize("huber", [0.0, 1.0])
@pytest.mark.parametrize("variant", [0, 2])
def test_mode0_solves_the_five_windows(five, solved, variant, huber):
    wins, starts, priors, const, _ = five[variant]
    rc, msg, st, inv, summ, pcost, n_dev = solved[(variant, huber)]
    assert rc == 0 and n_dev == 0, (rc, msg, n_dev)
    assert [len(s) for s in st] == [2, 3, 4, 8, 8] and st[0].shape[1] == (17 if variant == 2 else 16)
    assert (summ[:, 2] > 0).all() and (summ[:, 1] < summ[:, 0]).all(), summ  # every window takes a successful step
    for w, p in enumerate(priors):
        assert (pcost[w, 0] > 0) == (p is not None), (w, pcost)
    start = os_.odo_window(wins[3], starts[3])[1] if variant == 2 else starts[3][0]
    assert np.array_equal(bits(st[3][1]), bits(start[1]))  # a constant state did not move, GNSS fix or not
    assert not np.array_equal(bits(st[3][2]), bits(start[2]))


@pytest.mark.parametrize("variant", [0, 2])
def test_the_huber_problem_is_another_problem(five, solved, variant):
    for w in range(5):
        assert not np.array_equal(bits(solved[(variant, 0.0)][2][w]), bits(solved[(variant, 1.0)][2][w])), w
    assert not np.array_equal(bits(solved[(variant, 0.0)][4]), bits(solved[(variant, 1.0)][4]))


@pytest.mark.parametrize("variant", [0, 2])
def test_the_device_switch_names_the_missing_entry(lib, five, variant):
    wins, starts = five[variant][0], five[variant][1]
    for mode in (2, 3, 4, 5):
        rc, msg, st, _, summ, _, n_dev = _solve(lib, five, variant, mode=mode, n=2, device_nav=1, gnss_huber=1.0)
        assert rc == -4 and msg.startswith("icg_nav_set is not in this build"), (mode, rc, msg)
        start = os_.odo_window(wins[0], starts[0])[1] if variant == 2 else starts[0][0]
        assert not summ.any() and np.array_equal(st[0], start) and n_dev <= 0  # nothing was computed


def test_invalid_modes_are_refused(lib, five):
    wins, starts, priors = five[0][0][:1], five[0][1][:1], five[0][2][:1]
    for mode, variant, nav in ((9, 0, 0), (6, 0, 0), (-1, 0, 0), (0, 4, 0), (0, -1, 0), (0, 0, 2), (0, 0, 16)):
        rc, msg, _, _, summ, _, _ = nsd.solve_nav_batch(lib, wins, starts, priors, mode, variant=variant, device_nav=nav)
        assert rc == -1 and "mode" in msg and not summ.any(), (mode, variant, nav, rc, msg)


def test_with_the_stand_in_priors_the_windows_are_the_older_entries(lib, five):
    """nav_factors = 0: the bits of icgh_backend_solve_preint_batch (variant 0) and icgh_backend_solve_preint_odo_batch (variant 2)"""
    wins, starts, priors, const, _ = five[0]
    a = _solve(lib, five, 0, nav_factors=0)
    b = psd.solve_preint_batch(lib, wins, starts, priors, 0, variant=0, state_const=const)
    wins, starts, priors, const, results = five[2]
    c = _solve(lib, five, 2, nav_factors=0)
    d = os_.solve_preint_odo_batch(lib, wins, starts, results, priors, 0, variant=2, state_const=const)
    for x, y in ((a, b), (c, d)):
        assert x[0] == 0 and y[0] == 0, (x[1], y[1])
        for w in range(5):
            assert np.array_equal(bits(x[2][w]), bits(y[2][w])) and np.array_equal(bits(x[3][w]), bits(y[3][w])), w
        assert np.array_equal(bits(x[4]), bits(y[4])) and np.array_equal(bits(x[5]), bits(y[5]))
    assert not np.array_equal(bits(a[2][0]), bits(_solve(lib, five, 0)[2][0]))  # (the navigation factors make another problem of it)
