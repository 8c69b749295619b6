"""icgh_backend_solve_preint_odo_batch without a GPU, on the oracle-backed build of the host layer: the five windows of prior_solve_data (2 to
8 states, one without a prior, one with a constant state, one far start with rejected steps) with 17-wide states, 10-wide mix blocks and
PreintegrationOdoFactors built from integration results of preint_odo_data.integrate_ld in float64.  Mode 0 solves them at both variants,
EarthOdo is another problem than Odo, the device modes say which entry the build lacks, invalid modes and variants are refused."""
import ctypes as C

import numpy as np
import pytest

import preint_odo_data as od
import preint_odo_solve_data as os_
import prior_solve_data as ps
from ctypes_util import bits


@pytest.fixture(scope="module")
def lib():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


@pytest.fixture(scope="module")
def five(oracle):
    return os_.five_windows(oracle)


@pytest.fixture(scope="module")
def results(five):
    wins, starts, _, _ = five
    return {v: os_.integrate_on_host(v, wins, starts) for v in od.VARIANTS}


@pytest.fixture(scope="module")
def solved(lib, five, results):
    wins, starts, priors, const = five
    return {v: os_.solve_preint_odo_batch(lib, wins, starts, results[v], priors, 0, variant=v, state_const=const) for v in od.VARIANTS}


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_mode0_solves_the_five_windows(five, solved, variant):
    wins, starts, priors, const = five
    rc, msg, st, inv, summ, pcost, n_dev = solved[variant]
    assert rc == 0 and n_dev == 0, (rc, msg, n_dev)
    assert [len(s) for s in st] == [2, 3, 4, 8, 8]
    ps.check_conditions(summ, pcost, priors)  # every window's cost goes down, the far start rejects a step, every prior has a cost at the start
    start17 = os_.odo_window(wins[3], starts[3])[1]
    assert np.array_equal(bits(st[3][1]), bits(start17[1]))  # a constant state did not move
    assert not np.array_equal(bits(st[3][2]), bits(start17[2]))
    assert any(s[0, 16] != od.SODO or s[1, 16] != od.SODO for s in st)  # the scale factor is a free parameter of the solve


def test_earth_odo_solves_another_problem(five, solved):
    for w in range(len(five[0])):
        assert not np.array_equal(bits(solved[od.ODO][2][w]), bits(solved[od.EARTH_ODO][2][w])), w


def test_device_modes_name_the_missing_entry(lib, five, results):
    wins, starts, priors, _ = five
    res = results[od.ODO][:3]  # (the intervals of the first two windows: 1 + 2)
    for mode in (4, 5):
        rc, msg, st, _, summ, _, n_dev = os_.solve_preint_odo_batch(lib, wins[:2], starts[:2], res, priors[:2], mode)
        assert rc == -4 and msg.startswith("icg_preint_odo_set is not in this build"), (mode, rc, msg)
        assert not summ.any() and np.array_equal(st[0], os_.odo_window(wins[0], starts[0])[1]) and n_dev <= 0  # nothing was computed
    names = {1: "icg_reproj_solve_windows", 2: "icg_reproj_host_parts_build", 3: "icg_marg_prior_evaluate_resident"}
    for mode, name in names.items():
        rc, msg, _, _, summ, _, _ = os_.solve_preint_odo_batch(lib, wins[:1], starts[:1], res[:1], priors[:1], mode)
        assert rc == -4 and msg.startswith(name + " ") and not summ.any(), (mode, rc, msg)


def test_invalid_modes_and_variants_are_refused(lib, five, results):
    wins, starts, priors, _ = five
    res = results[od.ODO][:1]
    for mode, variant in ((9, 2), (6, 2), (-1, 2), (0, 0), (0, 1), (0, 4)):
        rc, msg, _, _, summ, _, _ = os_.solve_preint_odo_batch(lib, wins[:1], starts[:1], res, priors[:1], mode, variant=variant)
        assert rc == -1 and "mode" in msg and not summ.any(), (mode, variant, rc, msg)
