"""icgh_backend_solve_preint_batch without a GPU, on the oracle-backed build of the host layer: mode 0 at the Normal variant is
icgh_backend_solve_prior_batch's mode 0 (the same windows, built by the same code), the Earth variant solves another problem, and the device
modes say which entry the build lacks."""
import ctypes as C

import numpy as np
import pytest

import preint_solve_data as qs
import prior_solve_data as ps
from ctypes_util import bits


@pytest.fixture(scope="module")
def lib():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


@pytest.fixture(scope="module")
def five(oracle):
    return ps.five_windows(oracle)


@pytest.fixture(scope="module")
def normal(lib, five):
    wins, starts, priors, const = five
    return qs.solve_preint_batch(lib, wins, starts, priors, 0, variant=0, state_const=const)


def test_mode0_normal_variant_is_the_prior_entrys_mode0(lib, five, normal):
    wins, starts, priors, const = five
    rc, msg, st, inv, summ, pcost, n_dev = normal
    assert rc == 0 and n_dev == 0, (rc, msg, n_dev)
    rc0, msg0, st0, inv0, summ0, pcost0 = ps.solve_prior_batch(lib, wins, starts, priors, 0, state_const=const)
    assert rc0 == 0, msg0
    ps.check_conditions(summ, pcost, priors)
    for w in range(len(wins)):
        assert np.array_equal(bits(st[w]), bits(st0[w])) and np.array_equal(bits(inv[w]), bits(inv0[w])), w
    assert np.array_equal(bits(summ), bits(summ0)) and np.array_equal(bits(pcost), bits(pcost0))


def test_mode0_earth_variant_solves_another_problem(lib, five, normal):
    wins, starts, priors, const = five
    rc, msg, st, inv, summ, pcost, _ = qs.solve_preint_batch(lib, wins, starts, priors, 0, variant=1, state_const=const)
    assert rc == 0, msg
    assert (summ[:, 2] > 0).all() and (summ[:, 1] < summ[:, 0]).all(), summ  # every window's cost went down
    for w in range(len(wins)):
        assert not np.array_equal(bits(st[w]), bits(normal[2][w])), w
    assert np.array_equal(bits(st[3][1]), bits(starts[3][0][1]))  # a constant state did not move


def test_device_modes_name_the_missing_entry(lib, five):
    wins, starts, priors, _ = five
    for mode in (4, 5):
        rc, msg, st, _, summ, _, n_dev = qs.solve_preint_batch(lib, wins[:2], starts[:2], priors[:2], mode)
        assert rc == -4 and "is not in this build" in msg, (mode, rc, msg)
        assert msg.startswith("icg_preint_set "), (mode, msg)
        assert not summ.any() and np.array_equal(st[0], starts[0][0]) and n_dev <= 0  # nothing was computed
    names = {1: "icg_reproj_solve_windows", 2: "icg_reproj_host_parts_build", 3: "icg_marg_prior_evaluate_resident"}
    for mode, name in names.items():
        rc, msg, _, _, summ, _, _ = qs.solve_preint_batch(lib, wins[:1], starts[:1], priors[:1], mode)
        assert rc == -4 and msg.startswith(name + " ") and not summ.any(), (mode, rc, msg)
    for mode, variant in ((9, 0), (6, 0), (-1, 0), (0, 2)):
        rc, msg, _, _, summ, _, _ = qs.solve_preint_batch(lib, wins[:1], starts[:1], priors[:1], mode, variant=variant)
        assert rc == -1 and "mode" in msg and not summ.any(), (mode, variant, rc, msg)
    # icgh_backend_solve_prior_batch keeps its own mode range
    rc, msg, _, _, _, _ = ps.solve_prior_batch(lib, wins[:1], starts[:1], priors[:1], 4)
    assert rc == -1 and "mode" in msg, (rc, msg)
