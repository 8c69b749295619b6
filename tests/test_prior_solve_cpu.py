"""icgh_backend_solve_prior_batch without a GPU, on the oracle-backed build of the host layer: mode 0 solves windows with a marginalization
prior given as arrays, the prior's own Evaluate agrees with its restatement in numpy at the start and at the end, a robustified prior is
accepted, and the device modes say which entry the build lacks."""
import ctypes as C

import numpy as np
import pytest

import prior_solve_data as ps
from ctypes_util import bits


@pytest.fixture(scope="module")
def lib():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


@pytest.fixture(scope="module")
def five(oracle):
    return ps.five_windows(oracle)


def test_mode0_final_cost_is_what_the_priors_evaluate_predicts(lib, five):
    wins, starts, priors, const = five
    rc, msg, st, inv, summ, pcost = ps.solve_prior_batch(lib, wins, starts, priors, 0, state_const=const)
    assert rc == 0, msg
    ps.check_conditions(summ, pcost, priors)
    for w, p in enumerate(priors):
        if p is None:
            assert not pcost[w].any()
            continue
        # the entry's values come from the cost function's Evaluate; the restatement sums in another order: a few ulps of r terms
        for at, states in ((0, starts[w][0]), (1, st[w])):
            assert abs(pcost[w, at] - ps.prior_cost(p, states)) <= 1e-10 * max(1.0, pcost[w, at]), (w, at, pcost[w])
        # the prior is part of the window's cost at both ends, and the solve lowered the whole
        assert summ[w, 0] >= pcost[w, 0] and summ[w, 1] >= pcost[w, 1] and summ[w, 1] < summ[w, 0], (w, summ[w], pcost[w])
    # the same windows without their priors reach another optimum: the prior took part in the solve
    rc, msg, st_n, _, summ_n, _ = ps.solve_prior_batch(lib, wins, starts, [None] * len(wins), 0, state_const=const)
    assert rc == 0, msg
    assert np.array_equal(bits(st_n[1]), bits(st[1])) and summ_n[1, 1] == summ[1, 1]  # (the window without a prior: the same solve)
    for w, p in enumerate(priors):
        if p is not None:
            assert summ_n[w, 1] < summ[w, 1] and not np.array_equal(bits(st_n[w]), bits(st[w])), w
    # a constant state did not move
    assert np.array_equal(bits(st[3][1]), bits(starts[3][0][1]))


def test_device_modes_name_the_missing_entry(lib, five):
    wins, starts, priors, const = five
    names = {1: "icg_reproj_solve_windows", 2: "icg_reproj_host_parts_build", 3: "icg_marg_prior_evaluate_resident"}
    for mode in (1, 2, 3):
        rc, msg, st, _, summ, _ = ps.solve_prior_batch(lib, wins[:2], starts[:2], priors[:2], mode)
        assert rc == -4 and "is not in this build" in msg, (mode, rc, msg)
        assert msg.startswith(names[mode] + " "), (mode, msg)
        assert not summ.any() and np.array_equal(st[0], starts[0][0])  # nothing was computed
    rc, msg, _, _, _, _ = ps.solve_prior_batch(lib, wins[:1], starts[:1], priors[:1], 7)
    assert rc == -1 and "mode" in msg, (rc, msg)


def test_robustified_prior_is_accepted(lib, five):
    wins, starts, priors, _ = five
    rc, msg, st, _, summ, pcost = ps.solve_prior_batch(lib, wins[:1], starts[:1], priors[:1], 0, robust=[0.5])
    assert rc == 0, msg
    assert summ[0, 2] > 0 and summ[0, 1] < summ[0, 0] and pcost[0, 0] > 0, (summ, pcost)
    rc, msg, st_q, _, summ_q, _ = ps.solve_prior_batch(lib, wins[:1], starts[:1], priors[:1], 0)
    assert rc == 0, msg
    assert summ[0, 0] < summ_q[0, 0]  # the loss is in the cost: Huber of a squared norm above delta^2 is below it
