"""Inputs and drivers of the M3 -> M4 hand-off tests (icg_marg_linearize_batch_keep, icg_marg_prior_set_from_kept,
icgh_backend_marg_handoff): the heterogeneous batch of reduced systems whose linearization is kept, the prior set built on it, and the
ctypes driver of the host-layer entry."""
import ctypes as C

import numpy as np

import marg_factor_data as mf
from backend_utils import marg_problem_args
import marg_linearize_data as ml
from ctypes_util import ErrBuf, ptr

# (P, m) of the kept batch: r = 1, 6, 61, 142 (the last size whose working matrix fits LDS) and 143 (the first on global scratch), a
# rank-deficient window (r = 142) and a second window with m = 0 (r = 30)
KEPT_SHAPES = [(1, 0), (8, 2), (67, 6), (157, 15), (158, 15)]
KEPT_R = [1, 6, 61, 142, 143, 142, 30]


def kept_systems():
    s = [ml.spd_system(P, m, 20 + k) for k, (P, m) in enumerate(KEPT_SHAPES)] + [ml.rank_deficient_system(6), ml.spd_system(30, 0, 31)]
    assert [x["P"] - x["m"] for x in s] == KEPT_R
    return s


# window w of the set takes kept window SRC[w]: a non-identity permutation, kept window 3 twice, one window from the host
SRC = [3, 0, 2, -1, 1, 3, 4]


def set_priors():
    """block layouts of tests/test_gpu_marg_prior_resident.py (blocks out of column order, uncovered columns, a single pose whose
    point takes dq.w < 0) for the windows of SRC; J0 / e0 of the kept windows are filled in by the test, the host window keeps its own"""
    rng = np.random.RandomState(5)
    s61, s142, s255, s143 = [7, 9] * 4 + [1], mf.C2_SIZES, [7, 9] * 17, mf.C2_SIZES + [1]
    priors = [mf.make_prior(s142, 44, order=rng.permutation(len(s142))), mf.make_prior([1], 41), mf.make_prior(s61, 43, order=rng.permutation(len(s61))),
              mf.make_prior(s255, 45, order=rng.permutation(len(s255)), gap_after=3, gap=2), mf.make_prior([7], 42),
              mf.make_prior(s142, 46), mf.make_prior(s143, 47, order=rng.permutation(len(s143)))]
    assert [p["r"] for p in priors] == [142, 1, 61, 257, 6, 142, 143]
    return priors


def set_points(priors, seed):
    pts = [mf.make_x(p, seed + k, negate=(0, 2)) for k, p in enumerate(priors)]
    assert mf.dq_w(priors[4], pts[4])[0] < 0  # the single pose takes the dq.w < 0 branch
    return pts


def backend_marg_handoff(lib, P, n_windows, mode, dense_window=-1, jitter=1e-3, huber=1.0, prior_weight=100.0, host_threads=4, seed=5, perturb=1e-3,
                         solve_iters=0):
    """icgh_backend_marg_handoff (capi_marg_handoff.cc) on n_windows jittered copies of problem P (marg_data.make_problem).  mode 0: the
    priors are shipped, 1: kept and handed off, 3: kept, released before the set.  Returns (rc, message, dict of outputs)."""
    args, K, L = marg_problem_args(P, huber, prior_weight)
    cap = 6 * K + L + 7
    counts, timers = np.zeros(7, np.int32), np.zeros(5)
    res, grad = np.zeros(n_windows * cap), np.zeros(n_windows * cap)
    sq, sq_res = np.zeros(n_windows), np.zeros(n_windows)
    states, inv_out, summ = np.zeros((n_windows, K, 7)), np.zeros((n_windows, L)), np.zeros((n_windows, 4))
    err = ErrBuf()
    rc = lib.icgh_backend_marg_handoff(int(mode), int(n_windows), int(dense_window), C.c_double(jitter), *args, int(host_threads), C.c_uint64(seed),
                                       C.c_double(perturb), int(solve_iters), ptr(counts), ptr(res), ptr(grad), ptr(sq), ptr(sq_res), ptr(states), ptr(inv_out), ptr(summ),
                                       ptr(timers), *err.args)
    g, R = int(counts[0]), int(counts[1])
    out = dict(priors=g, residuals=res[:R], gradient=grad[:R], sq_norm=sq[:g], sq_norm_resident=sq_res[:g], handed_off=int(counts[2]), tagged=int(counts[3]),
               structured=int(counts[4]), dense=int(counts[5]), solver_handed_off=int(counts[6]), states=states[:g], invdepth=inv_out[:g], summary=summ[:g],
               timers_ms=timers)
    return rc, err.text(), out
