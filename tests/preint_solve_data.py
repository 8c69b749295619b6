"""Shared by the device-preintegration solver tests and profiles/preint_solve_probe.py: icgh_backend_solve_preint_batch on the windows of
prior_solve_data."""
import ctypes as C

import numpy as np

from vio_data import _ptrs, batch_leading_args


def solve_preint_batch(lib, wins, starts, priors, mode, variant=0, state_const=None, robust=None, preint_robust=None, iters=25, prior_weight=100.0, huber=1.0,
                       timer=None):
    """icgh_backend_solve_preint_batch: prior_solve_data.solve_prior_batch's arguments plus the variant of the intervals (0 Normal, 1 Earth) and
    preint_robust[w], the Huber delta on window w's preintegration factors (0 = none)
    -> (rc, message, states, invdepth, summary W x 4, prior cost W x 2, preintegration factors resident on the device)"""
    W = len(wins)
    i32, f64 = (lambda a: np.ascontiguousarray(a, np.int32)), (lambda a: np.ascontiguousarray(a, np.float64))
    args, st, inv, keep = batch_leading_args(wins, starts, iters, prior_weight, huber)
    pr = lambda key, conv: [None if p is None else conv(p[key]) for p in priors]
    p_r, p_nb = i32([0 if p is None else p["r"] for p in priors]), i32([0 if p is None else len(p["size"]) for p in priors])
    p_size, p_index, p_param, p_x0, p_J0, p_e0 = pr("size", i32), pr("index", i32), pr("param", i32), pr("x0", f64), pr("J0", f64), pr("e0", f64)
    rob = f64(np.zeros(W) if robust is None else robust)
    prob = f64(np.zeros(W) if preint_robust is None else preint_robust)
    sc = [None] * W if state_const is None else [None if c is None else i32(c) for c in state_const]
    summ, pcost, ms, err = np.zeros((W, 4)), np.zeros((W, 2)), C.c_double(0), C.create_string_buffer(512)
    n_dev = C.c_int32(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.icgh_backend_solve_preint_batch(*args, p(p_r), p(p_nb), _ptrs(p_size), _ptrs(p_index), _ptrs(p_param), _ptrs(p_x0), _ptrs(p_J0), _ptrs(p_e0), p(rob),
                                             _ptrs(sc), p(summ), p(pcost), C.byref(ms), int(variant), p(prob), C.byref(n_dev), int(mode), err, 512)
    if timer is not None:
        timer.append(ms.value)
    return rc, err.value.decode(), st, inv, summ, pcost, n_dev.value
