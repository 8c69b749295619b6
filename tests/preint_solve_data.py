"""Shared by the device-preintegration solver tests and profiles/preint_solve_probe.py: icgh_backend_solve_preint_batch on the windows of
prior_solve_data."""
import ctypes as C

import numpy as np

from ctypes_util import f64, ptr
from prior_solve_data import call_batch


def solve_preint_batch(lib, wins, starts, priors, mode, variant=0, state_const=None, robust=None, preint_robust=None, iters=25, prior_weight=100.0, huber=1.0,
                       timer=None):
    """icgh_backend_solve_preint_batch: prior_solve_data.solve_prior_batch's arguments plus the variant of the intervals (0 Normal, 1 Earth) and
    preint_robust[w], the Huber delta on window w's preintegration factors (0 = none)
    -> (rc, message, states, invdepth, summary W x 4, prior cost W x 2, preintegration factors resident on the device)"""
    prob, n_dev = f64(np.zeros(len(wins)) if preint_robust is None else preint_robust), C.c_int32(-1)
    out = call_batch(lib.icgh_backend_solve_preint_batch, wins, starts, mode, iters, prior_weight, huber, timer, priors, state_const, robust,
                     after=[int(variant), ptr(prob), C.byref(n_dev)])
    return (*out, n_dev.value)
