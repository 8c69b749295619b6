"""Shared by the navigation-factor solver tests and profiles/nav_solve_probe.py: icgh_backend_solve_nav_batch on the windows of
prior_solve_data (variants 0, 1: states of 16, intervals integrated by the entry) and preint_odo_solve_data (variants 2, 3: states of 17, the
integration results given), with the product's navigation factors in place of the stand-in priors and a GNSS fix on every state."""
import ctypes as C

import numpy as np

import preint_data as pd
import preint_odo_data as od
import preint_odo_solve_data as osd
from ctypes_util import ErrBuf, f64, i32, ptr, ptrs

GNSS_STD = np.array([0.05, 0.05, 0.08])
GNSS_LEVER = np.array([0.12, -0.30, 0.25])


def _qmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def gnss_fixes(win, seed):
    """a fix per state of a vio_data window: the antenna's true position with noise of GNSS_STD; every fourth with an outlier of 20 sigma, so that a
    Huber loss of 1 has members inside and outside its kernel"""
    rng = np.random.RandomState(seed)
    S = np.asarray(win["states"], np.float64)
    blh = np.stack([S[k, :3] + _qmat(S[k, 3:7]) @ GNSS_LEVER + rng.normal(0, GNSS_STD) for k in range(len(S))])
    blh[::4] += 20 * GNSS_STD * rng.choice([-1.0, 1.0], (len(blh[::4]), 3))
    return np.ascontiguousarray(blh)


def nav_factor_count(wins):
    """pose prior + mix prior + error factor per window, a GNSS factor per state"""
    return sum(3 + len(w["states"]) for w in wins)


def solve_nav_batch(lib, wins, starts, priors, mode, variant=0, device_nav=0, nav_factors=1, gnss_huber=0.0, results=None, state_const=None, iters=25,
                    prior_weight=100.0, huber=1.0, timer=None):
    """icgh_backend_solve_nav_batch.  variants 2, 3 take `results`, the integration results of every interval, window after window
    (preint_odo_solve_data.integrate_on_host / integrate_on_device); gnss_huber: a scalar or one delta per window, 0 = no loss
    -> (rc, message, states, invdepth, summary W x 4, prior cost W x 2, navigation factors resident on the device)"""
    W = len(wins)
    odo = variant in (2, 3)  # (anything else is laid out at 16: the entry refuses what it does not know before it reads)
    offsets, imu = [i32(w["offsets"]) for w in wins], [f64(w["imu"]) for w in wins]
    given = osd.result_arrays(wins, results) if odo else [[None] * W] * 7
    st, win, n_int = osd.window_arrays(wins, starts, odo)
    p_r, p_nb, tables, consts = osd.prior_arrays(priors, W, state_const)
    blh = [gnss_fixes(w, 300 + k) for k, w in enumerate(wins)]
    gh = f64(np.broadcast_to(np.asarray(gnss_huber, np.float64), (W,)))
    summ, pcost, ms, err, n_dev = np.zeros((W, 4)), np.zeros((W, 2)), C.c_double(0), ErrBuf(), C.c_int32(-1)
    par9, par19 = f64(pd.PARAMS), f64(od.params19(osd.PARAMS25, od.ABV))
    rc = lib.icgh_backend_solve_nav_batch(
        W, int(variant), ptr(n_int), ptrs(offsets), ptrs(imu), ptr(par9), *osd.as_args(given), ptr(par19), ptrs(st), *osd.as_args(win), C.c_double(prior_weight),
        C.c_double(huber), int(iters), ptr(p_r), ptr(p_nb), *osd.as_args(tables), ptrs(consts), int(nav_factors), ptrs(blh), ptr(f64(GNSS_STD)), ptr(f64(GNSS_LEVER)),
        ptr(gh), ptr(summ), ptr(pcost), C.byref(ms), C.byref(n_dev), int(mode), int(device_nav), *err.args)
    if timer is not None:
        timer.append(ms.value)
    return rc, err.text(), st, win[7], summ, pcost, n_dev.value
