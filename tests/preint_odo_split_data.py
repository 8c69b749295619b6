"""Shared by the tests of the split odometer preintegration evaluation (PreintegrationOdo::evaluateGiven on the host, icg_preint_odo_set /
icg_preint_odo_evaluate_resident on the device): the five kinds of evaluation point and the call of icgh_backend_preint_odo_eval_split,
which builds its factors from GIVEN integration results (dicts with variant, delta 20, jac 19x19, cov 19x19, dt, pn rows x 4, iewn 3)."""

import numpy as np

import preint_odo_data as od
import reproj_data as rd
from ctypes_util import ErrBuf, f64, i32, ptr

POINT_KINDS = ("end_state", "perturbed", "bias_equal", "large_bias_step", "sodo_equal")


def eval_point(kind, delta20, cur16, s0_17):
    """pose0[7] mix0[10] pose1[7] mix1[10] for an interval that started at s0_17 and whose integration ended at cur16 with delta20.
    delta.bg / delta.sodo of the integration are the start state's: end_state and bias_equal have bg0 == delta.bg exactly (rotation angle
    0), perturbed a difference of 1e-4 rad/s, large_bias_step one of about 0.1 rad/s; sodo_equal has sodo0 == delta.sodo exactly (the
    first-order scale correction of s vanishes) with sodo1 != sodo0, every other kind that moves mix0 moves sodo0 too."""
    delta20, cur16, s0 = np.asarray(delta20, np.float64), np.asarray(cur16, np.float64), np.asarray(s0_17, np.float64)
    pose0, pose1 = s0[:7].copy(), cur16[:7].copy()
    mix0 = np.concatenate([s0[7:10], delta20[10:16], [delta20[19]]])
    mix1 = np.concatenate([cur16[7:10], delta20[10:16], [delta20[19]]])
    if kind == "end_state":
        pass
    elif kind == "perturbed":
        pose1 = rd.pose_plus(pose1, np.array([0.01, -0.02, 0.01, 0.001, 0.002, -0.001]))
        pose0 = rd.pose_plus(pose0, np.array([-0.005, 0.004, 0.002, -0.002, 0.001, 0.0015]))
        mix0 = mix0 + np.array([0.01, -0.02, 0.005, 1e-4, -0.5e-4, 0.7e-4, 1e-3, -2e-3, 0.5e-3, 5e-4])
        mix1 = mix1 + np.array([-0.01, 0.01, 0.002, -1e-5, 2e-5, 1e-5, 1e-4, 1e-4, -1e-4, -3e-4])
    elif kind == "bias_equal":
        pose1 = rd.pose_plus(pose1, np.array([0.02, 0.01, -0.01, -0.002, 0.001, 0.003]))
        mix0 = mix0 + np.array([0.02, 0.01, -0.01, 0, 0, 0, 2e-3, 1e-3, -1e-3, 2e-4])
    elif kind == "large_bias_step":
        pose1 = rd.pose_plus(pose1, np.array([0.01, -0.02, 0.01, 0.001, 0.002, -0.001]))
        mix0 = mix0 + np.array([0, 0, 0, 0.06, -0.07, 0.04, 0, 0, 0, 1e-3])
    elif kind == "sodo_equal":
        pose1 = rd.pose_plus(pose1, np.array([0.01, 0.02, -0.01, 0.002, -0.001, 0.001]))
        mix0 = mix0 + np.array([0.01, 0.0, -0.01, 2e-5, 1e-5, -3e-5, 1e-3, 0, -1e-3, 0])
        mix1 = mix1 + np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 2e-3])
    else:
        raise ValueError(kind)
    return np.concatenate([pose0, mix0, pose1, mix1])


def eval_split(lib, results, points, par25=None, abv=od.ABV, q_corr_in=None, q_nn_in=None):
    """icgh_backend_preint_odo_eval_split on a list of integration results -> dict of arrays (one row per factor), with what
    icg_preint_odo_set takes (variant, delta, jac, sqrt_info, dt, env, q_nn, pn_rows per factor) beside the evaluations"""
    n = len(results)
    variant = i32([r["variant"] for r in results])
    delta = f64(np.stack([np.asarray(r["delta"], np.float64).reshape(20) for r in results]))
    jac = f64(np.stack([np.asarray(r["jac"], np.float64).reshape(361) for r in results]))
    cov = f64(np.stack([np.asarray(r["cov"], np.float64).reshape(361) for r in results]))
    dt = f64([float(r["dt"]) for r in results])
    iewn = f64(np.stack([np.asarray(r["iewn"], np.float64).reshape(3) for r in results]))
    rows = [np.asarray(r["pn"], np.float64).reshape(-1, 4) if r["variant"] == od.EARTH_ODO else np.zeros((0, 4)) for r in results]
    pn_off = i32(np.cumsum([0] + [len(r) for r in rows]))
    pn = f64(np.concatenate(rows + [np.zeros((1, 4))]))  # (a valid pointer for a list without rows)
    pts = f64(np.stack(points)).reshape(n, 34)
    qin = None if q_corr_in is None else f64(q_corr_in).reshape(n, 4)
    qnin = None if q_nn_in is None else f64(q_nn_in).reshape(n, 4)
    par19 = f64(od.params19(od.params25() if par25 is None else par25, abv))
    o = dict(r_eval=np.zeros((n, 19)), J_eval=np.zeros((n, 646)), r_given=np.zeros((n, 19)), J_given=np.zeros((n, 646)), q_corr=np.zeros((n, 4)),
             q_nn=np.zeros((n, 4)), sqrt_info=np.zeros((n, 361)), env=np.zeros((n, 4)), ok=np.full(n, -1, np.int32))
    err = ErrBuf()
    rc = lib.icgh_backend_preint_odo_eval_split(n, ptr(variant), ptr(par19), ptr(delta), ptr(jac), ptr(cov), ptr(dt), ptr(pn_off), ptr(pn), ptr(iewn),
                                                ptr(pts), ptr(qin), ptr(qnin), ptr(o["r_eval"]), ptr(o["J_eval"]), ptr(o["r_given"]), ptr(o["J_given"]),
                                                ptr(o["q_corr"]), ptr(o["q_nn"]), ptr(o["sqrt_info"]), ptr(o["env"]), ptr(o["ok"]), *err.args)
    assert rc == 0, (rc, err.value)
    o.update(points=pts, variant=variant, delta=delta, jac=jac, dt=dt, pn_rows=rows)
    return o


def j_blocks(J):
    """n x 646 -> the four blocks n x 19 x (7, 10, 7, 10)"""
    J = np.asarray(J).reshape(-1, 646)
    return [J[:, a:b].reshape(len(J), 19, w) for a, b, w in ((0, 133, 7), (133, 323, 10), (323, 456, 7), (456, 646, 10))]
