"""Shared by the tests of the split preintegration evaluation (Preintegration::evaluateGiven on the host, icg_preint_set /
icg_preint_evaluate_resident on the device): the intervals, the four evaluation points and the call of icgh_backend_preint_eval_split."""

import numpy as np

import preint_data as pd
import reproj_data as rd
from ctypes_util import ErrBuf, ptr

POINT_KINDS = ("end_state", "perturbed", "bias_equal", "large_bias_step")


def intervals(lens, seed0=20):
    """-> (imu rows per interval, start state per interval)"""
    imus = [pd.make_interval(n, seed=seed0 + i) for i, n in enumerate(lens)]
    states = [pd.state(p=(i, 1, 0), v=(2, 0.1 * i, 0)) for i in range(len(lens))]
    return imus, states


def eval_point(kind, state0, cur):
    """pose0[7] mix0[9] pose1[7] mix1[9] for an interval that starts at state0 and whose integration ended at cur.  delta.bg of the
    integration is state0's bg: end_state and bias_equal have bg0 == delta.bg exactly (rotation angle 0), perturbed a difference of 1e-4 rad/s,
    large_bias_step one of about 0.1 rad/s."""
    pose0, mix0 = pd.split(np.asarray(state0, np.float64))
    pose1, mix1 = pd.split(np.asarray(cur, np.float64))
    if kind == "end_state":
        pass
    elif kind == "perturbed":
        pose1 = rd.pose_plus(pose1, np.array([0.01, -0.02, 0.01, 0.001, 0.002, -0.001]))
        pose0 = rd.pose_plus(pose0, np.array([-0.005, 0.004, 0.002, -0.002, 0.001, 0.0015]))
        mix0 = mix0 + np.array([0.01, -0.02, 0.005, 1e-4, -0.5e-4, 0.7e-4, 1e-3, -2e-3, 0.5e-3])
        mix1 = mix1 + np.array([-0.01, 0.01, 0.002, -1e-5, 2e-5, 1e-5, 1e-4, 1e-4, -1e-4])
    elif kind == "bias_equal":
        pose1 = rd.pose_plus(pose1, np.array([0.02, 0.01, -0.01, -0.002, 0.001, 0.003]))
        mix0 = mix0 + np.array([0.02, 0.01, -0.01, 0, 0, 0, 2e-3, 1e-3, -1e-3])
    elif kind == "large_bias_step":
        pose1 = rd.pose_plus(pose1, np.array([0.01, -0.02, 0.01, 0.001, 0.002, -0.001]))
        mix0 = mix0 + np.array([0, 0, 0, 0.06, -0.07, 0.04, 0, 0, 0])
    else:
        raise ValueError(kind)
    return np.concatenate([pose0, mix0, pose1, mix1])


def eval_split(lib, variant, imus, states, points, q_corr_in=None):
    """icgh_backend_preint_eval_split -> dict of arrays (one row per interval)"""
    n = len(imus)
    offsets = np.cumsum([0] + [len(m) for m in imus]).astype(np.int32)
    total = int(offsets[-1])
    imu = np.ascontiguousarray(np.concatenate(imus), np.float64)
    s0 = np.ascontiguousarray(np.stack(states), np.float64)
    pts = np.ascontiguousarray(np.stack(points), np.float64)
    qin = None if q_corr_in is None else np.ascontiguousarray(q_corr_in, np.float64).reshape(n, 4)
    o = dict(cur=np.zeros((n, 16)), r_eval=np.zeros((n, 15)), J_eval=np.zeros((n, 480)), r_given=np.zeros((n, 15)), J_given=np.zeros((n, 480)), q_corr=np.zeros((n, 4)),
             q_nn=np.zeros((n, 4)), sqrt_info=np.zeros((n, 225)), delta=np.zeros((n, 16)), jac=np.zeros((n, 225)), dt=np.zeros(n), env=np.zeros((n, 4)),
             pn_off=np.zeros(n + 1, np.int32), pn=np.zeros((max(total, 1), 4)), ok=np.full(n, -1, np.int32))
    err = ErrBuf()
    rc = lib.icgh_backend_preint_eval_split(int(variant), n, ptr(offsets), ptr(imu), ptr(s0), ptr(np.ascontiguousarray(pd.PARAMS, np.float64)), ptr(pts), ptr(qin),
                                            ptr(o["cur"]), ptr(o["r_eval"]), ptr(o["J_eval"]), ptr(o["r_given"]), ptr(o["J_given"]), ptr(o["q_corr"]), ptr(o["q_nn"]),
                                            ptr(o["sqrt_info"]), ptr(o["delta"]), ptr(o["jac"]), ptr(o["dt"]), ptr(o["env"]), ptr(o["pn_off"]), ptr(o["pn"]),
                                            max(total, 1), ptr(o["ok"]), *err.args)
    assert rc == 0, (rc, err.value)
    o["pn"] = o["pn"][:int(o["pn_off"][-1])]
    o["points"] = pts
    o["variant"] = np.full(n, int(variant), np.int32)
    return o


def current_states(lib, variant, imus, states):
    """the integration's own end state per interval"""
    return list(eval_split(lib, variant, imus, states, [np.concatenate([s, s]) for s in states])["cur"])
