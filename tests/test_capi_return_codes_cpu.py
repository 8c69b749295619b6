"""The return codes and messages of the host layer's C entries (host/capi_*.cc) that the Python drivers branch on, on the oracle-backed host
layer and at the smallest input that reaches each path: -4 and "<entry> is not in this build" for a device mode without its entry point,
-1 for a mode that is neither 0 nor 1 and for invalid arguments (n_windows = 0, a NULL batch).  The other CPU tests only ask for rc != 0
there.  (rc 0 on a valid call, i.e. the unprepared / unintegrated factor DID fail, is asserted by the drivers in backend_utils.py.)"""
import ctypes as C

import numpy as np

import marg_factor_data as mf
import marg_linearize_data as ml
import preint_data as pd
from ctypes_util import ErrBuf, ptr

MARK = -7.25


def _lib():
    from stream_utils import ORACLE_HOST
    return C.CDLL(ORACLE_HOST)


def _one_interval():
    imu = np.ascontiguousarray(pd.make_interval(5, seed=3))
    s0 = np.ascontiguousarray(pd.state()[None, :])
    ep = np.ascontiguousarray(np.concatenate([s0[0], s0[0]])[None, :])
    return np.array([0, 5], np.int32), imu, s0, np.ascontiguousarray(pd.PARAMS), ep


def test_preintegration_device_entries_refuse_with_minus_4():
    lib = _lib()
    off, imu, s0, params, ep = _one_interval()
    out = [np.full(k, MARK) for k in (16, 15, 480, 15, 480, 225, 225)]
    ok = [np.full(1, 77, np.int32), np.full(1, 77, np.int32)]
    err = ErrBuf()
    rc = lib.icgh_backend_preint_device(1, 1, ptr(off), ptr(imu), ptr(s0), ptr(params), ptr(ep), *[ptr(a) for a in out], ptr(ok[0]), ptr(ok[1]), *err.args)
    assert rc == -4 and err.value == b"icg_preint_evaluate_batch is not in this build", (rc, err.value)
    assert all(np.all(a == MARK) for a in out) and ok[0][0] == 77 and ok[1][0] == 77
    out6 = np.full(6, MARK)
    err = ErrBuf()
    rc = lib.icgh_backend_preint_eval_time(1, 1, ptr(off), ptr(imu), ptr(s0), ptr(params), ptr(ep), 1, 1, ptr(out6), *err.args)
    assert rc == -4 and err.value == b"icg_preint_evaluate_batch is not in this build", (rc, err.value)
    assert np.all(out6 == MARK)


def test_marg_linearize_return_codes():
    lib = _lib()
    one = ml.batch()[3:4]  # one window, P = 1, m = 0
    assert [(s["P"], s["m"]) for s in one] == [(1, 0)]
    rc, msg, out, sec = ml.backend_marg_linearize(lib, 1, one, mark=MARK)
    assert rc == -4 and msg == "icg_marg_linearize_batch is not in this build", (rc, msg)
    for mode in (2, -1):
        rc, msg, out, sec = ml.backend_marg_linearize(lib, mode, one, mark=MARK)
        assert rc == -1 and msg == "icgh_backend_marg_linearize: mode is neither 0 (host) nor 1 (device)", (rc, msg)
        assert np.all(out["J0"] == MARK) and np.all(sec == MARK)
    P, m, H, b = ml.pack(one)
    J0, e0, sec = np.full(1, MARK), np.full(1, MARK), np.full(2, MARK)
    err = ErrBuf()

    def call(n, J0_):
        return lib.icgh_backend_marg_linearize(0, n, ptr(P), ptr(m), ptr(H), ptr(b), C.c_double(ml.EPS), 1, 0, None, None, ptr(J0_), ptr(e0), None, None, None,
                                               ptr(sec), *err.args)

    assert call(0, J0) == -1 and err.value == b"icgh_backend_marg_linearize: invalid argument", err.value  # n_windows = 0
    assert call(1, None) == -1 and err.value == b"icgh_backend_marg_linearize: invalid argument", err.value  # a required output missing
    assert np.all(J0 == MARK) and np.all(e0 == MARK) and np.all(sec == MARK)
    bad = [dict(one[0], m=1)]  # m = P
    rc, msg, out, sec = ml.backend_marg_linearize(lib, 0, bad, mark=MARK)
    assert rc == -1 and msg == "icgh_backend_marg_linearize: window 0 is not a valid system", (rc, msg)
    rc, msg, out, sec = ml.backend_marg_linearize(lib, 0, one, reps=0)
    assert rc == 0 and sec[0] >= 0 and sec[1] == 0, (rc, msg, sec)  # a lone pass is timed; no kernel time in the host mode


def test_marg_factor_return_codes():
    lib = _lib()
    p = mf.make_prior([1], 1)
    x = [[mf.make_x(p, 1)]]
    rc, msg, res, jac, grad, sq, sec = mf.backend_marg_factor(lib, 1, [p], x, mark=MARK)
    assert rc == -4 and msg == "icg_marg_prior_set is not in this build", (rc, msg)
    for mode in (2, -1):
        rc, msg, res, jac, grad, sq, sec = mf.backend_marg_factor(lib, mode, [p], x, mark=MARK)
        assert rc == -1 and msg == "icgh_backend_marg_factor: mode is neither 0 (host) nor 1 (device)", (rc, msg)
        assert np.all(res == MARK) and np.all(sec == MARK)
    a = mf.pack([p])
    xs, res, sec = np.ascontiguousarray(x[0][0], np.float64), np.full(1, MARK), np.full(2, MARK)
    err = ErrBuf()

    def call(n, n_points):
        return lib.icgh_backend_marg_factor(0, n, ptr(a["r"]), ptr(a["block_off"]), ptr(a["block_size"]), ptr(a["block_index"]), ptr(a["x0"]), ptr(a["J0"]),
                                            ptr(a["e0"]), n_points, ptr(xs), 1, 0, ptr(res), None, None, None, ptr(sec), *err.args)

    assert call(0, 1) == -1 and err.value == b"icgh_backend_marg_factor: invalid argument", err.value  # n_windows = 0
    assert call(1, 0) == -1 and err.value == b"icgh_backend_marg_factor: invalid argument", err.value  # n_points = 0
    assert np.all(res == MARK) and np.all(sec == MARK)
    bad = dict(p, index=np.array([1], np.int32))  # index + local size > r
    rc, msg, res, *_ = mf.backend_marg_factor(lib, 0, [bad], x, mark=MARK)
    assert rc == -1 and msg == "icgh_backend_marg_factor: window 0 is not a valid prior" and np.all(res == MARK), (rc, msg)
    rc, msg, res, jac, grad, sq, sec = mf.backend_marg_factor(lib, 0, [p], x, reps=0)
    assert rc == 0 and sec[0] == 0 and sec[1] >= 0, (rc, msg, sec)  # no set in the host mode; a lone pass is timed


def test_batch_entries_reject_a_null_batch():
    lib = _lib()
    lib.icgh_batch_dump.restype = C.c_long
    err = ErrBuf(64)
    assert lib.icgh_batch_dump(None, 0, 0, None, C.c_long(0)) == -1
    assert lib.icgh_batch_replay(None, 1, *err.args) == -1 and lib.icgh_batch_replay_concurrent(None, 1, *err.args) == -1
    assert lib.icgh_batch_stats(None, 0, None) == -1 and lib.icgh_batch_engine(None) == -1 and lib.icgh_batch_groups(None) == 0
    assert err.value == b""
