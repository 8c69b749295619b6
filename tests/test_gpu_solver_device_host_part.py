"""WindowSolverBatch with the host-factor parts built on the device (setDeviceHostPart) against the host pool: every state and summary is
the same bits in mode 0 (host), 1 (device reduced solve) and 2 (device reduced solve + device host part), on windows with the estimator's
factor mix (icgh_backend_solve_vio_batch) and on the reprojection + pose-prior problems of the other batch tests."""
import ctypes as C

import numpy as np
import pytest

import reduced_solve_utils as ru
import reproj_data as rd
import test_host_part_cpu as thp
import test_host_solver_cpu as ths
import vio_data as vd
from host_part_data import solve_vio_batch
from ctypes_util import bits

pytestmark = pytest.mark.gpu


def _far_start(W, seed=77):
    """a start far from the optimum: metres and half-radians on the poses, m/s on the velocities, e-folds on the inverse depths"""
    rng = np.random.RandomState(seed)
    s = W["states"].copy()
    for k in range(1, len(s)):
        s[k, :7] = rd.pose_plus(s[k, :7], rng.normal(0, [1.0] * 3 + [0.5] * 3))
        s[k, 7:10] += rng.normal(0, 1.0, 3)
    return s, W["invdepth"] * np.exp(rng.normal(0, 1.0, len(W["invdepth"])))


def _first_states(W, K):
    """the leading K states of a window: their intervals and the reprojection factors among them (vio_data keeps landmarks with two
    observations besides the reference, which a window of two states cannot have)"""
    keep = (W["ii"] < K) & (W["jj"] < K)
    lms = np.unique(W["ll"][keep])
    return dict(W, offsets=W["offsets"][:K], imu=np.ascontiguousarray(W["imu"][:W["offsets"][K - 1]]), states=W["states"][:K], invdepth=W["invdepth"][lms],
                obs=np.ascontiguousarray(W["obs"][:, keep]), ii=W["ii"][keep], jj=W["jj"][keep], ll=np.searchsorted(lms, W["ll"][keep]).astype(np.int32))


def test_three_modes_give_identical_bits_on_visual_inertial_windows(oracle):
    import harness
    lib = C.CDLL(harness.HOST_LIB)
    # 2, 3, 4, 8 and 8 states; the last two with the dense factor over their mix blocks (72 columns: past one wave)
    wins = [vd.make_vio_window(oracle, n_intervals=n, per=20, n_lm=30, seed=10 + n + k) for k, n in enumerate((2, 2, 3, 7, 7))]
    wins[0] = _first_states(wins[0], 2)
    assert [len(w["states"]) for w in wins] == [2, 3, 4, 8, 8] and all(w["obs"].shape[1] > 0 for w in wins)
    wins[2] = vd.make_vio_window(oracle, n_intervals=3, per=20, n_lm=30, seed=13)
    starts = [vd.perturbed_start(w, seed=k) for k, w in enumerate(wins)]
    starts[2] = _far_start(wins[2])
    dense = [0, 0, 0, 1, 1]
    res = {}
    for mode in (0, 1, 2):
        rc, msg, st, inv, summ = solve_vio_batch(lib, wins, starts, dense, mode)
        assert rc == 0, (mode, msg)
        res[mode] = (st, inv, summ)
    st0, inv0, summ0 = res[0]
    assert summ0[2, 3] > 0, summ0  # the far start has a rejected step: a re-damped system without a rebuild
    assert (summ0[:, 2] > 0).all() and (summ0[:, 1] < summ0[:, 0]).all(), summ0
    for mode in (1, 2):
        st, inv, summ = res[mode]
        assert np.array_equal(bits(summ), bits(summ0)), (mode, summ, summ0)
        for w in range(len(wins)):
            assert np.array_equal(bits(st[w]), bits(st0[w])) and np.array_equal(bits(inv[w]), bits(inv0[w])), (mode, w)


def test_batch_problems_with_both_device_switches():
    import harness
    lib = C.CDLL(harness.HOST_LIB)
    probs = ths._batch_problems()
    rc, msg, host = thp._parts(lib, probs, 0, 0)
    assert rc == 0, msg
    rc, msg, dev = thp._parts(lib, probs, 1, 1)
    assert rc == 0, msg
    ru.assert_same_results(dev, host)
    assert any(r["summary"][4] + r["summary"][6] > 0 for r in host) and all(r["summary"][3] > 0 for r in host)
    rc, msg, _ = thp._parts(lib, probs, 0, 1)  # the parts are built where the device solve reads them: not without it
    assert rc == -2 and "setDeviceReducedSolve" in msg, (rc, msg)
