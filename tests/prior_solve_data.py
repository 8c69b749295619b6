"""Shared by the device-prior tests and profiles/prior_solve_probe.py: marginalization priors over the states of vio_data windows as plain
arrays, icgh_backend_solve_prior_batch, and the prior's cost restated in numpy."""
import ctypes as C

import numpy as np

from ctypes_util import ErrBuf, f64, i32, ptr, ptrs
from vio_data import batch_leading_args


def make_prior(win, states, seed, weight=10.0, e0_scale=0.5):
    """A prior over the pose and mix blocks of the given states of a vio_data window, linearized at the window's true states: the blocks
    listed in a shuffled order, their columns handed out in another; J0 = weight (I + 0.25 U), U uniform in (-1, 1); e0 normal."""
    rng = np.random.RandomState(seed)
    blocks = [(2 * k, 7) for k in states] + [(2 * k + 1, 9) for k in states]
    blocks = [blocks[i] for i in rng.permutation(len(blocks))]
    index, col = [0] * len(blocks), 0
    for b in rng.permutation(len(blocks)):
        index[b] = col
        col += 6 if blocks[b][1] == 7 else 9
    r = col
    x0 = [win["states"][c // 2, 7:] if c % 2 else win["states"][c // 2, :7] for c, _ in blocks]
    return dict(r=r, size=np.array([s for _, s in blocks], np.int32), index=np.array(index, np.int32), param=np.array([c for c, _ in blocks], np.int32),
                x0=np.ascontiguousarray(np.concatenate(x0)), J0=np.ascontiguousarray(weight * (np.eye(r) + 0.25 * rng.uniform(-1, 1, (r, r)))),
                e0=rng.normal(0, e0_scale, r))


def prior_cost(prior, states):
    """0.5 |e0 + J0 dx|^2 at states (K x 16) with dx as MarginalizationFactor::Evaluate forms it"""
    dx, off = np.zeros(prior["r"]), 0
    for size, index, code in zip(prior["size"], prior["index"], prior["param"]):
        x0 = prior["x0"][off:off + size]
        off += size
        x = states[code // 2, 7:] if code % 2 else states[code // 2, :7]
        if size == 7:
            q0, q = x0[3:], x[3:]
            a = np.array([-q0[0], -q0[1], -q0[2], q0[3]]) / (q0 @ q0)
            dq = np.array([a[3] * q[0] + a[0] * q[3] + a[1] * q[2] - a[2] * q[1], a[3] * q[1] + a[1] * q[3] + a[2] * q[0] - a[0] * q[2],
                           a[3] * q[2] + a[2] * q[3] + a[0] * q[1] - a[1] * q[0], a[3] * q[3] - a[0] * q[0] - a[1] * q[1] - a[2] * q[2]])
            dx[index:index + 3] = x[:3] - x0[:3]
            dx[index + 3:index + 6] = (-2.0 if dq[3] < 0 else 2.0) * dq[:3]
        else:
            dx[index:index + size] = x - x0
    e = prior["e0"] + prior["J0"] @ dx
    return 0.5 * float(e @ e)


def call_batch(entry, wins, starts, mode, iters, prior_weight, huber, timer, priors=None, state_const=None, robust=None, before=(), after=()):
    """One of the host layer's batch solves on vio_data windows from the given (states, invdepth) starts:
    entry(W .. iters, *before, [prior_r .. state_const,] summary, [prior cost,] &ms, *after, mode, err, errlen); the bracketed arguments
    when priors (a list of make_prior's dicts or None) is given.  A list given as timer receives the entry's own time of the solve in ms
    -> (rc, message, states, invdepth, summary W x 4, prior cost W x 2 or None)"""
    W = len(wins)
    args, st, inv, keep = batch_leading_args(wins, starts, iters, prior_weight, huber)
    args += before
    summ, pcost, ms, err = np.zeros((W, 4)), None, C.c_double(0), ErrBuf()
    if priors is not None:
        pr = lambda key, conv: [None if p is None else conv(p[key]) for p in priors]
        p_r, p_nb = i32([0 if p is None else p["r"] for p in priors]), i32([0 if p is None else len(p["size"]) for p in priors])
        tables = [pr("size", i32), pr("index", i32), pr("param", i32), pr("x0", f64), pr("J0", f64), pr("e0", f64)]
        rob = f64(np.zeros(W) if robust is None else robust)
        tables.append([None] * W if state_const is None else [None if c is None else i32(c) for c in state_const])
        pcost = np.zeros((W, 2))
        args += [ptr(p_r), ptr(p_nb), *[ptrs(t) for t in tables[:6]], ptr(rob), ptrs(tables[6]), ptr(summ), ptr(pcost)]
    else:
        args.append(ptr(summ))
    rc = entry(*args, C.byref(ms), *after, int(mode), *err.args)
    if timer is not None:
        timer.append(ms.value)
    return rc, err.text(), st, inv, summ, pcost


def solve_prior_batch(lib, wins, starts, priors, mode, state_const=None, robust=None, iters=25, prior_weight=100.0, huber=1.0, timer=None):
    """icgh_backend_solve_prior_batch on vio_data windows from the given (states, invdepth) starts; priors[w]: make_prior's dict or None;
    state_const[w]: flags per state or None; robust[w]: the Huber delta of the prior's loss, 0 = none
    -> (rc, message, states, invdepth, summary W x 4, prior cost W x 2)"""
    return call_batch(lib.icgh_backend_solve_prior_batch, wins, starts, mode, iters, prior_weight, huber, timer, priors, state_const, robust)


def _first_states(W, K):
    """the leading K states of a window: their intervals and the reprojection factors among them"""
    keep = (W["ii"] < K) & (W["jj"] < K)
    lms = np.unique(W["ll"][keep])
    return dict(W, offsets=W["offsets"][:K], imu=np.ascontiguousarray(W["imu"][:W["offsets"][K - 1]]), states=W["states"][:K], invdepth=W["invdepth"][lms],
                obs=np.ascontiguousarray(W["obs"][:, keep]), ii=W["ii"][keep], jj=W["jj"][keep], ll=np.searchsorted(lms, W["ll"][keep]).astype(np.int32))


def five_windows(oracle):
    """The windows of the device-prior solver tests: 2, 3, 4, 8 and 8 states, 20 IMU samples per interval, 30 landmarks.  Window 1 has no
    prior; window 2 starts far from the optimum; window 3's prior spans state 1, which is constant (its block has fewer columns than rows);
    the priors of windows 0, 2 and 4 span every state.  -> (windows, starts, priors, state_const)"""
    import reproj_data as rd
    import vio_data as vd
    wins = [vd.make_vio_window(oracle, n_intervals=n, per=20, n_lm=30, seed=10 + n + k) for k, n in enumerate((2, 2, 3, 7, 7))]
    wins[0] = _first_states(wins[0], 2)
    wins[2] = vd.make_vio_window(oracle, n_intervals=3, per=20, n_lm=30, seed=13)
    starts = [vd.perturbed_start(w, seed=k) for k, w in enumerate(wins)]
    rng = np.random.RandomState(77)  # a far start: metres and half-radians on the poses, m/s on the velocities, e-folds on the inverse depths
    s = wins[2]["states"].copy()
    for k in range(1, len(s)):
        s[k, :7] = rd.pose_plus(s[k, :7], rng.normal(0, [1.0] * 3 + [0.5] * 3))
        s[k, 7:10] += rng.normal(0, 1.0, 3)
    starts[2] = (s, wins[2]["invdepth"] * np.exp(rng.normal(0, 1.0, len(wins[2]["invdepth"]))))
    priors = [make_prior(wins[0], range(2), 31), None, make_prior(wins[2], range(4), 35), make_prior(wins[3], [0, 1, 2, 5], 34), make_prior(wins[4], range(8), 35)]
    const = [None, None, None, [0, 1, 0, 0, 0, 0, 0, 0], None]
    return wins, starts, priors, const


def check_conditions(summ, pcost, priors):
    """what the five windows must show on the host path for the comparison of the modes to mean something"""
    assert (summ[:, 2] > 0).all() and (summ[:, 1] < summ[:, 0]).all(), summ  # every window takes a successful step
    assert summ[2, 3] > 0, summ  # the far start has a rejected step: a re-damped system without a rebuild
    for w, p in enumerate(priors):
        assert (pcost[w, 0] > 0) == (p is not None), (w, pcost)  # every prior's cost at the start is non-zero
