"""Marginalization priors for the M4 tests (icg_marg_prior_set / icg_marg_prior_evaluate, icgh_backend_marg_factor): block layouts, seeded
priors, evaluation points, the packing of many priors into the entry's arrays and the plain-Python sums the device's optional outputs are
held to."""

import numpy as np

import reproj_data as rd
from ctypes_util import ErrBuf, ptr

C2_SIZES = [7, 9] * 9 + [7, 1]      # the estimator's window: 9 x (pose, mix) + extrinsic + td, r = 142
C4_SIZES = [7, 9] * 14 + [7, 1]     # r = 217
SCENARIO_SIZES = [7] * 5 + [1] * 40 + [7, 1]  # the shape of capi_marg.cc's marginalization scenario: poses, inverse depths, extrinsic, td (r = 77)
R512_SIZES = [7] * 80 + [1] * 32    # r = 512


def local(size):
    return 6 if size == 7 else size


def layout(sizes, order=None, gap_after=None, gap=0):
    """(block_size, block_index, r): columns handed out in `order` (default: list order), `gap` uncovered columns after the
    `gap_after`-th block handed out"""
    sizes = [int(s) for s in sizes]
    order = list(range(len(sizes))) if order is None else list(order)
    index = [0] * len(sizes)
    col = 0
    for n, b in enumerate(order):
        index[b] = col
        col += local(sizes[b])
        if gap_after is not None and n == gap_after:
            col += gap
    return np.array(sizes, np.int32), np.array(index, np.int32), col


def make_prior(sizes, seed, order=None, gap_after=None, gap=0, quat_scale=1.0):
    size, index, r = layout(sizes, order, gap_after, gap)
    rng = np.random.default_rng(seed)
    x0 = []
    for s in size:
        v = rng.normal(0, 1, int(s))
        if s == 7:
            v[3:] = v[3:] / np.linalg.norm(v[3:]) * quat_scale
        x0.append(v)
    return dict(r=r, size=size, index=index, x0=np.concatenate(x0), J0=rng.normal(0, 1, (r, r)), e0=rng.normal(0, 1, r))


def make_x(prior, seed, negate=()):
    """x0 moved by PoseParameterization::Plus / small additive steps; the quaternion of the 7-blocks listed in `negate` (positions among
    the 7-blocks) has its sign flipped (the same rotation, dq.w < 0)"""
    rng = np.random.default_rng(seed)
    out, off, n7 = [], 0, 0
    for s in prior["size"]:
        s = int(s)
        v = prior["x0"][off:off + s].copy()
        if s == 7:
            unit = v.copy()
            unit[3:] /= np.linalg.norm(unit[3:])
            v = rd.pose_plus(unit, rng.normal(0, 1e-2, 6))
            if n7 in negate:
                v[3:] = -v[3:]
            n7 += 1
        else:
            v = v + rng.normal(0, 1e-2, s)
        out.append(v)
        off += s
    return np.concatenate(out)


def dq_w(prior, x):
    """w of q0^-1 * q per 7-block, as MarginalizationFactor::Evaluate forms it"""
    out, off = [], 0
    for s in prior["size"]:
        s = int(s)
        if s == 7:
            q0, q = prior["x0"][off + 3:off + 7], x[off + 3:off + 7]
            n2 = q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2] + q0[3] * q0[3]
            ax, ay, az, aw = -q0[0] / n2, -q0[1] / n2, -q0[2] / n2, q0[3] / n2
            out.append(aw * q[3] - ax * q[0] - ay * q[1] - az * q[2])
        off += s
    return np.array(out)


def batch():
    """the heterogeneous batch of the tests, in this order: C2, C4, scenario, r = 1, r = 512, out of column order with a gap, non-unit x0,
    r = 32 and r = 33 (the set's store kernel transposes J0 in 32 x 32 tiles: exactly one tile, and one tile with a row and a column of
    slivers).  Returns (priors, points); in every prior with at least two 7-blocks, two of them take the dq.w < 0 branch."""
    priors = [make_prior(C2_SIZES, 11), make_prior(C4_SIZES, 12), make_prior(SCENARIO_SIZES, 13), make_prior([1], 14),
              make_prior(R512_SIZES, 15), make_prior([7, 3, 1, 9, 7], 16, order=[3, 0, 4, 1, 2], gap_after=1, gap=4),
              make_prior([7, 9, 7, 1], 17, quat_scale=1.01), make_prior([9, 9, 9, 1, 1, 1, 1, 1], 18), make_prior([9, 9, 9, 3, 3], 19)]
    assert [p["r"] for p in priors[7:]] == [32, 33]
    points = [make_x(p, 100 + k, negate=(0, 1)) for k, p in enumerate(priors)]
    return priors, points


def pack(priors):
    """the arrays of icg_marg_prior_set"""
    r = np.array([p["r"] for p in priors], np.int32)
    off = np.concatenate([[0], np.cumsum([len(p["size"]) for p in priors])]).astype(np.int32)
    cat = lambda k, t: np.ascontiguousarray(np.concatenate([np.asarray(p[k]).ravel() for p in priors]), t)
    return dict(r=r, block_off=off, block_size=cat("size", np.int32), block_index=cat("index", np.int32), x0=cat("x0", np.float64),
                J0=cat("J0", np.float64), e0=cat("e0", np.float64))


def set_args(priors):
    a = pack(priors)
    return a["r"], a["block_off"], a["block_size"], a["block_index"], a["x0"], a["J0"], a["e0"]


def split(priors, flat, kind):
    """per-window views of a flat output: kind 'r' (residuals / gradient) or 'jac'"""
    out, off = [], 0
    for p in priors:
        n = p["r"] if kind == "r" else p["r"] * int(p["size"].sum())
        out.append(flat[off:off + n])
        off += n
    assert off == len(flat)
    return out


def sequential_gradient(J0, e):
    """J0^T e, every column summed from 0 in row order, one rounded multiply and one rounded add per term"""
    r = len(e)
    g = np.zeros(r)
    for k in range(r):
        s = np.float64(0.0)
        for i in range(r):
            s = s + J0[i, k] * e[i]
        g[k] = s
    return g


def sequential_sq_norm(e):
    s = np.float64(0.0)
    for v in e:
        s = s + v * v
    return float(s)


def backend_marg_factor(lib, mode, priors, points, want=(True, True, True), host_threads=4, reps=0, mark=None):
    """icgh_backend_marg_factor.  points: list of evaluation points, each a list of per-window x.  Returns (rc, message, residuals,
    jacobians, gradient, sq_norm, seconds), outputs shaped (n_points, ...); `mark` fills the outputs beforehand."""
    a = pack(priors)
    x = np.ascontiguousarray(np.concatenate([np.concatenate(pt) for pt in points]), np.float64)
    n, npt = len(priors), len(points)
    R = int(a["r"].sum())
    NJ = int(sum(p["r"] * int(p["size"].sum()) for p in priors))
    fill = 0.0 if mark is None else mark
    res = np.full((npt, R), fill)
    jac = np.full((npt, NJ), fill) if want[0] else None
    grad = np.full((npt, R), fill) if want[1] else None
    sq = np.full((npt, n), fill) if want[2] else None
    sec = np.full(2, fill)
    err = ErrBuf()
    rc = lib.icgh_backend_marg_factor(int(mode), n, ptr(a["r"]), ptr(a["block_off"]), ptr(a["block_size"]), ptr(a["block_index"]), ptr(a["x0"]),
                                      ptr(a["J0"]), ptr(a["e0"]), npt, ptr(x), int(host_threads), int(reps), ptr(res), ptr(jac), ptr(grad), ptr(sq),
                                      ptr(sec), *err.args)
    return rc, err.text(), res, jac, grad, sq, sec
