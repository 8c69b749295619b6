"""Members of a navigation-factor set for the product classes (host/nav_factors.h) and the resident set (icg_nav_set): the 48 seeded cases
of nav_utils.factor_cases() (kinds 0..3), the odometer widths (kinds 4, 5), a GNSS member with a zero lever arm, the flat packing both
sides take, and the driver of icgh_backend_nav_eval."""
import numpy as np

import nav_utils as nu
from ctypes_util import ErrBuf, f64, i32, ptr

SHAPES = {0: (3, 7), 1: (6, 9), 2: (6, 7), 3: (9, 9), 4: (7, 10), 5: (10, 10)}  # residuals x block width by kind
# ImuErrorFactor's constants (reference imu_error_factor.h)
GRY_BIAS_STD = 7200 / 3600.0 * np.pi / 180.0
ACC_BIAS_STD = 2.0e4 * 1.0e-5
ODO_SCALE_STD = 2.0e4 * 1.0e-6


def odo_cases(seed=19, n=4):
    """(kind, aux, x) of kinds 4 and 5: the 10-wide mix block (velocity, gyroscope bias, accelerometer bias, odometer scale)"""
    rng = np.random.RandomState(seed)
    sig = np.array([1, 1, 1, 1e-3, 1e-3, 1e-3, 0.05, 0.05, 0.05, 0.01])
    cases = []
    for _ in range(n):
        cases.append((4, np.zeros(0), rng.normal(0, sig)))
        mix = rng.normal(0, sig)
        cases.append((5, np.concatenate([mix + rng.normal(0, 0.01, 10), rng.uniform(1e-3, 0.3, 10)]), mix))
    return cases


def zero_lever_gnss(seed=23):
    """a GNSS member whose lever arm is +0.0: the rotation columns of its Jacobian are signed zeros"""
    rng = np.random.RandomState(seed)
    q = rng.normal(size=4)
    pose = np.concatenate([rng.normal(0, 30, 3), q / np.linalg.norm(q)])
    return (0, np.concatenate([pose[:3] + rng.normal(0, 0.2, 3), rng.uniform(0.01, 0.5, 3), np.zeros(3)]), pose)


def one_of_each():
    """one member per kind 0..5; the GNSS member is golden case 3's (the non-unit quaternion)"""
    base, odo = nu.factor_cases(), odo_cases()
    gnss = base[4 * 3]
    assert gnss[0] == 0 and abs(np.linalg.norm(gnss[2][3:]) - 1) > 0.1
    return [gnss, base[1], base[2], base[3], odo[0], odo[1]]


def mixed_set():
    """kinds 0 3 1 2 5 4 0: every kind, the non-unit GNSS member first, the zero-lever one last"""
    by = one_of_each()
    return [by[0], by[3], by[1], by[2], by[5], by[4], zero_lever_gnss()]


def tiled(cases, n):
    return [cases[k % len(cases)] for k in range(n)]


def pack(cases):
    """-> kind n, aux_off n + 1, aux, points, point_off n (a block after a gap of one double, so that offsets are not the packed ones)"""
    kind = i32([c[0] for c in cases])
    auxs = [f64(c[1]).reshape(-1) for c in cases]
    aux_off = i32(np.concatenate([[0], np.cumsum([len(a) for a in auxs])]))
    aux = f64(np.concatenate(auxs + [np.zeros(1)]))
    point_off, pts, at = [], [], 0
    for c in cases:
        x = f64(c[2]).reshape(-1)
        assert len(x) == SHAPES[c[0]][1]
        pts += [np.full(1, np.nan), x]
        point_off.append(at + 1)
        at += 1 + len(x)
    return kind, aux_off, aux, f64(np.concatenate(pts)), i32(point_off)


def offsets(kind):
    nr = np.array([SHAPES[int(k)][0] for k in kind])
    nj = np.array([SHAPES[int(k)][0] * SHAPES[int(k)][1] for k in kind])
    return np.concatenate([[0], np.cumsum(nr)]), np.concatenate([[0], np.cumsum(nj)])


def host_eval(lib, cases, huber=None, corr_in=None):
    """icgh_backend_nav_eval -> dict r, J, r_corr, J_corr (flat), corr n x 3, sq n, shape n x 3"""
    kind, aux_off, aux, points, point_off = pack(cases)
    n = len(kind)
    ro, jo = offsets(kind)
    out = {"r": np.zeros(ro[-1]), "J": np.zeros(jo[-1]), "r_corr": np.zeros(ro[-1]), "J_corr": np.zeros(jo[-1]), "corr": np.zeros((n, 3)),
           "sq": np.zeros(n), "shape": np.zeros((n, 3), np.int32)}
    hub = None if huber is None else f64(huber).reshape(n)
    cin = None if corr_in is None else f64(corr_in).reshape(n, 3)
    err = ErrBuf()
    rc = lib.icgh_backend_nav_eval(n, ptr(kind), ptr(aux_off), ptr(aux), ptr(points), ptr(point_off), ptr(hub), ptr(cin), ptr(out["r"]), ptr(out["J"]),
                                   ptr(out["r_corr"]), ptr(out["J_corr"]), ptr(out["corr"]), ptr(out["sq"]), ptr(out["shape"]), *err.args)
    assert rc == 0, (rc, err.text())
    out["r_off"], out["j_off"] = ro, jo
    return out


def corrected_numpy(r, J, s1, a, scale):
    """the corrector in ResidualBlockInfo::Evaluate's operation order on one member (J nr x nc) -> (r', J')"""
    r, J = np.array(r, np.float64), np.array(J, np.float64)
    nr, nc = J.shape
    out = J.copy()
    for c in range(nc):
        rtj = np.float64(0.0)
        for k in range(nr):
            rtj = rtj + r[k] * J[k, c]
        for k in range(nr):
            out[k, c] = s1 * (J[k, c] - a * r[k] * rtj)
    return r * scale, out
