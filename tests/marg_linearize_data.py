"""Reduced systems for the M3 tests (icg_marg_linearize_batch, icgh_backend_marg_linearize): seeded (H, b, m) of the shapes the issue
lists, the packing into the entry's flat arrays, the ctypes driver of the host-layer entry, and the quantities of a linearization that do
not depend on the eigen-solver's sign / basis choices.

Every b is -H x for a modest x, so b lies in the range of H: the prior's cost and J0^T e0 are then well conditioned however badly H is
scaled, and rank decisions are the only place where rounding could flip a result — the tests assert that no eigenvalue is near the floor."""
import ctypes as C
import functools

import numpy as np

import ctypes_util
from ctypes_util import ErrBuf, ptr

EPS = 1e-8  # the reference's floor (marginalization_info.h:30)


def _spd(P, rng, rows_per_col=4):
    A = rng.normal(0, 1, (rows_per_col * P, P))
    return A.T @ A / (rows_per_col * P)


def _system(name, H, m, rng):
    H = 0.5 * (H + H.T)
    x = rng.normal(0, 1, H.shape[0])
    return dict(name=name, P=H.shape[0], m=int(m), H=np.ascontiguousarray(H), b=-(H @ x))


def spd_system(P, m, seed, name=None):
    rng = np.random.default_rng(seed)
    return _system(name or f"spd{P}_{m}", _spd(P, rng) + 0.05 * np.eye(P), m, rng)


def rank_deficient_system(seed):
    """P = 157, m = 15; the Schur complement is A^T A with A of 100 x 142 (rank 100) up to rounding"""
    rng = np.random.default_rng(seed)
    m, r = 15, 142
    A = rng.normal(0, 1, (100, r))
    M = _spd(m, rng) + 0.5 * np.eye(m)
    B = 0.1 * rng.normal(0, 1, (m, r))
    H = np.zeros((m + r, m + r))
    H[:m, :m], H[:m, m:], H[m:, :m] = M, B, B.T
    H[m:, m:] = A.T @ A + B.T @ np.linalg.solve(M, B)
    return _system("rank_deficient", H, m, rng)


def badly_scaled_system(seed, P=60, m=10):
    """diagonal spread 1e-6 ... 1e6: D C D with a well-conditioned C (eigenvalues in about [0.6, 1.5])"""
    rng = np.random.default_rng(seed)
    Cm = _spd(P, rng, rows_per_col=20)
    d = 10.0 ** rng.permutation(np.linspace(-3, 3, P))
    return _system("badly_scaled", d[:, None] * Cm * d[None, :], m, rng)


def zero_row_system(seed, P=50, m=8, where=None, name="zero_row"):
    rng = np.random.default_rng(seed)
    H = _spd(P, rng) + 0.05 * np.eye(P)
    k = P - 1 if where is None else where
    H[k, :] = 0.0
    H[:, k] = 0.0
    return _system(name, H, m, rng)


def golden_system(oracle):
    """the full normal equations of the scenario behind tests/golden/marg_ref_golden.npz (capi_marg.cc icgh_backend_marginalize: reprojection
    factors with Huber 1.0 + the PosePriorFactor of weight 100 on pose 0), assembled by the oracle as backend_utils.oracle_marginalized_system
    does; m = pose 0 + its landmarks.  Returns (system, problem)."""
    import backend_utils as bu
    import marg_data as md
    P = md.make_problem(**bu.MARG_GOLDEN_ARGS)
    w = P["w"]
    r_, J_ = oracle.reproj_eval(P["obs"], P["ii"], P["jj"], P["ll"], w["poses"], w["ext"], w["invdepth"], w["td"], huber=1.0)
    H, b = oracle.reproj_accumulate_normal(r_, J_, P["ii"], P["jj"], P["ll"], P["col_pose"], P["col_ext"], P["col_lm"], P["col_td"], P["local_size"])
    Jp = 100.0 * np.eye(6)
    rp = np.zeros(6)
    rp[0] = 100.0 * -0.01
    c0 = P["col_pose"][0]
    H[c0:c0 + 6, c0:c0 + 6] += Jp.T @ Jp
    b[c0:c0 + 6] -= Jp.T @ rp
    return dict(name="golden", P=int(P["local_size"]), m=int(P["m"]), H=np.ascontiguousarray(H), b=np.ascontiguousarray(b)), P


def golden_m():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marg_ref_golden.npz"))
    assert int(g["r"]) == 37
    return int(g["m"])


def batch():
    """the heterogeneous batch of the tests: SPD systems of the shapes C2 (157, 15), C4 (232, 15), the golden scenario's (37 + m, m),
    (1, 0), (2, 1), (256, 0); a rank-deficient Hp; a badly scaled system; a zero row / column in the retained block (the last index: the
    solver's scale == 0 branch) and one in the marginalized block (an m-block eigenvalue of exactly 0: status bit 2)"""
    gm = golden_m()
    return [spd_system(157, 15, 1, "c2"), spd_system(232, 15, 2, "c4"), spd_system(37 + gm, gm, 10, "golden_shape"), spd_system(1, 0, 3),
            spd_system(2, 1, 4), spd_system(256, 0, 5), rank_deficient_system(6), badly_scaled_system(7), zero_row_system(8),
            zero_row_system(9, where=3, name="zero_row_m")]


def pack(systems):
    P = np.array([s["P"] for s in systems], np.int32)
    m = np.array([s["m"] for s in systems], np.int32)
    H = np.ascontiguousarray(np.concatenate([s["H"].ravel() for s in systems]), np.float64)
    b = np.ascontiguousarray(np.concatenate([s["b"].ravel() for s in systems]), np.float64)
    return P, m, H, b


def split(systems, out):
    """per-window dicts of the flat outputs (dict with J0, e0, Hp, bp, evals, min_ev_m, status; None entries stay None)"""
    res, o1, o2 = [], 0, 0
    for w, s in enumerate(systems):
        r = s["P"] - s["m"]
        d = {}
        for k in ("J0", "Hp"):
            d[k] = None if out.get(k) is None else out[k][o2:o2 + r * r].reshape(r, r)
        for k in ("e0", "bp", "evals"):
            d[k] = None if out.get(k) is None else out[k][o1:o1 + r]
        d["min_ev_m"] = None if out.get("min_ev_m") is None else float(out["min_ev_m"][w])
        d["status"] = None if out.get("status") is None else int(out["status"][w])
        res.append(d)
        o1, o2 = o1 + r, o2 + r * r
    return res


def backend_marg_linearize(lib, mode, systems, eps=EPS, want=(True, True, True, True, True), host_threads=4, reps=0, mark=None):
    """icgh_backend_marg_linearize.  want: Hp, bp, evals, min_ev_m, status.  Returns (rc, message, flat outputs dict, seconds); `mark`
    fills the outputs beforehand."""
    P, m, H, b = pack(systems)
    n = len(systems)
    r = P.astype(np.int64) - m
    nr, nrr = int(r.sum()), int((r * r).sum())
    fill = 0.0 if mark is None else mark
    out = dict(J0=np.full(nrr, fill), e0=np.full(nr, fill), Hp=np.full(nrr, fill) if want[0] else None, bp=np.full(nr, fill) if want[1] else None,
               evals=np.full(nr, fill) if want[2] else None, min_ev_m=np.full(n, fill) if want[3] else None,
               status=np.full(n, int(fill), np.int32) if want[4] else None)
    sec = np.full(2, fill)
    err = ErrBuf()
    rc = lib.icgh_backend_marg_linearize(int(mode), n, ptr(P), ptr(m), ptr(H), ptr(b), C.c_double(eps), int(host_threads), int(reps), ptr(out["Hp"]),
                                         ptr(out["bp"]), ptr(out["J0"]), ptr(out["e0"]), ptr(out["evals"]), ptr(out["min_ev_m"]), ptr(out["status"]),
                                         ptr(sec), *err.args)
    return rc, err.text(), out, sec


def host_eigenvalues(lib, A):
    """symmetricEigen of the host layer (icgh_symmetric_eigen) on A: eigenvalues ascending"""
    A = np.ascontiguousarray(A, np.float64)
    n = A.shape[0]
    ev, V = np.zeros(n), np.zeros((n, n))
    assert lib.icgh_symmetric_eigen(n, ptr(A), ptr(ev), ptr(V)) == 0
    return ev


def assert_no_eigenvalue_near_the_floor(lib, systems, host, eps=EPS):
    """from the HOST eigenvalues alone: none of the m-blocks' or reduced systems' eigenvalues lies in (eps / 10, 10 eps)"""
    for s, h in zip(systems, host):
        m = s["m"]
        evs = [h["evals"]]
        if m > 0:
            evs.append(host_eigenvalues(lib, 0.5 * (s["H"][:m, :m] + s["H"][:m, :m].T)))
        for ev in evs:
            near = (ev > eps / 10) & (ev < 10 * eps)
            assert not near.any(), (s["name"], ev[near])


def dx_of(system, seed=77):
    r = system["P"] - system["m"]
    return np.random.default_rng(seed + r).normal(0, 1e-2, r)


def invariants(system, d):
    """what a linearization determines whatever the eigenvectors' signs and bases: J0^T J0, J0^T e0, the cost at a perturbed point"""
    e = d["e0"] + d["J0"] @ dx_of(system)
    return dict(JtJ=d["J0"].T @ d["J0"], Jte=d["J0"].T @ d["e0"], cost=0.5 * float(e @ e))


same_bits = functools.partial(ctypes_util.same_bits, nan_payload=True)  # M3's outputs are held to every bit, those of a NaN too
