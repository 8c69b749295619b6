"""GPU parity of the reduced camera solve (csrc/chol.hip): icg_chol_solve_batch and icg_reproj_solve_windows against the host layer's
choleskySolve (icgh_dense_cholesky_solve).  The device performs the host's IEEE operations in the host's order, so every comparison is
np.array_equal on the float64 bit patterns: no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

import reduced_solve_utils as ru
import reproj_data as rd
from ctypes_util import bits

pytestmark = pytest.mark.gpu

# odd and even n, dot8 lengths below 8 / on a multiple of 8 / with a tail, the lane wrap at 64 and 128, the last sizes that live in LDS and
# the first that take the global-scratch path (n (n + 1) / 2 + n doubles against 160 KiB: 200 fits, 201 does not), and the widest system
SIZES = [1, 2, 3, 7, 8, 9, 10, 15, 16, 17, 23, 64, 65, 67, 129, 157, 200, 201, 512]


@pytest.fixture(scope="module")
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hostlib():
    import harness
    return C.CDLL(harness.HOST_LIB)


@pytest.fixture(scope="module")
def systems():
    return [ru.spd(n, 100 + n) for n in SIZES]


@pytest.fixture(scope="module")
def host(hostlib, systems):
    """the reference, computed once: (rc, x, L) per system"""
    return [ru.host_cholesky(hostlib, A, b) for A, b in systems]


def _same(dev, ref):
    x, L, st = dev
    return st == 0 and np.array_equal(bits(x), bits(ref[1])) and np.array_equal(bits(np.tril(L)), bits(ref[2]))


def test_spd_systems_equal_the_host_bit_for_bit(ctx, systems, host):
    assert [h[0] for h in host] == [0] * len(SIZES)  # a failing reference cannot hide a failure
    dev = ru.device_cholesky(ctx, systems)
    for n, d, h in zip(SIZES, dev, host):
        assert d[2] == 0, n
        assert np.array_equal(bits(d[0]), bits(h[1])), (n, np.abs(d[0] - h[1]).max())
        assert np.array_equal(bits(np.tril(d[1])), bits(h[2])), (n, np.abs(np.tril(d[1]) - h[2]).max())
        assert not np.triu(d[1], 1).any(), n  # nothing is written above the diagonal


def test_a_system_is_the_same_bits_alone_reversed_and_in_a_crowd(ctx, systems, host):
    for n, s, h in zip(SIZES, systems, host):
        assert _same(ru.device_cholesky(ctx, [s])[0], h), n
    for n, d, h in zip(reversed(SIZES), ru.device_cholesky(ctx, systems[::-1]), reversed(host)):
        assert _same(d, h), n
    k = SIZES.index(67)
    crowd = ru.device_cholesky(ctx, [systems[k]] * 300)  # more waves than one workgroup holds
    assert all(_same(d, host[k]) for d in crowd)


def _failing():
    out = {}
    A, b = ru.spd(6, 1)
    A[0, 0] = -1.0
    out["pivot 0"] = (A, b)
    A, b = ru.spd(4, 2)
    A[0, 0], A[1, 0], A[0, 1], A[1, 1] = 1.0, 2.0, 2.0, 1.0  # d1 = 1 - 4
    out["second pivot of a tile"] = (A, b)
    A, b = ru.spd(7, 3)
    A[6, 6] = 0.0
    out["last pivot of an odd n"] = (A, b)
    A, b = ru.spd(9, 4)
    A[3, 1] = A[1, 3] = np.nan
    out["NaN"] = (A, b)
    return out


def test_failure_paths_follow_the_host(ctx, hostlib):
    bad = _failing()
    for name, (A, b) in bad.items():
        assert ru.host_cholesky(hostlib, A, b)[0] == -1, name
        x, _, st = ru.device_cholesky(ctx, [(A, b)])[0]
        assert st == 1 and not x.any(), name
    good = [ru.spd(11, 5), ru.spd(66, 6)]
    ref = [ru.host_cholesky(hostlib, A, b) for A, b in good]
    assert [r[0] for r in ref] == [0, 0]
    for name, s in bad.items():  # a failing system between two good ones
        dev = ru.device_cholesky(ctx, [good[0], s, good[1]])
        assert dev[1][2] == 1 and not dev[1][0].any(), name
        assert _same(dev[0], ref[0]) and _same(dev[2], ref[1]), name


def test_argument_errors_name_the_system(ctx):
    import icgvins
    A, b = ru.spd(3, 7)
    with pytest.raises(icgvins.IcgError, match=r"rc=-1: .*system 1: n = 0"):
        ctx.chol_solve_batch([3, 0], A, b)
    big = np.eye(513)
    with pytest.raises(icgvins.IcgError, match=r"rc=-5: .*system 1: n = 513"):
        ctx.chol_solve_batch([3, 513], np.concatenate([A.reshape(-1), big.reshape(-1)]), np.concatenate([b, np.ones(513)]))
    n = np.array([3], np.int32)
    rc = ctx.lib.icg_chol_solve_batch(ctx.h, 1, n.ctypes.data_as(C.c_void_p), A.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), None, None, None)
    assert rc == -1 and b"NULL" in ctx.lib.icg_last_error(ctx.h)


def _two_windows():
    """two small windows with 6 and 3 keyframes: different Pw under a common P"""
    wins = [rd.make_window(14, 6, seed=41, pixel_noise=1.0), rd.make_window(9, 3, seed=42, pixel_noise=1.0)]
    pose_off = np.concatenate([[0], np.cumsum([w["poses"].shape[0] for w in wins])])
    lm_off = np.concatenate([[0], np.cumsum([len(w["invdepth"]) for w in wins])]).astype(np.int32)
    fac_off = np.concatenate([[0], np.cumsum([w["obs_soa"].shape[1] for w in wins])]).astype(np.int32)
    g = dict(obs=np.concatenate([w["obs_soa"] for w in wins], axis=1),
             ii=np.concatenate([w["idx_i"] + pose_off[k] for k, w in enumerate(wins)]).astype(np.int32),
             jj=np.concatenate([w["idx_j"] + pose_off[k] for k, w in enumerate(wins)]).astype(np.int32),
             ll=np.concatenate([w["idx_lm"] + lm_off[k] for k, w in enumerate(wins)]).astype(np.int32),
             poses=np.concatenate([w["poses"] for w in wins]), ext=np.stack([w["ext"] for w in wins]),
             inv=np.concatenate([w["invdepth"] for w in wins]), td=np.array([w["td"] for w in wins]), fac_off=fac_off, lm_off=lm_off)
    # window 0: six poses, the extrinsic and td (43 columns); window 1: three poses and the extrinsic (24 columns)
    col_pose = np.concatenate([6 * np.arange(6), 6 * np.arange(3)]).astype(np.int32)
    g.update(col_pose=col_pose, col_ext=np.array([36, 18], np.int32), col_td=np.array([42, -1], np.int32), Pw=np.array([43, 24], np.int32), P=43)
    return g


def test_solve_windows_equals_host_step(hostlib):
    import icgvins
    g = _two_windows()
    P, Pw, W, n_lm = g["P"], g["Pw"], 2, len(g["inv"])
    rng = np.random.RandomState(9)
    ctx = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    ctx.reproj_set_factors(g["obs"], g["ii"], g["jj"], g["ll"])
    ctx.reproj_set_windows(g["fac_off"], g["lm_off"])
    ctx.reproj_eval_windows(g["poses"], g["ext"], g["inv"], g["td"], huber=1.0)
    with pytest.raises(icgvins.IcgError, match="rc=-1: .*icg_reproj_schur_windows_resident first"):  # nothing resident yet
        ctx.reproj_solve_windows(P, Pw, [1, 1], np.ones((W, P)), np.ones((W, P)), n_lm)
    damp = np.array([1e-4, 1e-3])
    # the host factors' part of each window: a full-rank block on its leading Pw columns (what priors contribute), zero beyond
    H, hs = np.zeros((W, P, P)), np.zeros((W, P))
    for w in range(W):
        M = rng.normal(0, 30.0, (Pw[w], Pw[w]))
        H[w, :Pw[w], :Pw[w]] = M @ M.T
        hs[w, :Pw[w]] = rng.normal(0, 1.0, Pw[w])
    packed = lambda w: np.concatenate([H[w, i, :i + 1] for i in range(Pw[w])])

    def host_step(S, s, dg, radius, solve):
        """solver_batch_hip.cc's reduced-solve phase in numpy around icgh_dense_cholesky_solve"""
        dc, st, dd, rhs = np.zeros((W, P)), np.zeros(W, np.int32), np.zeros((W, P)), s + hs
        for w in range(W):
            n = Pw[w]
            dd[w, :n] = np.minimum(np.maximum(dg[w, :n], 1e-6), 1e32) / radius[w]
            if not solve[w]:
                continue
            Ab = np.zeros((n, n))
            for i in range(n):
                Ab[i, :i + 1] = S[w, i, :i + 1] + H[w, i, :i + 1]
            Ab[np.arange(n), np.arange(n)] += dd[w, :n]
            rc, x, _ = ru.host_cholesky(hostlib, Ab, rhs[w, :n])
            assert rc == 0, w  # the reference itself must solve
            dc[w, :n] = x
        return dc, st, dd, rhs

    def compare(got, ref_dc, ref_st, ref_dl, ref_terms):
        dc, st, dl, terms = got
        assert np.array_equal(st, ref_st)
        for name, a, b in (("delta_c", dc, ref_dc), ("delta_l", dl, ref_dl), ("lm_terms", terms, ref_terms)):
            assert np.array_equal(bits(a), bits(b)), (name, np.abs(a - b).max())

    # step 1: both windows solve, both host parts arrive
    S, s, dg, _ = ctx.reproj_schur_windows_view(P, g["col_pose"], g["col_ext"], g["col_td"], damp=damp)
    dc1, st1, dd1, rhs1 = host_step(S, s, dg, [1e4, 1e4], [1, 1])
    assert dc1[0].any() and dc1[1, :24].any() and not dc1[1, 24:].any()
    dl1, terms1 = ctx.reproj_backsub_windows(P, dc1, n_lm)
    with pytest.raises(icgvins.IcgError, match="rc=-1"):  # the view form leaves nothing resident either
        ctx.reproj_solve_windows(P, Pw, [1, 1], dd1, rhs1, n_lm)
    s_r, dg_r, _ = ctx.reproj_schur_windows_resident(P, g["col_pose"], g["col_ext"], g["col_td"], damp=damp)
    assert np.array_equal(bits(s_r), bits(s)) and np.array_equal(bits(dg_r), bits(dg))
    got = ctx.reproj_solve_windows(P, Pw, [1, 1], dd1, rhs1, n_lm, host_part_new=[1, 1], host_S=np.concatenate([packed(0), packed(1)]))
    compare(got, dc1, st1, dl1, terms1)
    # step 2 (a re-damped step): smaller radius, no part is shipped (the resident ones are reused), window 1 does not solve
    dc2, st2, dd2, rhs2 = host_step(S, s, dg, [2.5e3, 1e4], [1, 0])
    assert not np.array_equal(dc2[0], dc1[0]) and not dc2[1].any()
    dl2, terms2 = ctx.reproj_backsub_windows(P, dc2, n_lm)
    compare(ctx.reproj_solve_windows(P, Pw, [1, 0], dd2, rhs2, n_lm, host_part_new=[0, 0]), dc2, st2, dl2, terms2)
    compare(ctx.reproj_solve_windows(P, Pw, [1, 0], dd2, rhs2, n_lm), dc2, st2, dl2, terms2)
    # another schur form rewrites the window systems the back-substitution reads: the resident reduced systems are stale and refused ...
    damp3 = np.array([3e-3, 1e-4])
    S3, s3, dg3, _ = ctx.reproj_schur_windows_view(P, g["col_pose"], g["col_ext"], g["col_td"], damp=damp3)
    assert not np.array_equal(S3, S)
    dc3, st3, dd3, rhs3 = host_step(S3, s3, dg3, [1e4, 1e4], [1, 1])
    dl3, terms3 = ctx.reproj_backsub_windows(P, dc3, n_lm)
    with pytest.raises(icgvins.IcgError, match="rc=-1: .*icg_reproj_schur_windows_resident"):
        ctx.reproj_solve_windows(P, Pw, [1, 1], dd3, rhs3, n_lm)
    # ... while the host parts outlive it: the resident form with that damping, no part shipped, is the host step on S3
    ctx.reproj_schur_windows_resident(P, g["col_pose"], g["col_ext"], g["col_td"], damp=damp3)
    compare(ctx.reproj_solve_windows(P, Pw, [1, 1], dd3, rhs3, n_lm), dc3, st3, dl3, terms3)
    ctx.close()
