"""Resident back-end buffers replaced under a live context (icg_grow, csrc/ctx.hip), together with the invalidation that belongs to each.

One context runs a small call, then a call that cannot fit what the small one left (asserted from the sizes and each site's slack rule, so
no test passes without a reallocation), then the small one again.  Every output is held, bit for bit, to the same call on a fresh context:
there is no tolerance in this file.  What a replaced buffer held must be refused or absent afterwards, never served from stale memory.
The inputs are those of the existing suites (schur_edge_data, reduced_solve_utils, marg_factor_data, marg_linearize_data)."""
import ctypes as C

import numpy as np
import pytest

import marg_factor_data as mf
import marg_linearize_data as ml
import reduced_solve_utils as ru
import schur_edge_checks as K
import schur_edge_data as D
import test_schur_edges_cpu as T
from ctypes_util import bits

pytestmark = pytest.mark.gpu

LDS_BYTES = 160 * 1024  # per workgroup on gfx950: what the LDS / global-scratch thresholds of chol.hip and marg_linearize.hip come from


def _ctx():
    import icgvins
    return icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)


def _fresh(fn, *args):
    c = _ctx()
    try:
        return fn(c, *args)
    finally:
        c.close()


def _assert_same(got, exp, what):
    """nested tuples / lists / dicts of arrays and scalars, float64 compared on the bit patterns"""
    if isinstance(exp, dict):
        assert set(got) == set(exp), what
        for k in exp:
            _assert_same(got[k], exp[k], (what, k))
    elif isinstance(exp, (tuple, list)):
        assert len(got) == len(exp), what
        for k, (a, b) in enumerate(zip(got, exp)):
            _assert_same(a, b, (what, k))
    elif exp is None:
        assert got is None, what
    else:
        a, b = np.asarray(got), np.asarray(exp)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
        same = np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
        assert same, (what, "differs from the same call on a fresh context")


# ---- factor set and window systems ---------------------------------------------------------------------------------------------------------
def _sys_doubles(P, Ls):
    """what schur_impl asks of d_sys for windows of Ls landmarks at width P: H | b | inv per window, + 8"""
    return sum((P + L) ** 2 + (P + L) + L for L in Ls) + 8


def _single(ctx, case):
    """every single-window entry point on the case -> all outputs"""
    P, L = case["P"], case["L"]
    cols = (case["col_pose"], case["col_ext"], case["col_td"])
    ctx.reproj_set_factors(case["obs_soa"], case["idx_i"], case["idx_j"], case["idx_lm"])
    r, J = ctx.reproj_eval_resident(case["poses"], case["ext"], case["invdepth"], case["td"], huber=case["huber"], fetch=True)
    Hb = ctx.reproj_accumulate_normal(P + L, cols[0], cols[1], P + np.arange(L, dtype=np.int32), cols[2])
    first = ctx.reproj_schur(P, *cols, active=case["active"], damp=1e-4)
    hll = ctx.reproj_landmark_diag(L)
    back = ctx.reproj_backsub(P, np.random.RandomState(17).normal(0, 1e-3, P), L)
    redamped = ctx.reproj_schur(P, *cols, active=case["active"], reassemble=False, damp=3e-3)
    return r, J, Hb, first, hll, back, redamped, ctx.reproj_cost(case["active"]), ctx.reproj_fetch_residuals()


def _batch(ctx, B, resident_solve=None):
    """the many-window entry points on a concatenated batch (schur_edge_checks.concat) -> all outputs; resident_solve = (host_S or None):
    icg_reproj_schur_windows_resident + icg_reproj_solve_windows instead of the copying forms"""
    W, P, n_lm = len(B["td"]), B["P"], len(B["inv"])
    args = (P, B["col_pose"], B["col_ext"], B["col_td"])
    ctx.reproj_set_factors(B["obs"], B["ii"], B["jj"], B["ll"])
    ctx.reproj_set_windows(B["fac_off"], B["lm_off"])
    ctx.reproj_eval_windows(B["poses"], B["ext"], B["inv"], B["td"], huber=1.5)
    damp = np.full(W, 1e-4)
    if resident_solve is None:
        out = ctx.reproj_schur_windows(*args, active=B["active"], damp=damp)
        dc = np.random.RandomState(23).normal(0, 1e-3, (W, P))
        return (out, ctx.reproj_landmark_diag_windows(n_lm), ctx.reproj_backsub_windows(P, dc, n_lm), ctx.reproj_cost_windows(B["active"]),
                ctx.reproj_fetch_residuals())
    s, dg, cost = ctx.reproj_schur_windows_resident(*args, active=B["active"], damp=damp)
    return (s, dg, cost) + tuple(_solve(ctx, B, s, dg, resident_solve[0]))


def test_factor_set_and_window_systems_regrow():
    import icgvins
    narrow = min((w[0] for w in T.WIDTH), key=lambda c: (c["P"], c["L"]))
    wide = max((w[0] for w in T.WIDTH), key=lambda c: (c["P"], c["L"]))
    det = K.concat(D.determinism_batch())
    # the wide call fits neither the per-factor buffers (n + n / 4 + 64 factors) nor d_sys (+ 25 %) the narrow one left
    n_small, n_wide = len(narrow["idx_i"]), len(wide["idx_i"])
    assert n_wide > n_small + n_small // 4 + 64, (n_small, n_wide)
    d_small, d_wide = _sys_doubles(narrow["P"], [narrow["L"]]), _sys_doubles(wide["P"], [wide["L"]])
    assert d_wide > d_small + d_small // 4, (d_small, d_wide)
    exp_narrow, exp_wide, exp_det = _fresh(_single, narrow), _fresh(_single, wide), _fresh(_batch, det)
    ctx = _ctx()
    try:
        _assert_same(_single(ctx, narrow), exp_narrow, "narrow, first")
        _assert_same(_single(ctx, wide), exp_wide, "wide")
        # the narrow system went with the buffer it lived in: nothing of its width is left to re-damp
        with pytest.raises(icgvins.IcgError, match="rc=-1:"):
            ctx.reproj_schur(narrow["P"], narrow["col_pose"], narrow["col_ext"], narrow["col_td"], reassemble=False, damp=1e-3)
        _assert_same(_single(ctx, narrow), exp_narrow, "narrow, after the wide one")
        _assert_same(_batch(ctx, det), exp_det, "two windows, after the single ones")
    finally:
        ctx.close()


# ---- resident reduced systems --------------------------------------------------------------------------------------------------------------
def _host_parts(W, P):
    """an SPD host part per window (reduced_solve_utils.spd), packed lower triangles, flat"""
    return np.concatenate([ru.spd(P, 900 + w)[0][np.tril_indices(P)] for w in range(W)])


def _solve(ctx, B, s, dg, host_S):
    W, P = len(B["td"]), B["P"]
    dd = np.minimum(np.maximum(dg, 1e-6), 1e32) / 1e4
    send = None if host_S is None else np.ones(W, np.uint8)
    return ctx.reproj_solve_windows(P, np.full(W, P, np.int32), np.ones(W, np.uint8), dd, s, len(B["inv"]), host_part_new=send, host_S=host_S)


def test_resident_reduced_systems_regrow():
    two = K.concat(D.clamp_batch())
    p97 = next(w[0] for w in T.WIDTH if w[0]["P"] == 97)
    three = K.concat(D.determinism_batch() + [p97])
    W2, P2, W3, P3 = 2, two["P"], 3, three["P"]
    assert len(two["td"]) == W2 and len(three["td"]) == W3 and P3 > P2
    # d_red_S (W P^2 doubles) and d_red_H (W P (P + 1) / 2) are allocated exactly: the second shape fits neither
    assert W3 * P3 * P3 > W2 * P2 * P2 and W3 * P3 * (P3 + 1) // 2 > W2 * P2 * (P2 + 1) // 2
    h2, h3 = _host_parts(W2, P2), _host_parts(W3, P3)
    exp_two, exp_three = _fresh(_batch, two, (h2,)), _fresh(_batch, three, (h3,))
    exp_two_bare = _fresh(_batch, two, (None,))
    assert not np.array_equal(exp_two[3], exp_two_bare[3])  # (the host part changes delta_c: the two cannot be confused)
    ctx = _ctx()
    try:
        _assert_same(_batch(ctx, two, (h2,)), exp_two, "two windows, first")
        _assert_same(_batch(ctx, three, (h3,)), exp_three, "three wider windows")
        # the first shape's host part is not resident any more: a solve that does not send it again gets A = S + dd ...
        _assert_same(_batch(ctx, two, (None,)), exp_two_bare, "two windows again, host part not sent")
        # ... and with the part sent again, the first result
        _assert_same(_batch(ctx, two, (h2,)), exp_two, "two windows again, host part sent")
    finally:
        ctx.close()


# ---- Cholesky scratch and LDS opt-in -------------------------------------------------------------------------------------------------------
def test_cholesky_scratch_and_lds_opt_in():
    import harness
    hostlib = C.CDLL(harness.HOST_LIB)
    work = lambda n: (n * (n + 1) // 2 + n) * 8  # chol.hip: the packed factor and the right-hand side of a system
    n_glob, n_optin = 201, 157
    assert work(n_glob) > LDS_BYTES  # global scratch: none is allocated before this call
    assert 48 * 1024 < work(n_optin) <= LDS_BYTES  # in LDS, above the default a launch may ask for
    assert work(3) <= 48 * 1024
    ctx = _ctx()
    try:
        for n in (3, n_glob, n_optin, 3):
            A, b = ru.spd(n, 100 + n)
            rc, x, L = ru.host_cholesky(hostlib, A, b)
            assert rc == 0, n
            (dx, dL, st), = ru.device_cholesky(ctx, [(A, b)])
            assert st == 0 and np.array_equal(bits(dx), bits(x)) and np.array_equal(bits(np.tril(dL)), bits(L)), n
    finally:
        ctx.close()


# ---- prior set and linearization scratch ---------------------------------------------------------------------------------------------------
def _prior(ctx, priors, points):
    ctx.marg_prior_set(*mf.set_args(priors))
    return ctx.marg_prior_evaluate(np.concatenate(points), want_jac=True, want_grad=True, want_sq_norm=True)


def _linearize(ctx, systems):
    return ctx.marg_linearize_batch(*ml.pack(systems), eps=ml.EPS)


def test_prior_set_regrows():
    priors, points = mf.batch()
    small, large = ([priors[3]], [points[3]]), (priors[:3], points[:3])
    # J, e0, x0 and the layout block are allocated exactly: three windows of r >= 77 against one of r = 1
    assert small[0][0]["r"] == 1 and all(p["r"] >= 77 for p in large[0])
    exp_small, exp_large = _fresh(_prior, *small), _fresh(_prior, *large)
    ctx = _ctx()
    try:
        _assert_same(_prior(ctx, *small), exp_small, "one small window, first")
        _assert_same(_prior(ctx, *large), exp_large, "three larger windows")
        _assert_same(_prior(ctx, *small), exp_small, "one small window, after the larger ones")
    finally:
        ctx.close()


def test_linearization_scratch_regrows():
    systems = ml.batch()
    fits, too_big = [systems[4]], [systems[1]]
    need = lambda s: (max(2 * s["m"] ** 2 + (s["P"] - s["m"]) * s["m"], (s["P"] - s["m"]) ** 2) + 2 * max(s["m"], s["P"] - s["m"])) * 8  # marg_linearize.hip
    assert need(fits[0]) <= 48 * 1024 and need(too_big[0]) > LDS_BYTES  # the second works in the global scratch (exact size), which the first left at r doubles
    exp_fits, exp_big = _fresh(_linearize, fits), _fresh(_linearize, too_big)
    ctx = _ctx()
    try:
        _assert_same(_linearize(ctx, fits), exp_fits, "in LDS, first")
        _assert_same(_linearize(ctx, too_big), exp_big, "in the global scratch")
        _assert_same(_linearize(ctx, fits), exp_fits, "in LDS, after the large one")
    finally:
        ctx.close()


# ---- create / destroy ----------------------------------------------------------------------------------------------------------------------
def test_create_use_every_buffer_destroy_twice():
    """return codes only (the binding raises on any other than ICG_OK): every growable buffer exists when the context is destroyed"""
    two = K.concat(D.clamp_batch())
    narrow = min((w[0] for w in T.WIDTH), key=lambda c: (c["P"], c["L"]))
    priors, points = mf.batch()
    systems = ml.batch()
    for _ in range(2):
        ctx = _ctx()
        _single(ctx, narrow)  # factor set, part_1's plan, d_sys
        _batch(ctx, two, (_host_parts(2, two["P"]),))  # d_lmwin, part_w's plan, d_red_S, d_red_H
        ru.device_cholesky(ctx, [ru.spd(201, 301)])  # d_chol_scratch
        _prior(ctx, [priors[3]], [points[3]])  # the prior set's four buffers
        _linearize(ctx, [systems[4]])  # d_lin_scratch
        ctx.close()
