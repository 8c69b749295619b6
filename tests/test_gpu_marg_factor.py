"""GPU parity: resident, batched marginalization-prior evaluation (M4, icg_marg_prior_set / icg_marg_prior_evaluate) against the CPU
oracle, the host layer and the reference golden.

Residuals and Jacobian blocks are + - * / only, formed in the oracle's order without contraction on either side: they are held to the
oracle's bit patterns (a NaN must sit where the oracle's sits).  Gradient (J0^T e) and squared norm (e . e) have no oracle entry: they are
held, bit for bit, to a plain Python loop over numpy.float64 scalars in the order the header states.  Against the reference-code golden the
bounds are those of backend_utils.check_marginalization_golden: cost 1e-8 max(1, cost), gradient 1e-7 max(1, max|grad|); the measured
maxima are printed."""
import ctypes as C
import itertools

import numpy as np
import pytest

import backend_utils as bu
import marg_data as md
import marg_factor_data as mf
from ctypes_util import ptr, same_bits

pytestmark = pytest.mark.gpu

MARK = -7.25


def _new_ctx():
    import icgvins
    return icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)


@pytest.fixture(scope="module")
def ctx():
    c = _new_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    import oracle_lib
    return oracle_lib.load()


@pytest.fixture(scope="module")
def hostlib():
    import harness
    return C.CDLL(harness.HOST_LIB)


@pytest.fixture(scope="module")
def cases():
    return mf.batch()


def _evaluate(c, priors, points, **want):
    c.marg_prior_set(*mf.set_args(priors))
    return c.marg_prior_evaluate(np.concatenate(points), **want)


def test_heterogeneous_batch_equals_the_oracle_bit_for_bit(ctx, oracle, cases):
    priors, points = cases
    assert [p["r"] for p in priors[:5]] == [142, 217, 77, 1, 512]
    # the dq.w < 0 branch is really taken: in two 7-blocks of every prior that has two, and nowhere else
    for p, x in zip(priors, points):
        w = mf.dq_w(p, x)
        assert int((w < 0).sum()) == min(2, len(w)) and np.all(w[2:] > 0)
    assert sum(int((mf.dq_w(p, x) < 0).sum()) for p, x in zip(priors, points)) >= 2
    assert abs(np.linalg.norm(priors[6]["x0"][3:7]) - 1.01) < 1e-12
    res, jac, _, _ = _evaluate(ctx, priors, points, want_jac=True)
    res_w, jac_w = mf.split(priors, res, "r"), mf.split(priors, jac, "jac")
    for w, (p, x) in enumerate(zip(priors, points)):
        e, J = oracle.marg_factor_eval(p["size"], p["index"], p["x0"], x, p["J0"], p["e0"])
        assert np.all(np.isfinite(e))
        assert same_bits(res_w[w], e), w
        assert same_bits(jac_w[w], J), w


def test_zero_norm_linearization_quaternion_gives_the_oracles_non_finite_values(ctx, oracle):
    p = mf.make_prior([7, 2, 7], 31)
    p["x0"][3:7] = 0.0
    x = mf.make_x(mf.make_prior([7, 2, 7], 31), 32)
    res, jac, _, _ = _evaluate(ctx, [p], [x], want_jac=True)
    e, J = oracle.marg_factor_eval(p["size"], p["index"], p["x0"], x, p["J0"], p["e0"])
    assert not np.all(np.isfinite(e))
    assert np.array_equal(np.isnan(res), np.isnan(e)) and np.array_equal(np.isinf(res), np.isinf(e))
    assert same_bits(res, e) and same_bits(jac, J)


def test_a_window_evaluates_to_the_same_bits_alone_and_in_any_batch(ctx, cases):
    priors, points = cases
    res, jac, grad, sq = _evaluate(ctx, priors, points, want_jac=True, want_grad=True, want_sq_norm=True)
    res_w, jac_w, grad_w = mf.split(priors, res, "r"), mf.split(priors, jac, "jac"), mf.split(priors, grad, "r")
    for w, (p, x) in enumerate(zip(priors, points)):
        r1, j1, g1, s1 = _evaluate(ctx, [p], [x], want_jac=True, want_grad=True, want_sq_norm=True)
        assert same_bits(r1, res_w[w]) and same_bits(j1, jac_w[w]) and same_bits(g1, grad_w[w]) and same_bits(s1, sq[w]), w
    rp, rx = priors[::-1], points[::-1]
    res_r, jac_r, grad_r, sq_r = _evaluate(ctx, rp, rx, want_jac=True, want_grad=True, want_sq_norm=True)
    rr, jr, gr = mf.split(rp, res_r, "r"), mf.split(rp, jac_r, "jac"), mf.split(rp, grad_r, "r")
    n = len(priors)
    for w in range(n):
        assert same_bits(rr[n - 1 - w], res_w[w]) and same_bits(jr[n - 1 - w], jac_w[w]) and same_bits(gr[n - 1 - w], grad_w[w]), w
        assert same_bits(sq_r[n - 1 - w], sq[w]), w


def test_the_set_stays_resident_and_a_new_set_replaces_it(ctx, cases):
    priors, points = cases
    want = dict(want_jac=True, want_grad=True, want_sq_norm=True)

    def fresh(ps, xs):
        c = _new_ctx()
        try:
            return _evaluate(c, ps, xs, **want)
        finally:
            c.close()

    def same(a, b):
        return all(same_bits(u, v) for u, v in zip(a, b))

    ctx.marg_prior_set(*mf.set_args(priors))
    for k in range(3):  # one set, three points
        xs = [mf.make_x(p, 200 + 10 * k + w, negate=(k,)) for w, p in enumerate(priors)]
        got = ctx.marg_prior_evaluate(np.concatenate(xs), **want)
        assert same(got, fresh(priors, xs)), k
    fewer = priors[2:4]
    xs = [mf.make_x(p, 300 + w) for w, p in enumerate(fewer)]
    ctx.marg_prior_set(*mf.set_args(fewer))
    assert same(ctx.marg_prior_evaluate(np.concatenate(xs), **want), fresh(fewer, xs))
    more = priors + [mf.make_prior(mf.R512_SIZES, 41), mf.make_prior([7, 9] * 30 + [7, 1], 42), mf.make_prior(mf.C4_SIZES, 43)]
    xs = [mf.make_x(p, 400 + w, negate=(1,)) for w, p in enumerate(more)]
    ctx.marg_prior_set(*mf.set_args(more))
    assert same(ctx.marg_prior_evaluate(np.concatenate(xs), **want), fresh(more, xs))


def test_optional_outputs_in_every_combination(ctx, cases):
    priors, points = cases
    a = mf.pack(priors)
    x = np.ascontiguousarray(np.concatenate(points))
    R, NJ, n = int(a["r"].sum()), int(sum(p["r"] * int(p["size"].sum()) for p in priors)), len(priors)
    ctx.marg_prior_set(*mf.set_args(priors))
    p_ = ptr
    ref = None
    for wj, wg, ws in itertools.product((False, True), repeat=3):
        res, jac, grad, sq = np.full(R, MARK), np.full(NJ, MARK), np.full(R, MARK), np.full(n, MARK)
        rc = ctx.lib.icg_marg_prior_evaluate(ctx.h, p_(x), p_(res), p_(jac) if wj else None, p_(grad) if wg else None, p_(sq) if ws else None)
        assert rc == 0, ctx.lib.icg_last_error(ctx.h)
        if ref is None:
            ref = res.copy()
        assert same_bits(res, ref), (wj, wg, ws)
        assert wj or np.all(jac == MARK)
        assert wg or np.all(grad == MARK)
        assert ws or np.all(sq == MARK)
        if wj and wg and ws:
            full = (jac.copy(), grad.copy(), sq.copy())
    jac, grad, sq = full
    res_w, grad_w = mf.split(priors, ref, "r"), mf.split(priors, grad, "r")
    for w, p in enumerate(priors):
        assert same_bits(grad_w[w], mf.sequential_gradient(p["J0"], res_w[w])), w
        assert same_bits(sq[w], mf.sequential_sq_norm(res_w[w])), w


def test_reference_golden(ctx, hostlib):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marg_ref_golden.npz"))
    P = md.make_problem(**bu.MARG_GOLDEN_ARGS)
    w = P["w"]
    out = bu.backend_marginalize(hostlib, P, huber=1.0, prior_weight=100.0)
    ids = [int(i) for i in out["ids"]]
    x = np.concatenate([bu._marg_perturbation(i, w) for i in ids])
    out = bu.backend_marginalize(hostlib, P, huber=1.0, prior_weight=100.0, x_eval=x)  # J0, e0 and the host's residual of one run
    assert [int(i) for i in out["ids"]] == ids

    def x0_of(i):
        if i < 100000:
            return np.asarray(w["poses"][i], np.float64)
        if i < 900000:
            return np.array([w["invdepth"][i - 100000]], np.float64)
        return np.asarray(w["ext"], np.float64) if i == 900000 else np.array([w["td"]], np.float64)

    x0 = np.concatenate([x0_of(i) for i in ids])
    index = out["index"] - out["m"]
    ctx.marg_prior_set([out["r"]], [0, len(ids)], out["size"], index, x0, out["J0"], out["e0"])
    res, _, grad, sq = ctx.marg_prior_evaluate(x, want_grad=True, want_sq_norm=True)
    assert same_bits(res, out["res"])
    cols = []
    for k in np.argsort(out["ids"]):
        c0 = int(index[k])
        cols.extend(range(c0, c0 + mf.local(int(out["size"][k]))))
    cost, gsorted = float(sq[0]), grad[np.array(cols)]
    d_cost, d_grad = abs(cost - float(g["cost"])), float(np.abs(gsorted - g["grad"]).max())
    print(f"marg golden: |cost - golden| = {d_cost:.3e} (cost {float(g['cost']):.6e}), max |grad - golden| = {d_grad:.3e} "
          f"(max |grad| {float(np.abs(g['grad']).max()):.6e})")
    assert d_cost < 1e-8 * max(1.0, float(g["cost"]))
    assert d_grad < 1e-7 * max(1.0, float(np.abs(g["grad"]).max()))


def test_host_layer_device_mode_equals_host_mode_bit_for_bit(hostlib):
    priors = [mf.make_prior(mf.C2_SIZES, 1000 + w) for w in range(256)]
    points = [[mf.make_x(p, 5000 + 300 * k + w, negate=(k, k + 3)) for w, p in enumerate(priors)] for k in range(3)]
    rc0, msg0, res0, jac0, grad0, sq0, _ = mf.backend_marg_factor(hostlib, 0, priors, points, host_threads=8)
    assert rc0 == 0, msg0
    rc1, msg1, res1, jac1, grad1, sq1, sec = mf.backend_marg_factor(hostlib, 1, priors, points, mark=MARK)
    assert rc1 == 0, msg1
    assert sec[0] > 0 and sec[1] > 0
    assert same_bits(res1, res0) and same_bits(jac1, jac0) and same_bits(grad1, grad0) and same_bits(sq1, sq0)
    assert not np.array_equal(res0[0], res0[1]) and not np.array_equal(res0[1], res0[2])


def test_errors_leave_the_outputs_and_the_context_intact(oracle, cases):
    import icgvins
    priors, points = cases
    c = _new_ctx()
    try:
        c.prof_enable(True)
        lib, p_ = c.lib, ptr
        msg = lambda: lib.icg_last_error(c.h).decode()
        good = priors[0]
        x = np.ascontiguousarray(points[0])
        outs = [np.full(good["r"], MARK), np.full(good["r"] * int(good["size"].sum()), MARK), np.full(good["r"], MARK), np.full(1, MARK)]

        def evaluate_fails():
            rc = lib.icg_marg_prior_evaluate(c.h, p_(x), *[p_(o) for o in outs])
            assert rc == -1 and "icg_marg_prior_evaluate" in msg(), (rc, msg())
            assert all(np.all(o == MARK) for o in outs)

        def set_rc(r, off, size, index, n=None):
            r, off, size, index = (np.ascontiguousarray(v, np.int32) for v in (r, off, size, index))
            big = int(max(1, np.abs(r).max()))
            z = np.zeros(big * big + 16)
            return lib.icg_marg_prior_set(c.h, len(r) if n is None else n, p_(r), p_(off), p_(size), p_(index), p_(z), p_(z), p_(z))

        evaluate_fails()  # before any set
        assert set_rc([3, 0], [0, 1, 2], [3, 1], [0, 0]) == -1 and "window 1" in msg()  # r = 0
        assert set_rc([12], [0, 2], [7, 7], [0, 7]) == -1 and "window 0" in msg()  # index + local > r
        assert set_rc([6, 6, 6], [0, 1, 0, 1], [7], [0]) == -1 and "window 1" in msg()  # block_off not monotone
        assert set_rc([2], [0, 1], [0], [0]) == -1 and "window 0" in msg()  # size <= 0
        assert set_rc([2], [0, 1], [1], [-1]) == -1 and "window 0" in msg()  # index < 0
        assert set_rc([2], [0, 1], [1], [0], n=0) == -1  # n_windows <= 0
        assert lib.icg_marg_prior_set(c.h, 1, None, None, None, None, None, None, None) == -1  # NULL
        over = icgvins.MARG_MAX_R + 1
        assert set_rc([4, over], [0, 1, 2], [4, 1], [0, 0]) == -5 and "window 1" in msg()  # above the limit
        evaluate_fails()  # a failed set leaves no set behind
        c.sync()
        assert not any(k.startswith("marg") for k in c.prof()), c.prof()  # nothing was launched
        # a valid set that a failed one follows is gone as well, and the context still works afterwards
        c.marg_prior_set(*mf.set_args([good]))
        assert set_rc([3, 0], [0, 1, 2], [3, 1], [0, 0]) == -1
        evaluate_fails()
        c.marg_prior_set(*mf.set_args([good]))
        res, jac, _, _ = c.marg_prior_evaluate(x, want_jac=True)
        e, J = oracle.marg_factor_eval(good["size"], good["index"], good["x0"], x, good["J0"], good["e0"])
        assert same_bits(res, e) and same_bits(jac, J)
        assert c.prof()["marg_eval"][0] == 1
    finally:
        c.close()
