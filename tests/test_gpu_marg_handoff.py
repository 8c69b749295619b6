"""GPU: the linearized priors stay on the device between M3 and M4.  icg_marg_linearize_batch_keep returns the bits of
icg_marg_linearize_batch; a prior set built by icg_marg_prior_set_from_kept evaluates to the bits of the set built by icg_marg_prior_set
from the downloaded J0 / e0, with the kept linearization in the same context and in another one; the kept linearization's lifetime and the
argument errors (which launch nothing and leave no set resident); the host chain marginalize -> clear -> set -> evaluate and a mode-3
WindowSolverBatch solve with keeping on equal the same chain with keeping off, bit for bit.  No tolerance anywhere: every comparison is
between two paths that move the same doubles."""
import ctypes as C

import numpy as np
import pytest

import marg_factor_data as mf
import marg_handoff_data as mh
import marg_linearize_data as ml
from ctypes_util import bits, ptr

pytestmark = pytest.mark.gpu

def _ctx():
    import icgvins
    return icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)


@pytest.fixture()
def ctx():
    c = _ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def kept_ref():
    """the kept batch through the plain entry, once: (systems, packed inputs, flat outputs)"""
    systems = mh.kept_systems()
    args = ml.pack(systems)
    c = _ctx()
    out = c.marg_linearize_batch(*args)
    c.close()
    return systems, args, out


def _same_outputs(got, ref, keys):
    for k in keys:
        if ref[k].dtype == np.int32:
            assert np.array_equal(got[k], ref[k]), k
        else:
            assert np.array_equal(bits(got[k]), bits(ref[k])), k


def test_keep_variant_equals_the_plain_entry(ctx, kept_ref):
    systems, args, ref = kept_ref
    assert ref["status"][5] & 4  # the rank-deficient window is one
    got, kid = ctx.marg_linearize_batch_keep(*args)
    assert kid != 0
    _same_outputs(got, ref, ("J0", "e0", "Hp", "bp", "evals", "min_ev_m", "status"))
    got2, kid2 = ctx.marg_linearize_batch_keep(*args, want_J0=False, want_e0=False)
    assert kid2 not in (0, kid) and got2["J0"] is None and got2["e0"] is None
    _same_outputs(got2, ref, ("Hp", "bp", "evals", "min_ev_m", "status"))
    # what was kept with both NULL is the same linearization: a set built from it evaluates like one built from the reference's arrays
    priors = [mf.make_prior([1] * r, 60 + k) for k, r in enumerate(mh.KEPT_R)]
    for p, d in zip(priors, ml.split(systems, ref)):
        p["J0"], p["e0"] = d["J0"], d["e0"]
    a = mf.pack(priors)
    x = np.concatenate([mf.make_x(p, 70 + k) for k, p in enumerate(priors)])
    ctx.marg_prior_set_from_kept(kid2, np.arange(len(priors)), a["r"], a["block_off"], a["block_size"], a["block_index"], a["x0"])
    got_eval = ctx.marg_prior_evaluate(x, want_grad=True, want_sq_norm=True)
    ctx.marg_prior_set(*mf.set_args(priors))
    ref_eval = ctx.marg_prior_evaluate(x, want_grad=True, want_sq_norm=True)
    for g, r in zip(got_eval, ref_eval):
        assert (g is None) == (r is None) and (g is None or np.array_equal(bits(g), bits(r)))


@pytest.mark.parametrize("other_context", [False, True])
def test_hand_off_equals_shipping(ctx, kept_ref, other_context):
    systems, args, ref = kept_ref
    owner = _ctx() if other_context else ctx
    try:
        _, kid = owner.marg_linearize_batch_keep(*args, want_J0=False, want_e0=False, want_Hp=False, want_bp=False, want_evals=False)
        kept = ml.split(systems, ref)
        priors = mh.set_priors()
        src = np.array(mh.SRC, np.int32)
        assert sorted(src[src >= 0]) != list(src[src >= 0]) and list(src).count(3) == 2 and list(src).count(-1) == 1
        host = [p for p, s in zip(priors, src) if s < 0]
        for p, s in zip(priors, src):
            if s >= 0:
                p["J0"], p["e0"] = kept[s]["J0"].copy(), kept[s]["e0"].copy()
        a = mf.pack(priors)
        J0_host = np.concatenate([p["J0"].ravel() for p in host])
        e0_host = np.concatenate([p["e0"].ravel() for p in host])
        ctx.prof_enable(True)
        ctx.marg_prior_set_from_kept(kid, src, a["r"], a["block_off"], a["block_size"], a["block_index"], a["x0"], J0_host, e0_host)
        points = [np.concatenate(mh.set_points(priors, seed)) for seed in (100, 200)]
        got = [(ctx.marg_prior_evaluate(x, want_jac=True, want_grad=True, want_sq_norm=True), ctx.marg_prior_evaluate_resident(x)) for x in points]
        prof = ctx.prof()
        assert prof["marg_set_from"][0] == 1 and "marg_set" not in prof  # the new store kernel ran, the shipping one did not
        ctx.marg_prior_set(*mf.set_args(priors))
        for x, (g, g_res) in zip(points, got):
            r = ctx.marg_prior_evaluate(x, want_jac=True, want_grad=True, want_sq_norm=True)
            for name, gv, rv in zip(("residuals", "jacobians", "gradient", "sq_norm"), g, r):
                assert np.array_equal(bits(gv), bits(rv)), name
            assert np.array_equal(bits(g_res), bits(ctx.marg_prior_evaluate_resident(x)))
            assert np.array_equal(bits(g_res), bits(g[3]))
        assert not np.array_equal(bits(got[0][0][0]), bits(got[1][0][0]))
    finally:
        if other_context:
            owner.close()


def test_lifetime_and_errors(ctx, kept_ref):
    import icgvins
    systems, args, ref = kept_ref
    priors = mh.set_priors()
    src = np.array(mh.SRC, np.int32)
    a = mf.pack(priors)
    host = [p for p, s in zip(priors, src) if s < 0]
    J0_host = np.concatenate([p["J0"].ravel() for p in host])
    e0_host = np.concatenate([p["e0"].ravel() for p in host])
    x = np.concatenate(mh.set_points(priors, 100))
    res = np.zeros(int(a["r"].sum()))
    p_ = ptr

    def call(c, kid, **over):
        v = dict(src=src, r=a["r"], block_off=a["block_off"], block_size=a["block_size"], block_index=a["block_index"], x0=a["x0"], J0=J0_host, e0=e0_host)
        v.update(over)
        rc = c.lib.icg_marg_prior_set_from_kept(c.h, C.c_uint64(kid), len(a["r"]), p_(v["src"]), p_(v["r"]), p_(v["block_off"]), p_(v["block_size"]),
                                                p_(v["block_index"]), p_(v["x0"]), p_(v["J0"]), p_(v["e0"]))
        return rc, c.lib.icg_last_error(c.h).decode()

    def nothing_resident_nothing_launched(c, before):
        c.sync()
        assert c.prof() == before, (before, c.prof())
        assert c.lib.icg_marg_prior_evaluate(c.h, p_(x), p_(res), None, None, None) == -1 and b"no prior set is resident" in c.lib.icg_last_error(c.h)
        assert not res.any()
        c.sync()
        assert c.prof() == before

    owner = _ctx()
    try:
        _, kid = owner.marg_linearize_batch_keep(*args, want_Hp=False, want_bp=False, want_evals=False)
        ctx.prof_enable(True)
        # every failing call below starts from a resident set: a failed call leaves none
        cases = [("unknown id", dict(kid=kid + 1000), "is gone"),
                 ("r mismatch", dict(r=np.concatenate([a["r"][:1], [1], a["r"][2:]]).astype(np.int32), src=np.array([3, 1] + mh.SRC[2:], np.int32)), "window 1: r = 1, kept window 1 has r = 6"),
                 ("src out of range", dict(src=np.array([3, 7] + mh.SRC[2:], np.int32)), "window 1: src = 7, the kept linearization has 7 windows"),
                 ("src below -1", dict(src=np.array([3, -2] + mh.SRC[2:], np.int32)), "window 1: src = -2"),
                 ("-1 with NULL host arrays", dict(J0=None, e0=None), "window 3: src = -1 and no host J0 / e0"),
                 ("NULL src", dict(src=None), "NULL argument"), ("NULL r", dict(r=None), "NULL argument"), ("NULL x0", dict(x0=None), "NULL argument"),
                 ("NULL block_off", dict(block_off=None), "NULL argument")]
        for name, over, text in cases:
            ctx.marg_prior_set(*mf.set_args(priors))
            ctx.sync()
            before = ctx.prof()
            k = over.pop("kid", kid)
            rc, msg = call(ctx, k, **over)
            assert rc == -1 and text in msg and "icg_marg_prior_set_from_kept" in msg, (name, rc, msg)
            nothing_resident_nothing_launched(ctx, before)
        assert ctx.lib.icg_marg_prior_set_from_kept(None, C.c_uint64(kid), len(a["r"]), p_(src), p_(a["r"]), p_(a["block_off"]), p_(a["block_size"]),
                                                    p_(a["block_index"]), p_(a["x0"]), p_(J0_host), p_(e0_host)) == -1
        # too many windows: the capacity code, as in icg_marg_prior_set
        ctx.sync()
        before = ctx.prof()
        rc = ctx.lib.icg_marg_prior_set_from_kept(ctx.h, C.c_uint64(kid), 65536, p_(src), p_(a["r"]), p_(a["block_off"]), p_(a["block_size"]), p_(a["block_index"]),
                                                  p_(a["x0"]), p_(J0_host), p_(e0_host))
        assert rc == -5 and b"65536 windows" in ctx.lib.icg_last_error(ctx.h)
        nothing_resident_nothing_launched(ctx, before)
        # the keep entry's own arguments
        assert owner.lib.icg_marg_linearize_batch_keep(None, 1, None, None, None, None, C.c_double(1e-8), None, None, None, None, None, None, None, None) == -1
        # the id is good ...
        rc, msg = call(ctx, kid)
        assert rc == 0, msg
        # ... until a later linearize call on the owner, also a failing one and one of the plain entry
        for later in ("failing", "plain", "keep"):
            if later == "failing":
                assert owner.lib.icg_marg_linearize_batch(owner.h, 0, None, None, None, None, C.c_double(1e-8), None, None, None, None, None, None, None) == -1
            elif later == "plain":
                owner.marg_linearize_batch(*ml.pack(systems[:2]), want_Hp=False, want_bp=False, want_evals=False)
            else:
                _, newer = owner.marg_linearize_batch_keep(*args, want_Hp=False, want_bp=False, want_evals=False)
                assert newer != kid
            ctx.sync()
            before = ctx.prof()
            rc, msg = call(ctx, kid)
            assert rc == -1 and "is gone" in msg, (later, rc, msg)
            nothing_resident_nothing_launched(ctx, before)
            _, kid_next = owner.marg_linearize_batch_keep(*args, want_Hp=False, want_bp=False, want_evals=False)
            assert kid_next > kid  # never reused
            assert call(ctx, kid_next)[0] == 0
            kid = kid_next
        # after the release
        owner.marg_linearized_release()
        ctx.sync()
        before = ctx.prof()
        rc, msg = call(ctx, kid)
        assert rc == -1 and "is gone" in msg, (rc, msg)
        nothing_resident_nothing_launched(ctx, before)
        assert owner.lib.icg_marg_linearized_release(None) == -1
        # after the owner is destroyed
        _, kid = owner.marg_linearize_batch_keep(*args, want_Hp=False, want_bp=False, want_evals=False)
        assert call(ctx, kid)[0] == 0
        owner.close()
        ctx.sync()
        before = ctx.prof()
        rc, msg = call(ctx, kid)
        assert rc == -1 and "is gone" in msg, (rc, msg)
        nothing_resident_nothing_launched(ctx, before)
        # a set of shipped windows alone needs no linearization
        only = [priors[3]]
        b = mf.pack(only)
        ctx.marg_prior_set_from_kept(0, [-1], b["r"], b["block_off"], b["block_size"], b["block_index"], b["x0"], b["J0"], b["e0"])
        xo = mh.set_points(priors, 100)[3]
        got = ctx.marg_prior_evaluate(xo, want_sq_norm=True)
        ctx.marg_prior_set(*mf.set_args(only))
        exp = ctx.marg_prior_evaluate(xo, want_sq_norm=True)
        assert np.array_equal(bits(got[0]), bits(exp[0])) and np.array_equal(bits(got[3]), bits(exp[3]))
    finally:
        owner.close()


@pytest.fixture(scope="module")
def host_lib():
    import harness
    return C.CDLL(harness.HOST_LIB)


@pytest.fixture(scope="module")
def problem():
    import marg_data as md
    return md.make_problem(n_lm=80, n_kf=6, seed=2)


@pytest.fixture(scope="module")
def shipped_chain(host_lib, problem):
    """six jittered structured windows and one on the dense path, keeping off, with the solve: the reference of the two tests below"""
    rc, msg, out = mh.backend_marg_handoff(host_lib, problem, 7, 0, dense_window=2, solve_iters=4)
    assert rc == 0, msg
    assert out["priors"] == 7 and out["dense"] == 1 and out["handed_off"] == 0 and out["tagged"] == 0 and out["solver_handed_off"] == 0
    return out


EVAL_KEYS = ("residuals", "gradient", "sq_norm", "sq_norm_resident")


def test_host_chain_keeping_on_equals_keeping_off(host_lib, problem, shipped_chain):
    off = shipped_chain
    assert off["residuals"].any() and np.array_equal(bits(off["sq_norm"]), bits(off["sq_norm_resident"]))
    rc, msg, on = mh.backend_marg_handoff(host_lib, problem, 7, 1, dense_window=2)
    assert rc == 0, msg
    assert (on["priors"], on["structured"], on["dense"]) == (off["priors"], off["structured"], off["dense"])
    for k in EVAL_KEYS:
        assert np.array_equal(bits(on[k]), bits(off[k])), k
    # every device-linearized window was handed off; the dense window was shipped
    assert on["handed_off"] == on["tagged"] and 1 <= on["handed_off"] < 7, on
    # the kept linearization released before the set: the same bits, everything shipped
    rc, msg, rel = mh.backend_marg_handoff(host_lib, problem, 7, 3, dense_window=2)
    assert rc == 0, msg
    assert rel["handed_off"] == 0 and rel["tagged"] == on["tagged"]
    for k in EVAL_KEYS:
        assert np.array_equal(bits(rel[k]), bits(off[k])), k


def test_solver_with_handed_off_priors_equals_shipped(host_lib, problem, shipped_chain):
    off = shipped_chain
    rc, msg, on = mh.backend_marg_handoff(host_lib, problem, 7, 1, dense_window=2, solve_iters=4)
    assert rc == 0, msg
    assert on["solver_handed_off"] >= 1 and on["solver_handed_off"] == on["tagged"]
    for k in ("states", "invdepth", "summary"):
        assert np.array_equal(bits(on[k]), bits(off[k])), k
    assert (off["summary"][:, 0] > 0).all() and (off["summary"][:, 2:].sum(axis=1) > 0).all()  # every window was solved: a cost, and LM steps taken
