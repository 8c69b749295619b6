"""GPU parity: the Schur step and the linearization of many reduced systems in one call (M3, icg_marg_linearize_batch) against the host
layer's linearizeReduced, the CPU oracle (orc_marginalize) and the reference golden.

The device runs the host's eigen-solver with every sum in the host's order; the one operation that may round differently is hypot, so
the comparisons are on what a linearization determines whatever the eigenvectors' signs and bases — Hp, bp, the eigenvalues, J0^T J0,
J0^T e0 and the cost at a perturbed point — to 1e-8 x scale (the bound backend_utils uses for Hp and bp), and rank decisions (status bits,
eigenvalues above the floor) must be the host's exactly: the inputs keep every eigenvalue a decade away from the floor, asserted from the
host's eigenvalues.  Determinism is bit for bit.  The measured maxima are printed."""
import concurrent.futures
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import backend_utils as bu
import marg_data as md
import marg_factor_data as mf
import marg_linearize_data as ml
from ctypes_util import ptr

pytestmark = pytest.mark.gpu

MARK = -7.25
KEYS = ("Hp", "bp", "evals", "min_ev_m", "status")


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
def systems():
    return ml.batch()


def _device(c, systems, **want):
    return ml.split(systems, c.marg_linearize_batch(*ml.pack(systems), eps=ml.EPS, **want))


def _same(a, b):
    return all(ml.same_bits(a[k], b[k]) for k in ("J0", "e0", "Hp", "bp", "evals")) and a["status"] == b["status"] and \
        ml.same_bits(a["min_ev_m"], b["min_ev_m"])


def test_heterogeneous_batch_equals_the_host_mode_and_the_oracle(ctx, oracle, hostlib, systems):
    rc, msg, out, _ = ml.backend_marg_linearize(hostlib, 0, systems, host_threads=8)
    assert rc == 0, msg
    host = ml.split(systems, out)
    ml.assert_no_eigenvalue_near_the_floor(hostlib, systems, host)
    dev = _device(ctx, systems)
    worst = {}

    def hold(name, what, err, scale):
        worst[what] = max(worst.get(what, 0.0), err / scale)
        assert err <= 1e-8 * scale, (name, what, err / scale)

    for s, d, h in zip(systems, dev, host):
        J0, e0, Hp, bp = oracle.marginalize(s["H"], s["b"], s["m"])
        orc = dict(J0=J0, e0=e0, Hp=Hp, bp=bp)
        inv = ml.invariants(s, d)
        assert d["status"] & 1 == 0, s["name"]
        assert d["status"] & 6 == h["status"], (s["name"], d["status"], h["status"])
        assert int((d["evals"] > ml.EPS).sum()) == int((h["evals"] > ml.EPS).sum()), s["name"]
        assert (np.isinf(d["min_ev_m"]) and d["min_ev_m"] > 0) if s["m"] == 0 else np.isfinite(d["min_ev_m"])
        sev = max(1.0, float(np.abs(h["evals"]).max()))
        hold(s["name"], "evals", np.abs(d["evals"] - h["evals"]).max(), sev)
        if s["m"] > 0:
            hold(s["name"], "min_ev_m", abs(d["min_ev_m"] - h["min_ev_m"]), sev)
        for tag, ref in (("host", h), ("oracle", orc)):
            rinv = ml.invariants(s, ref)
            sc, sb = float(np.abs(ref["Hp"]).max()), max(1.0, float(np.abs(ref["bp"]).max()))
            hold(s["name"], "Hp vs " + tag, np.abs(d["Hp"] - ref["Hp"]).max(), sc)
            hold(s["name"], "bp vs " + tag, np.abs(d["bp"] - ref["bp"]).max(), sb)
            hold(s["name"], "J0^T J0 vs " + tag, np.abs(inv["JtJ"] - rinv["JtJ"]).max(), sc)
            hold(s["name"], "J0^T e0 vs " + tag, np.abs(inv["Jte"] - rinv["Jte"]).max(), sb)
            hold(s["name"], "cost vs " + tag, abs(inv["cost"] - rinv["cost"]), max(1.0, rinv["cost"]))
    print("M3 device, largest error / scale over the batch: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    same = sum(int(ml.same_bits(d["J0"], h["J0"]) and ml.same_bits(d["e0"], h["e0"])) for d, h in zip(dev, host))
    print(f"M3 device: J0 and e0 bit-identical to the host mode in {same} of {len(systems)} windows")


def test_host_layer_device_mode_is_the_c_entry(ctx, hostlib, systems):
    rc, msg, out, sec = ml.backend_marg_linearize(hostlib, 1, systems, reps=1)
    assert rc == 0, msg
    assert sec[0] > 0 and sec[1] > 0
    for a, b in zip(ml.split(systems, out), _device(ctx, systems)):
        assert _same(a, b)


def test_reference_golden(ctx, oracle):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marg_ref_golden.npz"))
    s, P = ml.golden_system(oracle)
    w = P["w"]
    assert s["m"] == int(g["m"]) and s["P"] - s["m"] == int(g["r"])
    ids = [int(i) for i in g["ids"]]
    # the oracle's retained column order (poses ascending, extrinsic, td) is the golden's id-sorted order
    assert ids == sorted(ids) and [i for i in ids if i < 100000] == [k for k in range(1, len(P["col_pose"])) if P["col_pose"][k] >= 0]
    assert ids[-2:] == [900000, 900001] and len(ids) == len([i for i in ids if i < 100000]) + 2
    d = _device(ctx, [s])[0]
    sc = float(np.abs(g["Hp"]).max())
    d_Hp, d_bp = float(np.abs(d["Hp"] - g["Hp"]).max()), float(np.abs(d["bp"] - g["bp"]).max())
    assert d_Hp < 1e-8 * sc and d_bp < 1e-8 * max(1.0, float(np.abs(g["bp"]).max()))
    # the prior through M4: cost and gradient at the golden's evaluation point
    size = np.array([7 if i != 900001 else 1 for i in ids], np.int32)
    index = np.concatenate([[0], np.cumsum([mf.local(int(v)) for v in size])[:-1]]).astype(np.int32)

    def x0_of(i):
        if i < 100000:
            return np.asarray(w["poses"][i], np.float64)
        return np.asarray(w["ext"], np.float64) if i == 900000 else np.array([w["td"]], np.float64)

    x0 = np.concatenate([x0_of(i) for i in ids])
    x = np.concatenate([bu._marg_perturbation(i, w) for i in ids])
    ctx.marg_prior_set([int(g["r"])], [0, len(ids)], size, index, x0, d["J0"], d["e0"])
    _, _, grad, sq = ctx.marg_prior_evaluate(x, want_grad=True, want_sq_norm=True)
    d_cost, d_grad = abs(float(sq[0]) - float(g["cost"])), float(np.abs(grad - g["grad"]).max())
    print(f"M3 golden: max |Hp - golden| / scale = {d_Hp / sc:.3e}, max |bp - golden| = {d_bp:.3e}, |cost - golden| = {d_cost:.3e} "
          f"(cost {float(g['cost']):.6e}), max |grad - golden| = {d_grad:.3e} (max |grad| {float(np.abs(g['grad']).max()):.6e})")
    assert d_cost < 1e-8 * max(1.0, float(g["cost"]))
    assert d_grad < 1e-7 * max(1.0, float(np.abs(g["grad"]).max()))


def test_a_window_gives_the_same_bits_alone_in_any_batch_and_run_after_run(ctx, systems):
    dev = _device(ctx, systems)
    again = _device(ctx, systems)
    rev = _device(ctx, systems[::-1])[::-1]
    for w, s in enumerate(systems):
        alone = _device(ctx, [s])[0]
        assert _same(alone, dev[w]) and _same(again[w], dev[w]) and _same(rev[w], dev[w]), s["name"]
    c2 = _new_ctx()  # another context: nothing of a result lives in the context
    try:
        other = _device(c2, systems[2:5])
    finally:
        c2.close()
    assert all(_same(a, b) for a, b in zip(other, dev[2:5]))


def test_optional_outputs_in_every_combination(ctx, systems):
    some = [systems[k] for k in (2, 3, 4, 7, 9)]
    P, m, H, b = ml.pack(some)
    r = P.astype(np.int64) - m
    nr, nrr, n = int(r.sum()), int((r * r).sum()), len(some)
    p_ = ptr
    ref = ctx.marg_linearize_batch(P, m, H, b, eps=ml.EPS)
    for want in itertools.product((False, True), repeat=5):
        bufs = dict(Hp=np.full(nrr, MARK), bp=np.full(nr, MARK), evals=np.full(nr, MARK), min_ev_m=np.full(n, MARK),
                    status=np.full(n, int(MARK), np.int32))
        J0, e0 = np.full(nrr, MARK), np.full(nr, MARK)
        opt = [p_(bufs[k]) if on else None for k, on in zip(KEYS, want)]
        rc = ctx.lib.icg_marg_linearize_batch(ctx.h, n, p_(P), p_(m), p_(H), p_(b), C.c_double(ml.EPS), opt[0], opt[1], p_(J0), p_(e0), opt[2],
                                              opt[3], opt[4])
        assert rc == 0, ctx.lib.icg_last_error(ctx.h)
        assert ml.same_bits(J0, ref["J0"]) and ml.same_bits(e0, ref["e0"]), want
        for k, on in zip(KEYS, want):
            if not on:
                assert np.all(bufs[k] == (int(MARK) if k == "status" else MARK)), (want, k)
            elif k == "status":
                assert np.array_equal(bufs[k], ref[k]), (want, k)
            else:
                assert ml.same_bits(bufs[k], ref[k]), (want, k)


def test_errors_leave_the_outputs_and_the_context_intact(oracle, systems):
    import icgvins
    c = _new_ctx()
    try:
        c.prof_enable(True)
        lib, p_ = c.lib, (lambda a: None if a is None else a.ctypes.data_as(C.c_void_p))
        msg = lambda: lib.icg_last_error(c.h).decode()
        outs = [np.full(4096, MARK) for _ in range(6)] + [np.full(8, int(MARK), np.int32)]
        z = np.zeros(4096)

        def call(P, m, n=None, H=z, b=z, J0=outs[2], e0=outs[3], eps=ml.EPS):
            P, m = np.ascontiguousarray(P, np.int32), np.ascontiguousarray(m, np.int32)
            return lib.icg_marg_linearize_batch(c.h, len(P) if n is None else n, p_(P), p_(m), p_(H), p_(b), C.c_double(eps), p_(outs[0]), p_(outs[1]),
                                                p_(J0), p_(e0), p_(outs[4]), p_(outs[5]), p_(outs[6]))

        assert call([4, 0], [1, 0]) == -1 and "window 1" in msg()  # P <= 0
        assert call([4, 3, 5], [1, 3, 2]) == -1 and "window 1" in msg()  # m = P
        assert call([4, 3], [-1, 0]) == -1 and "window 0" in msg()  # m < 0
        assert call([4], [1], n=0) == -1  # n_windows <= 0
        assert call([4], [1], H=None) == -1 and call([4], [1], b=None) == -1  # NULL inputs
        assert call([4], [1], J0=None) == -1 and call([4], [1], e0=None) == -1  # NULL required outputs
        assert lib.icg_marg_linearize_batch(c.h, 1, None, None, p_(z), p_(z), C.c_double(ml.EPS), None, None, p_(outs[2]), p_(outs[3]), None, None, None) == -1
        assert call([4], [1], eps=-1.0) == -1
        assert call([4, icgvins.MARG_LIN_MAX_P + 1], [1, 0]) == -5 and "window 1" in msg()  # above the cap
        assert call([4, icgvins.MARG_LIN_MAX_P + 1, 0], [1, 0, 0]) == -1 and "window 2" in msg()  # invalid wins over capacity
        assert all(np.all(o == (int(MARK) if o.dtype == np.int32 else MARK)) for o in outs)
        c.sync()
        assert not any(k.startswith("marg") for k in c.prof()), c.prof()  # nothing was launched
        # the context works afterwards
        s = systems[2]
        d = ml.split([s], c.marg_linearize_batch(*ml.pack([s]), eps=ml.EPS))[0]
        J0, e0, Hp, bp = oracle.marginalize(s["H"], s["b"], s["m"])
        assert np.abs(d["Hp"] - Hp).max() <= 1e-8 * np.abs(Hp).max() and np.abs(d["bp"] - bp).max() <= 1e-8 * max(1.0, np.abs(bp).max())
        assert sum(v[0] for k, v in c.prof().items() if k.startswith("marg_lin")) == 1
    finally:
        c.close()


def test_marginalization_batch_with_the_device_linearization(hostlib, oracle):
    """icgh_backend_marginalize_batch mode 2 (MarginalizationBatch::setDeviceLinearization) on 256 jittered C2 windows plus one window that
    takes the dense path: the structured / dense counts of mode 0, every window against the oracle's own assembly + Schur complement
    (the check of backend_utils.check_marginalization_batch), mode 2 bit-identical to itself across two runs"""
    P = md.make_problem(n_lm=300, n_kf=10, seed=2)
    W, dense = 257, 5
    a = bu.backend_marginalize_batch(hostlib, P, W, 0, dense)
    b = bu.backend_marginalize_batch(hostlib, P, W, 2, dense)
    b2 = bu.backend_marginalize_batch(hostlib, P, W, 2, dense)
    assert (b["structured"], b["dense"]) == (a["structured"], a["dense"]) == (W - 1, 1)
    assert a["m"] == b["m"] and a["r"] == b["r"]
    for k in ("Hp", "bp", "J0", "e0"):
        assert np.array_equal(b[k], b2[k]), k
    layout = bu.backend_marginalize(hostlib, P)
    params = bu.batch_window_parameters(P, W)
    assert layout["r"] == b["r"] and layout["m"] == b["m"]

    def expected(k):
        sp = None
        if k == dense:
            l0 = int(P["ll"][0])
            sp = (l0, params[k]["invdepth"][l0] * 1.01, 50.0)
        return bu.oracle_marginalized_system(oracle, P, params[k], layout, scalar_prior=sp)

    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        exp = list(ex.map(expected, range(W)))
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in range(W):
        Hp_exp, bp_exp = exp[k]
        sc, sb = np.abs(Hp_exp).max(), max(1.0, np.abs(bp_exp).max())
        for got in (a, b):
            assert np.abs(got["Hp"][k] - Hp_exp).max() < 1e-8 * sc, (k, np.abs(got["Hp"][k] - Hp_exp).max() / sc)
            assert np.abs(got["bp"][k] - bp_exp).max() < 1e-8 * sb, k
        # mode 2 against mode 0, with the bounds check_marginalization_batch holds the batch to against the per-window path
        e = [np.abs(b["Hp"][k] - a["Hp"][k]).max() / sc, np.abs(b["bp"][k] - a["bp"][k]).max() / sb,
             np.abs(b["J0"][k].T @ b["J0"][k] - a["J0"][k].T @ a["J0"][k]).max() / sc,
             np.abs(b["J0"][k].T @ b["e0"][k] - a["J0"][k].T @ a["e0"][k]).max() / sb]
        worst = [max(u, v) for u, v in zip(worst, e)]
        assert e[0] < 1e-9 and e[1] < 1e-9 and e[2] < 1e-7 and e[3] < 1e-7, (k, e)
    assert np.abs(b["Hp"][1] - b["Hp"][0]).max() > 1e-6 * np.abs(b["Hp"][0]).max()  # (the jitter moved the windows)
    print(f"marginalization batch, device linearization against the default: Hp {worst[0]:.2e}, bp {worst[1]:.2e}, J0^T J0 {worst[2]:.2e}, "
          f"J0^T e0 {worst[3]:.2e} (error / scale, largest of {W} windows); {a['seconds'] * 1e3:.2f} ms default, {b['seconds'] * 1e3:.2f} ms device")
