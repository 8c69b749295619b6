"""GPU: the resident preintegration factors as the host-part kernel reads them.  icg_reproj_host_parts_build_preint (residuals and Jacobians
taken from the resident P2 set on the device) gives the part, s and diag icg_reproj_host_parts_build gives on the same context when it is fed
the fetched residuals and the numpy-gathered columns of the fetched Jacobians; a later rebuild with -1 keeps the gathered Jacobian; a window
has the same bits alone and in the batch; the prior entry is the case without preintegration blocks; the argument errors name window and block
and launch nothing.  Bit patterns throughout.

The set is built from the device's own integration results and square-root information with arbitrary unit quaternions in place of the
host's: what is compared here is the gather, not the evaluation (tests/test_gpu_preint_resident.py holds that to the host's bits)."""
import numpy as np
import pytest

import marg_factor_data as mf
import preint_data as pd
import preint_split_data as sd
from test_gpu_marg_prior_resident import _columns, _gathered, _partition
from ctypes_util import bits, i32

pytestmark = pytest.mark.gpu

FILL = 7.0
P = 48
ALL = np.array(list(range(0, 6)) + list(range(7, 16)) + list(range(16, 22)) + list(range(23, 32)), np.int32)  # all four blocks free
SECOND = ALL[15:]  # the first state constant


@pytest.fixture()
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


def _unit(rng, n, scale):
    q = np.concatenate([rng.normal(0, scale, (n, 3)), np.ones((n, 1))], axis=1)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _resident_set(ctx):
    """six factors (N E N E E N) of 21-sample intervals -> the two evaluations' arguments"""
    n = 6
    imus, states = sd.intervals([21] * n, seed0=70)
    off = (np.arange(n + 1) * 21).astype(np.int32)
    cur, delta, jac, cov, dt, pn = ctx.preint_batch(1, off, np.concatenate(imus), np.stack(states), pd.PARAMS)
    pn_rows = pn.reshape(n, 21, 4)[:, :20].reshape(-1, 4)
    pn_off = (np.arange(n + 1) * 20).astype(np.int32)
    env = np.tile(pd.PARAMS[5:9], (n, 1))
    pts = [np.stack([sd.eval_point(kind, states[i], cur[i]) for i in range(n)]) for kind in ("perturbed", "large_bias_step")]
    _, _, S, status = ctx.preint_evaluate_batch(1, delta, jac, cov, dt, env, pts[0], pn_off, pn_rows)
    assert np.all(status == 0)
    rng = np.random.RandomState(3)
    ctx.preint_set([0, 1, 0, 1, 1, 0], delta, jac, S, dt, env, _unit(rng, n, 1e-5), pn_off, pn_rows)
    return pts, [_unit(rng, n, 1e-3), _unit(rng, n, 3e-2)]


def _j32(J480):
    return np.concatenate([J480[0:105].reshape(15, 7), J480[105:240].reshape(15, 9), J480[240:345].reshape(15, 7), J480[345:480].reshape(15, 9)], axis=1)


def _arrays(layout, Pw, rebuild):
    """the raw arguments of icg_reproj_host_parts_build_preint.  A block is ("ord", J, r, cols), ("prior", p, prior_cols, cols, how) or
    ("preint", f, preint_cols, cols, how), how = "gather" / "keep"; the resident blocks' slots in r are NaN"""
    blocks = [b for win in layout for b in win]
    a = dict(Pw=i32(Pw), rebuild=np.ascontiguousarray(rebuild, np.uint8), blk_off=i32(np.concatenate([[0], np.cumsum([len(w) for w in layout])])))
    nr, nf, cols, r, prior_of, preint_of, pc, qc, jac_off, Js, at = [], [], [], [], [], [], [], [], [], [], 0
    for b in blocks:
        if b[0] == "ord":
            nr.append(b[1].shape[0]), nf.append(b[1].shape[1]), cols.append(b[3]), r.append(b[2]), prior_of.append(-1), preint_of.append(-1)
            jac_off.append(at), Js.append(b[1].ravel())
            at += b[1].size
        else:
            nr.append(b[5] if b[0] == "prior" else 15), nf.append(len(b[3])), cols.append(b[3]), r.append(np.full(nr[-1], np.nan))
            prior_of.append(b[1] if b[0] == "prior" else -1), preint_of.append(b[1] if b[0] == "preint" else -1)
            (pc if b[0] == "prior" else qc).append(b[2])
            jac_off.append(-1 if b[4] == "keep" else (-2 if b[0] == "prior" else -3))
    cat = lambda xs, t: np.ascontiguousarray(np.concatenate(xs), t) if xs else None
    a.update(nr=i32(nr), nf=i32(nf), cols=cat(cols, np.int32), r=cat(r, np.float64), prior_of=i32(prior_of), preint_of=i32(preint_of), prior_cols=cat(pc, np.int32),
             preint_cols=cat(qc, np.int32), jac_off=np.ascontiguousarray(jac_off, np.int64), J=cat(Js, np.float64))
    return a


def _call(ctx, a, W, entry="preint", **over):
    a = dict(a)
    a.update(over)
    sizes = [int(a["Pw"][w]) * (int(a["Pw"][w]) + 1) // 2 if a["rebuild"][w] else 0 for w in range(W)]
    s, dg, part = np.full((W, P), FILL), np.full((W, P), FILL), np.full(max(1, sum(sizes)), FILL)
    lead = (P, a["Pw"], a["rebuild"], a["blk_off"], a["nr"], a["nf"], a["cols"], a["jac_off"], a["J"], a["r"], s, dg, part, a["prior_of"], a["prior_cols"])
    if entry == "preint":
        rc = ctx.reproj_host_parts_build_preint_raw(*lead, a["preint_of"], a["preint_cols"])
    else:
        rc = ctx.reproj_host_parts_build_prior_raw(*lead)
    parts, at = [], 0
    for w in range(W):
        parts.append(part[at:at + sizes[w]].copy() if a["rebuild"][w] else None)
        at += sizes[w]
    return rc, ctx.lib.icg_last_error(ctx.h).decode(), (s, dg, parts), part


def _same(got, ref, rebuilt):
    (gs, gd, gp), (rs, rdg, rp) = got, ref
    for w in rebuilt:
        assert np.array_equal(bits(gp[w]), bits(rp[w])), ("part", w)
        assert np.array_equal(bits(gs[w]), bits(rs[w])) and np.array_equal(bits(gd[w]), bits(rdg[w])), ("s / diag", w)


def _layout(rng, prior, how):
    mk = lambda nr, cols, scale=1.0: ("ord", rng.normal(0, scale, (nr, len(cols))), rng.normal(0, 1.0, nr), np.asarray(cols, np.int32))
    pc = _columns(prior)[0]
    layout = [[("preint", 3, ALL, np.arange(0, 30), how), ("preint", 1, ALL, np.arange(15, 45), how)],  # two factors sharing the middle state's columns
              [("preint", 0, SECOND, np.arange(0, 15), how), mk(9, range(6, 15), 10.0)],  # the first state constant: nf = 15
              [mk(6, range(0, 6), 30.0), ("preint", 4, ALL, 3 + rng.permutation(30), how), ("prior", 0, pc, np.arange(34, 40), how, prior["r"])],
              [],  # rebuilt, no host block
              [mk(3, [1, 5, 2]), ("preint", 5, ALL, np.arange(30), how)],  # not rebuilt: its block only places the others' columns
              [("preint", 2, ALL, rng.permutation(30), how)]]
    return layout, [45, 20, 40, 10, 30, 30], [1, 1, 1, 1, 0, 1]


def _reference(ctx, layout, Pw, rebuild, r_fetch, J_fetch, prior, prior_res, prior_jac):
    """icg_reproj_host_parts_build fed what the resident blocks hold: the fetched residuals and the numpy-gathered columns"""
    wins = []
    for win in layout:
        out = []
        for b in win:
            if b[0] == "ord":
                out.append((b[1], b[2], b[3], False))
            elif b[0] == "preint":
                out.append((np.ascontiguousarray(_j32(J_fetch[b[1]])[:, b[2]]), r_fetch[b[1]], b[3], False))
            else:
                out.append((_gathered(prior, prior_jac, _columns(prior)[1]), prior_res, b[3], False))
        wins.append(out)
    s, dg = np.full((len(layout), P), FILL), np.full((len(layout), P), FILL)
    return ctx.reproj_host_parts_build(P, Pw, wins, rebuild=rebuild, host_s=s, host_diag=dg)


def test_build_from_resident_factors_equals_build_from_fetched_ones(ctx):
    pts, qcs = _resident_set(ctx)
    prior = mf.make_prior([7], 42)
    ctx.marg_prior_set(*mf.set_args([prior]))
    x = mf.make_x(prior, 100)
    _partition(ctx, 6)
    layout, Pw, rebuild = _layout(np.random.RandomState(9), prior, "gather")
    rebuilt = [w for w in range(6) if rebuild[w]]
    keep_layout = [[b if b[0] == "ord" else b[:4] + ("keep",) + b[5:] for b in win] for win in layout]
    # first rebuild at point 1: residuals and Jacobians are taken where they are
    ctx.marg_prior_evaluate_resident(x)
    ctx.preint_evaluate_resident(pts[0], qcs[0])
    r1, J1 = ctx.preint_fetch_resident()
    rc, msg, got1, _ = _call(ctx, _arrays(layout, Pw, rebuild), 6)
    assert rc == 0, msg
    # a window alone (the others not rebuilt): the same bits
    only0 = [1, 0, 0, 0, 0, 0]
    rc, msg, alone, _ = _call(ctx, _arrays(layout, Pw, only0), 6)
    assert rc == 0, msg
    _same(alone, got1, [0])
    assert alone[2][1] is None and (alone[0][1:] == FILL).all()
    # second rebuild at point 2, residual only: -1 keeps the Jacobian gathered at point 1
    ctx.preint_evaluate_resident(pts[1], qcs[1], want_jac=False)
    r2, _ = ctx.preint_fetch_resident(want_jac=False)
    rc, msg, got2, _ = _call(ctx, _arrays(keep_layout, Pw, rebuild), 6)
    assert rc == 0, msg
    res, jac = ctx.marg_prior_evaluate(x, want_jac=True)[:2]
    ref1 = _reference(ctx, layout, Pw, rebuild, r1, J1, prior, res, jac)
    ref2 = _reference(ctx, layout, Pw, rebuild, r2, J1, prior, res, jac)
    _same(got1, ref1, rebuilt)
    _same(got2, ref2, rebuilt)
    assert not np.array_equal(bits(r1), bits(r2))
    for w in (0, 1, 2, 5):
        assert np.array_equal(bits(got1[2][w]), bits(got2[2][w])) and not np.array_equal(bits(got1[0][w]), bits(got2[0][w])), w
    assert not got1[2][3].any() and not got1[0][3].any()  # the window without host blocks: a zero part
    for got in (got1, got2):  # the window that is not rebuilt: nothing of it was written
        assert got[2][4] is None and (got[0][4] == FILL).all() and (got[1][4] == FILL).all()
    ctx.prof_enable(True)
    ctx.preint_evaluate_resident(pts[0], qcs[0])
    rc, msg, again, _ = _call(ctx, _arrays(layout, Pw, rebuild), 6)
    assert rc == 0, msg
    _same(again, ref1, rebuilt)  # a gather over a kept layout
    ctx.sync()
    prof = ctx.prof()
    assert prof["host_part_prior"][0] == 1 and prof["host_part"][0] == 1
    ctx.prof_enable(False)


def test_prior_entry_is_the_case_without_preintegration_blocks(ctx):
    prior = mf.make_prior([7], 42)
    ctx.marg_prior_set(*mf.set_args([prior]))
    ctx.marg_prior_evaluate_resident(mf.make_x(prior, 100))
    _partition(ctx, 6)
    layout, Pw, rebuild = _layout(np.random.RandomState(9), prior, "gather")
    layout = [[b for b in win if b[0] != "preint"] for win in layout]
    a = _arrays(layout, Pw, rebuild)
    rebuilt = [w for w in range(6) if rebuild[w]]
    rc, msg, by_prior, _ = _call(ctx, a, 6, entry="prior")
    assert rc == 0, msg
    for over in (dict(preint_of=None, preint_cols=None), dict(preint_cols=None), dict()):
        rc, msg, by_preint, _ = _call(ctx, a, 6, **over)
        assert rc == 0, msg
        _same(by_preint, by_prior, rebuilt)
    assert by_prior[2][2].any()


def test_argument_errors_name_window_and_block_and_launch_nothing(ctx):
    pts, qcs = _resident_set(ctx)
    prior = mf.make_prior([7], 42)
    _partition(ctx, 6)
    layout, Pw, rebuild = _layout(np.random.RandomState(9), prior, "gather")
    good = _arrays(layout, Pw, rebuild)
    ctx.prof_enable(True)

    def refused(text, **over):
        ctx.sync()
        before = ctx.prof()
        rc, msg, (s, dg, _), part = _call(ctx, good, 6, **over)
        assert rc == -1 and text in msg and msg.startswith("icg_reproj_host_parts_build_pre"), (text, rc, msg)
        assert (s == FILL).all() and (dg == FILL).all() and (part == FILL).all(), text
        ctx.sync()
        assert ctx.prof() == before, (text, before, ctx.prof())

    changed = lambda key, idx, val: {key: np.concatenate([good[key][:idx], [val], good[key][idx + 1:]]).astype(good[key].dtype)}
    # no prior set for window 2's prior block is a prior-entry error; here: the preintegration set is there but nothing was evaluated
    refused("window 0, block 0: no preintegration set is resident and evaluated with Jacobians")
    ctx.marg_prior_set(*mf.set_args([prior]))
    ctx.marg_prior_evaluate_resident(mf.make_x(prior, 100))
    ctx.preint_evaluate_resident(pts[0], qcs[0], want_jac=False)
    refused("window 0, block 0: no preintegration set is resident and evaluated with Jacobians")
    ctx.preint_evaluate_resident(pts[0], qcs[0])
    refused("window 0, block 1: factor 6 outside the resident set of 6", **changed("preint_of", 1, 6))
    refused("window 1, block 0: 14 residuals, a preintegration factor has 15", **changed("nr", 2, 14))
    for bad in (32, -1, 6, 22):
        refused(f"window 0, block 0: preintegration column {bad} ", **changed("preint_cols", 3, bad))
    refused("window 2, block 2: both a prior (0) and a preintegration factor (1)", **changed("preint_of", 6, 1))
    refused("window 2, block 0: ICG_HP_JAC_FROM_PREINT for a block that is no preintegration factor", **changed("jac_off", 4, -3))
    refused("a preintegration block without preint_cols", preint_cols=None)
    # -3 without preint_of: the prior entry's own name
    ctx.sync()
    before = ctx.prof()
    rc, msg, _, part = _call(ctx, good, 6, entry="prior")
    assert rc == -1 and msg.startswith("icg_reproj_host_parts_build_prior:") and "ICG_HP_JAC_FROM_PREINT" in msg and (part == FILL).all(), (rc, msg)
    ctx.sync()
    assert ctx.prof() == before
    # a new set invalidates what was evaluated; then the good call goes through
    _resident_set(ctx)
    refused("no preintegration set is resident and evaluated")
    ctx.preint_evaluate_resident(pts[0], qcs[0])
    rc, msg, _, _ = _call(ctx, good, 6)
    assert rc == 0, msg
    ctx.prof_enable(False)
