"""GPU: the resident ODOMETER preintegration factors as the host-part kernel reads them.  icg_reproj_host_parts_build_preint_odo (residuals
and Jacobians taken from the resident odometer P2 set on the device, row stride 34) gives the part, s and diag icg_reproj_host_parts_build
gives on the same context when it is fed the fetched residuals and the numpy-gathered columns of the fetched Jacobians; a later rebuild with
-1 keeps the gathered Jacobian; a window may hold a 15-state resident factor, an odometer one and a resident prior at once; the three older
entries are the new one with NULL for its arguments and give the bits they gave; the argument errors name window and block, launch nothing
and touch no output.  Bit patterns throughout.

The sets are built from the device's own integration results and square-root information with arbitrary unit quaternions in place of the
host's: what is compared here is the gather, not the evaluation (tests/test_gpu_preint_odo_resident.py holds that to the host's bits)."""
import numpy as np
import pytest

import marg_factor_data as mf
import preint_odo_data as od
import preint_odo_split_data as sd
from test_gpu_host_part_preint import ALL as ALL15
from test_gpu_host_part_preint import _j32, _resident_set as _resident_set15, _unit
from test_gpu_marg_prior_resident import _columns, _gathered, _partition
from ctypes_util import bits, i32

pytestmark = pytest.mark.gpu

FILL = 7.0
P = 64
ALL = np.array(list(range(0, 6)) + list(range(7, 17)) + list(range(17, 23)) + list(range(24, 34)), np.int32)  # all four blocks free: 32 columns
SECOND = ALL[16:]  # the first state constant
CODE = {"prior": -2, "preint": -3, "odo": -4}


@pytest.fixture()
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


def _resident_set(ctx):
    """six odometer factors (O E O E E O) of 21-sample intervals resident -> the two evaluations' (points, correction quaternions)"""
    n = 6
    variants = [2, 3, 2, 3, 3, 2]
    imus = [od._imu9(21, 80 + i) for i in range(n)]
    states = [od.state17(p=(i, 1, 0), v=(2, 0.1 * i, 0)) for i in range(n)]
    par25 = od.params25()
    off = (np.arange(n + 1) * 21).astype(np.int32)
    cur, delta, jac, cov, dt, pn = ctx.preint_odo_batch(3, off, np.concatenate(imus), np.stack(states), par25)
    pn_rows = pn.reshape(n, 21, 4)[:, :20].reshape(-1, 4)
    pn_off = (np.arange(n + 1) * 20).astype(np.int32)
    env = np.tile(par25[5:9], (n, 1))
    pts = [np.stack([sd.eval_point(kind, delta[i], cur[i], states[i]) for i in range(n)]) for kind in ("perturbed", "large_bias_step")]
    _, _, S, status = ctx.preint_odo_evaluate_batch(3, delta, jac, cov, dt, env, pts[0], pn_off, pn_rows)
    assert np.all(status == 0)
    rng = np.random.RandomState(4)
    ctx.preint_odo_set(variants, delta, jac, S, dt, env, _unit(rng, n, 1e-5), pn_off, pn_rows)
    return pts, [_unit(rng, n, 1e-3), _unit(rng, n, 3e-2)]


def _j34(J646):
    return np.concatenate([J646[0:133].reshape(19, 7), J646[133:323].reshape(19, 10), J646[323:456].reshape(19, 7), J646[456:646].reshape(19, 10)], axis=1)


def _arrays(layout, Pw, rebuild):
    """the raw arguments of icg_reproj_host_parts_build_preint_odo.  A block is ("ord", J, r, cols), or (family, member, member_cols, cols, how
    [, nr]) with family "prior" / "preint" / "odo" and how = "gather" / "keep"; the resident blocks' slots in r are NaN"""
    blocks = [b for win in layout for b in win]
    a = dict(Pw=i32(Pw), rebuild=np.ascontiguousarray(rebuild, np.uint8), blk_off=i32(np.concatenate([[0], np.cumsum([len(w) for w in layout])])))
    nr, nf, cols, r, jac_off, Js, at = [], [], [], [], [], [], 0
    of = {f: [] for f in CODE}
    fc = {f: [] for f in CODE}
    for b in blocks:
        for f in CODE:
            of[f].append(b[1] if b[0] == f else -1)
        if b[0] == "ord":
            nr.append(b[1].shape[0]), nf.append(b[1].shape[1]), cols.append(b[3]), r.append(b[2])
            jac_off.append(at), Js.append(b[1].ravel())
            at += b[1].size
        else:
            nr.append(b[5] if b[0] == "prior" else 15 if b[0] == "preint" else 19), nf.append(len(b[3])), cols.append(b[3]), r.append(np.full(nr[-1], np.nan))
            fc[b[0]].append(b[2])
            jac_off.append(-1 if b[4] == "keep" else CODE[b[0]])
    cat = lambda xs, t: np.ascontiguousarray(np.concatenate(xs), t) if xs else None
    a.update(nr=i32(nr), nf=i32(nf), cols=cat(cols, np.int32), r=cat(r, np.float64), jac_off=np.ascontiguousarray(jac_off, np.int64), J=cat(Js, np.float64),
             prior_of=i32(of["prior"]), preint_of=i32(of["preint"]), odo_of=i32(of["odo"]), prior_cols=cat(fc["prior"], np.int32),
             preint_cols=cat(fc["preint"], np.int32), odo_cols=cat(fc["odo"], np.int32))
    return a


def _call(ctx, a, W, entry="odo", **over):
    a = dict(a)
    a.update(over)
    sizes = [int(a["Pw"][w]) * (int(a["Pw"][w]) + 1) // 2 if a["rebuild"][w] else 0 for w in range(W)]
    s, dg, part = np.full((W, P), FILL), np.full((W, P), FILL), np.full(max(1, sum(sizes)), FILL)
    lead = (P, a["Pw"], a["rebuild"], a["blk_off"], a["nr"], a["nf"], a["cols"], a["jac_off"], a["J"], a["r"], s, dg, part)
    if entry == "odo":
        rc = ctx.reproj_host_parts_build_preint_odo_raw(*lead, a["prior_of"], a["prior_cols"], a["preint_of"], a["preint_cols"], a["odo_of"], a["odo_cols"])
    elif entry == "preint":
        rc = ctx.reproj_host_parts_build_preint_raw(*lead, a["prior_of"], a["prior_cols"], a["preint_of"], a["preint_cols"])
    elif entry == "prior":
        rc = ctx.reproj_host_parts_build_prior_raw(*lead, a["prior_of"], a["prior_cols"])
    else:
        rc = ctx.reproj_host_parts_build_raw(*lead)
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
    layout = [[("odo", 3, ALL, np.arange(0, 32), how), ("odo", 1, ALL, np.arange(16, 48), how)],  # two factors sharing the middle state's columns
              [("odo", 0, SECOND, np.arange(0, 16), how), mk(9, range(6, 15), 10.0)],  # the first state constant: nf = 16
              [mk(6, range(0, 6), 30.0), ("odo", 4, ALL, 3 + rng.permutation(32), how), ("prior", 0, pc, np.arange(36, 42), how, prior["r"])],
              [],  # rebuilt, no host block
              [mk(3, [1, 5, 2]), ("odo", 5, ALL, np.arange(32), how)],  # not rebuilt: its block only places the others' columns
              [("preint", 2, ALL15, rng.permutation(30), how), ("odo", 2, ALL, 30 + rng.permutation(32), how)]]  # a 15-state and an odometer factor
    return layout, [48, 20, 42, 10, 32, 62], [1, 1, 1, 1, 0, 1]


def _reference(ctx, layout, Pw, rebuild, odo, fifteen, prior, prior_res, prior_jac):
    """icg_reproj_host_parts_build fed what the resident blocks hold: the fetched residuals and the numpy-gathered columns"""
    wins = []
    for win in layout:
        out = []
        for b in win:
            if b[0] == "ord":
                out.append((b[1], b[2], b[3], False))
            elif b[0] == "odo":
                out.append((np.ascontiguousarray(_j34(odo[1][b[1]])[:, b[2]]), odo[0][b[1]], b[3], False))
            elif b[0] == "preint":
                out.append((np.ascontiguousarray(_j32(fifteen[1][b[1]])[:, b[2]]), fifteen[0][b[1]], b[3], False))
            else:
                out.append((_gathered(prior, prior_jac, _columns(prior)[1]), prior_res, b[3], False))
        wins.append(out)
    s, dg = np.full((len(layout), P), FILL), np.full((len(layout), P), FILL)
    return ctx.reproj_host_parts_build(P, Pw, wins, rebuild=rebuild, host_s=s, host_diag=dg)


def _everything_resident(ctx):
    """the odometer set, a 15-state set and a prior set resident in one context, all evaluated at their first point"""
    pts, qcs = _resident_set(ctx)
    pts15, qcs15 = _resident_set15(ctx)
    prior = mf.make_prior([7], 42)
    ctx.marg_prior_set(*mf.set_args([prior]))
    x = mf.make_x(prior, 100)
    ctx.marg_prior_evaluate_resident(x)
    ctx.preint_evaluate_resident(pts15[0], qcs15[0])
    ctx.preint_odo_evaluate_resident(pts[0], qcs[0])
    return pts, qcs, prior, x


def test_build_from_resident_factors_equals_build_from_fetched_ones(ctx):
    pts, qcs, prior, x = _everything_resident(ctx)
    _partition(ctx, 6)
    layout, Pw, rebuild = _layout(np.random.RandomState(9), prior, "gather")
    rebuilt = [w for w in range(6) if rebuild[w]]
    keep_layout = [[b if b[0] == "ord" else b[:4] + ("keep",) + b[5:] for b in win] for win in layout]
    fifteen = ctx.preint_fetch_resident()
    r1, J1 = ctx.preint_odo_fetch_resident()
    # first rebuild at point 1: residuals and Jacobians are taken where they are
    rc, msg, got1, _ = _call(ctx, _arrays(layout, Pw, rebuild), 6)
    assert rc == 0, msg
    # a window alone (the others not rebuilt): the same bits
    rc, msg, alone, _ = _call(ctx, _arrays(layout, Pw, [1, 0, 0, 0, 0, 0]), 6)
    assert rc == 0, msg
    _same(alone, got1, [0])
    assert alone[2][1] is None and (alone[0][1:] == FILL).all()
    # second rebuild at point 2, residual only: -1 keeps the Jacobian gathered at point 1
    ctx.preint_odo_evaluate_resident(pts[1], qcs[1], want_jac=False)
    r2, _ = ctx.preint_odo_fetch_resident(want_jac=False)
    rc, msg, got2, _ = _call(ctx, _arrays(keep_layout, Pw, rebuild), 6)
    assert rc == 0, msg
    res, jac = ctx.marg_prior_evaluate(x, want_jac=True)[:2]
    ref1 = _reference(ctx, layout, Pw, rebuild, (r1, J1), fifteen, prior, res, jac)
    ref2 = _reference(ctx, layout, Pw, rebuild, (r2, J1), fifteen, prior, res, jac)
    _same(got1, ref1, rebuilt)
    _same(got2, ref2, rebuilt)
    assert not np.array_equal(bits(r1), bits(r2))
    for w in (0, 1, 2, 5):
        assert np.array_equal(bits(got1[2][w]), bits(got2[2][w])) and not np.array_equal(bits(got1[0][w]), bits(got2[0][w])), w
        assert got1[2][w].any()
    assert not got1[2][3].any() and not got1[0][3].any()  # the window without host blocks: a zero part
    for got in (got1, got2):  # the window that is not rebuilt: nothing of it was written
        assert got[2][4] is None and (got[0][4] == FILL).all() and (got[1][4] == FILL).all()
    ctx.prof_enable(True)
    ctx.preint_odo_evaluate_resident(pts[0], qcs[0])
    rc, msg, again, _ = _call(ctx, _arrays(layout, Pw, rebuild), 6)
    assert rc == 0, msg
    _same(again, ref1, rebuilt)  # a gather over a kept layout
    ctx.sync()
    prof = ctx.prof()
    assert prof["host_part_prior"][0] == 1 and prof["host_part"][0] == 1  # no new accumulation kernel: the two launches of the older entries
    ctx.prof_enable(False)


def test_the_older_entries_are_the_new_one_without_its_arguments(ctx):
    """the 15-state test's own input (priors and 15-state factors, no odometer block) through every entry that takes it"""
    import test_gpu_host_part_preint as t15
    pts15, qcs15 = _resident_set15(ctx)
    prior = mf.make_prior([7], 42)
    ctx.marg_prior_set(*mf.set_args([prior]))
    x = mf.make_x(prior, 100)
    ctx.marg_prior_evaluate_resident(x)
    ctx.preint_evaluate_resident(pts15[0], qcs15[0])
    r15, J15 = ctx.preint_fetch_resident()
    _partition(ctx, 6)
    layout, Pw, rebuild = t15._layout(np.random.RandomState(9), prior, "gather")
    rebuilt = [w for w in range(6) if rebuild[w]]
    a = _arrays(layout, Pw, rebuild)
    assert a["odo_cols"] is None and (a["odo_of"] < 0).all()
    res, jac = ctx.marg_prior_evaluate(x, want_jac=True)[:2]
    ref = _reference(ctx, layout, Pw, rebuild, None, (r15, J15), prior, res, jac)  # icg_reproj_host_parts_build on fetched values
    assert ref[2][0].any() and ref[2][2].any()
    rc, msg, old, _ = _call(ctx, a, 6, entry="preint")
    assert rc == 0, msg
    _same(old, ref, rebuilt)
    for over in (dict(), dict(odo_of=None), dict(odo_of=None, odo_cols=None)):
        rc, msg, new, _ = _call(ctx, a, 6, **over)
        assert rc == 0, msg
        _same(new, ref, rebuilt)
    # the prior entry and the plain entry on the blocks they take
    no_factors = [[b for b in win if b[0] != "preint"] for win in layout]
    b = _arrays(no_factors, Pw, rebuild)
    rc, msg, by_prior, _ = _call(ctx, b, 6, entry="prior")
    assert rc == 0, msg
    rc, msg, by_new, _ = _call(ctx, b, 6, preint_of=None, preint_cols=None, odo_of=None)
    assert rc == 0, msg
    _same(by_new, by_prior, rebuilt)
    plain = [[blk for blk in win if blk[0] == "ord"] for win in layout]
    c = _arrays(plain, Pw, rebuild)
    rc, msg, by_plain, _ = _call(ctx, c, 6, entry="plain")
    assert rc == 0, msg
    rc, msg, by_new, _ = _call(ctx, c, 6, prior_of=None, preint_of=None, odo_of=None)
    assert rc == 0, msg
    _same(by_new, by_plain, rebuilt)
    assert by_plain[2][1].any()


def test_argument_errors_name_window_and_block_and_launch_nothing(ctx):
    pts, qcs = _resident_set(ctx)
    pts15, qcs15 = _resident_set15(ctx)
    prior = mf.make_prior([7], 42)
    ctx.marg_prior_set(*mf.set_args([prior]))
    ctx.marg_prior_evaluate_resident(mf.make_x(prior, 100))
    ctx.preint_evaluate_resident(pts15[0], qcs15[0])
    _partition(ctx, 6)
    layout, Pw, rebuild = _layout(np.random.RandomState(9), prior, "gather")
    good = _arrays(layout, Pw, rebuild)
    ctx.prof_enable(True)

    def refused(text, entry="odo", **over):
        ctx.sync()
        before = ctx.prof()
        rc, msg, (s, dg, _), part = _call(ctx, good, 6, entry=entry, **over)
        assert rc == -1 and text in msg and msg.startswith("icg_reproj_host_parts_build_pre"), (text, rc, msg)
        assert (s == FILL).all() and (dg == FILL).all() and (part == FILL).all(), text
        ctx.sync()
        assert ctx.prof() == before, (text, before, ctx.prof())
        return msg

    changed = lambda key, idx, val: {key: np.concatenate([good[key][:idx], [val], good[key][idx + 1:]]).astype(good[key].dtype)}
    # blocks of the call: 0, 1 | 2, 3 | 4, 5, 6 | | 7, 8 | 9, 10.  The odometer set is there but nothing was evaluated
    refused("window 0, block 0: no odometer preintegration set is resident and evaluated with Jacobians")
    ctx.preint_odo_evaluate_resident(pts[0], qcs[0], want_jac=False)
    refused("window 0, block 0: no odometer preintegration set is resident and evaluated with Jacobians")
    ctx.preint_odo_evaluate_resident(pts[0], qcs[0])
    msg = refused("window 0, block 1: factor 6 outside the resident odometer set of 6", **changed("odo_of", 1, 6))
    assert msg.startswith("icg_reproj_host_parts_build_preint_odo:")
    refused("window 1, block 0: 18 residuals, an odometer preintegration factor has 19", **changed("nr", 2, 18))
    for bad in (34, -1, 6, 23):
        refused(f"window 0, block 0: odometer preintegration column {bad} ", **changed("odo_cols", 3, bad))
    refused("window 2, block 2: both a prior (0) and an odometer preintegration factor (1)", **changed("odo_of", 6, 1))
    refused("window 5, block 0: both a preintegration factor (2) and an odometer preintegration factor (0)", **changed("odo_of", 9, 0))
    refused("window 2, block 2: both a prior (0) and a preintegration factor (1)", **changed("preint_of", 6, 1))
    refused("window 2, block 0: ICG_HP_JAC_FROM_PREINT_ODO for a block that is no odometer preintegration factor", **changed("jac_off", 4, -4))
    refused("window 2, block 2: ICG_HP_JAC_FROM_PREINT_ODO for a block that is no odometer preintegration factor", **changed("jac_off", 6, -4))
    refused("window 0, block 0: ICG_HP_JAC_FROM_PREINT for a block that is no preintegration factor", **changed("jac_off", 0, -3))
    refused("an odometer preintegration block without preint_odo_cols", odo_cols=None)
    # -4 without preint_odo_of: the older entry's own name
    msg = refused("ICG_HP_JAC_FROM_PREINT_ODO", entry="preint")
    assert msg.startswith("icg_reproj_host_parts_build_preint:")
    # a new set invalidates what was evaluated; a failed set leaves none; then the good call goes through
    _resident_set(ctx)
    refused("no odometer preintegration set is resident and evaluated")
    assert ctx.lib.icg_preint_odo_set(ctx.h, 0, None, None, None, None, None, None, None, None, None) == -1
    refused("no odometer preintegration set is resident and evaluated")
    _resident_set(ctx)
    ctx.preint_odo_evaluate_resident(pts[0], qcs[0])
    rc, msg, _, _ = _call(ctx, good, 6)
    assert rc == 0, msg
    ctx.prof_enable(False)
