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
import host_part_family_utils as hp
from host_part_family_utils import FILL, _partition
from host_part_family_utils import arrays as _arrays, layout15 as _layout, resident_set15 as _resident_set, same as _same
from ctypes_util import bits

pytestmark = pytest.mark.gpu

P = 48


@pytest.fixture()
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


def _call(ctx, a, W, entry="preint", **over):
    return hp.call(ctx, a, W, entry, P=P, **over)


def _reference(ctx, layout, Pw, rebuild, r_fetch, J_fetch, prior, prior_res, prior_jac):
    return hp.reference(ctx, layout, Pw, rebuild, hp.sources(prior, prior_res, prior_jac, fifteen=(r_fetch, J_fetch)), P=P)


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
