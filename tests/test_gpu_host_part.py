"""GPU parity of icg_reproj_host_parts_build (csrc/host_part.hip) with its host twin icgh_host_part_from_blocks: the packed part, s and
diag as bit patterns, for a heterogeneous batch in one call, each window alone, the batch reversed and tiled to 300 windows; the kept
Jacobians, the windows a call does not rebuild, the part as icg_reproj_solve_windows reads it, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import host_part_data as hp
import reduced_solve_utils as ru
import reproj_data as rd
from ctypes_util import bits

pytestmark = pytest.mark.gpu

FILL = 7.0  # what the outputs hold before a call: rows a call must not write keep it


@pytest.fixture(scope="module")
def hostlib():
    import harness
    return C.CDLL(harness.HOST_LIB)


@pytest.fixture(scope="module")
def reference(hostlib):
    """the batch and the twin's results for it, computed once: (windows, parts, s, diag)"""
    wins = hp.batch()
    rc, msg, parts, s, dg = hp.twin(hostlib, hp.P_BATCH, wins)
    assert rc == 0, msg
    return wins, parts, s, dg


def partition(ctx, W):
    """a resident partition of W windows (the host parts need nothing else of it): one tiny window of reprojection factors, W times"""
    w = rd.make_window(3, 2, seed=5)
    n, K, L = w["obs_soa"].shape[1], w["poses"].shape[0], len(w["invdepth"])
    ctx.reproj_set_factors(np.tile(w["obs_soa"], (1, W)), np.concatenate([w["idx_i"] + K * k for k in range(W)]),
                           np.concatenate([w["idx_j"] + K * k for k in range(W)]), np.concatenate([w["idx_lm"] + L * k for k in range(W)]))
    ctx.reproj_set_windows(n * np.arange(W + 1), L * np.arange(W + 1))


def build(ctx, P, wins, keep=None, rebuild=None, s=None, dg=None):
    """one icg_reproj_host_parts_build call; keep: set of (window, block) that go up as -1"""
    keep = keep or set()
    blocks = [[(J, r, cols, (w, b) in keep) for b, (J, r, cols) in enumerate(win["blocks"])] for w, win in enumerate(wins)]
    W = len(wins)
    s = np.full((W, P), FILL) if s is None else s
    dg = np.full((W, P), FILL) if dg is None else dg
    return ctx.reproj_host_parts_build(P, [win["Pw"] for win in wins], blocks, rebuild=rebuild, host_s=s, host_diag=dg)


def same(got, parts, s, dg, order):
    gs, gd, gp = got
    for k, w in enumerate(order):
        assert np.array_equal(bits(gp[k]), bits(parts[w])), ("part", k, w)
        assert np.array_equal(bits(gs[k]), bits(s[w])) and np.array_equal(bits(gd[k]), bits(dg[w])), ("s / diag", k, w)


@pytest.fixture()
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


def test_batch_in_one_call_reversed_and_alone(ctx, reference):
    wins, parts, s, dg = reference
    W, P = len(wins), hp.P_BATCH
    partition(ctx, W)
    same(build(ctx, P, wins), parts, s, dg, range(W))
    same(build(ctx, P, wins), parts, s, dg, range(W))  # run after run (and in place: the kept layout did not change)
    rev = list(range(W))[::-1]
    same(build(ctx, P, [wins[w] for w in rev]), parts, s, dg, rev)
    assert bits(parts[3])[1] == 0 and bits(s[3])[0] == 0  # the -0.0 window: the reference itself holds +0.0
    partition(ctx, 1)
    for w in range(W):
        same(build(ctx, P, [wins[w]]), parts, s, dg, [w])


def test_batch_tiled_to_300_windows(ctx, reference):
    wins, parts, s, dg = reference
    order = [k % len(wins) for k in range(300)]
    partition(ctx, 300)
    same(build(ctx, hp.P_BATCH, [wins[w] for w in order]), parts, s, dg, order)


def test_one_column_and_nan(ctx, hostlib):
    partition(ctx, 1)
    one = [dict(Pw=1, blocks=[(np.array([[3.0]]), np.array([-2.0]), np.array([0], np.int32))])]
    rc, msg, parts, s, dg = hp.twin(hostlib, 1, one)
    assert rc == 0 and parts[0][0] == 9.0 and s[0, 0] == 6.0 and dg[0, 0] == 9.0, msg
    same(build(ctx, 1, one), parts, s, dg, [0])
    # a NaN in J: the same cells are NaN (the payload is not compared)
    rng = np.random.RandomState(3)
    J = rng.normal(0, 1, (4, 3))
    J[2, 1] = np.nan
    bad = [dict(Pw=6, blocks=[(J, rng.normal(0, 1, 4), np.array([4, 0, 2], np.int32)), (rng.normal(0, 1, (2, 2)), rng.normal(0, 1, 2), np.array([1, 0], np.int32))])]
    rc, msg, parts, s, dg = hp.twin(hostlib, 6, bad)
    assert rc == 0, msg
    gs, gd, gp = build(ctx, 6, bad)
    for got, ref in ((gp[0], parts[0]), (gs[0], s[0]), (gd[0], dg[0])):
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).any()
        ok = ~np.isnan(ref)
        assert np.array_equal(bits(got[ok]), bits(ref[ok]))


def _keep_windows(rng, Pw):
    mk = lambda nr, cols, scale: (rng.normal(0, scale, (nr, len(cols))), rng.normal(0, 1.0, nr), np.asarray(cols, np.int32))
    return [dict(Pw=int(Pw[0]), blocks=[mk(20, range(3, 23), 20.0), mk(6, range(0, 6), 30.0), mk(int(Pw[0]), range(int(Pw[0])), 5.0)]),
            dict(Pw=int(Pw[1]), blocks=[mk(int(Pw[1]), rng.permutation(int(Pw[1])), 40.0), mk(9, range(6, 15), 10.0)])]


def test_kept_jacobians_untouched_windows_and_the_solve(hostlib):
    import icgvins
    import test_gpu_chol_solve as tcs
    g = tcs._two_windows()
    P, Pw, W, n_lm = g["P"], g["Pw"], 2, len(g["inv"])
    rng = np.random.RandomState(17)
    ctx = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    ctx.reproj_set_factors(g["obs"], g["ii"], g["jj"], g["ll"])
    ctx.reproj_set_windows(g["fac_off"], g["lm_off"])
    ctx.reproj_eval_windows(g["poses"], g["ext"], g["inv"], g["td"], huber=1.0)
    damp = np.array([1e-4, 1e-3])
    S, s_vis, dg_vis, _ = ctx.reproj_schur_windows_view(P, g["col_pose"], g["col_ext"], g["col_td"], damp=damp)
    first = _keep_windows(rng, Pw)
    # second call: new residuals everywhere, a new Jacobian for block 1 of window 0 only
    second = [dict(Pw=w["Pw"], blocks=[(J, rng.normal(0, 1.0, len(r)), cols) for J, r, cols in w["blocks"]]) for w in first]
    J01 = rng.normal(0, 30.0, second[0]["blocks"][1][0].shape)
    second[0]["blocks"][1] = (J01, second[0]["blocks"][1][1], second[0]["blocks"][1][2])
    # third call: window 1 alone, with another first block
    third = [second[0], dict(Pw=second[1]["Pw"], blocks=[(rng.normal(0, 40.0, second[1]["blocks"][0][0].shape),) + second[1]["blocks"][0][1:], second[1]["blocks"][1]])]
    ref = {}
    for name, wins in (("first", first), ("second", second), ("third", third)):
        rc, msg, parts, s, dg = hp.twin(hostlib, P, wins)
        assert rc == 0, msg
        ref[name] = (parts, s, dg)
    # the solve the device must reproduce: window 0 with the part of the second call, window 1 with the part of the third
    final = [ref["second"][0][0], ref["third"][0][1]]
    dd = np.zeros((W, P))
    rhs = s_vis + np.stack([ref["second"][1][0], ref["third"][1][1]])
    systems = []
    for w in range(W):
        n = Pw[w]
        dd[w, :n] = np.minimum(np.maximum(dg_vis[w, :n] + [ref["second"][2], ref["third"][2]][w][w, :n], 1e-6), 1e32) / 1e4
        A, at = np.zeros((n, n)), 0
        for i in range(n):
            A[i, :i + 1] = S[w, i, :i + 1] + final[w][at:at + i + 1]
            at += i + 1
        A[np.arange(n), np.arange(n)] += dd[w, :n]
        systems.append((A, rhs[w, :n]))
    solved = ru.device_cholesky(ctx, systems)
    assert all(st == 0 for _, _, st in solved)
    # as the solver does it: the resident reduction first, then the parts
    ctx.reproj_schur_windows_resident(P, g["col_pose"], g["col_ext"], g["col_td"], damp=damp)
    with pytest.raises(icgvins.IcgError, match=r"rc=-1: .*window 0, block 0: no kept Jacobian"):
        build(ctx, P, first, keep={(0, 0)})
    same(build(ctx, P, first), *ref["first"], range(W))
    # (old J, new r) for the kept blocks: they are given here with a Jacobian of the right shape that must not be read
    sent = [dict(Pw=w["Pw"], blocks=list(w["blocks"])) for w in second]
    keep = {(0, 0), (0, 2), (1, 0), (1, 1)}
    for w, b in keep:
        J, r, cols = sent[w]["blocks"][b]
        sent[w]["blocks"][b] = (np.full(J.shape, np.nan), r, cols)
    same(build(ctx, P, sent, keep=keep), *ref["second"], range(W))
    # window 0 is not rebuilt: its rows of s and diag keep what they held, part_out carries window 1 only, and its kept Jacobian is used
    s3, dg3 = np.full((W, P), FILL), np.full((W, P), FILL)
    sent3 = [third[0], dict(Pw=third[1]["Pw"], blocks=[third[1]["blocks"][0], (np.full(third[1]["blocks"][1][0].shape, np.nan),) + third[1]["blocks"][1][1:]])]
    gs, gd, gp = build(ctx, P, sent3, keep={(1, 1)}, rebuild=[0, 1], s=s3, dg=dg3)
    assert gp[0] is None and (gs[0] == FILL).all() and (gd[0] == FILL).all()
    parts3, sr3, dr3 = ref["third"]
    assert np.array_equal(bits(gp[1]), bits(parts3[1])) and np.array_equal(bits(gs[1]), bits(sr3[1])) and np.array_equal(bits(gd[1]), bits(dr3[1]))
    # both resident parts as icg_reproj_solve_windows reads them: window 0's survived the third call
    dc, st, _, _ = ctx.reproj_solve_windows(P, Pw, [1, 1], dd, rhs, n_lm)
    assert not st.any()
    for w in range(W):
        assert np.array_equal(bits(dc[w, :Pw[w]]), bits(solved[w][0])), w
        assert not dc[w, Pw[w]:].any()
    # a kept Jacobian of another shape, and a block count that differs from the kept one
    wrong = [sent3[0], dict(Pw=sent3[1]["Pw"], blocks=[sent3[1]["blocks"][0], (np.zeros((8, 9)),) + (np.zeros(8), sent3[1]["blocks"][1][2])])]
    with pytest.raises(icgvins.IcgError, match=r"rc=-1: .*window 1, block 1: the kept Jacobian is 9 x 9, not 8 x 9"):
        build(ctx, P, wrong, keep={(1, 1)}, rebuild=[0, 1])
    fewer = [sent3[0], dict(Pw=sent3[1]["Pw"], blocks=[sent3[1]["blocks"][0]])]
    with pytest.raises(icgvins.IcgError, match=r"rc=-1: .*window 1: 1 blocks, 2 kept"):
        build(ctx, P, fewer, keep={(1, 0)}, rebuild=[0, 1])
    # P is the resident reduced systems' P
    with pytest.raises(icgvins.IcgError, match=r"rc=-1: .*P = 44, the resident reduced systems have 43"):
        build(ctx, P + 1, third)
    # and nothing of that changed what is resident
    dc2, _, _, _ = ctx.reproj_solve_windows(P, Pw, [1, 1], dd, rhs, n_lm)
    assert np.array_equal(bits(dc2), bits(dc))
    ctx.close()


def test_argument_errors(ctx, hostlib):
    import icgvins
    rng = np.random.RandomState(23)
    mk = lambda nr, cols: (rng.normal(0, 1, (nr, len(cols))), rng.normal(0, 1, nr), np.asarray(cols, np.int32))
    good = [dict(Pw=8, blocks=[mk(3, [1, 5, 2])]), dict(Pw=6, blocks=[mk(2, [0, 3]), mk(4, [5, 4, 3, 2])])]
    P = 8
    f = hp.flat(P, good)
    s, dg, part = np.full((2, P), FILL), np.full((2, P), FILL), np.full(sum(f["cells"]), FILL)
    rb = np.ones(2, np.uint8)

    def call(**over):
        a = dict(f, rebuild=rb, s=s, dg=dg, part=part)
        a.update(over)
        rc = ctx.reproj_host_parts_build_raw(a["P"], a["Pw"], a["rebuild"], a["blk_off"], a["nr"], a["nf"], a["cols"], a["jac_off"], a["J"], a["r"], a["s"], a["dg"],
                                             a["part"])
        return rc, ctx.lib.icg_last_error(ctx.h).decode()

    def untouched():
        return (s == FILL).all() and (dg == FILL).all() and (part == FILL).all()

    rc, msg = call()
    assert rc == -1 and "no window partition" in msg and untouched(), (rc, msg)
    partition(ctx, 2)
    changed = lambda key, idx, val: {key: np.concatenate([f[key][:idx], [val], f[key][idx + 1:]]).astype(f[key].dtype)}
    cases = [(dict(Pw=None), -1, "NULL"), (dict(s=None), -1, "NULL"), (dict(r=None), -1, "NULL"), (dict(J=None), -1, "window 0, block 0"),
             (changed("Pw", 1, 0), -1, "window 1: Pw = 0"), (changed("Pw", 1, 9), -1, "window 1: Pw = 9"), (changed("nr", 1, 0), -1, "window 1, block 0"),
             (changed("nf", 2, -1), -1, "window 1, block 1"), (changed("cols", 4, 6), -1, "window 1, block 0: column 6 outside"),
             (changed("cols", 4, -1), -1, "window 1, block 0: column -1 outside"), (changed("cols", 6, 5), -1, "window 1, block 1: column 5 twice"),
             (changed("jac_off", 2, -1), -1, "window 1, block 1: no kept Jacobian"), (changed("jac_off", 0, -2), -1, "window 0, block 0: jac_off = -2"),
             (dict(P=513), -5, "512"), (changed("nr", 2, icgvins.HOST_PART_MAX_NR + 1), -5, "window 1, block 1: 1025 residuals")]
    for over, code, text in cases:
        rc, msg = call(**over)
        assert rc == code and text in msg and untouched(), (over.keys(), rc, msg)
    # the next valid call gives the right bits
    rc, msg = call()
    assert rc == 0, msg
    rc, msg, parts, sr, dr = hp.twin(hostlib, P, good)
    assert rc == 0, msg
    assert np.array_equal(bits(part), bits(np.concatenate(parts))) and np.array_equal(bits(s), bits(sr)) and np.array_equal(bits(dg), bits(dr))
