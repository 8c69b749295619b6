"""GPU: icg_marg_linearize_resident (csrc/marg_linearize.hip) forms the reduced systems of the selected windows on the device from their
resident halves (the packed host-factor part of icg_reproj_host_parts_build, the lower triangle of S of icg_reproj_schur_windows_resident)
and linearizes them with the kernels of icg_marg_linearize_batch.  The reference: S from icg_reproj_schur_windows_view, the parts from
part_out, H_ref = mirror(part + S) in numpy, every other output from icg_marg_linearize_batch(H_ref, b).  Every comparison is on float64
bit patterns: no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

import marg_factor_data as mf
import reproj_data as rd
from ctypes_util import bits, ptr

pytestmark = pytest.mark.gpu

# (landmarks, keyframes, free poses (the last ones), extrinsic free, td free) -> Pw = 6 free + 6 ext + td:
# 1 (td alone), 7, 31 and 37 (either side of the 32-wide tile edge), 43, 67, and 24 poses with a handful of landmarks: 151 columns, whose
# r = 145 working matrix does not fit in LDS (the global-scratch instantiation).  P = 151 is common: every narrower window has stride != width.
SPEC = [(8, 3, 0, False, True), (8, 3, 1, False, True), (10, 6, 5, False, True), (10, 6, 6, False, True), (14, 6, 6, True, True),
        (20, 10, 10, True, True), (6, 24, 24, True, True)]
PW = [1, 7, 31, 37, 43, 67, 151]
P = 151
NO_PART = 3  # this window never receives a host part: +0.0 + S
WIDE = 6     # the 151-column window: m = 6 only (about 40 ms a run)
OUT_KEYS = ("J0", "e0", "Hp", "bp", "evals", "min_ev_m", "status")


def _group():
    """the windows of SPEC as one partition (the layout of test_gpu_chol_solve._two_windows for any number of windows)"""
    wins = [rd.make_window(L, K, seed=60 + k, pixel_noise=1.0) for k, (L, K, _, _, _) in enumerate(SPEC)]
    pose_off = np.concatenate([[0], np.cumsum([w["poses"].shape[0] for w in wins])])
    lm_off = np.concatenate([[0], np.cumsum([len(w["invdepth"]) for w in wins])]).astype(np.int32)
    fac_off = np.concatenate([[0], np.cumsum([w["obs_soa"].shape[1] for w in wins])]).astype(np.int32)
    g = dict(obs=np.concatenate([w["obs_soa"] for w in wins], axis=1),
             ii=np.concatenate([w["idx_i"] + pose_off[k] for k, w in enumerate(wins)]).astype(np.int32),
             jj=np.concatenate([w["idx_j"] + pose_off[k] for k, w in enumerate(wins)]).astype(np.int32),
             ll=np.concatenate([w["idx_lm"] + lm_off[k] for k, w in enumerate(wins)]).astype(np.int32),
             poses=np.concatenate([w["poses"] for w in wins]), ext=np.stack([w["ext"] for w in wins]),
             inv=np.concatenate([w["invdepth"] for w in wins]), td=np.array([w["td"] for w in wins]), fac_off=fac_off, lm_off=lm_off)
    col_pose, col_ext, col_td, Pw = [], [], [], []
    for L, K, free, ext, td in SPEC:
        col_pose += [-1] * (K - free) + [6 * k for k in range(free)]
        c = 6 * free
        col_ext.append(c if ext else -1)
        c += 6 if ext else 0
        col_td.append(c if td else -1)
        Pw.append(c + (1 if td else 0))
    assert Pw == PW
    g.update(col_pose=np.array(col_pose, np.int32), col_ext=np.array(col_ext, np.int32), col_td=np.array(col_td, np.int32), Pw=np.array(Pw, np.int32))
    return g


def _blocks():
    """seeded host-factor blocks per window (J nr x nf, r, cols, keep = False): columns out of order, blocks that overlap, a block of
    magnitude 1e8 beside one of 1e-8 (window 2), a block over every column (the dense prior's shape), none for NO_PART"""
    rng = np.random.RandomState(77)
    out = []
    for w, n in enumerate(PW):
        blocks = []
        if w != NO_PART:
            shapes = [(min(n, 15), min(n, 15)), (n, n), (3, min(n, 9)), (min(n, 6), min(n, 6))]
            for k, (nr, nf) in enumerate(shapes):
                scale = 30.0
                if w == 2 and k == 2:
                    scale = 1e8
                if w == 2 and k == 3:
                    scale = 1e-8
                cols = rng.permutation(n)[:nf].astype(np.int32)
                blocks.append((rng.normal(0, scale, (nr, nf)), rng.normal(0, 1.0, nr), cols, False))
        out.append(blocks)
    return out


def _ctx():
    import icgvins
    return icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)


def _resident(c, g):
    """the partition evaluated, its reduced systems and host parts resident -> (S of the view form, parts)"""
    W = len(SPEC)
    c.reproj_set_factors(g["obs"], g["ii"], g["jj"], g["ll"])
    c.reproj_set_windows(g["fac_off"], g["lm_off"])
    c.reproj_eval_windows(g["poses"], g["ext"], g["inv"], g["td"], huber=1.0)
    args = (P, g["col_pose"], g["col_ext"], g["col_td"])
    S, s, dg, _ = c.reproj_schur_windows_view(*args, damp=np.zeros(W), min_diag=0.0, max_diag=0.0)
    s_r, dg_r, _ = c.reproj_schur_windows_resident(*args, damp=np.zeros(W), min_diag=0.0, max_diag=0.0)
    assert np.array_equal(bits(s_r), bits(s))
    rebuild = np.array([w != NO_PART for w in range(W)], np.uint8)
    _, _, parts = c.reproj_host_parts_build(P, g["Pw"], _blocks(), rebuild=rebuild)
    return S, parts


@pytest.fixture(scope="module")
def world():
    """one context with everything resident, the numpy reference of every window's H, seeded right-hand sides"""
    c = _ctx()
    g = _group()
    S, parts = _resident(c, g)
    H_ref = []
    for w, n in enumerate(PW):
        H = np.zeros((n, n))
        for i in range(n):
            part = parts[w][i * (i + 1) // 2:i * (i + 1) // 2 + i + 1] if parts[w] is not None else np.zeros(i + 1)
            H[i, :i + 1] = part + S[w, i, :i + 1]
            H[:i + 1, i] = H[i, :i + 1]
        H_ref.append(H)
    rng = np.random.RandomState(5)
    b = [rng.normal(0, 1.0, n) for n in PW]
    yield dict(ctx=c, g=g, H=H_ref, b=b, parts=parts)
    c.close()


@pytest.fixture(scope="module")
def plain():
    """a context of its own for the reference calls of icg_marg_linearize_batch"""
    c = _ctx()
    yield c
    c.close()


def _call(world, wins, ms, **kw):
    b = np.concatenate([world["b"][w] for w in wins])
    return world["ctx"].marg_linearize_resident(P, wins, [PW[w] for w in wins], ms, b, **kw)


def _ref(plain, world, wins, ms):
    H = np.concatenate([world["H"][w].ravel() for w in wins])
    b = np.concatenate([world["b"][w] for w in wins])
    return plain.marg_linearize_batch([PW[w] for w in wins], ms, H, b)


def _same(got, ref, what):
    for k in OUT_KEYS:
        if ref[k].dtype == np.int32:
            assert np.array_equal(got[k], ref[k]), (what, k)
        else:
            assert np.array_equal(bits(got[k]), bits(ref[k])), (what, k)


def _split(wins, ms, out):
    """per system: the bit patterns of every output"""
    res, r_at, rr_at, h_at = [], 0, 0, 0
    for k, (w, m) in enumerate(zip(wins, ms)):
        r, n = PW[w] - m, PW[w]
        d = {key: bits(out[key][rr_at:rr_at + r * r]) for key in ("J0", "Hp")}
        d.update({key: bits(out[key][r_at:r_at + r]) for key in ("e0", "bp", "evals")})
        d["min_ev_m"], d["status"] = bits(out["min_ev_m"][k:k + 1]), out["status"][k:k + 1].copy()
        d["H"] = bits(out["H"][h_at:h_at + n * n])
        res.append(d)
        r_at, rr_at, h_at = r_at + r, rr_at + r * r, h_at + n * n
    return res


def test_formed_systems_and_every_output_equal_the_reference(world, plain):
    assert world["parts"][NO_PART] is None and all(p is not None for w, p in enumerate(world["parts"]) if w != NO_PART)
    assert np.abs(world["parts"][2]).max() > 1e14  # the 1e8 block is in
    prof_ctx = world["ctx"]
    prof_ctx.prof_enable(True)
    prof_ctx.sync()
    count = lambda name: prof_ctx.prof().get(name, (0, 0.0))[0]
    forms, globals_ = count("marg_form_h"), count("marg_lin_global")
    for m in (0, 6, 15, "Pw - 1"):
        wins = [w for w in range(len(PW)) if (m == "Pw - 1" and w != WIDE) or (m != "Pw - 1" and m < PW[w] and (w != WIDE or m == 6))]
        ms = [PW[w] - 1 if m == "Pw - 1" else m for w in wins]
        got = _call(world, wins, ms)
        H_ref = np.concatenate([world["H"][w].ravel() for w in wins])
        assert np.array_equal(bits(got["H"]), bits(H_ref)), m
        _same(got, _ref(plain, world, wins, ms), m)
        assert np.isfinite(got["J0"]).all() and np.isfinite(got["e0"]).all(), m
    prof_ctx.sync()
    assert count("marg_form_h") == forms + 4 and count("marg_lin_global") == globals_ + 1  # one form launch per call; the wide window ran on global scratch
    prof_ctx.prof_enable(False)


def test_a_window_is_the_same_bits_alone_reversed_and_in_a_subset(world):
    wins = list(range(len(PW)))
    ms = [0, 3, 15, 6, 15, 15, 6]
    every = _split(wins, ms, _call(world, wins, ms))
    rev = _split(wins[::-1], ms[::-1], _call(world, wins[::-1], ms[::-1]))[::-1]
    sub_w = [5, 0, 3]
    sub = _split(sub_w, [ms[w] for w in sub_w], _call(world, sub_w, [ms[w] for w in sub_w]))
    for w in wins:
        if w != WIDE:  # (the wide window is in `every` and `rev` already)
            alone = _split([w], [ms[w]], _call(world, [w], [ms[w]]))[0]
            assert all(np.array_equal(alone[k], every[w][k]) for k in alone), w
        assert all(np.array_equal(rev[w][k], every[w][k]) for k in every[w]), w
    for k, w in enumerate(sub_w):
        assert all(np.array_equal(sub[k][key], every[w][key]) for key in every[w]), w


def test_the_resident_systems_are_only_read(world):
    c, g = world["ctx"], world["g"]
    W, n_lm = len(PW), len(g["inv"])
    rng = np.random.RandomState(3)
    dd, rhs = np.full((W, P), 1e6), rng.normal(0, 1.0, (W, P))
    solve = [1] * (W - 1) + [0]
    before = c.reproj_solve_windows(P, g["Pw"], solve, dd, rhs, n_lm)
    assert not before[1][:W - 1].any() and before[0][0, 0] != 0
    _call(world, [4, 1, NO_PART], [6, 0, 15])
    after = c.reproj_solve_windows(P, g["Pw"], solve, dd, rhs, n_lm)
    assert np.array_equal(before[1], after[1])
    for a, b in zip((before[0], before[2], before[3]), (after[0], after[2], after[3])):
        assert np.array_equal(bits(a), bits(b))


def test_keep_form_feeds_a_prior_set(world, plain):
    wins, ms = [4, 0, 2, 1], [0, 0, 0, 0]
    sizes = {43: [7] * 7 + [1], 1: [1], 31: [7] * 5 + [1], 7: [7, 1]}
    ref = _call(world, wins, ms)
    got, kid = _call(world, wins, ms, keep=True, want_J0=False, want_e0=False)
    assert kid != 0 and got["J0"] is None and got["e0"] is None
    for k in ("Hp", "bp", "evals", "min_ev_m", "H"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    priors = [mf.make_prior(sizes[PW[w]], 80 + k) for k, w in enumerate(wins)]
    r_at, rr_at = 0, 0
    for p in priors:
        r = p["r"]
        p["J0"], p["e0"] = ref["J0"][rr_at:rr_at + r * r].reshape(r, r).copy(), ref["e0"][r_at:r_at + r].copy()
        r_at, rr_at = r_at + r, rr_at + r * r
    a = mf.pack(priors)
    x = np.concatenate([mf.make_x(p, 90 + k) for k, p in enumerate(priors)])
    plain.marg_prior_set_from_kept(kid, np.arange(len(priors)), a["r"], a["block_off"], a["block_size"], a["block_index"], a["x0"])
    kept = plain.marg_prior_evaluate(x, want_grad=True, want_sq_norm=True)
    plain.marg_prior_set(*mf.set_args(priors))
    shipped = plain.marg_prior_evaluate(x, want_grad=True, want_sq_norm=True)
    for u, v in zip(kept, shipped):
        assert (u is None) == (v is None) and (u is None or np.array_equal(bits(u), bits(v)))
    # the id lives by the rules of icg_marg_linearize_batch_keep: the next linearize call on the owning context drops it
    _call(world, [0], [0])
    import icgvins
    with pytest.raises(icgvins.IcgError, match="is gone"):
        plain.marg_prior_set_from_kept(kid, np.arange(len(priors)), a["r"], a["block_off"], a["block_size"], a["block_index"], a["x0"])


def test_argument_errors_name_position_and_window(world):
    import icgvins
    c = world["ctx"]
    p_ = ptr
    FILL = 7.25
    wins0, Pw0, m0 = np.array([4, 1, 2], np.int32), np.array([43, 7, 31], np.int32), np.array([6, 0, 15], np.int32)
    b0 = np.concatenate([world["b"][w] for w in wins0])
    r = Pw0 - m0
    nrr, nr, nh = int((r * r).sum()), int(r.sum()), int((Pw0.astype(np.int64) ** 2).sum())

    def call(ctx=c, P_=P, n=3, win=wins0, Pw=Pw0, m=m0, b=b0, eps=1e-8, J0=True, e0=True, keep=False):
        out = dict(Hp=np.full(nrr, FILL), bp=np.full(nr, FILL), J0=np.full(nrr, FILL) if J0 else None, e0=np.full(nr, FILL) if e0 else None,
                   evals=np.full(nr, FILL), min_ev_m=np.full(3, FILL), status=np.full(3, 99, np.int32), H=np.full(nh, FILL))
        kid = C.c_uint64(12345)
        rc = ctx.lib.icg_marg_linearize_resident(ctx.h, int(P_), int(n), p_(win), p_(Pw), p_(m), p_(b), C.c_double(eps), p_(out["Hp"]), p_(out["bp"]),
                                                 p_(out["J0"]), p_(out["e0"]), p_(out["evals"]), p_(out["min_ev_m"]), p_(out["status"]), p_(out["H"]),
                                                 C.byref(kid) if keep else None)
        untouched = all(v is None or (v == (99 if v.dtype == np.int32 else FILL)).all() for v in out.values())
        return rc, ctx.lib.icg_last_error(ctx.h).decode(), untouched, int(kid.value)

    i32 = lambda *v: np.array(v, np.int32)
    cases = [("another P", dict(P_=150), "no resident reduced systems of 150 columns"),
             ("NULL win", dict(win=None), "NULL argument"), ("NULL Pw", dict(Pw=None), "NULL argument"), ("NULL m", dict(m=None), "NULL argument"),
             ("NULL b", dict(b=None), "NULL argument"), ("NULL J0, plain form", dict(J0=False), "NULL argument"),
             ("NULL e0, plain form", dict(e0=False), "NULL argument"),
             ("n_sel = 0", dict(n=0), "n_sel = 0"), ("n_sel < 0", dict(n=-2), "n_sel = -2"),
             ("window above the partition", dict(win=i32(4, 7, 2)), "position 1: window 7 outside the partition of 7"),
             ("negative window", dict(win=i32(4, 1, -1)), "position 2: window -1 outside the partition of 7"),
             ("window twice", dict(win=i32(4, 1, 4)), "position 2: window 4 is listed twice"),
             ("Pw = 0", dict(Pw=i32(43, 0, 31)), "position 1, window 1: Pw = 0 (1 .. 151)"),
             ("Pw above P", dict(Pw=i32(43, 7, 152)), "position 2, window 2: Pw = 152 (1 .. 151)"),
             ("part of another width", dict(Pw=i32(42, 7, 31)), "position 0, window 4: the resident host part has 43 columns, not 42"),
             ("m = Pw", dict(m=i32(6, 7, 15)), "position 1, window 1: m = 7"), ("m < 0", dict(m=i32(-1, 0, 15)), "position 0, window 4: m = -1"),
             ("eps < 0", dict(eps=-1e-9), "eps = -1e-09"), ("eps NaN", dict(eps=float("nan")), "eps = ")]
    c.prof_enable(True)
    try:
        c.sync()
        before = c.prof()
        for name, over, text in cases:
            for keep in (False, True):
                if keep and name.startswith("NULL J0") or keep and name.startswith("NULL e0"):
                    continue  # (optional in the keep form)
                rc, msg, untouched, kid = call(keep=keep, **over)
                assert rc == -1 and text in msg and "icg_marg_linearize_resident" in msg, (name, rc, msg)
                assert untouched, name
                assert not keep or kid == 0, name
            c.sync()
            assert c.prof() == before, name
        # no resident reduced systems at all: a fresh context
        fresh = _ctx()
        try:
            rc, msg, untouched, _ = call(ctx=fresh)
            assert rc == -1 and "no resident reduced systems of 151 columns" in msg and untouched, (rc, msg)
        finally:
            fresh.close()
        assert c.lib.icg_marg_linearize_resident(None, P, 3, p_(wins0), p_(Pw0), p_(m0), p_(b0), C.c_double(1e-8), None, None, None, None, None, None, None,
                                                 None, None) == -1
        # too many systems: the capacity code of icg_marg_linearize_batch
        rc, msg, untouched, _ = call(n=65536)
        assert rc == -5 and "65536 windows" in msg and untouched, (rc, msg)
        # a failed call drops what the context kept, as icg_marg_linearize_batch does
        out, kid = _call(world, [1], [0], keep=True)
        assert kid != 0
        rc, msg, _, _ = call(n=0)
        assert rc == -1
        with pytest.raises(icgvins.IcgError, match="is gone"):
            c.marg_prior_set_from_kept(kid, [0], [7], [0, 2], [7, 1], [0, 6], np.array([0, 0, 0, 0, 0, 0, 1, 0.0]))
        c.sync()
        assert c.prof()["marg_form_h"][0] == before.get("marg_form_h", (0, 0))[0] + 1  # only the good call launched
    finally:
        c.prof_enable(False)
