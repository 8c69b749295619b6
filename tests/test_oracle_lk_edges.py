"""CPU side of the LK edge tests (lk_edge_data.py): (a) the inputs reach the bounds and paths of csrc/lk.hip they were built for — conditions
on the oracle's per-level trace (orc_lk_track_trace), not measurements — and (b) the oracle itself is right there, against the independent
numpy LK of test_oracle_lk_float_bound.py.  The GPU side (test_gpu_lk_edges.py) then compares the kernels with the oracle on the same bytes."""
import numpy as np
import pytest

import lk_edge_data as D
import test_oracle_lk_float_bound as fb

WEAK, OUT, CONVERGED, OSCILLATION, CAP, SKIPPED = 2, 3, 4, 5, 6, 1


@pytest.fixture(scope="module")
def traced(oracle):
    """case letter -> [(sub-case, clahe_a, clahe_b, out, status, err, trace)]: every sub-case run once, shared by the tests below"""
    assert (oracle.LK_EXITS["weak"], oracle.LK_EXITS["out"], oracle.LK_EXITS["converged"], oracle.LK_EXITS["oscillation"], oracle.LK_EXITS["cap"],
            oracle.LK_EXITS["skipped"]) == (WEAK, OUT, CONVERGED, OSCILLATION, CAP, SKIPPED)
    res = {}
    for letter, make in D.CASES.items():
        res[letter] = []
        for case in make():
            name, w, h, a, b, pts, guess = case
            assert a.shape == (h, w) and b.shape == (h, w) and a.dtype == np.uint8 and b.dtype == np.uint8
            assert pts.dtype == np.float32 and guess.dtype == np.float32 and pts.shape == guess.shape == (len(pts), 2)
            assert np.isfinite(pts).all() and np.isfinite(guess).all() and max(np.abs(pts).max(), np.abs(guess).max()) <= 1e6
            ca, cb = oracle.clahe(a), oracle.clahe(b)
            res[letter].append((case, ca, cb) + oracle.lk_track_trace(ca, cb, pts, guess))
    return res


def test_trace_returns_what_lk_track_returns(oracle, traced):
    """the trace is observation only: points, status and err are byte-identical to orc_lk_track's on every sub-case"""
    for runs in traced.values():
        for (name, w, h, a, b, pts, guess), ca, cb, out, st, err, tr in runs:
            o2, s2, e2 = oracle.lk_track(ca, cb, pts, guess)
            assert np.array_equal(st, s2), name
            assert out.tobytes() == o2.tobytes() and err.tobytes() == e2.tobytes(), name
            assert tr["levels"] == np.count_nonzero(tr["exit"][0]), name


def test_case_a_saturates_the_window_sums(oracle, traced):
    """lk.hip's bounds: a lane's 7-pixel partial < 2^27 (dx^2) / 2^28 (b), window totals split into 16-bit halves above 2^32.  The inputs get
    there: windows that are TRACKED at level 0 (status 1: the iterations ran on these sums) with A11 >= 2^32 and with min(A11, A22) >= 2^31,
    |b| >= 2^31, and a 7-pixel run of dx^2 above 2^26 (half the lane bound) in the derivative image."""
    a11 = both = 0
    bmax = run7 = 0
    for (name, w, h, a, b, pts, guess), ca, cb, out, st, err, tr in traced["A"]:
        A0 = tr["A"][:, 0]
        tracked = (st == 1) & (tr["iters"][:, 0] > 0)
        a11 += int((tracked & (A0[:, 0] >= 2 ** 32)).sum())
        both += int((tracked & (np.minimum(A0[:, 0], A0[:, 2]) >= 2 ** 31)).sum())
        bmax = max(bmax, int(tr["bmax"][tracked, 0].max(initial=0)))
        dx2 = oracle.scharr(ca)[..., 0].astype(np.int64) ** 2
        run7 = max(run7, int(sum(dx2[:, k:w - 6 + k] for k in range(7)).max()))
        if "stripes" in name:  # A22 = 0: every point weak on every level, with the largest A11 there is
            assert (tr["exit"] == WEAK).all() and not st.any() and A0[:, 0].max() >= 7e9
    assert a11 >= 20 and both >= 20, (a11, both)
    assert bmax >= 2 ** 31, bmax
    assert run7 >= 2 ** 26, run7


def test_case_b_levels_and_statuses(traced):
    assert [(c[0][1], c[0][2]) for c in traced["B"]] == D.SIZES_B
    assert [c[6]["levels"] for c in traced["B"]] == D.LEVELS_B == [4, 4, 3, 2, 2, 1]
    for (name, w, h, *_), ca, cb, out, st, err, tr in traced["B"]:
        assert 0 < st.sum() < len(st), name
        assert (tr["exit"][:, tr["levels"]:] == 0).all() and (tr["exit"][:, :tr["levels"]] != 0).all(), name


def test_case_c_coordinate_classes(traced):
    w, h = 320, 240
    cls = D.case_c_classes(w, h)
    frac = lambda v: v - np.floor(v)
    assert (frac(cls["integer"]) == 0).all() and (frac(cls["half"]) == 0.5).all()
    assert (np.nextafter(cls["below_integer"], np.float32(1e9)) == np.floor(cls["below_integer"]) + 1).all()
    f = frac(cls["tiny_fraction"].astype(np.float64))
    assert (f == 2.0 ** -15).any() and (f == 2.0 ** -20).any() and ((f == 0) | (f == 2.0 ** -15) | (f == 2.0 ** -20)).all()
    neg = cls["negative"]
    assert ((neg.min(1) < 0) & (neg.min(1) > -11)).all()
    po = cls["prev_outside"]
    dist = np.maximum(np.maximum(-po[:, 0], po[:, 0] - (w - 1)), np.maximum(-po[:, 1], po[:, 1] - (h - 1)))
    assert sorted(set(dist.tolist())) == list(D.OUTSIDE_C)
    runs = {c[0][0]: c for c in traced["C"]}
    (name, _, _, _, _, pts, guess), ca, cb, out, st, err, tr = runs["C_classes"]
    n0 = sum(len(v) for v in cls.values())
    lo = n0 - len(po)
    assert np.array_equal(pts[lo:n0], po)
    ex = tr["exit"][lo:n0]
    assert (ex[:, 0] == SKIPPED).all() and not st[lo:n0].any()                  # level 0 "continue" ...
    assert ((ex[:, 1:] != SKIPPED).any(1)).any() and (ex == SKIPPED).all(1).any()  # ... after coarse levels that ran, and on every level
    (_, _, _, _, _, pts_g, guess_g), _, _, _, st_g, _, tr_g = runs["C_guess_outside"]
    dist_g = np.maximum(np.maximum(-guess_g[:, 0], guess_g[:, 0] - (w - 1)), np.maximum(-guess_g[:, 1], guess_g[:, 1] - (h - 1)))
    assert sorted(set(dist_g.tolist())) == list(D.OUTSIDE_C)
    assert 0 < st_g.sum() < len(st_g)                                             # both statuses among the outside points
    assert ((tr_g["exit"] == OUT) & (tr_g["iters"] == 0)).any()                   # a first window already outside
    (_, _, _, _, _, pts_p, guess_p), _, _, _, st_p, _, tr_p = runs["C_pulled_out"]
    pulled = (tr_p["exit"] == OUT) & (tr_p["iters"] >= 1)                         # started inside, pulled out
    assert pulled[:, 0].sum() >= 5 and pulled[:, 1:].sum() >= 5


def test_case_d_travels_inside_a_level(traced):
    """the next image's 32x32 tile holds the 22x22 support with a margin of 5: in-level travel above 5 px re-stages it"""
    for (name, *_), ca, cb, out, st, err, tr in traced["D"]:
        far = (tr["travel"].max(1) > 5) & (st == 1)
        assert far.sum() >= 10, (name, far.sum())


def test_case_e_flips_the_eigenvalue_verdict(traced):
    runs = {c[0][0]: c for c in traced["E"]}
    assert (runs["E_constant"][6]["exit"] == WEAK).all() and (runs["E_constant"][6]["A"] == 0).all()
    on_blob = np.array([runs[f"E_blob{a}"][6]["exit"][:6, 0] for a in D.AMPS_E])  # (amplitude, point)
    weak = on_blob == WEAK
    assert weak.any() and (~weak).any()
    assert (weak.any(0) & (~weak).any(0)).any()  # one and the same point flips inside the sweep


def test_every_exit_kind_is_taken(traced):
    """Reached with the inputs as committed: all five exits (weak, out of image, converged, oscillation, 30-iteration cap) plus the 'continue' of a
    previous-image window outside the level — six of six, counted over all cases per (point, level): weak 9180, out of image 868, converged 28110,
    oscillation 5344, cap 797, skipped 69."""
    kinds = np.concatenate([c[6]["exit"].ravel() for runs in traced.values() for c in runs])
    count = {k: int((kinds == k).sum()) for k in (WEAK, OUT, CONVERGED, OSCILLATION, CAP, SKIPPED)}
    print("exit kinds (point, level):", count)
    assert all(v > 0 for v in count.values()), count
    assert (np.concatenate([c[6]["iters"].ravel() for runs in traced.values() for c in runs]) == 30).any()


# ---- (b) the oracle against the independent float-accumulating LK -------------------------------------------------------------------
def _pick(letter, runs):
    """at most 20 points per case: sub-cases evenly, and inside a sub-case evenly spaced indices — for case A the tracked windows with the
    largest min(A11, A22), where the exact-integer sums are furthest from anything the other tests reach"""
    if letter == "F":
        runs = runs[-1:]  # (the sub-cases are prefixes of one list)
    q = max(1, 20 // len(runs))
    for run in runs[:20]:
        (name, w, h, a, b, pts, guess), ca, cb, out, st, err, tr = run
        n = len(pts)
        if letter == "A" and st.any():
            score = np.where(st == 1, np.minimum(tr["A"][:, 0, 0], tr["A"][:, 0, 2]), -1)
            idx = np.argsort(-score, kind="stable")[:q]
        else:
            idx = (np.arange(min(q, n)) * n) // min(q, n) + n // (2 * min(q, n))
        yield run, np.unique(idx)


@pytest.mark.parametrize("letter", list(D.CASES))
def test_oracle_matches_independent_float_lk(traced, letter, monkeypatch):
    """Status equal and positions within max(2e-3 px, 4 x spread), spread = the largest distance between the independent implementation's own
    two float accumulation orders (raster, 4 lanes) on the same points.  A status may differ only where the two orders disagree with each
    other (a threshold decision inside float rounding).  Measured spread / largest distance to the oracle, px:
    A 1.2e-4 / 1.2e-4, B 9.2e-5 / 9.2e-5, C 8.4e-5 / 8.4e-5, D 0.198 / 0.214 (one track of the smooth image that runs into the 30-iteration cap:
    the two float orders part from each other as far as from the oracle), E 0 / 0 (few windows of the faint blob are tracked at all),
    F 9.9e-5 / 9.9e-5."""
    spread = worst = 0.0
    checked = 0
    for ((name, w, h, a, b, pts, guess), ca, cb, out, st, err, tr), idx in _pick(letter, traced[letter]):
        monkeypatch.setattr(fb, "MAXLEVEL", tr["levels"] - 1)  # (that file builds the pyramid of full-size frames: 4 levels)
        r_pts, r_st = fb.lk_float(ca, cb, pts[idx], guess[idx], "raster")
        l_pts, l_st = fb.lk_float(ca, cb, pts[idx], guess[idx], "lanes4")
        settled = r_st == l_st
        assert np.array_equal(st[idx][settled], r_st[settled]), name
        ok = settled & (r_st == 1)
        checked += len(idx)
        if ok.any():
            spread = max(spread, float(np.abs(r_pts[ok] - l_pts[ok]).max()))
            worst = max(worst, float(np.abs(out[idx][ok] - r_pts[ok]).max()), float(np.abs(out[idx][ok] - l_pts[ok]).max()))
    print(f"case {letter}: {checked} points, spread {spread:.3g} px, oracle within {worst:.3g} px")
    assert 0 < checked <= 20
    assert worst <= max(2e-3, 4 * spread), (worst, spread)
