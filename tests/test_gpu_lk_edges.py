"""GPU parity of k_lk_track / k_lk_track_fb / k_lk_finish / k_keep_indices (csrc/lk.hip) with the CPU oracle on the edge inputs of
lk_edge_data.py: saturated window sums, small and odd pyramids, positions on and around every rounding edge of the weight and epoch
arithmetic, long in-level travel, weak texture, and point counts around the kernels' chunk sizes.  test_oracle_lk_edges.py proves on the CPU
that the inputs reach those edges.  Everything is compared bit for bit (status bytes, uint32 views of every float), as in test_gpu_frontend.py."""
import numpy as np
import pytest

import lk_edge_data as D
import synth
from test_gpu_geometry import grid_for

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _camera(w, h):
    s = w / 640.0
    return [synth.CAM_640[0] * s, synth.CAM_640[1] * s, w / 2.0, h / 2.0] + list(synth.CAM_640[4:])


def _context(w, h, max_points=512):
    import icgvins
    c = icgvins.Context(w, h, n_slots=2, max_batch=2, max_points=max_points)
    c.set_camera(_camera(w, h))
    return c


def _check_pair(oracle, c, case, loaded=None):
    """one sub-case on a context of its size: single-direction track (status, points, err) and forward/backward track (status, points,
    undistorted points, keep list) against the oracle"""
    name, w, h, a, b, pts, guess = case
    if loaded is None:
        c.preprocess([0, 1], [a, b])
        loaded = oracle.clahe(a), oracle.clahe(b)
        assert np.array_equal(c.download(0, 0), loaded[0]) and np.array_equal(c.download(1, 0), loaded[1]), name
    ca, cb = loaded
    exp_pts, exp_st, exp_err = oracle.lk_track(ca, cb, pts, guess)
    got_pts, got_st, got_err = c.lk_track(0, 1, pts, guess)
    bad = np.nonzero((got_st != exp_st) | (_bits(got_pts) != _bits(exp_pts)).any(1) | (_bits(got_err) != _bits(exp_err)))[0]
    assert bad.size == 0, (name, "lk_track", bad[:8], pts[bad[:8]], got_pts[bad[:8]], exp_pts[bad[:8]], got_st[bad[:8]], exp_st[bad[:8]])
    exp_pts, exp_st = oracle.lk_track_fb(ca, cb, pts, guess)
    got_pts, got_st, got_und, keep = c.lk_track_fb(0, 1, pts, guess, want_undist=True, want_keep=True)
    bad = np.nonzero((got_st != exp_st) | (_bits(got_pts) != _bits(exp_pts)).any(1))[0]
    assert bad.size == 0, (name, "lk_track_fb", bad[:8], pts[bad[:8]], got_pts[bad[:8]], exp_pts[bad[:8]], got_st[bad[:8]], exp_st[bad[:8]])
    assert np.array_equal(keep, np.nonzero(exp_st)[0]), name
    assert np.array_equal(_bits(got_und), _bits(oracle.undistort(_camera(w, h), exp_pts))), name
    return loaded


def _run_cases(oracle, cases, max_points=512):
    w, h = cases[0][1], cases[0][2]
    c = _context(w, h, max_points)
    try:
        loaded, frames = None, None
        for case in cases:
            assert (case[1], case[2]) == (w, h)
            if frames is None or case[3] is not frames[0] or case[4] is not frames[1]:
                loaded, frames = None, (case[3], case[4])  # (sub-cases that share their frames are preprocessed once)
            loaded = _check_pair(oracle, c, case, loaded)
    finally:
        c.close()


@pytest.mark.parametrize("pattern", ["stripes", "checker", "quilt", "blocks", "noise"])
def test_saturated_contrast(oracle, pattern):
    """A: binary width-2 patterns: window sums above 2^32 (the 16-bit split of the wave reductions), lane partials near their 2^27 / 2^28
    bounds, Scharr terms at 4 x 4016 in the packed 16-bit stencil, and iterations that end by oscillation and by the 30-iteration cap"""
    cases = [c for c in D.case_a() if c[0].startswith(f"A_{pattern}_")]
    assert len(cases) == 3
    _run_cases(oracle, cases)


@pytest.mark.parametrize("size", D.SIZES_B, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_and_odd_pyramids(oracle, size):
    """B: 4, 4, 3, 2, 2 and 1 pyramid levels with odd level sizes, down to levels smaller than the kernel's 24x24 and 32x32 LDS tiles (both
    reflect at the border); preprocessing (CLAHE with 2x2 .. 16x13 tiles, pyrDown) is checked level by level on the way"""
    case = [c for c in D.case_b() if (c[1], c[2]) == tuple(size)][0]
    name, w, h, a, b, pts, guess = case
    c = _context(w, h)
    try:
        c.preprocess([0, 1], [a, b])
        levels = D.LEVELS_B[D.SIZES_B.index(tuple(size))]
        assert c.levels() == levels
        pyr = []
        for slot, img in ((0, a), (1, b)):
            exp = [oracle.clahe(img)]
            for _ in range(1, levels):
                exp.append(oracle.pyrdown(exp[-1]))
            for l in range(levels):
                got = c.download(slot, l)
                assert got.shape == exp[l].shape and np.array_equal(got, exp[l]), (name, slot, l)
            pyr.append(exp[0])
        _check_pair(oracle, c, case, tuple(pyr))
        if tuple(size) == (333, 257):  # detection at an odd size
            grid = grid_for(w, h, 100)
            q = np.full(grid[0] * grid[1], grid[5], np.int32)
            out, cnt, blk = c.detect([0], grid, [0, 0], np.zeros((0, 2)), q, 200)
            exp_pts, exp_blk = oracle.detect(pyr[0], grid, np.zeros((0, 2)), q, 200)
            assert cnt[0] == len(exp_pts) and cnt[0] > 20
            assert np.array_equal(blk[0, :cnt[0]], exp_blk)
            assert np.array_equal(_bits(out[0, :cnt[0]]), _bits(exp_pts))
    finally:
        c.close()


def test_positions(oracle):
    """C: integer, x.5, just-below-integer and 2^-15 / 2^-20 fractions (Q14 weights by the magic-constant rint, the epoch test on the bit
    pattern of the carried fraction), negative coordinates, previous points and guesses 12 .. 400 px outside the image (level-0 and
    coarse-level 'continue'), and tracks that start inside and are pulled out"""
    _run_cases(oracle, D.case_c())


def test_long_travel_inside_a_level(oracle):
    """D: guesses wrong by 24 .. 60 px on a smooth image: the window leaves the 32x32 tile of the next image and is re-staged inside a level"""
    for case in D.case_d():
        _run_cases(oracle, [case])


def test_weak_texture(oracle):
    """E: a constant image (all sums zero) and a faint 3x3 blob swept through the division-free minimum-eigenvalue threshold"""
    for case in D.case_e():
        _run_cases(oracle, [case])


def test_point_counts(oracle):
    """F: n around the 64-lane wave, k_lk_finish's 256-thread blocks, k_keep_indices' 1024-wide chunks and icg_xcd_chunked's tail, with about a
    third of the points lost so that the keep list is a real compaction"""
    cases = D.case_f()
    assert [len(c[5]) for c in cases] == list(D.COUNTS_F)
    _run_cases(oracle, cases, max_points=4096)
