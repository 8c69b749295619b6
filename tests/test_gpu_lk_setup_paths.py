"""GPU parity of the two level set-up paths of k_lk_track / k_lk_track_fb (csrc/lk.hip) with the CPU oracle, bit for bit (status bytes, uint32
views of every float), through the entry points test_gpu_lk_edges.py uses.  A level whose 22x22 derivative support lies inside the image
takes the blend-first path (one Q14 blend of the 23x23 grid through LDS, then a 32-bit Scharr stencil); a support that reaches over a border
keeps the form that masks the derivative plane.  The inputs sit on both sides of that test at every level, at the stencil's saturation, on
the rounding edges of the weights, and where lane 63 (which owns no pixels) would read if it were active."""
import numpy as np
import pytest

import lk_edge_data as D
import synth
from test_gpu_lk_edges import _context, _run_cases

pytestmark = pytest.mark.gpu
F32 = np.float32
MOVE = (1.3, -0.7)


def _guess(pts, move=MOVE):
    return (pts + F32(0.8) * np.array(move, F32)).astype(F32)


def _flush_coords(size, scale, fracs):
    """coordinates c (level 0) whose window start floor(c / scale - 10) on the level of that scale is 0 / size - 22 (support flush with the
    border, still inside) and -1 / size - 21 (one pixel outside), at each fractional offset"""
    out = []
    for f in fracs:
        out += [scale * (10.0 + f), scale * (9.0 + f), scale * (size - 12.0 + f), scale * (size - 11.0 + f)]
    return out


@pytest.mark.parametrize("w,h,levels", [(96, 64, 2), (96, 88, 3)], ids=["96x64", "96x88"])
def test_support_flush_with_every_border(oracle, w, h, levels):
    """(a) window starts ipx == 0, ipx + 22 == W, the same in y, and one pixel outside each, on level 0 and on the coarsest level.  96x64 has
    the levels 96x64 and 48x32 (a third, 24x16, would be no larger than the window: icg_ctx_create stops before it); 96x88 is the smallest
    height with three (96x88, 48x44, 24x22: the coarsest support fits in one position in y and three in x)"""
    c = _context(w, h)
    try:
        assert c.levels() == levels
    finally:
        c.close()
    img = synth.texture(w, h, seed=301)
    nxt = synth.shift_image(img, *MOVE)
    pts = []
    for lvl in (0, levels - 1):
        s = float(1 << lvl)
        wl, hl = w >> lvl, h >> lvl
        xs, ys = _flush_coords(wl, s, (0.0, 0.5)), _flush_coords(hl, s, (0.0, 0.5))
        mids_x, mids_y = (48.3, 40.0), (h / 2 + 0.6, h / 2 - 4.0)
        pts += [(x, my) for x in xs for my in mids_y] + [(mx, y) for y in ys for mx in mids_x]
        pts += [(x, y) for x in xs[:4] for y in ys[:4]]  # the corners: flush / outside on both axes at once
    pts = np.array(pts, np.float64)
    pts = pts[(pts[:, 0] > -30) & (pts[:, 0] < w + 30) & (pts[:, 1] > -30) & (pts[:, 1] < h + 30)].astype(F32)
    # the level-0 cases are where they claim to be
    ipx, ipy = np.floor(pts[:, 0] - F32(10)), np.floor(pts[:, 1] - F32(10))
    inside = (ipx >= 0) & (ipx + 22 <= w) & (ipy >= 0) & (ipy + 22 <= h)
    for v in (0, w - 22):
        assert (inside & (ipx == v)).any()
    for v in (0, h - 22):
        assert (inside & (ipy == v)).any()
    for v in (-1, w - 21):
        assert (ipx == v).any()
    for v in (-1, h - 21):
        assert (ipy == v).any()
    _run_cases(oracle, [(f"flush_{w}x{h}", w, h, img, nxt, pts, _guess(pts))])


@pytest.mark.parametrize("pattern", ["stripes", "checker"])
def test_saturated_contrast_64(oracle, pattern):
    """(b) binary width-2 stripes and a checkerboard at 64x64: Scharr terms at +-4080 and B at its maximum in the 32-bit stencil, interior
    windows (10 <= x, y <= 52 on level 0) and border windows side by side"""
    w = h = 64
    img = {"stripes": D.stripes, "checker": D.checker}[pattern](w, h)
    grid = [(x + fx, y + fy) for x in (10, 21, 31, 42, 52) for y in (10, 31, 52) for fx, fy in ((0.0, 0.0), (0.5, 0.25))]
    cases = []
    for k, (mname, nxt, d) in enumerate([("roll2_0", np.roll(img, (0, 2), axis=(0, 1)), (2.0, 0.0)), ("roll1_2", np.roll(img, (2, 1), axis=(0, 1)), (1.0, 2.0)),
                                          ("shift", synth.shift_image(img, *MOVE), MOVE)]):
        pts = np.concatenate([synth.random_points(60, w, h, 0, seed=310 + k), np.array(grid)]).astype(F32)
        cases.append((f"sat64_{pattern}_{mname}", w, h, img, nxt, pts, _guess(pts, d)))
    _run_cases(oracle, cases)


def test_previous_point_fractions(oracle):
    """(c) previous-point fractions 0, 0.5, 1 - 2^-15 and 2^-20 on both axes (coordinates in [8, 16): a float there carries 2^-20), with the
    window start at 0 (flush) and at 3 on level 0"""
    w, h = 96, 64
    img = synth.texture(w, h, seed=302)
    nxt = synth.shift_image(img, *MOVE)
    fr = (0.0, 0.5, 1.0 - 2.0 ** -15, 2.0 ** -20)
    pts = np.array([(bx + fx, by + fy) for bx, by in ((10.0, 10.0), (13.0, 13.0), (13.0, 10.0)) for fx in fr for fy in fr], np.float64).astype(F32)
    frac = pts.astype(np.float64) - np.floor(pts.astype(np.float64))
    for f in fr:
        assert (frac[:, 0] == f).any() and (frac[:, 1] == f).any()  # (the float32 coordinates carry the fractions exactly)
    _run_cases(oracle, [("fractions_96x64", w, h, img, nxt, pts, _guess(pts))])


def test_lane_63_stays_inert(oracle):
    """(d) a constant image with one bright pixel in the top row of the window, columns 0..6 (lane 63 has the lane coordinates of lane 0: were
    its derivative outputs not zero, the pixel's gradients would enter the window sums twice), and one row below"""
    w, h = 96, 64
    img = np.full((h, w), 100, np.uint8)
    px, py = 40, 22
    img[py, px] = 255
    nxt = np.full((h, w), 100, np.uint8)
    nxt[py, px + 1] = 255
    pts = np.array([(px + 10 - k, py + 10 - r) for k in range(7) for r in (0, 1)], np.float64).astype(F32)
    _run_cases(oracle, [("lane63_pixel", w, h, img, nxt, pts, _guess(pts, (1.0, 0.0)))])
    # the pixel is texture enough for the track to be attempted at all (else the case would compare nothing)
    exp_pts, exp_st = oracle.lk_track_fb(oracle.clahe(img), oracle.clahe(nxt), pts, _guess(pts, (1.0, 0.0)))
    assert exp_st.any()


def test_forward_backward_130_points(oracle):
    """(e) k_lk_track_fb on 130 points, about a third of them lost (flat region, image border): both directions through the set-up paths"""
    name, w, h, img, nxt, pool, guess = D.case_f()[-1]
    n = 130
    ca, cb = oracle.clahe(img), oracle.clahe(nxt)
    _, st = oracle.lk_track_fb(ca, cb, pool[:600], guess[:600])
    good, lost = np.nonzero(st)[0], np.nonzero(st == 0)[0]
    pick = np.sort(np.concatenate([good[:n - n // 3], lost[:n // 3]]))  # in pool order: the lost ones stay mixed in
    assert len(pick) == n
    pts, gs = pool[pick].copy(), guess[pick].copy()
    _, exp_st = oracle.lk_track_fb(ca, cb, pts, gs)
    assert int((exp_st == 0).sum()) == n // 3
    _run_cases(oracle, [("fb_130", w, h, img, nxt, pts, gs)])
