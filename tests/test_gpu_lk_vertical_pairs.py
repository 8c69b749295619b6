"""GPU parity of k_lk_track (with err) and k_lk_track_fb (csrc/lk.hip) with the CPU oracle where the vertical pixel pairs of round 13 are
built and consumed, bit for bit (status bytes, uint32 views of every float), through the entry points test_gpu_lk_edges.py uses.  The pairs
(row r, row r + 1) at one column feed the Gauss-Newton blend (lk_fetch_J: fetched again whenever the integer window position changes, from a
tile that is re-staged when the window leaves it), the level-0 error epilogue and the interior level set-up; the border set-up keeps
horizontal pairs.  The classes of inputs below reach each of those, and the test checks from the inputs alone that every class is there."""
import numpy as np
import pytest

import synth
from test_gpu_lk_edges import _context, _run_cases
from test_gpu_lk_setup_paths import _flush_coords

pytestmark = pytest.mark.gpu
F32 = np.float32
MOVE = (1.3, -0.7)
HALF = F32(10)  # half window: a window starts at floor(p - 10)


def _off(n, lo, hi, seed):
    """n offsets whose magnitude is in [lo, hi] on EACH axis, signs mixed"""
    rng = np.random.RandomState(seed)
    return rng.uniform(lo, hi, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))


def _points(w, h, levels):
    """(points, guesses, class label per point)"""
    move = np.array(MOVE)
    pts, gs, cls = [], [], []

    def add(p, g, c):
        p = np.asarray(p, np.float64).reshape(-1, 2)
        pts.append(p), gs.append(np.asarray(g, np.float64).reshape(-1, 2)), cls.extend([c] * len(p))

    # (a) guesses 1.5 .. 3 px off the true shift on each axis: the integer window position changes between iterations of a level
    p = synth.random_points(64, w, h, 14, seed=1301).astype(np.float64)
    add(p, p + move + _off(len(p), 1.5, 3.0, 1302), "a")
    # (b) guesses 7 .. 12 px off: the window leaves the 10-pixel slack of the next image's tile, which is staged again inside a level
    p = synth.random_points(64, w, h, 14, seed=1303).astype(np.float64)
    add(p, p + move + _off(len(p), 7.0, 12.0, 1304), "b")
    # (c) window starts on four consecutive integer columns and rows
    p = np.array([(30.3 + i, 27.6 + k) for i in range(4) for k in range(4)])
    add(p, p + 0.8 * move, "c")
    # (d) fractional offsets 0 and 0.5, with points on integer positions (w00 = 2^14, the other weights 0)
    p = np.array([(bx + fx, by + fy) for bx, by in ((33.0, 30.0), (47.0, 25.0), (58.0, 36.0)) for fx in (0.0, 0.5) for fy in (0.0, 0.5)])
    add(p, p + 0.8 * move, "d")
    # (e) window starts on both sides of the interior test at every border, on level 0 and on the coarsest level
    for lvl in (0, levels - 1):
        s = float(1 << lvl)
        xs, ys = _flush_coords(w >> lvl, s, (0.0, 0.5)), _flush_coords(h >> lvl, s, (0.0, 0.5))
        p = np.array([(x, my) for x in xs for my in (h / 2 + 0.6, h / 2 - 4.0)] + [(mx, y) for y in ys for mx in (48.3, 40.0)]
                     + [(x, y) for x in xs[:4] for y in ys[:4]])
        p = p[(p[:, 0] > -30) & (p[:, 0] < w + 30) & (p[:, 1] > -30) & (p[:, 1] < h + 30)]
        add(p, p + 0.8 * move, "e%d" % lvl)
    return np.concatenate(pts).astype(F32), np.concatenate(gs).astype(F32), np.array(cls)


@pytest.mark.parametrize("w,h,levels", [(96, 64, 2), (96, 88, 3)], ids=["96x64", "96x88"])
def test_vertical_pairs_bit_exact(oracle, w, h, levels):
    """96x64 (levels 96x64, 48x32) and 96x88 (96x88, 48x44, 24x22): the smallest pyramids with two and three levels whose coarsest level
    still holds a window.  Both entry points, every float and status byte against the oracle."""
    ctx = _context(w, h)
    try:
        assert ctx.levels() == levels
    finally:
        ctx.close()
    img = synth.texture(w, h, seed=1300)
    nxt = synth.shift_image(img, *MOVE)
    pts, gs, cls = _points(w, h, levels)
    assert 200 <= len(pts) <= 512

    # the classes are where they claim to be, from the inputs alone
    off = np.abs(gs.astype(np.float64) - (pts.astype(np.float64) + np.array(MOVE)))
    in_a = ((off >= 1.5) & (off <= 3.0)).all(1)
    in_b = ((off >= 6.999) & (off <= 12.0)).all(1)
    assert (in_a & (cls == "a")).sum() >= 8 and (in_b & (cls == "b")).sum() >= 8
    ipx, ipy = np.floor(pts[:, 0] - HALF).astype(int), np.floor(pts[:, 1] - HALF).astype(int)
    c = cls == "c"
    assert c.sum() >= 8
    cols, rows = sorted(set(ipx[c])), sorted(set(ipy[c]))
    assert cols == list(range(cols[0], cols[0] + 4)) and rows == list(range(rows[0], rows[0] + 4))  # every byte phase of a row of the tile
    assert set(zip(ipx[c], ipy[c])) == {(x, y) for x in cols for y in rows}
    gx = np.floor(gs[:, 0] - HALF).astype(int)
    assert len(set(gx[c] & 3)) == 4  # ... and of the next image's tile at the level-0 start
    frac = pts.astype(np.float64) - np.floor(pts.astype(np.float64))
    d = (cls == "d") & np.isin(frac, (0.0, 0.5)).all(1)
    assert d.sum() >= 8 and (frac[d] == 0.0).all(1).any() and (frac[d] == 0.5).all(1).any()
    e0 = cls == "e0"
    inside = (ipx >= 0) & (ipx + 22 <= w) & (ipy >= 0) & (ipy + 22 <= h)
    assert (e0 & inside).sum() >= 8 and (e0 & ~inside).sum() >= 8
    for v in (0, w - 22):
        assert (e0 & inside & (ipx == v)).any()
    for v in (0, h - 22):
        assert (e0 & inside & (ipy == v)).any()
    for v in (-1, w - 21):
        assert (e0 & (ipx == v)).any()
    for v in (-1, h - 21):
        assert (e0 & (ipy == v)).any()
    # the coarsest level: the same on its own grid (a previous point is scaled by 2^-level exactly)
    sc = F32(1.0 / (1 << (levels - 1)))
    wl, hl = w >> (levels - 1), h >> (levels - 1)
    qx, qy = np.floor(pts[:, 0] * sc - HALF).astype(int), np.floor(pts[:, 1] * sc - HALF).astype(int)
    el = cls == "e%d" % (levels - 1)
    inside_l = (qx >= 0) & (qx + 22 <= wl) & (qy >= 0) & (qy + 22 <= hl)
    assert (el & inside_l).sum() >= 8 and (el & ~inside_l).sum() >= 8
    for v in (0, wl - 22, -1, wl - 21):
        assert (el & (qx == v)).any()
    for v in (0, hl - 22, -1, hl - 21):
        assert (el & (qy == v)).any()

    _run_cases(oracle, [(f"vertical_pairs_{w}x{h}", w, h, img, nxt, pts, gs)])
