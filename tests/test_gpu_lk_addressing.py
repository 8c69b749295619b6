"""k_lk_track_fb (csrc/lk.hip) loads the tiles that lie inside a pyramid level through a scalar base pointer — frame base + slot * slot bytes +
level offset — and ONE 32-bit byte offset row * pitch + col per lane.  Compared with the oracle bit for bit where that addressing can go
wrong: frames in the LAST slots of a context with several (the largest base the context has), levels whose pitch is not their width (64 ->
128, 333 -> 384, 167 -> 256, ...) and one whose pitch is (1280), windows ONE pixel inside the interior test on each side of every level
(the inside path then reads the first and the last bytes of the level), and guesses so far off that the next image's tile is re-staged
inside a level (the second call site of the tile load; lk_edge_data.py case D is the model).  One call per size."""
import numpy as np
import pytest

import lk_edge_data as D
import synth

F32 = np.float32
SIZES = [(64, 48), (333, 257), (1280, 720)]
MOVES = {(64, 48): (1.5, -1.25), (333, 257): (9.0, -11.5), (1280, 720): (-13.25, 10.0)}
WIN, HALF = 21, 10  # ICG_LK_WIN, ICG_LK_HALF


def levels(w, h):
    out = [(w, h)]
    while len(out) < 4:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= WIN or h <= WIN:
            break
        out.append((w, h))
    return out


def edge_points(w, h):
    """per level: previous points whose 24x24 tile of the previous image starts at column / row 0 or ends at the last one — on each of the
    four sides and in the two corners that hold the level's first and last byte"""
    pts = []
    for l, (wl, hl) in enumerate(levels(w, h)):
        s = float(1 << l)
        x_lo, x_hi, y_lo, y_hi = 11.5 * s, (wl - 12.5) * s, 11.5 * s, (hl - 12.5) * s
        xm, ym = ((wl - 24) // 2 + 11.25) * s, ((hl - 24) // 2 + 11.25) * s  # (a level may be exactly 24 high: the only row that is inside)
        pts += [(x_lo, ym), (x_hi, ym), (xm, y_lo), (xm, y_hi), (x_lo, y_lo), (x_hi, y_hi)]
    return np.array(pts, F32)


def tile_guesses(w, h, move):
    """per level: guesses whose 32x32 tile of the next image starts at column / row 0 or ends at the last one when the level is entered with
    them (exactly so on the coarsest level, where the guess is scaled; on the finer ones as far as the track above lands on the move)"""
    prev, guess = [], []
    for l, (wl, hl) in enumerate(levels(w, h)):
        if wl < 32 or hl < 32:
            continue
        s = float(1 << l)
        x_lo, x_hi, y_lo, y_hi = 15.5 * s, (wl - 16.5) * s, 15.5 * s, (hl - 16.5) * s
        for g in [(x_lo, y_lo), (x_hi, y_hi), (x_lo, y_hi), (x_hi, y_lo)]:
            guess.append(g)
            prev.append((g[0] - move[0], g[1] - move[1]))
    return np.array(prev, F32).reshape(-1, 2), np.array(guess, F32).reshape(-1, 2)


def make_case(w, h):
    move = MOVES[(w, h)]
    img = np.ascontiguousarray(D.smooth(w, h, seed=950 + w))  # (D.smooth hands back a column-major array for sizes off its lattice)
    nxt = synth.shift_image(img, *move)
    mv = np.array(move, F32)
    edge = edge_points(w, h)
    tp, tg = tile_guesses(w, h, move)
    inner = synth.random_points(16, w, h, min(40, h // 3), seed=951 + w)
    rng = np.random.RandomState(952 + w)
    far = synth.random_points(24, w, h, min(40, h // 3), seed=953 + w)
    ang, rad = rng.uniform(0, 2 * np.pi, len(far)), rng.uniform(24, 60, len(far)) * min(1.0, h / 240.0)
    far_guess = (far + mv + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)).astype(F32)
    pts = np.concatenate([edge, tp, inner, far]).astype(F32)
    guess = np.concatenate([edge + F32(0.8) * mv, tg, inner + F32(0.8) * mv, far_guess]).astype(F32)
    return img, nxt, pts, guess, len(edge), len(tp)


def check_reach(w, h, pts, guess, n_edge, n_tile):
    """float32, operation by operation as lk_track_wave: the previous-image tile of every edge point sits ON the level's border on its level
    and passes the interior test; the next-image tile of the coarsest level's guesses does"""
    lv = levels(w, h)
    hit = set()
    for k in range(n_edge):
        l, side = divmod(k, 6)
        wl, hl = lv[l]
        scale = F32(1.0 / (1 << l))
        ipx = int(np.floor(pts[k, 0] * scale - F32(HALF))) - 1
        ipy = int(np.floor(pts[k, 1] * scale - F32(HALF))) - 1
        assert 0 <= ipx and ipx + 24 <= wl and 0 <= ipy and ipy + 24 <= hl, (w, h, k, ipx, ipy)
        hit |= {(l, n) for n, on in (("left", ipx == 0), ("right", ipx + 24 == wl), ("top", ipy == 0), ("bottom", ipy + 24 == hl)) if on}
        if side == 4:
            assert ipx == 0 and ipy == 0
            hit.add((l, "first byte"))
        if side == 5:
            assert ipx + 24 == wl and ipy + 24 == hl
            hit.add((l, "last byte"))
    assert hit == {(l, n) for l in range(len(lv)) for n in ("left", "right", "top", "bottom", "first byte", "last byte")}, (w, h, hit)
    top = len(lv) - 1
    if lv[top][0] >= 32 and lv[top][1] >= 32:
        g = guess[n_edge + n_tile - 4:n_edge + n_tile]  # the coarsest level's four
        scale = F32(1.0 / (1 << top))
        jx = np.floor(g[:, 0] * scale - F32(HALF)).astype(int) - 5
        jy = np.floor(g[:, 1] * scale - F32(HALF)).astype(int) - 5
        assert jx[0] == 0 and jy[0] == 0 and jx[1] + 32 == lv[top][0] and jy[1] + 32 == lv[top][1], (w, h, jx, jy)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lk_tile_addressing(oracle, size):
    import icgvins
    w, h = size
    img, nxt, pts, guess, n_edge, n_tile = make_case(w, h)
    assert 40 <= len(pts) <= 100
    check_reach(w, h, pts, guess, n_edge, n_tile)
    ca, cb = oracle.clahe(img), oracle.clahe(nxt)
    _, st, _, tr = oracle.lk_track_trace(ca, cb, pts, guess)  # (the oracle's trace: observation only)
    assert st.sum() >= len(pts) // 2, (size, st.sum())  # forward tracks that live, so that the backward pass runs: the slots change roles
    if h >= 240:  # in-level travel above the tile's margin of 5 px re-stages the tile (64 x 48 has no room for such guesses)
        assert ((tr["travel"].max(1) > 5) & (st == 1)).sum() >= 3, (size, tr["travel"].max(1))
    exp_pts, exp_st = oracle.lk_track_fb(ca, cb, pts, guess)
    n_slots = 4
    c = icgvins.Context(w, h, n_slots=n_slots, max_batch=2, max_points=256)
    try:
        s = w / 640.0
        c.set_camera([synth.CAM_640[0] * s, synth.CAM_640[1] * s, w / 2.0, h / 2.0] + list(synth.CAM_640[4:]))
        assert c.levels() == len(levels(w, h))
        c.preprocess([n_slots - 2, n_slots - 1], [img, nxt])
        assert np.array_equal(c.download(n_slots - 2, 0), ca) and np.array_equal(c.download(n_slots - 1, 0), cb)
        got_pts, got_st = c.lk_track_fb(n_slots - 2, n_slots - 1, pts, guess)
    finally:
        c.close()
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    bad = np.nonzero((got_st != exp_st) | (bits(got_pts) != bits(exp_pts)).any(1))[0]
    assert bad.size == 0, (size, bad[:8], pts[bad[:8]], got_pts[bad[:8]], exp_pts[bad[:8]], got_st[bad[:8]], exp_st[bad[:8]])
