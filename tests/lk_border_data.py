"""Deterministic LK inputs whose tile loads cross the borders of a pyramid level (csrc/lk.hip: lk_load_I / lk_load_J, the mirrored-dword form
for levels of at least 32 x 32 and lk_stage_small below that), shared by the CPU test that proves the inputs reach every cell
(test_oracle_lk_border_tiles.py) and the GPU parity test (test_gpu_lk_border_tiles.py): both see identical bytes.

A CELL is (tile, level, side, k): the 24 x 24 tile of the previous image ("I", columns ipx - 1 .. ipx + 22) or the 32 x 32 tile of the next
image at the level's start ("J", columns inx - 5 .. inx + 26) reaches k columns or rows outside the level on that side.  I cells exist on every
level that takes the mirrored form; J cells on the coarsest level of the pyramid, where the guess is only scaled (on 200 x 120 that level is
50 x 30 and takes the general form, beside two levels on the mirrored one)."""
import numpy as np

import lk_edge_data as D
import synth

F32 = np.float32
WIN, HALF = 21, 10  # ICG_LK_WIN, ICG_LK_HALF
IT, JT, JM = 24, 32, 5  # LK_IT, LK_JT, LK_JM
SIZES = [(250, 254), (200, 120)]
MOVES = {(250, 254): (2.75, -1.5), (200, 120): (-1.75, 2.25)}
K_I = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 22)
K_J = K_I + (26,)
SIDES = ("left", "right", "top", "bottom")
CORNERS = (("left", "top"), ("right", "top"), ("left", "bottom"), ("right", "bottom"))
K_CORNER = 3


def levels(w, h):
    out = [(w, h)]
    while len(out) < 4:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= WIN or h <= WIN:
            break
        out.append((w, h))
    return out


def mirrored_levels(w, h):
    return [l for l, (wl, hl) in enumerate(levels(w, h)) if min(wl, hl) >= JT]


def _origin(n, side_lo, k, first, size):
    """integer window origin (ipx or inx) whose tile — first column at origin - first, `size` wide — reaches k outside on the low or high side
    of a level n wide; the fraction favours the window column that is still inside the level (its derivative is not masked to zero)"""
    if side_lo:
        return first - k, 0.75
    return n - 1 + k - (size - 1) + first, 0.25


def _middle(n, first, size):
    return (n - size) // 2 + first, 0.25


def _coord(origin, frac, level):
    return (origin + HALF + frac) * float(1 << level)  # exact in float32: a small multiple of 2^-2 times a power of two


def cell_points(w, h):
    """-> (cells, prev, guess): cells[i] = (tile, level, sides, k) of point i; prev / guess in level-0 pixels (float64 lists)"""
    lv, mv = levels(w, h), MOVES[(w, h)]
    top = len(lv) - 1
    cx, cy = 0.5 * w, 0.5 * h
    cells, prev, guess = [], [], []

    def add(tile, l, sides, k):
        wl, hl = lv[l]
        first, size = (1, IT) if tile == "I" else (JM, JT)
        ox, fx = _middle(wl, first, size)
        oy, fy = _middle(hl, first, size)
        for s in sides:
            if s in ("left", "right"):
                ox, fx = _origin(wl, s == "left", k, first, size)
            else:
                oy, fy = _origin(hl, s == "top", k, first, size)
        p = (_coord(ox, fx, l), _coord(oy, fy, l))
        cells.append((tile, l, tuple(sides), k))
        if tile == "I":
            prev.append(p)
            guess.append((p[0] + 0.8 * mv[0], p[1] + 0.8 * mv[1]))
        else:  # the previous point is the image centre: its own tiles are inside on every level
            prev.append((cx, cy))
            guess.append(p)

    for l in mirrored_levels(w, h):
        for side in SIDES:
            for k in K_I:
                add("I", l, (side,), k)
        for c in CORNERS:
            add("I", l, c, K_CORNER)
    for side in SIDES:
        for k in K_J:
            add("J", top, (side,), k)
    for c in CORNERS:
        add("J", top, c, K_CORNER)
    return cells, prev, guess


def restage_points(w, h):
    """points 8 .. 13 px inside each border with guesses wrong by 24 .. 60 px ALONG that border (lk_edge_data.py case D is the model): the window
    stays within 15 px of the border, where every 32 x 32 tile around it crosses the border, and travels far enough to be re-staged"""
    rng = np.random.RandomState(1000 + w)
    mv = MOVES[(w, h)]
    prev, guess = [], []
    for side in SIDES:
        for j in range(6):
            d = 8.0 + j
            t = rng.uniform(0.3, 0.7)
            off = rng.uniform(24, min(60, 0.25 * (w if side in ("top", "bottom") else h))) * (1 if j % 2 else -1)
            if side in ("left", "right"):
                p = (d if side == "left" else w - 1 - d, t * h)
                g = (p[0] + mv[0], p[1] + mv[1] + off)
            else:
                p = (t * w, d if side == "top" else h - 1 - d)
                g = (p[0] + mv[0] + off, p[1] + mv[1])
            prev.append(p)
            guess.append(g)
    return prev, guess


_CACHE = {}


def make_case(w, h):
    """-> dict(img, nxt, pts, guess, cells, n_cells, n_restage); computed once per size and shared (treat as read-only)"""
    if (w, h) not in _CACHE:
        mv = MOVES[(w, h)]
        img = texture(w, h)
        nxt = synth.shift_image(img, *mv)
        cells, cp, cg = cell_points(w, h)
        rp, rg = restage_points(w, h)
        pts = np.array(cp + rp, np.float64).astype(F32)
        guess = np.array(cg + rg, np.float64).astype(F32)
        _CACHE[(w, h)] = dict(img=img, nxt=nxt, pts=pts, guess=guess, cells=cells, n_cells=len(cells), n_restage=len(rp))
    return _CACHE[(w, h)]


MIX = {(250, 254): 0.6, (200, 120): 0.4}  # share of the noise; searched with the oracle alone (test_oracle_lk_border_tiles.py holds the criteria)


def texture(w, h):
    """lk_edge_data.smooth's wide basins (so that a guess tens of pixels off still travels) under uniform noise: enough of it that windows with a
    few columns or rows left inside the level pass the eigenvalue test on every level and that the coarse levels, where a point near the
    image's border has most of its window outside, do not throw the track out of the image before the level of its cell"""
    mix = MIX[(w, h)]
    base = np.ascontiguousarray(D.smooth(w, h, seed=960 + w)).astype(np.float64)
    fine = D.noise(w, h, 961 + w).astype(np.float64)
    return np.clip((1.0 - mix) * base + mix * fine, 0, 255).astype(np.uint8)
