"""The inputs of lk_border_data.py reach what test_gpu_lk_border_tiles.py needs them to reach, shown on the CPU with the oracle alone: where
each tile lies is restated in float32, operation by operation as lk_track_wave computes it, every (tile, level, side, k) cell is hit exactly,
and the oracle's trace shows that the cell's level is ITERATED for its point — not skipped by the range test or the eigenvalue test, which
would leave the tile loaded and unused.  No cell may be missing.  One kind of cell cannot be iterated on any image, the previous-image tile
22 outside: its window keeps one column (row) of the level, the border one, whose derivative across the border is identically zero; for
these the test asserts that very exit instead (see below)."""
import numpy as np
import pytest

import lk_border_data as B

F32 = np.float32


def tile_reach(coord, level, n, first, size):
    """(columns outside on the low side, on the high side) of the tile of a window whose level-0 coordinate is `coord`, in float32"""
    scale = F32(1.0 / (1 << level))
    o = int(np.floor(F32(F32(coord) * scale) - F32(B.HALF)))
    assert -B.WIN <= o <= n - 1, (coord, level, o)  # the window passes the kernel's range test
    lo = o - first
    return max(0, -lo), max(0, lo + size - n)


@pytest.mark.parametrize("size", B.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cells_are_reached_and_iterated(oracle, size):
    w, h = size
    case = B.make_case(w, h)
    lv = B.levels(w, h)
    assert lv == {(250, 254): [(250, 254), (125, 127), (63, 64), (32, 32)], (200, 120): [(200, 120), (100, 60), (50, 30)]}[size]
    assert B.mirrored_levels(w, h) == {(250, 254): [0, 1, 2, 3], (200, 120): [0, 1]}[size]
    pts, guess, cells = case["pts"], case["guess"], case["cells"]
    ca, cb = oracle.clahe(case["img"]), oracle.clahe(case["nxt"])
    _, st, _, tr = oracle.lk_track_trace(ca, cb, pts, guess)
    assert tr["levels"] == len(lv)
    hit = set()
    for i, (tile, l, sides, k) in enumerate(cells):
        wl, hl = lv[l]
        src = pts[i] if tile == "I" else guess[i]
        first, sz = (1, B.IT) if tile == "I" else (B.JM, B.JT)
        reach = dict(zip(B.SIDES, tile_reach(src[0], l, wl, first, sz) + tile_reach(src[1], l, hl, first, sz)))
        # (an axis the cell does not name has the tile centred; where the level is smaller than the tile — the general form only — the tile
        # is over on both sides there, and a named side leaves the opposite one what is left of the excess)
        want_reach = {}
        for (lo, hi), n in ((("left", "right"), wl), (("top", "bottom"), hl)):
            over = max(0, sz - n)
            if lo in sides:
                want_reach[lo], want_reach[hi] = k, max(0, over - k)
            elif hi in sides:
                want_reach[lo], want_reach[hi] = max(0, over - k), k
            else:
                want_reach[lo], want_reach[hi] = over - over // 2, over // 2
        assert reach == want_reach, (size, cells[i], reach, want_reach)
        assert l not in B.mirrored_levels(w, h) or sum(reach.values()) == k * len(sides)
        if tile == "I" and k == B.WIN + 1:
            # The one cell that no texture can iterate: the only window column (row) still inside the level is column (row) 0 or W - 1, where the
            # Scharr difference across the border is I(1) - I(-1) = 0 under reflect-101 and the plane is zero outside: A11 (A22) is exactly 0
            # and the level ends at the eigenvalue test.  The tile is loaded and differentiated all the same; assert exactly this reason.
            assert tr["exit"][i, l] == oracle.LK_EXITS["weak"] and tr["A"][i, l, 0 if sides[0] in ("left", "right") else 2] == 0, (size, cells[i])
            assert tr["A"][i, l, 2 if sides[0] in ("left", "right") else 0] > 0, (size, cells[i], tr["A"][i, l])  # the other plane sees the texture
        else:
            assert tr["iters"][i, l] >= 1, (size, cells[i], tr["exit"][i], tr["iters"][i])  # the level used its tiles
        hit.add(cells[i])
    want = {("I", l, (s,), k) for l in B.mirrored_levels(w, h) for s in B.SIDES for k in B.K_I}
    want |= {("I", l, c, B.K_CORNER) for l in B.mirrored_levels(w, h) for c in B.CORNERS}
    want |= {("J", len(lv) - 1, (s,), k) for s in B.SIDES for k in B.K_J} | {("J", len(lv) - 1, c, B.K_CORNER) for c in B.CORNERS}
    assert hit == want and len(cells) == len(want), (size, want - hit, hit - want)
    assert set(B.K_I) == set(range(1, 9)) | {12, 16, 22} and set(B.K_J) == set(B.K_I) | {26}


@pytest.mark.parametrize("size", B.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restage_points_travel_along_their_border(oracle, size):
    """per border: guesses wrong by 24 .. 60 px along it move the window by more than the J tile's margin inside a level (the tile is staged
    again), and the window is within 15 px of that border at the start and at the end — every 32 x 32 tile around such a window crosses it"""
    w, h = size
    case = B.make_case(w, h)
    n0, n = case["n_cells"], case["n_restage"]
    pts, guess = case["pts"][n0:], case["guess"][n0:]
    assert n == 24 and len(pts) == n
    ca, cb = oracle.clahe(case["img"]), oracle.clahe(case["nxt"])
    out, st, _, tr = oracle.lk_track_trace(ca, cb, case["pts"], case["guess"])
    out, travel = out[n0:], tr["travel"][n0:]
    d = np.abs(guess - pts - np.array(B.MOVES[size], F32)).max(1)
    assert (d >= 24).all() and (d <= 60).all()
    total = 0
    for s, side in enumerate(B.SIDES):
        sl = slice(6 * s, 6 * s + 6)
        depth = {"left": lambda p: p[:, 0], "right": lambda p: w - 1 - p[:, 0], "top": lambda p: p[:, 1], "bottom": lambda p: h - 1 - p[:, 1]}[side]
        near = (depth(guess[sl]) < 15) & (depth(out[sl]) < 15)
        n_side = int(((travel[sl].max(1) > B.JM) & near).sum())
        assert n_side >= 1, (size, side, travel[sl], depth(guess[sl]), depth(out[sl]))
        total += n_side
    assert total >= 6, (size, total)
