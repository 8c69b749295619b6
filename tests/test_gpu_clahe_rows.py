"""k_clahe_apply (csrc/image.hip) reads a row's vertical blend weights, and whether the row belongs to the workgroup's strip of tiles at all,
from a per-workgroup table that one thread per row fills while the LUTs are staged.  The preprocessed level 0 is compared with the oracle byte
for byte at heights whose strip boundaries fall on rows where y * inv_th - 0.5 is exactly integral (even tile heights), half-way between two
rows (odd ones) and off both by a rounding of 1 / th, at images cut off inside a strip, and at widths that take each form of the kernel: the
byte form with the table (256), the float form with the table (1000) and the float form whose staged LUTs leave no room for it (800)."""
import numpy as np
import pytest

import synth

T = 21  # ICG_CLAHE_TILES
HEIGHTS = (64, 65, 72, 100, 257, 720)
CASES = [(w, h) for w in (256, 1000) for h in HEIGHTS] + [(800, 65), (800, 100)]
F32 = np.float32


def geometry(w, h):
    """tile size as icg_frames_preprocess lays it out"""
    ew, eh = w, h
    if w % T or h % T:
        ew, eh = w + (T - w % T), h + (T - h % T)
    return ew // T, eh // T


def row_terms(h, th):
    """tyf = y * inv_th - 0.5 and its floor, in float32 operation by operation as the kernel computes them"""
    inv_th = F32(1.0) / F32(th)
    tyf = (np.arange(h, dtype=np.int32).astype(F32) * inv_th).astype(F32) - F32(0.5)
    return tyf, np.floor(tyf).astype(np.int32)


def pairs_per_chunk(w, tw):
    inv_tw = F32(1.0) / F32(tw)
    p = np.floor((np.arange(w, dtype=np.int32).astype(F32) * inv_tw).astype(F32) - F32(0.5)).astype(np.int32) + 1
    return [int(p[x0:x0 + 256].max() - p[x0:x0 + 256].min() + 1) for x0 in range(0, w, 256)]


def test_cases_reach_the_strip_boundaries():
    """every strip's candidate window [y_lo, y_hi) holds exactly the rows of its strip plus rows of the strip below and above that the table
    must mark; every row is taken by exactly one strip; the accepted rows of a strip are contiguous; integral, half-way and inexact boundary
    values all occur; and the three forms of the kernel are all taken"""
    integral = halfway = inexact = clipped = 0
    forms = set()
    for w, h in CASES:
        tw, th = geometry(w, h)
        tyf, tyr = row_terms(h, th)
        assert tyr.min() == -1 and np.array_equal(np.unique(tyr), np.arange(-1, tyr.max() + 1)), (w, h)  # both sides of every boundary occur
        taken = np.zeros(h, np.int32)
        for strip in range(T + 1):
            y_lo, y_hi = max((strip - 1) * th + th // 2 - 2, 0), min(strip * th + th // 2 + 3, h)
            if y_hi <= y_lo:
                continue
            assert y_hi - y_lo <= 128, (w, h, strip)  # the table's rows
            ys = np.arange(y_lo, y_hi)
            mine = tyr[ys] == strip - 1
            taken[ys[mine]] += 1
            if mine.any():
                assert np.all(np.diff(np.nonzero(mine)[0]) == 1), (w, h, strip)
                first, last = ys[mine][0], ys[mine][-1]
                # the window reaches past the strip on both sides unless the image ends there
                assert first == 0 or (first - 1 >= y_lo and tyr[first - 1] == strip - 2), (w, h, strip)
                assert last == h - 1 or (last + 1 < y_hi and tyr[last + 1] == strip), (w, h, strip)
                clipped += int(last == h - 1 and strip * th + th // 2 + 3 > h)
        assert np.all(taken == 1), (w, h, np.nonzero(taken != 1)[0][:8])
        first_rows = np.nonzero(np.diff(tyr) == 1)[0] + 1  # the first row of every strip but the top one
        frac = tyf[first_rows] - np.floor(tyf[first_rows])
        exact = (first_rows.astype(np.float64) / th - 0.5)  # the real-number value
        integral += int(np.sum((frac == 0) & (exact == np.floor(exact))))
        halfway += int(np.sum(np.floor(exact) != exact))
        inexact += int(np.sum((exact == np.floor(exact)) & (tyf[first_rows].astype(np.float64) != exact))) + \
            int(np.sum(tyf[first_rows - 1].astype(np.float64) != (first_rows - 1) / th - 0.5))
        for n in pairs_per_chunk(w, tw):
            forms.add("byte+table" if n > 8 else ("float+table" if n < 8 else "float"))
    assert integral >= 10 and halfway >= 10 and inexact >= 10 and clipped >= len(CASES), (integral, halfway, inexact, clipped)
    assert forms == {"byte+table", "float+table", "float"}, forms


@pytest.mark.gpu
@pytest.mark.parametrize("size", CASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_clahe_rows_match_the_oracle(oracle, size):
    import icgvins
    w, h = size
    img = synth.texture(w, h, seed=900 + w + h)
    c = icgvins.Context(w, h, n_slots=1, max_batch=1, max_points=64)
    try:
        c.preprocess([0], [img])
        got = c.download(0, 0)
    finally:
        c.close()
    exp = oracle.clahe(img)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (size, len(bad), bad[:8])
