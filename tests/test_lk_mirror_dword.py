"""lk_load4_mirror (csrc/lk.hip) restated in numpy: the dword of image columns x .. x + 3 of a row under reflect-101 comes from ONE dword
window that lies inside the row and a byte selector.  Checked against a plain per-byte reflect-101 for every x a tile load can ask for
(-26 .. W + 25: the J tile reaches 26 outside a level) on every level width at the threshold and around it, with every residue mod 4."""
import numpy as np
import pytest

SEQ = 0x0102030201000102  # the byte sequence 2 1 0 1 2 3 2 1 (0): a dword mirrored at both of its ends
WIDTHS = list(range(32, 41)) + [63, 125, 160, 1280]


def reflect101(i, n):
    while i < 0 or i >= n:
        if i < 0:
            i = -i
        if i >= n:
            i = 2 * (n - 1) - i
    return i


def window_and_selector(x, W):
    """start column of the dword that is loaded and the four byte indices into it, as the kernel computes them (int32 / uint32 arithmetic)"""
    x = np.asarray(x, np.int32)
    s = np.minimum(np.maximum(np.maximum(np.minimum(x, 2 * W - 5 - x), 0), -3 - x), W - 4).astype(np.int32)
    sh = np.minimum((8 * (x - s) + 16).astype(np.uint32), np.uint32(40))
    o = (sh // np.uint32(8)).astype(np.uint64)
    sel = ((np.uint64(SEQ) >> (np.uint64(8) * o)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    idx = np.stack([(sel >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(4)], -1).astype(np.int32)
    return s, idx, o.astype(np.int32)


@pytest.mark.parametrize("W", WIDTHS)
def test_mirrored_dword_is_reflect101(W):
    xs = np.arange(-26, W + 26, dtype=np.int32)
    s, idx, o = window_and_selector(xs, W)
    assert s.min() >= 0 and (s + 3).max() <= W - 1  # no load starts before column 0 or ends after column W - 1
    assert idx.min() >= 0 and idx.max() <= 3        # every selector byte picks one of the four loaded bytes
    want = np.array([[reflect101(int(x) + k, W) for k in range(4)] for x in xs], np.int32)
    assert np.array_equal(s[:, None] + idx, want), (W, xs[(s[:, None] + idx != want).any(1)])
    # the six kinds of dword, where the issue of this change places them
    kinds = {int(x): int(k) for x, k in zip(xs, o)}
    assert kinds[-2] == 0 and kinds[-1] == 1 and kinds[W - 3] == 3 and kinds[W - 2] == 4
    assert all(kinds[x] == 2 for x in range(0, W - 3)) and all(kinds[x] == 5 for x in list(range(-26, -2)) + list(range(W - 1, W + 26)))
    assert idx[xs == -2].tolist() == [[2, 1, 0, 1]] and idx[xs == -1].tolist() == [[1, 0, 1, 2]]
    assert idx[xs == W - 3].tolist() == [[1, 2, 3, 2]] and idx[xs == W - 2].tolist() == [[2, 3, 2, 1]] and idx[xs == -7].tolist() == [[3, 2, 1, 0]]


@pytest.mark.parametrize("H", WIDTHS)
def test_row_mirror_is_reflect101(H):
    """lk_mirror: (H - 1) - |(H - 1) - |y|| for the rows a tile can ask for"""
    ys = np.arange(-26, H + 26)
    assert [(H - 1) - abs((H - 1) - abs(int(y))) for y in ys] == [reflect101(int(y), H) for y in ys]


def test_clamp_holds_for_any_column():
    """whatever x is — far outside the range a tile can ask for — the window stays inside the row (the selector may then be meaningless)"""
    for W in (32, 33, 1280):
        s, idx, _ = window_and_selector(np.arange(-5000, 5000, dtype=np.int32), W)
        assert s.min() >= 0 and (s + 3).max() <= W - 1 and idx.min() >= 0 and idx.max() <= 3
