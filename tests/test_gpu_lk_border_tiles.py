"""k_lk_track_fb (csrc/lk.hip) loads a tile that crosses a border of its pyramid level as mirrored dwords when the level is at least 32 x 32
— one dword window inside the row and a v_perm per four pixels, the row index by a closed-form reflection — and through the general
reflect-101 loops on smaller levels.  Compared with the oracle bit for bit on points and status, one call per size (lk_border_data.py):
    250 x 254   levels 250 x 254, 125 x 127, 63 x 64, 32 x 32: widths of every residue mod 4, the coarsest level exactly on the threshold
    200 x 120   levels 200 x 120, 100 x 60 on the mirrored form beside 50 x 30 on the general one
with previous-image tiles 1 .. 8, 12, 16 and 22 columns or rows outside each side of every mirrored level, next-image tiles 1 .. 8, 12, 16,
22 and 26 outside at the coarsest level, tiles over the four corners, and guesses wrong by 24 .. 60 px along a border that re-stage the
next-image tile over it.  test_oracle_lk_border_tiles.py shows on the CPU that these inputs reach every such cell; pitch != width on every
level (256, 128, 128, 128 for 250 x 254), frames in the last slots as in test_gpu_lk_addressing.py."""
import numpy as np
import pytest

import lk_border_data as B
import synth


@pytest.mark.gpu
@pytest.mark.parametrize("size", B.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lk_border_tiles(oracle, size):
    import icgvins
    w, h = size
    case = B.make_case(w, h)
    img, nxt, pts, guess = case["img"], case["nxt"], case["pts"], case["guess"]
    assert 150 <= len(pts) <= 300
    ca, cb = oracle.clahe(img), oracle.clahe(nxt)
    exp_pts, exp_st = oracle.lk_track_fb(ca, cb, pts, guess)
    n_slots = 4
    c = icgvins.Context(w, h, n_slots=n_slots, max_batch=2, max_points=512)
    try:
        s = w / 640.0
        c.set_camera([synth.CAM_640[0] * s, synth.CAM_640[1] * s, w / 2.0, h / 2.0] + list(synth.CAM_640[4:]))
        assert c.levels() == len(B.levels(w, h))
        c.preprocess([n_slots - 2, n_slots - 1], [img, nxt])
        assert np.array_equal(c.download(n_slots - 2, 0), ca) and np.array_equal(c.download(n_slots - 1, 0), cb)
        got_pts, got_st = c.lk_track_fb(n_slots - 2, n_slots - 1, pts, guess)
    finally:
        c.close()
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    bad = np.nonzero((got_st != exp_st) | (bits(got_pts) != bits(exp_pts)).any(1))[0]
    cells = case["cells"] + [("restage",)] * case["n_restage"]
    assert bad.size == 0, (size, len(bad), [cells[i] for i in bad[:12]], pts[bad[:6]], got_pts[bad[:6]], exp_pts[bad[:6]], got_st[bad[:6]], exp_st[bad[:6]])
