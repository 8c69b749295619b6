"""CPU side of the detector edge tests (detect_edge_data.py): the inputs reach the edges of csrc/detect.hip they were built for — ROI extents
around the 60 x 64 block of a wave, grids with one block per ROI, tied responses whose order decides the result, flat ROIs, every reachable
exit of cornerSubPix, more blocks than one resident pass.  Conditions on the oracle's own maps and traces, not measurements.  The GPU side
(test_gpu_detect_edges.py) then compares the kernels with the oracle on the same bytes."""
import os
import re

import numpy as np
import pytest

import detect_edge_data as D

CONVERGED, CAP, OUT, SINGULAR = 1, 2, 3, 4


@pytest.fixture(scope="module")
def loaded(oracle):
    """case letter -> (CLAHE'd frames, calls, expected (points, block ids) per call and job): every call run once, shared by the tests below"""
    assert (oracle.SUBPIX_EXITS["converged"], oracle.SUBPIX_EXITS["cap"], oracle.SUBPIX_EXITS["out"], oracle.SUBPIX_EXITS["singular"]) == \
        (CONVERGED, CAP, OUT, SINGULAR)
    res = {}
    for letter, make in D.CASES.items():
        frames, calls = make()
        for f in frames:
            assert f.shape == (D.H, D.W) and f.dtype == np.uint8
        cl = [oracle.clahe(f) for f in frames]
        res[letter] = (cl, calls, [D.expected(oracle, cl, c) for c in calls])
    return res


def _local_maxima(eig):
    """(value, y, x) of the interior pixels above the quality threshold that are >= their eight neighbours (no mask)"""
    thresh = np.float32(float(eig.max()) * 0.01)
    nb = np.max([eig[1 + dy:eig.shape[0] - 1 + dy, 1 + dx:eig.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    c = eig[1:-1, 1:-1]
    ys, xs = np.nonzero((c > thresh) & (c >= nb) & (c != 0))
    return [(c[y, x], y + 1, x + 1) for y, x in zip(ys, xs)]


def _greedy(cands, rw, min_dist, quota, ascending_address):
    """featureselect.cpp's greedy selection over (value, y, x) candidates; ties by raster address, descending as OpenCV's sort leaves them or
    ascending"""
    sign = 1 if ascending_address else -1
    picked = []
    for v, y, x in sorted(cands, key=lambda c: (-c[0], sign * (c[1] * rw + c[2]))):
        if min_dist >= 1 and any(np.float32((x - px) ** 2 + (y - py) ** 2) < min_dist * min_dist for px, py in picked):
            continue
        picked.append((x, y))
        if len(picked) == quota:
            break
    return picked


def test_constants_are_the_kernels():
    """the numbers detect_edge_data.py copied from csrc/detect.hip are still the ones there"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ic-gvins_amd", "csrc", "detect.hip")).read()
    val = lambda name: int(re.search(r"^#define %s (\d+)" % name, src, re.M).group(1))
    assert (val("FE_TW"), val("FE_TH") * val("FE_WAVES")) == (D.FE_TW, D.FE_BH)
    assert (val("FE_RESIDENT_PER_XCD"), val("FE_WAVES")) == (D.FE_RESIDENT_PER_XCD, D.FE_WAVES)
    assert (val("DET_MAX_PER_BLOCK"), val("FE_MAX_RADIUS")) == (D.DET_MAX_PER_BLOCK, D.FE_MAX_RADIUS)
    assert "8 * FE_RESIDENT_PER_XCD" in src  # the launch cap of k_min_eig_nms


def test_case_a_extents_and_one_block_grids(loaded):
    """every ROI extent on either side of the block boundaries occurs; grids with one block per ROI (division by 1 in both steps of the block
    decoding), with one block per block row (division by 1 in the second step) and with one block row occur; every block of the grids of
    55 columns and more holds a corner, so that a block that was never processed shows as an empty one"""
    cl, calls, exp = loaded["A"]
    rws, rhs, one_block, one_per_row, one_row = set(), set(), 0, 0, 0
    for call, ((pts, blk),) in zip(calls, exp):
        g = call.grid
        assert g[0] * g[2] <= D.W and g[1] * g[3] <= D.H and g[2] > 6 and g[3] > 6 and 5 <= g[4] <= 10 and 8 <= g[5] <= 20
        R = D.rois(g)
        rws |= {r[2] for r in R}
        rhs |= {r[3] for r in R}
        gx, gy, n = D.device_blocks(g, len(R))
        one_block += gx * gy == 1
        one_per_row += gx == 1 and gy > 1
        one_row += gx > 1 and gy == 1
        per_block = np.bincount(blk, minlength=len(R))
        if g[2] == 7:
            assert (per_block[:-1] == 0).all()  # (2 x 2 ROIs have no interior pixel: nothing but the uncut last block can hold a corner)
        elif g[2] == 8:
            assert (per_block > 0).sum() >= len(R) // 4 and per_block.reshape(g[1], g[0]).any(1).all() and per_block.reshape(g[1], g[0]).any(0).all()
        else:
            assert (per_block > 0).all(), (g, per_block)
    assert rws >= D.RW_A and rhs >= D.RH_A
    assert one_block >= 3 and one_per_row >= 1 and one_row >= 1
    # the right and bottom image borders are reached by a ROI
    assert any(r[0] + r[2] == D.W and r[1] + r[3] == D.H for c in calls for r in D.rois(c.grid))


def test_case_b_exceeds_one_resident_pass(loaded):
    cl, calls, exp = loaded["B"]
    (call,) = calls
    gx, gy, n_blocks = D.device_blocks(call.grid, call.grid[0] * call.grid[1] * len(call.slots))
    assert n_blocks > D.BLOCKS_PER_PASS == 6144 and len(call.slots) == D.FRAMES_B
    # a second step exists for a workgroup of every XCD: its eighth of the groups of FE_WAVES blocks is longer than FE_RESIDENT_PER_XCD
    n_items = (n_blocks + D.FE_WAVES - 1) // D.FE_WAVES
    assert (n_items + 7) // 8 > D.FE_RESIDENT_PER_XCD
    # and the last XCD's range ends before a whole eighth (the `end` clamp) or exactly on it
    assert 8 * ((n_items + 7) // 8) >= n_items
    nblk = call.grid[0] * call.grid[1]
    for pts, blk in exp[0]:
        assert len(pts) > nblk  # every frame has corners, more than one per block on average
    assert len({e[0].tobytes() for e in exp[0]}) == D.FRAMES_B  # distinct frames, distinct results: a frame decoded as another one shows


def test_case_c_ties_decide_the_result(oracle, loaded):
    """each pattern has a tie group of >= 10 local maxima above the threshold and horizontally adjacent equal maxima; and the selection
    depends on the tie order: the same greedy selection with ties by ascending raster address picks a different point set"""
    cl, calls, exp = loaded["C"]
    R = D.rois(D.GRID_C + [0, D.DET_MAX_PER_BLOCK])
    for j, name in enumerate(D.PATTERNS_C):
        groups, pairs, differs = 0, 0, 0
        for k, roi in enumerate(R):
            eig = oracle.min_eigen_map(cl[j], roi)
            lm = _local_maxima(eig)
            vals, counts = np.unique([v for v, _, _ in lm], return_counts=True)
            groups = max(groups, int(counts.max()))
            at = {(y, x): v for v, y, x in lm}
            pairs += sum(1 for (y, x), v in at.items() if at.get((y, x + 1)) == v)
            for md, quota in ((0, 1), (2, 64), (6, 64)):
                ours = _greedy(lm, roi[2], md, quota, ascending_address=False)
                got = oracle.good_features(cl[j], None, roi, quota, 0.01, md)
                assert [tuple(p) for p in got.astype(int)] == ours, (name, k, md, quota)  # the restatement above is the oracle's selection
                differs += set(ours) != set(_greedy(lm, roi[2], md, quota, ascending_address=True))
        assert groups >= 10 and pairs >= 1 and differs >= len(R), (name, groups, pairs, differs)
    # quotas 1, 64 and 80 all occur; 80 is clamped: no block returns more than 64
    q = D.quotas_c()
    assert set(q) == {1, 64, 80}
    for call, per_job in zip(calls, exp):
        for pts, blk in per_job:
            per_block = np.bincount(blk, minlength=len(R))
            assert per_block.max() <= D.DET_MAX_PER_BLOCK and (per_block[q == 1] <= 1).all()
    # a quota of 80 has more than 64 candidates to choose from at min_dist 0: the clamp binds
    plain0 = [c.name for c in calls].index("C_plain_md0")
    assert any((np.bincount(blk, minlength=len(R))[q == 80] == D.DET_MAX_PER_BLOCK).any() for pts, blk in exp[plain0])
    # the discs change the result at every radius (they take out tied maxima) and leave corners in every job
    for md in set(D.MIN_DIST_C) & set(D.RADII_C):
        a, b = [c.name for c in calls].index("C_plain_md%d" % md), [c.name for c in calls].index("C_discs_md%d" % md)
        for (p0, _), (p1, _) in zip(exp[a], exp[b]):
            assert len(p1) > 0 and p0.tobytes() != p1.tobytes()


def test_case_c_disc_centres(loaded):
    """centres on both kinds of half-pixel ties (rint rounds to even: up and down) and on the corners of every ROI"""
    m = D.discs_c()
    half = m[(m % 1 == 0.5).any(1)]
    fl = np.floor(half[half % 1 == 0.5]).astype(int)
    assert (fl % 2 == 0).any() and (fl % 2 == 1).any()
    pts = {tuple(p) for p in m}
    for rx, ry, rw, rh in D.rois(D.GRID_C + [0, 64]):
        assert {(rx, ry), (rx + rw - 1, ry + rh - 1)} <= pts


def test_case_d_flat_rois(oracle, loaded):
    cl, calls, exp = loaded["D"]
    R = D.rois(D.GRID_D)
    names = [c.name for c in calls]
    # the constant frame: every ROI's maximum is exactly 0, no corner
    assert all(oracle.min_eigen_map(cl[0], roi).max() == 0 and oracle.min_eigen_map(cl[0], roi).min() == 0 for roi in R)
    assert len(exp[names.index("D_constant")][0][0]) == 0
    assert (np.bincount(exp[names.index("D_texture_after_constant")][0][1], minlength=12) > 0).all()
    # the partly flat frame: flat ROIs with a maximum of exactly 0 next to ROIs with corners
    per_block = np.bincount(exp[names.index("D_partly_flat")][0][1], minlength=12)
    for k, roi in enumerate(R):
        if k in D.FLAT_BLOCKS_D:
            assert oracle.min_eigen_map(cl[2], roi).max() == 0 and per_block[k] == 0, k
        elif k in D.TEXTURED_BLOCKS_D:
            assert per_block[k] > 0, k
    # the single square: only its block returns corners, fewer than the quota
    per_block = np.bincount(exp[names.index("D_one_square")][0][1], minlength=12)
    assert 0 < per_block[D.SQUARE_D[0]] < D.GRID_D[5] and per_block.sum() == per_block[D.SQUARE_D[0]]


def test_case_e_subpix_exits(oracle, loaded):
    """converged, 20-iteration cap, stepped out of the ROI through each of its four edges, moved more than 5 px and reset — on corners the
    detector itself picks in ROIs whose edges lie inside the image (the patch clamp there is the ROI's, not the image's); the trace's corners
    are the plain function's.  No input reaches the singular-determinant break."""
    cl, calls, exp = loaded["E"]
    g = D.GRID_E
    R = D.rois(g)
    kinds, sides, resets, near_edge = set(), set(), 0, set()
    for f in cl:
        for k in D.ROIS_E:
            rx, ry, rw, rh = roi = R[k]
            assert rx > 0 and ry > 0 and rx + rw < D.W and ry + rh < D.H
            picks = oracle.good_features(f, None, roi, g[5], 0.01, g[4])
            out, iters, kind, reset = oracle.corner_subpix_trace(f, roi, picks)
            assert out.tobytes() == oracle.corner_subpix(f, roi, picks).tobytes()
            assert ((kind == CAP) <= (iters == 20)).all() and (iters >= 1).all() and (kind != SINGULAR).all()
            kinds |= set(kind.tolist())
            resets += int(reset.sum())
            for (x, y), kd, rs in zip(out, kind, reset):
                if kd == OUT and not rs:
                    sides |= {s for s, c in (("left", x < 0), ("top", y < 0), ("right", x >= rw), ("bottom", y >= rh)) if c}
            # picks whose 13 x 13 patch is clamped at each ROI edge
            near_edge |= {s for s, c in (("left", (picks[:, 0] < 6).any()), ("top", (picks[:, 1] < 6).any()), ("right", (picks[:, 0] > rw - 8).any()),
                                         ("bottom", (picks[:, 1] > rh - 8).any())) if c}
    assert kinds == {CONVERGED, CAP, OUT}
    assert sides == {"left", "top", "right", "bottom"} == near_edge
    assert resets >= 4


def test_case_f_truncation_and_quotas(loaded):
    cl, calls, exp = loaded["F"]
    trunc, whole = calls
    assert [len(p) for p, _ in exp[0]] == [D.MAX_PER_JOB_F, D.MAX_PER_JOB_F]
    for j, s in enumerate(trunc.slots):  # the truncated result is the block-order prefix of the whole one
        jw = whole.slots.index(s)
        assert len(exp[1][jw][0]) > D.MAX_PER_JOB_F
        assert exp[0][j][0].tobytes() == exp[1][jw][0][:D.MAX_PER_JOB_F].tobytes() and np.array_equal(exp[0][j][1], exp[1][jw][1][:D.MAX_PER_JOB_F])
    q1 = whole.quotas[0]
    assert (q1 <= 0).sum() >= 4 and (q1 < 0).any() and (q1 == 0).any()
    per_block = np.bincount(exp[1][0][1], minlength=12)
    assert (per_block[q1 <= 0] == 0).all() and (per_block[q1 > 0] > 0).all() and (per_block <= np.maximum(q1, 0)).all()
