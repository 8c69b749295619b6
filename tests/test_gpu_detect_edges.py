"""GPU parity of k_min_eig_nms / k_select / k_subpix and icg_detect's host assembly (csrc/detect.hip) with the CPU oracle on the edge inputs of
detect_edge_data.py: ROI extents on either side of the 60 x 64 block of a wave (grids with one block per ROI or per block row among them),
more blocks than one resident pass, tied responses, min_dist 0 .. 3, flat ROIs, every reachable exit of cornerSubPix, quota clamping and
max_per_job truncation, refused grids.  test_oracle_detect_edges.py proves on the CPU that the inputs reach those edges.  Counts, block ids
and the uint32 views of the points are compared bit for bit, per block, as in test_gpu_geometry.py."""
import numpy as np
import pytest

import detect_edge_data as D
from test_gpu_geometry import grid_for

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _context(n_frames):
    import icgvins
    return icgvins.Context(D.W, D.H, n_slots=n_frames, max_batch=n_frames, max_points=64)


def _load(oracle, c, frames):
    """frames into slots 0 .. n-1; the CLAHE'd frames the detector reads, checked first so that a preprocessing difference is not blamed on it"""
    c.preprocess(list(range(len(frames))), frames)
    cl = [oracle.clahe(f) for f in frames]
    for s, f in enumerate(cl):
        assert np.array_equal(c.download(s, 0), f), s
    return cl


def _check_call(oracle, c, cl, call):
    mask_off = np.cumsum([0] + [len(m) for m in call.masks]).astype(np.int32)
    out, cnt, blk = c.detect(call.slots, call.grid, mask_off, np.concatenate(call.masks), np.concatenate(call.quotas), call.max_per_job)
    nblk = call.grid[0] * call.grid[1]
    total = 0
    for j, (exp_pts, exp_blk) in enumerate(D.expected(oracle, cl, call)):
        n = int(cnt[j])
        got = np.bincount(blk[j, :n], minlength=nblk) if n else np.zeros(nblk, np.int64)
        assert np.array_equal(got, np.bincount(exp_blk, minlength=nblk)), (call.name, j, "corners per block", got, np.bincount(exp_blk, minlength=nblk))
        assert n == len(exp_pts) and np.array_equal(blk[j, :n], exp_blk), (call.name, j)
        bad = np.nonzero((_bits(out[j, :n]) != _bits(exp_pts)).any(1))[0]
        assert bad.size == 0, (call.name, j, bad[:8], exp_blk[bad[:8]], out[j, bad[:8]], exp_pts[bad[:8]])
        total += n
    return total


def _run_case(oracle, letter):
    frames, calls = D.CASES[letter]()
    c = _context(len(frames))
    try:
        cl = _load(oracle, c, frames)
        return [_check_call(oracle, c, cl, call) for call in calls]
    finally:
        c.close()


def test_grid_geometry(oracle):
    """A: ROIs of 2 .. 256 columns and 2 .. 192 rows: one block per ROI (block index / 1), one block per block row, 1- and 2-pixel last blocks,
    exact multiples of the block, ROIs on the right and bottom image borders.  (A block that is never processed shows as a block without
    corners: the per-block counts are compared first.)"""
    totals = _run_case(oracle, "A")
    assert len(totals) == len(D.GRIDS_A) and min(totals[:9]) >= 20


def test_more_blocks_than_one_resident_pass(oracle):
    """B: 33 frames x 192 ROIs of one block = 6336 blocks in one launch, above the 6144 of 8 x 192 workgroups of 4 waves: some workgroups take
    a second step of the stride, and every frame must come out right"""
    (total,) = _run_case(oracle, "B")
    assert total > D.FRAMES_B * D.GRID_B[0] * D.GRID_B[1]


def test_ties(oracle):
    """C: hundreds of equal responses per ROI (order: response desc, raster address desc; plateau maxima are all candidates), min_dist 0
    (k_select's branch without a distance test), 1, 2 and 6, quotas 1, 64 and 80 (clamped to 64), discs of radius 0 .. 3 centred on
    half-pixel ties and ROI corners"""
    totals = _run_case(oracle, "C")
    assert min(totals) > 0


def test_degenerate_content(oracle):
    """D: a constant frame (every ROI's maximum is exactly 0.0: a non-zero key, threshold 0, no candidate), then a textured frame in the
    same context (the per-ROI accumulators were left clean), a frame with flat ROIs among textured ones, one square with a quota above its
    candidates"""
    totals = _run_case(oracle, "D")
    assert totals[0] == 0 and totals[1] > 100 and totals[2] > 0 and 0 < totals[3] < D.GRID_D[5]


def test_subpix_exits(oracle):
    """E: cornerSubPix converging, running into its 20 iterations, stepping out of the ROI through each edge, and moving more than 5 px
    (reset), with the patch clamped at ROI edges that lie inside the image"""
    (total,) = _run_case(oracle, "E")
    assert total > 100


def test_assembly(oracle):
    """F: max_per_job below a job's corners (the block-order prefix is kept), two jobs with different quotas, blocks at 0 and below"""
    totals = _run_case(oracle, "F")
    assert totals[0] == 2 * D.MAX_PER_JOB_F < totals[1]


def test_refused_grids(oracle):
    """G: grids icg_detect_check_grid refuses return ICG_ERR_INVALID and leave the outputs and the context untouched: the production grid of
    this size still equals the oracle afterwards"""
    import icgvins
    frames, _ = D.case_f()
    c = _context(1)
    try:
        cl = _load(oracle, c, frames[:1])
        for name, grid in D.refused_grids().items():
            with pytest.raises(icgvins.IcgError, match=r"icg_detect failed rc=-1:"):
                c.detect([0], grid, [0, 0], D.NO_MASK, D.full_quota(grid), 64)
        c.sync()
        grid = grid_for(D.W, D.H, 40)
        assert grid[0] * grid[2] <= D.W and grid[1] * grid[3] <= D.H
        call = D.Call("G_after_refusals", [0], grid, [D.NO_MASK], [D.full_quota(grid)], 64)
        assert _check_call(oracle, c, cl, call) > 0
    finally:
        c.close()
