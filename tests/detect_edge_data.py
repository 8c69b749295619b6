"""Deterministic detector inputs at the edges of csrc/detect.hip (k_min_eig_nms, k_select, k_subpix and the host assembly of icg_detect),
shared by the CPU test that proves the inputs reach those edges (test_oracle_detect_edges.py) and the GPU parity test
(test_gpu_detect_edges.py): both see identical bytes.

Every case function returns (frames, calls): raw u8 frames of W x H (frame i goes into slot i through preprocess / oracle.clahe like every
other frame) and a list of Call tuples, one icg_detect call each.  A call's job j reads slot slots[j], blanks discs of radius min_dist at
masks[j] and has the per-block quotas quotas[j]."""
from collections import namedtuple

import numpy as np

import lk_edge_data
import synth

W, H = 256, 192
F32 = np.float32

# the block of one wave of k_min_eig_nms (FE_TW x FE_TH * FE_WAVES), its launch cap (8 XCDs x FE_RESIDENT_PER_XCD workgroups of FE_WAVES
# waves: above 8 * 192 * 4 = 6144 blocks a workgroup takes a second step of its stride) and k_select's quota cap, as csrc/detect.hip has them
FE_TW, FE_BH = 60, 64
FE_RESIDENT_PER_XCD, FE_WAVES = 192, 4
BLOCKS_PER_PASS = 8 * FE_RESIDENT_PER_XCD * FE_WAVES
DET_MAX_PER_BLOCK = 64
FE_MAX_RADIUS = 1022

Call = namedtuple("Call", "name slots grid masks quotas max_per_job")
NO_MASK = np.zeros((0, 2), F32)


def rois(grid):
    """(rx, ry, rw, rh) per block, tracking.cc:632-645: every block but the last loses 5 columns and 5 rows"""
    bc, br, bw, bh = grid[:4]
    out = []
    for k in range(bc * br):
        rw, rh = (bw, bh) if k == bc * br - 1 else (bw - 5, bh - 5)
        out.append(((k % bc) * bw, (k // bc) * bh, rw, rh))
    return out


def device_blocks(grid, n_roi):
    """blocks of 60 x 64 that one launch of k_min_eig_nms decodes: gx * gy per ROI (detect_launch's arithmetic)"""
    gx, gy = (grid[2] + FE_TW - 1) // FE_TW, (grid[3] + FE_BH - 1) // FE_BH
    return gx, gy, gx * gy * n_roi


def full_quota(grid, q=None):
    return np.full(grid[0] * grid[1], grid[5] if q is None else q, np.int32)


def expected(oracle, clahe_frames, call):
    """per job (points, block ids) of the oracle; icg_detect clamps a quota to max_per_block, orc_detect takes the quota as it comes"""
    return [oracle.detect(clahe_frames[s], call.grid, call.masks[j], np.minimum(call.quotas[j], call.grid[5]), call.max_per_job)
            for j, s in enumerate(call.slots)]


def _single(name, grid, mask=NO_MASK, quota=None, slot=0, max_per_job=None):
    q = full_quota(grid) if quota is None else np.asarray(quota, np.int32)
    return Call(name, [slot], list(grid), [mask], [q], max_per_job or grid[0] * grid[1] * grid[5])


# ---- A: grid geometry -----------------------------------------------------------------------------------------------------------------
# [cols, rows, bw, bh, min_dist, per]: ROI extents 2, 3 (the smallest legal), 55 / 59, and both sides of the 60-column and 64-row block
# boundaries and of their doubles; (4, 3, 64, 64) touches the right and bottom image borders; (1, 1, 256, 192) is one ROI of 5 x 3 blocks.
# The launch decodes a block index with gx = ceil(bw / 60) and gy = ceil(bh / 64) blocks per ROI: (4, 3, 60, 64), (32, 24, 8, 8) and
# (36, 27, 7, 7) have ONE block per ROI (gx * gy == 1: division by 1 twice), (4, 2, 60, 96) one block per block row (gx == 1, gy == 2),
# (2, 3, 128, 64) one block row (gx == 3, gy == 1)
GRIDS_A = [
    [4, 3, 60, 64, 6, 12], [4, 3, 64, 64, 7, 10], [3, 2, 65, 69, 8, 12], [3, 2, 66, 70, 9, 14], [3, 2, 67, 71, 10, 16], [2, 1, 121, 129, 10, 20],
    [2, 1, 125, 133, 9, 18], [2, 1, 126, 134, 8, 16], [1, 1, 256, 192, 10, 20], [32, 24, 8, 8, 5, 8], [36, 27, 7, 7, 5, 8],
    [4, 2, 60, 96, 7, 12], [2, 3, 128, 64, 8, 14],
]
RW_A = {2, 3, 55, 60, 61, 62, 120, 121}
RH_A = {2, 3, 59, 64, 65, 66, 128, 129}


def case_a():
    return [synth.texture(W, H, seed=200)], [_single("A_%dx%d_%dx%d" % tuple(g[:4]), g) for g in GRIDS_A]


# ---- B: more blocks than one resident pass --------------------------------------------------------------------------------------------
GRID_B = [16, 12, 16, 16, 5, 8]
FRAMES_B = 33


def case_b():
    frames = [synth.texture(W, H, seed=210 + k) for k in range(FRAMES_B)]
    nblk = GRID_B[0] * GRID_B[1]
    return frames, [Call("B_stride", list(range(FRAMES_B)), list(GRID_B), [NO_MASK] * FRAMES_B, [full_quota(GRID_B)] * FRAMES_B, nblk * GRID_B[5])]


# ---- C: ties ----------------------------------------------------------------------------------------------------------------------------
GRID_C = [4, 3, 64, 64]
MIN_DIST_C = (0, 1, 2, 6)
RADII_C = (0, 1, 2, 3)
PATTERNS_C = ("checker8", "crossed", "quilt2")


def checker8(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return (((x // 4 + y // 4) % 2) * 255).astype(np.uint8)


def crossed(w, h):
    """vertical OR horizontal stripes of width 4, period 8"""
    y, x = np.mgrid[0:h, 0:w]
    return ((((x // 4) % 2) | ((y // 4) % 2)) * 255).astype(np.uint8)


def quotas_c():
    """1, 64 and 80 (clamped to max_per_block = 64) in turn over the twelve blocks"""
    return np.array([(1, 64, 80)[k % 3] for k in range(GRID_C[0] * GRID_C[1])], np.int32)


def discs_c():
    """disc centres on the four corners of every ROI, on half-pixel coordinates (rint: half to even, both parities) around the patterns'
    period-8 lattice, and on a coarse lattice that takes out some of the tied maxima of every block"""
    p = []
    for rx, ry, rw, rh in rois(GRID_C + [0, DET_MAX_PER_BLOCK]):
        p += [(rx, ry), (rx + rw - 1, ry), (rx, ry + rh - 1), (rx + rw - 1, ry + rh - 1)]
    p += [(8.0 * i + 0.5, 8.0 * j + 3.5) for i in range(1, 31, 3) for j in range(1, 23, 3)]
    p += [(8.0 * i + 3.5, 8.0 * j + 0.5) for i in range(2, 31, 3) for j in range(2, 23, 3)]
    p += [(8.0 * i - 0.5, 8.0 * j - 0.5) for i in range(3, 31, 3) for j in range(3, 23, 3)]
    p += [(4.0 * i, 4.0 * j) for i in range(1, 63, 5) for j in range(1, 47, 4)]
    return np.array(p, F32)


def case_c():
    """the three binary patterns as the three jobs of every call: without a mask at min_dist 0, 1, 2, 6 and with the discs of discs_c at
    radius (= min_dist) 0, 1, 2, 3"""
    frames = [checker8(W, H), crossed(W, H), lk_edge_data.quilt(W, H)]
    calls = []
    for masked, dists in ((False, MIN_DIST_C), (True, RADII_C)):
        for md in dists:
            grid = GRID_C + [md, DET_MAX_PER_BLOCK]
            m = discs_c() if masked else NO_MASK
            calls.append(Call("C_%s_md%d" % ("discs" if masked else "plain", md), [0, 1, 2], grid, [m] * 3, [quotas_c()] * 3,
                              GRID_C[0] * GRID_C[1] * DET_MAX_PER_BLOCK))
    return frames, calls


# ---- D: degenerate content --------------------------------------------------------------------------------------------------------------
GRID_D = [4, 3, 64, 64, 6, 20]
FLAT_RECTS_D = ((0, 0, 128, 128), (150, 100, W, H))  # x0, y0, x1, y1 of the constant parts of the partly flat frame
FLAT_BLOCKS_D = (0, 11)          # blocks whose ROI lies more than two CLAHE tiles (13 x 10 px) inside a constant part: flat after CLAHE too
TEXTURED_BLOCKS_D = (2, 3, 8, 9)  # blocks without a constant pixel
SQUARE_D = (6, 150, 90, 7)         # block, x, y, side of the single bright square


def case_d():
    """frame 0 constant, frame 1 textured (detected AFTER the constant frame in the same context), frame 2 textured in some blocks and
    constant in the others (CLAHE blends texture about a tile and a half into a constant part: the ROIs of blocks 0 and 11 stay flat, the
    other ROIs that touch a constant part fade out inside it), frame 3 one bright square"""
    const = np.full((H, W), 77, np.uint8)
    tex = synth.texture(W, H, seed=220)
    part = synth.texture(W, H, seed=221)
    for x0, y0, x1, y1 in FLAT_RECTS_D:
        part[y0:y1, x0:x1] = 60
    square = np.full((H, W), 50, np.uint8)
    _, x, y, s = SQUARE_D
    square[y:y + s, x:x + s] = 200
    calls = [_single("D_constant", GRID_D, slot=0), _single("D_texture_after_constant", GRID_D, slot=1), _single("D_partly_flat", GRID_D, slot=2),
             _single("D_one_square", GRID_D, slot=3)]
    return [const, tex, part, square], calls


# ---- E: sub-pixel exits -------------------------------------------------------------------------------------------------------------------
GRID_E = [4, 3, 64, 64, 6, 20]
ROIS_E = (5, 6)  # the two blocks whose ROI has all four edges inside the image
WEDGES_E = ((4, 0.5), (4, 0.7), (2, 0.4), (1, 0.3))  # (apex distance outside the ROI edge, half-width per pixel of length)
SHAPE_SEEDS_E = (1, 4, 5, 7)


def _wedge(img, ax, ay, direction, half_slope, length, v):
    """filled wedge with its apex at (ax, ay), opening along the unit axis `direction`"""
    y, x = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    dx, dy = direction
    t = (x - ax) * dx + (y - ay) * dy
    s = (x - ax) * (-dy) + (y - ay) * dx
    img[(t >= 0) & (t <= length) & (np.abs(s) <= half_slope * t)] = v


def wedge_frame(off, half_slope):
    """on a flat frame, one wedge per ROI edge whose apex lies `off` px OUTSIDE that edge: the two visible edges meet outside the ROI, which is
    where cornerSubPix steps to"""
    img = np.full((H, W), 90, np.uint8)
    R = rois(GRID_E)
    for k in ROIS_E:
        rx, ry, rw, rh = R[k]
        _wedge(img, rx - off, ry + 15, (1, 0), half_slope, 25, 220)
        _wedge(img, rx + rw - 1 + off, ry + 40, (-1, 0), half_slope, 25, 20)
        _wedge(img, rx + 20, ry - off, (0, 1), half_slope, 20, 220)
        _wedge(img, rx + 45, ry + rh - 1 + off, (0, -1), half_slope, 20, 20)
    return img


def shape_frame(seed):
    """on a dimmed texture, filled rectangles with a side 1 .. 6 px inside each of the four ROI edges and an L shape near the bottom right
    corner (the distances are a seeded permutation of 1 .. 6)"""
    rng = np.random.RandomState(seed)
    img = (synth.texture(W, H, seed=seed) // 3 + 40).astype(np.uint8)
    R = rois(GRID_E)
    for k in ROIS_E:
        rx, ry, rw, rh = R[k]
        ds = rng.permutation(6) + 1
        v = int(rng.choice([200, 230, 20, 0]))
        img[ry + 8:ry + 16, rx + ds[0]:rx + ds[0] + 9] = v
        img[ry + ds[1]:ry + ds[1] + 7, rx + 24:rx + 36] = v
        img[ry + 30:ry + 40, rx + rw - 1 - ds[2] - 8:rx + rw - ds[2]] = v
        img[ry + rh - 1 - ds[3] - 6:ry + rh - ds[3], rx + 10:rx + 22] = v
        x0, y0 = rx + rw - 1 - ds[4] - 10, ry + rh - 1 - ds[5] - 10
        img[y0:y0 + 11, x0 + 7:x0 + 11] = 255 - v
        img[y0 + 7:y0 + 11, x0:x0 + 11] = 255 - v
    return img


def case_e():
    frames = [wedge_frame(*p) for p in WEDGES_E] + [shape_frame(s) for s in SHAPE_SEEDS_E]
    n = len(frames)
    return frames, [Call("E_subpix", list(range(n)), list(GRID_E), [NO_MASK] * n, [full_quota(GRID_E)] * n, 12 * GRID_E[5])]


# ---- F: assembly --------------------------------------------------------------------------------------------------------------------------
GRID_F = [4, 3, 64, 64, 8, 10]
MAX_PER_JOB_F = 40


def case_f():
    """two jobs in one call: every block at the full quota / quotas from -3 to 10 with blocks at 0 and below; max_per_job below either
    job's total, so that the assembly keeps the block-order prefix"""
    frames = [synth.texture(W, H, seed=230), synth.texture(W, H, seed=231)]
    q1 = np.array([3, 0, 10, -3, 1, 10, 0, 7, -1, 2, 10, 5], np.int32)
    return frames, [Call("F_truncated", [0, 1], list(GRID_F), [NO_MASK, NO_MASK], [full_quota(GRID_F), q1], MAX_PER_JOB_F),
                    Call("F_whole", [1, 0], list(GRID_F), [NO_MASK, NO_MASK], [q1, full_quota(GRID_F)], 12 * GRID_F[5])]


# ---- G: refused grids -----------------------------------------------------------------------------------------------------------------------
def refused_grids():
    return {"block_w_6": [4, 3, 6, 64, 6, 10], "max_per_block_65": [4, 3, 64, 64, 6, DET_MAX_PER_BLOCK + 1],
            "min_dist_1023": [4, 3, 64, 64, FE_MAX_RADIUS + 1, 10], "cols_x_bw_above_width": [5, 3, 52, 64, 6, 10]}


CASES = {"A": case_a, "B": case_b, "C": case_c, "D": case_d, "E": case_e, "F": case_f}
