"""Inputs for the preprocessing kernels (csrc/image.hip) at their clip, rounding, strip and tile-shape edges, with the three things the tests
need that do not come from the code under test:

  * clahe_numpy / pyrdown_numpy: a vectorised numpy restatement of SURVEY.md B.2 / B.3, float32 operation by operation, with OpenCV's padding
    rule (both dimensions are padded iff either is not a multiple of 21);
  * tile_shapes / apply_forms / pyr_steps: a Python mirror of the launch geometry (which path of k_clahe_lut a tile takes, which form of
    k_clahe_apply a chunk takes, which strips of k_pyrdown_rows reflect columns, how a level is cut into bands);
  * deterministic content builders (texture, planted clip excesses, flat images, stripes).

tests/test_oracle_preprocess_edges.py pins the oracle to the restatement at every case and asserts, from the restatement and the mirror alone,
that the cases reach the edges they are named for; tests/test_gpu_preprocess_edges.py compares the kernels with the oracle at the same cases."""
import numpy as np

import synth
from test_gpu_clahe_rows import T, geometry, pairs_per_chunk, row_terms

F32 = np.float32
MAX_LEVELS, LK_WIN = 4, 21  # ICG_MAX_LEVELS, ICG_LK_WIN
STRIP_OUT = 128             # PR_STRIP_OUT
FCOLS, ROWS = 8, 128        # CLAHE_FCOLS, CLAHE_ROWS


def _reflect(idx, n):
    idx = np.abs(idx)
    return np.where(idx >= n, 2 * (n - 1) - idx, idx)


def padded_geometry(w, h):
    """(tw, th, padded) under OpenCV's rule; the same numbers as test_gpu_clahe_rows.geometry, which mirrors the host code"""
    padded = bool(w % T or h % T)
    ew, eh = (w + (T - w % T), h + (T - h % T)) if padded else (w, h)
    assert (ew // T, eh // T) == geometry(w, h)
    return ew // T, eh // T, padded


def clip_limit(tw, th):
    return max(1, int(3.0 * (tw * th) / 256))


# ----------------------------------------------------------------------------------------------------------------------------------------
# restatements
def clahe_numpy(img):
    """-> (out_u8, res_f32, luts[T, T, 256], per_tile_info); per_tile_info = dict(clipped, batch, residual: [T*T] and hist: [T*T, 256], the
    tile histograms BEFORE clipping and redistribution, clip, scaled: the float32 products cdf * lut_scale the LUT bytes are rounded from)"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    tw, th, padded = padded_geometry(w, h)
    ext = img[_reflect(np.arange(T * th), h)][:, _reflect(np.arange(T * tw), w)] if padded else img
    area = tw * th
    clip = clip_limit(tw, th)
    scale = F32(255.0) / F32(area)
    tile_id = (np.arange(T * th) // th)[:, None] * T + (np.arange(T * tw) // tw)[None, :]
    raw = np.bincount((tile_id * 256 + ext).ravel(), minlength=T * T * 256).reshape(T * T, 256).astype(np.int64)
    clipped = np.maximum(raw - clip, 0).sum(1)
    batch, residual = clipped // 256, clipped % 256
    hist = np.minimum(raw, clip) + batch[:, None]
    for k in np.nonzero(residual)[0]:
        step = max(256 // int(residual[k]), 1)
        hist[k, np.arange(0, 256, step)[:residual[k]]] += 1
    assert np.all(hist.sum(1) == area)
    scaled = np.cumsum(hist, 1).astype(F32) * scale
    luts = np.clip(np.rint(scaled), 0, 255).astype(np.uint8).reshape(T, T, 256)

    def axis(n, t):
        f = np.arange(n, dtype=F32) * (F32(1.0) / F32(t)) - F32(0.5)
        i1 = np.floor(f).astype(np.int64)
        a = (f - i1.astype(F32)).astype(F32)
        return np.maximum(i1, 0), np.minimum(i1 + 1, T - 1), a, F32(1) - a

    tx1, tx2, xa, xa1 = axis(w, tw)
    ty1, ty2, ya, ya1 = axis(h, th)
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    l11, l12 = luts[Y1, X1, img].astype(F32), luts[Y1, X2, img].astype(F32)
    l21, l22 = luts[Y2, X1, img].astype(F32), luts[Y2, X2, img].astype(F32)
    res = (l11 * xa1[None, :] + l12 * xa[None, :]) * ya1[:, None] + (l21 * xa1[None, :] + l22 * xa[None, :]) * ya[:, None]
    assert res.dtype == F32
    out = np.clip(np.rint(res), 0, 255).astype(np.uint8)
    info = dict(clipped=clipped, batch=batch, residual=residual, hist=raw, clip=clip, scaled=scaled)
    return out, res, luts, info


def _pyr_taps(n):
    return _reflect(2 * np.arange((n + 1) // 2)[:, None] + np.arange(-2, 3)[None, :], n)


def pyrdown_sums(img):
    """the unrounded 5 x 5 sums (256 x the weighted mean), exact integers"""
    k = np.array([1, 4, 6, 4, 1], np.int64)
    h, w = img.shape
    tmp = (img.astype(np.int64)[:, _pyr_taps(w)] * k).sum(-1)
    return (tmp[_pyr_taps(h), :] * k[None, :, None]).sum(1)


def pyrdown_numpy(img):
    return ((pyrdown_sums(img) + 128) >> 8).astype(np.uint8)


def level_sizes(w, h):
    out = [(w, h)]
    while len(out) < MAX_LEVELS:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= LK_WIN or h <= LK_WIN:
            break
        out.append((w, h))
    return out


def pyramid_numpy(level0):
    out = [level0]
    for _ in level_sizes(level0.shape[1], level0.shape[0])[1:]:
        out.append(pyrdown_numpy(out[-1]))
    return out


def saturated_windows(level0):
    """where level 0 holds a 5 x 5 all-255 window (reflect-101) centred on an even (x, y): the set of {"interior", "left", "right", "top",
    "bottom"} positions at which one occurs.  Such a window is the only one that drives k_pyrdown_rows' packed 16-bit sums to their maximum."""
    h, w = level0.shape
    m = level0 == 255
    full = m[:, _pyr_taps(w)].all(-1)[_pyr_taps(h), :].all(1)  # dh x dw
    ys, xs = np.nonzero(full)
    cx, cy = 2 * xs, 2 * ys
    where = set()
    left, right, top, bottom = cx < 2, cx + 2 > w - 1, cy < 2, cy + 2 > h - 1
    for name, sel in (("left", left), ("right", right), ("top", top), ("bottom", bottom), ("interior", ~(left | right | top | bottom))):
        if sel.any():
            where.add(name)
    return where


# ----------------------------------------------------------------------------------------------------------------------------------------
# launch geometry
def tile_shapes(w, h):
    """per tile of k_clahe_lut, as the kernel derives them: ndw, nin, the x_begin & 3 phase, fast, and why not"""
    tw, th, _ = padded_geometry(w, h)
    out = []
    for ty in range(T):
        for tx in range(T):
            x_begin, x_end, y_begin = tx * tw, tx * tw + tw, ty * th
            xa = x_begin & ~3
            ndw = (((x_end + 3) & ~3) - xa) >> 2
            nin = ndw - 2
            why = set()
            if nin < 1:
                why.add("nin<1")
            if nin > 16:
                why.add("nin>16")
            if y_begin + th > h:
                why.add("bottom")
            if xa + 4 * ndw > w:
                why.add("right")
            out.append(dict(ndw=ndw, nin=nin, phase=x_begin & 3, fast=not why, why=frozenset(why)))
    return out


def apply_forms(w, h):
    """the <FLT, TAB> form of k_clahe_apply every 256-pixel chunk takes"""
    tw, th, _ = padded_geometry(w, h)
    tab = th + 5 <= ROWS
    forms = []
    for n in pairs_per_chunk(w, tw):
        if n < FCOLS and tab:
            forms.append((True, True))
        elif n <= FCOLS:
            forms.append((True, False))
        else:
            forms.append((False, tab))
    return forms


def strip_rows_fit(w, h):
    """the candidate rows of every strip of k_clahe_apply partition the image (what test_gpu_clahe_rows asserts for its own sizes)"""
    _, th, _ = padded_geometry(w, h)
    _, tyr = row_terms(h, th)
    taken = np.zeros(h, np.int32)
    for strip in range(T + 1):
        y_lo, y_hi = max((strip - 1) * th + th // 2 - 2, 0), min(strip * th + th // 2 + 3, h)
        if y_hi > y_lo:
            ys = np.arange(y_lo, y_hi)
            taken[ys[tyr[ys] == strip - 1]] += 1
    return bool(np.all(taken == 1))


def pyr_steps(w, h):
    """per pyrDown step: source and destination size, n_strips, the edge flag of every strip, band_rows, and whether the last band is partial"""
    sizes = level_sizes(w, h)
    out = []
    for level, ((sw, sh), (dw, dh)) in enumerate(zip(sizes[:-1], sizes[1:])):
        n_strips = (dw + STRIP_OUT - 1) // STRIP_OUT
        edge = [s == 0 or 2 * (s + 1) * STRIP_OUT + 4 > sw for s in range(n_strips)]
        # what the predicate stands for: some output column of the strip has a tap 2 x - 2 .. 2 x + 2 outside the source row
        needs = [s == 0 or 2 * (min((s + 1) * STRIP_OUT, dw) - 1) + 2 > sw - 1 for s in range(n_strips)]
        band_rows = 32 if dh >= 256 else 16 if dh >= 128 else 8
        out.append(dict(level=level, sw=sw, sh=sh, dw=dw, dh=dh, n_strips=n_strips, edge=edge, needs=needs, band_rows=band_rows,
                        partial=dh % band_rows != 0))
    return out


# ----------------------------------------------------------------------------------------------------------------------------------------
# contents
def planted(w, h, targets, seed=0):
    """tile k (row-major) is filled so that exactly one bin, value (7 k) % 256, exceeds the clip limit, by targets[k % len(targets)]; the other
    pixels are spread over the other values with at most `clip` each, and the pixels are shuffled inside the tile.  Tiles that reach into
    the padding are filled inside the image only (their histogram then also counts reflected pixels: the restatement reports what was reached)."""
    tw, th, _ = padded_geometry(w, h)
    clip = clip_limit(tw, th)
    rng = np.random.RandomState(seed)
    img = np.zeros((h, w), np.uint8)
    for k in range(T * T):
        ty, tx = divmod(k, T)
        y0, x0 = ty * th, tx * tw
        y1, x1 = min(y0 + th, h), min(x0 + tw, w)
        n = max(y1 - y0, 0) * max(x1 - x0, 0)
        if n == 0:
            continue
        heavy = (7 * k) % 256
        n_heavy = min(clip + targets[k % len(targets)], n)
        rest = n - n_heavy
        assert rest <= 255 * clip, (w, h, k)
        others = (heavy + 1 + np.arange(255)) % 256
        counts = rest // 255 + (np.arange(255) < rest % 255)
        vals = np.concatenate([np.full(n_heavy, heavy), np.repeat(others, counts)]).astype(np.uint8)
        img[y0:y1, x0:x1] = rng.permutation(vals).reshape(y1 - y0, x1 - x0)
    return img


def _stripes(kind, w, h):
    y, x = np.mgrid[0:h, 0:w]
    on = {"cols": x % 2 == 0, "rows": y % 2 == 0, "checker": (x // 2 + y // 2) % 2 == 0, "halves": x >= w // 2}[kind]
    return np.where(on, 255, 0).astype(np.uint8)


EXTREMES = ("flat0", "flat255", "flat100", "cols", "rows", "checker", "halves")
STRIPES = EXTREMES[3:]

# planted excesses per size (tile area, clip): the first two lists are the ones the cases are named for; the others put the same boundary
# residuals through padded, tiny and thin tiles.  Lists without a 0 leave every tile with its heavy bin over the limit.
PLANTED = {
    (672, 336): (0, 1, 2, 3, 85, 86, 127, 128, 129, 255, 256, 257, 506),
    (651, 483): (0, 1, 128, 255, 256, 511, 512, 513, 705),
    (640, 480): (1, 2, 3, 85, 86, 127, 128, 129, 255, 256, 300, 512, 700),
    (630, 357): (1, 2, 3, 85, 86, 127, 128, 129, 255, 256, 257, 500),
}
PLANTED_DEFAULT = (1, 2, 3, 85, 86, 127, 128, 129, 255, 256, 257)


def make(w, h, content):
    if content == "texture":
        return synth.texture(w, h, seed=1300 + w + h)
    if content == "planted":
        return planted(w, h, PLANTED.get((w, h), PLANTED_DEFAULT), seed=w + h)
    if content.startswith("flat"):
        return np.full((h, w), int(content[4:]), np.uint8)
    return _stripes(content, w, h)


CLAHE_FULL = [(672, 336), (651, 483), (640, 480), (630, 357), (672, 100), (100, 336), (1512, 42), (1533, 42),
              (42, 42), (63, 63), (84, 84), (105, 105), (189, 63)]
CLAHE_TALL = [(256, 2604), (1000, 2604)]
# (the predicate flips between source widths 515 and 516; what it stands for, a reflected tap in strip 1, flips between 512 and 513: 512 and
# 1024, whose level 1 is 512 wide, are the widths at which a strip that is not the first is full AND reflects)
PYR_SIZES = [(513, 90), (515, 90), (516, 90), (517, 90), (518, 90), (519, 90), (1031, 90), (1032, 90), (1029, 90),
             (64, 253), (64, 254), (64, 256), (64, 258), (64, 509), (64, 510), (64, 512), (64, 514), (512, 90), (1024, 90)]

CASES = [(w, h, c) for w, h in CLAHE_FULL for c in ("texture", "planted") + EXTREMES] + \
        [(w, h, c) for w, h in CLAHE_TALL for c in ("texture",) + STRIPES] + \
        [(w, h, c) for w, h in PYR_SIZES for c in ("texture", "flat255") + STRIPES]
SIZES = CLAHE_FULL + CLAHE_TALL + PYR_SIZES


def case_id(case):
    return f"{case[0]}x{case[1]}-{case[2]}"


# ----------------------------------------------------------------------------------------------------------------------------------------
# what a case reaches, from the restatement alone (small numbers only: the images are not kept)
_SUMMARY = {}


def _ties(x):
    """(number of exact k + 0.5 values with k even, with k odd)"""
    k = np.floor(x)
    tie = (x - k) == F32(0.5)
    even = (k.astype(np.int64) % 2) == 0
    return int(np.sum(tie & even)), int(np.sum(tie & ~even))


def restate(case):
    """-> (img, luts, levels): the restatement's LUTs and every pyramid level of the case; its summary is recorded on the way"""
    w, h, content = case
    img = make(w, h, content)
    out, res, luts, info = clahe_numpy(img)
    levels = pyramid_numpy(out)
    if case not in _SUMMARY:
        over = info["hist"] > info["clip"]
        single = np.nonzero(over.sum(1) == 1)[0]
        _SUMMARY[case] = dict(
            pairs=set(zip(info["batch"].tolist(), info["residual"].tolist())),
            unclipped=bool(np.any(info["clipped"] == 0)),
            bin_at_clip=bool(np.any(info["hist"] == info["clip"])), bin_over_by_one=bool(np.any(info["hist"] == info["clip"] + 1)),
            lone_bins=set(np.argmax(over[single], 1).tolist()),
            lut_ties=_ties(info["scaled"]), apply_ties=_ties(res), res_max=float(res.max()), res_min=float(res.min()),
            saturated=saturated_windows(out))
    return img, luts, levels


def summary(case):
    if case not in _SUMMARY:
        restate(case)
    return _SUMMARY[case]
