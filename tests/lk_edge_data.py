"""Deterministic LK inputs at the edges of k_lk_track_fb's arithmetic (csrc/lk.hip), shared by the CPU test that proves the inputs reach those
edges (test_oracle_lk_edges.py) and the GPU parity test (test_gpu_lk_edges.py): both see identical bytes.

Every case function returns a list of sub-cases (name, w, h, img_a, img_b, prev_pts, guess): raw u8 images (they go through preprocess /
oracle.clahe like every other frame) and float32 (n, 2) points.  Every coordinate is finite and |coord| <= 1e6: non-finite or int-overflowing
coordinates are undefined in the reference and must not be sent to the GPU."""
import numpy as np

import synth

F32 = np.float32
SHIFT = (1.3, -0.7)


def _pts(*parts):
    return np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in parts]).astype(F32)


def _roll(img, dx, dy):
    return np.roll(img, (dy, dx), axis=(0, 1))


# ---- A: saturated contrast ------------------------------------------------------------------------------------------------------------
def stripes(w, h):
    """vertical stripes of width 2 (period 4): |Ix| at its maximum at every pixel, Iy = 0"""
    return np.tile(((np.arange(w) // 2) % 2 * 255).astype(np.uint8), (h, 1))


def checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return (((x // 2 + y // 2) % 2) * 255).astype(np.uint8)


def quilt(w, h, patch=32):
    """patches alternating vertical and horizontal width-2 stripes: windows across a seam have both A11 and A22 saturated"""
    y, x = np.mgrid[0:h, 0:w]
    vertical = ((x // patch + y // patch) % 2) == 0
    return (np.where(vertical, (x // 2) % 2, (y // 2) % 2) * 255).astype(np.uint8)


def blocks(w, h, seed):
    rng = np.random.RandomState(seed)
    b = rng.randint(0, 2, ((h + 1) // 2, (w + 1) // 2)).astype(np.uint8) * 255
    return np.repeat(np.repeat(b, 2, 0), 2, 1)[:h, :w].copy()


def noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)


def case_a():
    w, h = 320, 240
    patterns = [("stripes", stripes(w, h)), ("checker", checker(w, h)), ("quilt", quilt(w, h)), ("blocks", blocks(w, h, 101)),
                ("noise", noise(w, h, 102))]
    # on the quilt's patch seams and 4 px to either side of them (a window two thirds in one patch: one window sum saturated, the other large)
    seams = [(32.0 * i + dx, 32.0 * j + dy) for i in range(1, 10, 2) for j in range(1, 7, 2)
             for dx, dy in ((0.0, 16.0), (16.0, 0.0), (0.25, -0.5), (-4.0, 16.0), (4.0, 16.0), (16.0, -4.0), (16.0, 4.0))]
    out = []
    for k, (name, img) in enumerate(patterns):
        moves = [("roll2_0", _roll(img, 2, 0), (2.0, 0.0)), ("roll1_2", _roll(img, 1, 2), (1.0, 2.0)),
                 ("shift", synth.shift_image(img, *SHIFT), SHIFT)]
        for m, (mname, nxt, d) in enumerate(moves):
            pts = _pts(synth.random_points(150, w, h, 0, seed=110 + 3 * k + m), seams)
            guess = (pts + F32(0.8) * np.array(d, F32)).astype(F32)
            out.append((f"A_{name}_{mname}", w, h, img, nxt, pts, guess))
    return out


# ---- B: small and odd pyramids --------------------------------------------------------------------------------------------------------
SIZES_B = [(333, 257), (176, 178), (160, 121), (87, 45), (45, 47), (32, 32)]
LEVELS_B = [4, 4, 3, 2, 2, 1]
INSIDE_B = (0.5, 5.0, 10.0, 10.5, 11.0, 21.5)


def border_points(w, h):
    """the four corners, the edge midpoints, points 0.5 .. 21.5 px inside each border, and two points whose window has left the image"""
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    p = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (cx, 0), (cx, h - 1), (0, cy), (w - 1, cy)]
    for d in INSIDE_B:
        p += [(d, cy), (w - 1 - d, cy), (cx, d), (cx, h - 1 - d)]
    p += [(-12.0, cy), (cx, h + 10.5)]
    return p


def case_b():
    out = []
    for k, (w, h) in enumerate(SIZES_B):
        img = synth.texture(w, h, seed=120 + k)
        nxt = synth.shift_image(img, *SHIFT)
        pts = _pts(synth.random_points(100, w, h, 0, seed=130 + k), border_points(w, h))
        guess = (pts + F32(0.8) * np.array(SHIFT, F32)).astype(F32)
        out.append((f"B_{w}x{h}", w, h, img, nxt, pts, guess))
    return out


# ---- C: positions ---------------------------------------------------------------------------------------------------------------------
OUTSIDE_C = (12.0, 22.0, 60.0, 400.0)
MOVE_C = (-6.3, 3.7)


def case_c_classes(w=320, h=240):
    """name -> (prev, guess offset or absolute guess) per coordinate class; see case_c"""
    anchors = [(40.0 + 48.0 * i, 36.0 + 42.0 * j) for i in range(6) for j in range(5)]
    below = lambda v: np.nextafter(F32(v + 1), F32(0))
    cls = {}
    cls["integer"] = _pts(anchors)
    cls["half"] = _pts(anchors) + F32(0.5)
    cls["below_integer"] = np.array([[below(x), below(y)] for x, y in anchors], F32)
    # 2^-15 and 2^-20 above an integer; 2^-20 is representable in float32 up to 16 (the window origin is the coordinate minus 10)
    cls["tiny_fraction"] = _pts([(x + 2.0 ** -15, y + 2.0 ** -15) for x, y in anchors[:10]],
                                [(10 + 2.0 ** -20, 12 + 2.0 ** -20), (12 + 2.0 ** -20, 50.0), (60.0, 10 + 2.0 ** -20), (3 + 2.0 ** -20, 15 + 2.0 ** -20),
                                 (2.0 ** -20, 100.0), (150.0, 2.0 ** -20), (2.0 ** -15, 2.0 ** -15), (11 + 2.0 ** -20, 13 + 2.0 ** -15)])
    cls["negative"] = _pts([(-0.5, 60.0), (-3.25, 120.0), (-10.9, 100.0), (-10.999, 30.0), (70.0, -0.5), (160.0, -7.5), (250.0, -10.75),
                            (-2.0, -2.0), (-10.5, -10.5), (-6.0, 200.0)])
    outside = []
    for d in OUTSIDE_C:
        outside += [(-d, 120.0), (w - 1 + d, 100.0), (140.0, -d), (180.0, h - 1 + d), (-d, -d), (w - 1 + d, h - 1 + d)]
    cls["prev_outside"] = _pts(outside)
    return cls


def case_c():
    """One texture pair (the second frame moved by MOVE_C, so that tracks near the left and bottom borders are pulled out of the image).
    Sub-case 'classes': every coordinate class as prev with the guess at prev + 0.8 * move, and the same classes as the guess of an interior
    prev.  Sub-case 'guess_outside': interior prev, guesses outside the image by OUTSIDE_C.  Sub-case 'pulled_out': guesses that start inside
    (the first window is valid) on tracks that lead out."""
    w, h = 320, 240
    img = synth.texture(w, h, seed=140)
    nxt = synth.shift_image(img, *MOVE_C)
    mv = np.array(MOVE_C, F32)
    cls = case_c_classes(w, h)
    prev = np.concatenate(list(cls.values()))
    guess = (prev + F32(0.8) * mv).astype(F32)
    # the exact-coordinate classes once more as the guess itself (prev = the guess minus the move, rounded: an ordinary interior point)
    exact = np.concatenate([cls[k] for k in ("integer", "half", "below_integer", "tiny_fraction")])
    prev2 = np.clip(exact - mv, 12, None).astype(F32)
    out = [("C_classes", w, h, img, nxt, np.concatenate([prev, prev2]), np.concatenate([guess, exact]))]
    inner = _pts([(60.0 + 40.0 * (i % 6), 50.0 + 35.0 * (i // 6)) for i in range(24)])
    off = []
    for d in OUTSIDE_C:
        off += [(-d, 120.0), (w - 1 + d, 100.0), (140.0, -d), (180.0, h - 1 + d), (-d, -d), (w - 1 + d, h - 1 + d)]
    out.append(("C_guess_outside", w, h, img, nxt, inner, _pts(off)))
    # prev with its window still (partly) inside, near the left / bottom border; the move leads further out
    rng = np.random.RandomState(141)
    left = np.stack([rng.uniform(-10.9, -4.0, 40), rng.uniform(20, h - 20, 40)], 1)
    bottom = np.stack([rng.uniform(20, w - 20, 40), rng.uniform(h + 3.0, h + 9.9, 40)], 1)
    pull = _pts(left, bottom)
    out.append(("C_pulled_out", w, h, img, nxt, pull, pull.copy()))
    return out


# ---- D: long travel inside a level ----------------------------------------------------------------------------------------------------
def smooth(w, h, seed, octave=64, amp=230.0):
    """synth.texture's coarsest octave alone (bilinear value noise on a 64-px lattice), no blobs: one basin of attraction tens of pixels wide"""
    rng = np.random.RandomState(seed)
    g = rng.rand(h // octave + 3, w // octave + 3)
    ys, xs = np.arange(h) / octave, np.arange(w) / octave
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    v = (g[y0][:, x0] * (1 - fx) + g[y0][:, x0 + 1] * fx) * (1 - fy) + (g[y0 + 1][:, x0] * (1 - fx) + g[y0 + 1][:, x0 + 1] * fx) * fy
    return np.clip(amp * v + 10.0, 0, 255).astype(np.uint8)


def case_d():
    w, h = 320, 240
    out = []
    for k, move in enumerate([(9.0, -11.5), (-13.25, 10.0), (14.0, 12.5)]):
        img = smooth(w, h, seed=150 + k)
        nxt = synth.shift_image(img, *move)
        pts = synth.random_points(120, w, h, 40, seed=153 + k)
        rng = np.random.RandomState(156 + k)
        ang, rad = rng.uniform(0, 2 * np.pi, len(pts)), rng.uniform(24, 60, len(pts))
        guess = (pts + np.array(move, F32) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)).astype(F32)
        out.append((f"D_move{k}", w, h, img, nxt, pts, guess))
    return out


# ---- E: weak texture ------------------------------------------------------------------------------------------------------------------
AMPS_E = (1, 2, 3, 4, 6, 8, 12, 16)
BLOB_E = (150, 110, 3)  # x, y, side


def blob_image(w, h, amp, base=120):
    img = np.full((h, w), base, np.uint8)
    x, y, s = BLOB_E
    img[y:y + s, x:x + s] += amp
    return img


def blob_points():
    """points 0..5 sit on the blob (its corners, its centre, one edge midpoint); the rest step away from it until the window holds no blob"""
    x, y, s = BLOB_E
    on = [(x, y), (x + s - 1, y), (x, y + s - 1), (x + s - 1, y + s - 1), (x + s / 2.0, y + s / 2.0), (x + s / 2.0, y)]
    beside = [(x + s / 2.0 + d, y + s / 2.0 + e) for d in (-24.0, -14.5, -9.0, 9.0, 14.5, 24.0) for e in (-13.0, 0.0, 13.0)]
    return _pts(on, beside)


def case_e():
    w, h = 320, 240
    const = np.full((h, w), 77, np.uint8)
    pts = synth.random_points(60, w, h, 0, seed=160)
    out = [("E_constant", w, h, const, const.copy(), pts, (pts + F32(0.5)).astype(F32))]
    for amp in AMPS_E:
        img = blob_image(w, h, amp)
        p = blob_points()
        out.append((f"E_blob{amp}", w, h, img, synth.shift_image(img, *SHIFT), p, (p + F32(0.8) * np.array(SHIFT, F32)).astype(F32)))
    return out


# ---- F: counts ------------------------------------------------------------------------------------------------------------------------
COUNTS_F = (1, 63, 64, 65, 1023, 1024, 1025, 2500)
FLAT_F = (420, 0, 640, 190)  # x0, y0, x1, y1 of a flat region of the image


def case_f():
    """n points (every prefix of one pool) on one 640x480 pair; about a third are lost on purpose: a sixth lie in a flat region (weak), a sixth
    within 5 px of the image border (culled by the forward/backward track), in an order that mixes them into every prefix"""
    w, h = 640, 480
    img = synth.texture(w, h, seed=170)
    x0, y0, x1, y1 = FLAT_F
    img[y0:y1, x0:x1] = 90
    nxt = synth.shift_image(img, 2.4, -1.6)
    n = max(COUNTS_F)
    rng = np.random.RandomState(171)
    good = np.stack([rng.uniform(15, x0 - 20, n), rng.uniform(15, h - 15, n)], 1)
    flat = np.stack([rng.uniform(x0 + 25, x1 - 25, n), rng.uniform(y0 + 25, y1 - 25, n)], 1)
    edge = np.stack([rng.uniform(0, 4.5, n), rng.uniform(0, h - 1, n)], 1)
    edge[::2] = np.stack([rng.uniform(0, x0, n), rng.uniform(h - 4.5, h - 1, n)], 1)[::2]
    kind = rng.randint(0, 6, n)
    pool = np.where((kind == 0)[:, None], flat, np.where((kind == 1)[:, None], edge, good)).astype(F32)
    guess = (pool + np.array([2.0, -1.25], F32)).astype(F32)
    return [(f"F_n{k}", w, h, img, nxt, pool[:k].copy(), guess[:k].copy()) for k in COUNTS_F]


CASES = {"A": case_a, "B": case_b, "C": case_c, "D": case_d, "E": case_e, "F": case_f}
