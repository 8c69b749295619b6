"""GPU parity of k_fm_ransac_sets (csrc/ransac.hip) with the CPU oracle at the structural edges of its round schedule: the kernel draws,
solves and scores the hypothesis stream in rounds of 8, 8, 16, 32, 32 ... and discards what lies past the updated iteration bound, so the
masks must be the sequential algorithm's bit for bit wherever the consumed count (the oracle's `iters`) falls: on 1, on either side of every
round's size and of every round boundary, in the hundreds, and at the 1000 cap without a model.  Set sizes 15, 64, 65 and 300 (the 64-point
inlier words), sets above 1024 points (the LARGE form of the kernel, which small sets of the same call run too), and the lattice set of
test_gpu_geometry.py whose subsets are redrawn.  Every set was picked on the CPU by its oracle `iters`; the test asserts that count, so a
change of the schedule cannot empty it silently."""
import os
import re

import numpy as np
import pytest

from test_oracle_geometry import two_view

pytestmark = pytest.mark.gpu

ROUNDS = (8, 8, 16, 32)  # fm_round_size(0 .. 3) of csrc/ransac.hip; FM_HPW from there on


def _edges():
    e = {1}
    total = 0
    for r in ROUNDS:
        e |= {r - 1, r, r + 1}
        total += r
        e |= {total - 1, total, total + 1}
    return e


EDGES = _edges()  # 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65

# (oracle iters, seed, points, outlier fraction, noise) of two_view
SMALL = [
    (1, 101, 15, 0.0, 0.1), (1, 104, 64, 0.0, 0.1), (1, 102, 65, 0.0, 0.1), (1, 114, 300, 0.0, 0.1),
    (7, 142, 15, 0.0, 0.1), (7, 126, 64, 0.0, 0.1), (7, 179, 65, 0.0, 0.1), (7, 103, 300, 0.0, 0.1),
    (8, 116, 15, 0.1, 0.1), (8, 196, 64, 0.0, 0.1), (8, 144, 65, 0.0, 0.1), (8, 202, 300, 0.0, 0.1),
    (9, 227, 15, 0.0, 0.1), (9, 162, 64, 0.0, 0.1), (9, 293, 300, 0.0, 0.1),
    (15, 121, 15, 0.1, 0.4), (15, 292, 64, 0.05, 0.1), (15, 193, 65, 0.1, 0.1), (15, 119, 300, 0.05, 0.1),
    (16, 330, 15, 0.1, 0.1), (16, 341, 64, 0.1, 0.1), (16, 237, 65, 0.1, 0.1), (16, 119, 300, 0.1, 0.1),
    (17, 126, 15, 0.1, 0.4), (17, 186, 64, 0.1, 0.1), (17, 122, 65, 0.1, 0.1), (17, 109, 300, 0.1, 0.1),
    (31, 110, 15, 0.2, 0.4), (31, 391, 64, 0.1, 0.4), (31, 127, 65, 0.1, 0.4), (31, 164, 300, 0.1, 0.4),
    (32, 146, 15, 0.2, 0.4), (32, 108, 64, 0.1, 0.4), (32, 103, 300, 0.1, 0.4),
    (33, 114, 15, 0.2, 0.4), (33, 103, 65, 0.1, 0.4), (33, 109, 300, 0.1, 0.4),
    (63, 220, 15, 0.2, 0.4), (63, 304, 64, 0.2, 0.4), (63, 326, 65, 0.2, 0.4),
    (64, 248, 64, 0.2, 0.4), (64, 391, 65, 0.2, 0.4), (64, 126, 300, 0.2, 0.4),
    (65, 190, 64, 0.2, 0.4), (65, 305, 300, 0.2, 0.4),
    (473, 15, 64, 0.45, 0.3), (517, 16, 65, 0.4, 0.3), (373, 15, 300, 0.4, 0.3), (1000, 15, 300, 0.6, 0.3),
]
# one call with sets above 1024 points: every set of it runs the LARGE form
LARGE = [
    (8, 101, 1100, 0.05, 0.1), (9, 121, 1100, 0.05, 0.1), (231, 15, 1100, 0.4, 0.3), (1000, 25, 1500, 0.6, 0.3),
    (1, 104, 64, 0.0, 0.1), (7, 179, 65, 0.0, 0.1), (8, 116, 15, 0.1, 0.1), (9, 293, 300, 0.0, 0.1), (15, 193, 65, 0.1, 0.1),
    (16, 341, 64, 0.1, 0.1), (17, 126, 15, 0.1, 0.4), (33, 109, 300, 0.1, 0.4),
]


def _no_model(n, seed):
    """coordinates of the order of 1e25: every symmetric epipolar distance overflows float, no model ever has an inlier, the run takes all
    1000 iterations and finds nothing"""
    rng = np.random.RandomState(seed)
    return (rng.uniform(-1, 1, (n, 2)) * 1e25).astype(np.float32), (rng.uniform(-1, 1, (n, 2)) * 1e25).astype(np.float32)


def _lattice():
    """the sets of test_fm_ransac_check_subset_on_lattice_points: collinear triples (subsets rejected and redrawn), one line (no subset)"""
    gx, gy = np.meshgrid(np.arange(8, dtype=np.float32) * 35 + 90, np.arange(6, dtype=np.float32) * 35 + 70)
    p1 = np.stack([gx.ravel(), gy.ravel()], 1)
    rng = np.random.RandomState(3)
    p2 = (p1 * np.float32(1.01) + np.float32([4.0, -2.5])).astype(np.float32)
    p2[::7] += rng.uniform(-30, 30, (len(p2[::7]), 2)).astype(np.float32)
    line = np.stack([np.arange(24, dtype=np.float32) * 9 + 20, np.arange(24, dtype=np.float32) * 4 + 11], 1)
    return (p1, p2), (line, (line + np.float32(2.0)).astype(np.float32))


@pytest.fixture(scope="module")
def ctx():
    import icgvins
    c = icgvins.Context(1280, 720, n_slots=1, max_batch=1, max_points=8192)
    yield c
    c.close()


def _check(oracle, ctx, sets, want):
    """sets: (p1, p2); want: the oracle iters each set was picked for, or None.  Both entry points against the oracle, set by set."""
    offsets = np.cumsum([0] + [len(s[0]) for s in sets]).astype(np.int32)
    assert offsets[-1] <= 8192
    a, b = np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])
    masks = (ctx.fm_ransac(offsets, a, b), ctx.fm_ransac_device(offsets, a, b))
    hit = []
    for k, (p1, p2) in enumerate(sets):
        ok, exp, _, iters = oracle.fm_ransac(p1, p2)
        if want[k] is not None:
            assert iters == want[k], (k, len(p1), iters, want[k])
        hit.append((iters, len(p1), ok))
        for m in masks:
            got = m[offsets[k]:offsets[k + 1]]
            assert np.array_equal(got, exp), (k, len(p1), iters, int(got.sum()), int(exp.sum()))
    return hit


def test_schedule_is_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ic-gvins_amd", "csrc", "ransac.hip")).read()
    assert re.search(r"int fm_round_size\(int r\) \{ return r < 2 \? 8 : r == 2 \? 16 : FM_HPW; \}", src)
    assert re.search(r"^#define FM_HPW 32\b", src, re.M)
    assert ROUNDS == (8, 8, 16, 32)


def test_consumed_counts_on_every_edge_of_the_schedule(oracle, ctx):
    sets = [two_view(n, seed=seed, outlier_frac=frac, noise=noise)[:2] for _, seed, n, frac, noise in SMALL]
    want = [c[0] for c in SMALL]
    for n in (15, 64, 65, 300):
        sets.append(_no_model(n, 7 + n))
        want.append(1000)
    lat, line = _lattice()
    sets += [lat, line]
    want += [None, 0]
    hit = _check(oracle, ctx, sets, want)
    for n in (15, 64, 65, 300):
        at = {it for it, m, _ in hit if m == n}
        assert {1, 7, 8, 15, 16, 17, 31} <= at and max(at) == 1000, (n, sorted(at))
    assert sum(100 < it < 1000 for it, _, _ in hit) >= 3
    assert EDGES <= {it for it, _, _ in hit}
    assert [h for h in hit[len(SMALL):len(SMALL) + 4]] == [(1000, n, 0) for n in (15, 64, 65, 300)]  # the cap, nothing found
    assert hit[-1][0] == 0 and hit[-1][2] == 0  # no valid subset at all


def test_large_form_follows_the_same_schedule(oracle, ctx):
    sets = [two_view(n, seed=seed, outlier_frac=frac, noise=noise)[:2] for _, seed, n, frac, noise in LARGE]
    want = [c[0] for c in LARGE]
    sets.append(_no_model(1100, 5))
    want.append(1000)
    lat, _ = _lattice()
    sets.append(lat)
    want.append(None)
    hit = _check(oracle, ctx, sets, want)
    assert max(len(s[0]) for s in sets) > 1024
    assert {1, 7, 8, 9, 15, 16, 17, 33} <= {it for it, _, _ in hit}
    assert hit[len(LARGE)] == (1000, 1100, 0)
