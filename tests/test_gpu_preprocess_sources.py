"""Where icg_frames_preprocess takes its pixels from.  Frames that already live in device memory (the benchmark's and the tracker's path) are
read in place when the stride and every pointer of the batch are multiples of 4, and are otherwise staged, the whole batch, through the
context's pitched planes; BGR is always staged; and a call with more than 64 frames (PRE_MAX_JOBS) is cut into several launches whose staging
planes, LUTs and histograms are offset by the launch's first job.  Every level and every brightness mean must equal the oracle's for the
visible pixels.  Each device frame lies in its own region of stride * height + 16 bytes filled with 0xAA: every dword the kernels read lies
inside the allocation, and a stride gap that leaked into a histogram would show."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

FILL = 0xAA


def _levels_oracle(oracle, gray, levels):
    out = [oracle.clahe(gray)]
    for _ in range(1, levels):
        out.append(oracle.pyrdown(out[-1]))
    return out


def _check_slot(oracle, c, slot, gray, what):
    exp = _levels_oracle(oracle, gray, c.levels())
    for level, e in enumerate(exp):
        got = c.download(slot, level)
        assert got.shape == e.shape, (what, slot, level)
        bad = np.argwhere(got != e)
        assert bad.size == 0, (what, slot, level, len(bad), bad[:8].tolist())


class _Regions:
    """device regions of stride * height + 16 bytes each, 0xAA everywhere but the frame's pixels, which start `shift` bytes into the region"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, frame, stride, shift=0):
        rows, row_bytes = frame.shape[0], frame[0].size
        assert stride >= row_bytes and shift < 16
        host = np.full(stride * rows + 16, FILL, np.uint8)
        for y in range(rows):
            host[shift + y * stride: shift + y * stride + row_bytes] = frame[y].ravel()
        p = self.ctx.dev_alloc(host.size)
        self.ptrs.append(p)
        self.ctx.dev_upload(p, host)
        assert p % 256 == 0  # the allocator's alignment: `shift` alone decides the pointer's
        return p + shift

    def free(self):
        self.ctx.sync()
        for p in self.ptrs:
            self.ctx.dev_free(p)
        self.ptrs = []


@pytest.fixture(scope="module")
def contexts():
    import icgvins
    made = {(w, h): icgvins.Context(w, h, n_slots=2, max_batch=2, max_points=64) for w, h in ((333, 257), (256, 64))}
    yield made
    for c in made.values():
        c.close()


# (w, h, stride, shifts of the batch's frames, read in place?)
GRAY = [
    (333, 257, 336, (0,), True),     # in place, w % 4 != 0
    (333, 257, 333, (0,), False),    # odd stride: staged, 2-D copy
    (333, 257, 336, (2,), False),    # misaligned pointer: staged
    (256, 64, 256, (0,), True),      # in place
    (256, 64, 512, (0,), True),      # in place, with gaps
    (256, 64, 256, (1,), False),     # misaligned, stride == width == staging pitch: the linear device-to-device copy
    (256, 64, 256, (0, 1), False),   # only the second frame is misaligned: the whole batch is staged
    (256, 64, 512, (0, 0), True),    # two frames in place
]


@pytest.mark.parametrize("case", GRAY, ids=lambda c: f"{c[0]}x{c[1]}-stride{c[2]}-shift{'_'.join(map(str, c[3]))}")
def test_device_gray_sources(oracle, contexts, case):
    w, h, stride, shifts, in_place = case
    # the host code's rule, restated: in place iff the stride and every pointer are multiples of 4
    assert in_place == (stride % 4 == 0 and all(s % 4 == 0 for s in shifts))
    c = contexts[(w, h)]
    frames = [synth.texture(w, h, seed=1500 + 10 * GRAY.index(case) + k) for k in range(len(shifts))]  # no frame occurs in two cases or calls' slots
    slots = list(range(len(frames)))[::-1]
    others = [(s + 1) % 2 for s in slots]
    reg = _Regions(c)
    try:
        ptrs = [reg.put(f, stride, s) for f, s in zip(frames, shifts)]
        means = c.preprocess_device(slots, ptrs, stride, want_hist=True)
        for slot, f, m in zip(slots, frames, means):
            _check_slot(oracle, c, slot, f, case)
            assert m == oracle.histogram_mean(f), (case, slot)  # the visible columns only: a gap byte would add 0xAA counts
        # and without the histogram (the asynchronous form the benchmark uses), into the other slots
        c.preprocess_device(others, ptrs, stride)
        for slot, f in zip(others, frames):
            _check_slot(oracle, c, slot, f, (case, "no hist"))
    finally:
        reg.free()


@pytest.mark.parametrize("gap", (0, 5))
def test_device_bgr_sources(oracle, contexts, gap):
    w, h = 256, 64
    c = contexts[(w, h)]
    stride = 3 * w + gap
    rng = np.random.RandomState(40 + gap)
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2)]
    reg = _Regions(c)
    try:
        ptrs = [reg.put(f, stride) for f in frames]
        means = c.preprocess_device([1, 0], ptrs, stride, channels=3, want_hist=True)
        for slot, f, m in zip((1, 0), frames, means):
            gray = oracle.bgr2gray(f)
            _check_slot(oracle, c, slot, gray, ("bgr", gap))
            assert m == oracle.histogram_mean(gray), (gap, slot)
    finally:
        reg.free()


@pytest.mark.parametrize("channels", (1, 3))
def test_more_jobs_than_one_launch_holds(oracle, channels):
    """65 frames in one call: jobs 0..63 go in the first launch, job 64 alone in the second"""
    import icgvins
    w = h = 64
    n = 65
    c = icgvins.Context(w, h, n_slots=n, max_batch=n, max_points=64)
    try:
        if channels == 1:
            frames = [synth.texture(w, h, seed=1700 + k) for k in range(n)]
            grays = frames
        else:
            rng = np.random.RandomState(17)
            frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)]
            grays = [oracle.bgr2gray(f) for f in frames]
        assert len({g.tobytes() for g in grays}) == n
        slots = [(k * 7 + 3) % n for k in range(n)]  # a permutation: job k does not land in slot k
        assert sorted(slots) == list(range(n))
        means = c.preprocess(slots, frames, want_hist=True)
        for k in range(n):
            _check_slot(oracle, c, slots[k], grays[k], (channels, "job", k))
            assert means[k] == oracle.histogram_mean(grays[k]), (channels, k)
    finally:
        c.close()
