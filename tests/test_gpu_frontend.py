"""GPU parity tests (run on a real MI355X with -m gpu): HIP path through the C ABI vs the CPU oracle on identical
seeded inputs.  Integer/byte/index outputs must be bit-exact; float point coordinates must be bit-exact too because
both sides use exact-integer window sums and no FMA contraction (tolerance stated per test)."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx640():
    import icgvins
    c = icgvins.Context(640, 480, n_slots=4, max_batch=2, max_points=4096)
    c.set_camera(synth.CAM_640)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx1280():
    import icgvins
    c = icgvins.Context(1280, 720, n_slots=4, max_batch=2, max_points=8192)
    c.set_camera(synth.CAM_1280)
    yield c
    c.close()


def _pyr_oracle(oracle, img, levels):
    out = [oracle.clahe(img)]
    for _ in range(1, levels):
        out.append(oracle.pyrdown(out[-1]))
    return out


@pytest.mark.parametrize("size", [(640, 480), (1280, 720), (1278, 1022), (333, 257)])
def test_preprocess_bit_exact(oracle, size):
    import icgvins
    w, h = size
    c = icgvins.Context(w, h, n_slots=3, max_batch=2, max_points=64)
    try:
        imgs = [synth.texture(w, h, seed=20), synth.texture(w, h, seed=21)]
        hist = c.preprocess([2, 0], imgs, want_hist=True)
        levels = c.levels()
        for slot, img in zip((2, 0), imgs):
            exp = _pyr_oracle(oracle, img, levels)
            for l in range(levels):
                got = c.download(slot, l)
                assert got.shape == exp[l].shape
                assert np.array_equal(got, exp[l]), (size, slot, l, np.abs(got.astype(int) - exp[l].astype(int)).max())
        for k, img in enumerate(imgs):
            assert hist[k] == oracle.histogram_mean(img)
    finally:
        c.close()


def test_preprocess_bgr(oracle, ctx640):
    rng = np.random.RandomState(3)
    bgr = rng.randint(0, 256, (480, 640, 3)).astype(np.uint8)
    ctx640.preprocess([1], [bgr])
    exp = oracle.clahe(oracle.bgr2gray(bgr))
    assert np.array_equal(ctx640.download(1, 0), exp)


@pytest.mark.parametrize("shift", [(1.3, -0.7), (5.5, 3.25), (-9.0, 4.0)])
def test_lk_single_direction_bit_exact(oracle, ctx640, shift):
    w, h = 640, 480
    img = synth.texture(w, h, seed=30)
    nxt = synth.shift_image(img, *shift)
    ctx640.preprocess([0, 1], [img, nxt])
    a, b = oracle.clahe(img), oracle.clahe(nxt)
    pts = np.concatenate([synth.random_points(300, w, h, 2, seed=31),
                          np.array([[0.5, 0.5], [w - 1.0, h - 1.0], [-30.0, 10.0], [w + 25.0, 50.0], [320.0, -12.0]], np.float32)])
    guess = pts + np.float32(0.8) * np.array(shift, np.float32)
    exp_pts, exp_st, exp_err = oracle.lk_track(a, b, pts, guess)
    got_pts, got_st, got_err = ctx640.lk_track(0, 1, pts, guess)
    assert np.array_equal(got_st, exp_st)
    assert np.array_equal(got_pts.view(np.uint32), exp_pts.view(np.uint32))  # bit-exact floats
    assert np.array_equal(got_err.view(np.uint32), exp_err.view(np.uint32))


def test_lk_fb_bit_exact_c2(oracle, ctx1280):
    """BASELINE config C2 shape: 1280x720, 300 points."""
    w, h = 1280, 720
    img = synth.texture(w, h, seed=40)
    nxt = synth.shift_image(img, 3.4, -2.2)
    ctx1280.preprocess([0, 1], [img, nxt])
    a, b = oracle.clahe(img), oracle.clahe(nxt)
    pts = synth.random_points(300, w, h, 3, seed=41)
    guess = pts + np.array([2.5, -1.5], np.float32)
    exp_pts, exp_st = oracle.lk_track_fb(a, b, pts, guess)
    got_pts, got_st, got_und, keep = ctx1280.lk_track_fb(0, 1, pts, guess, want_undist=True, want_keep=True)
    assert np.array_equal(got_st, exp_st)
    assert np.array_equal(got_pts.view(np.uint32), exp_pts.view(np.uint32))
    assert np.array_equal(keep, np.nonzero(exp_st)[0])
    assert exp_st.sum() > 150
    exp_und = oracle.undistort(synth.CAM_1280, exp_pts)
    assert np.array_equal(got_und.view(np.uint32), exp_und.view(np.uint32))


def test_lk_fb_multi_stream_batch(oracle, ctx1280):
    """Two independent streams in one launch (slots 0->1 and 2->3) equal two separate oracle runs."""
    w, h = 1280, 720
    s0a, s1a = synth.texture(w, h, seed=50), synth.texture(w, h, seed=51)
    s0b, s1b = synth.shift_image(s0a, 1.5, 2.5), synth.shift_image(s1a, -4.0, 0.75)
    ctx1280.preprocess([0, 1], [s0a, s0b])
    ctx1280.preprocess([2, 3], [s1a, s1b])
    p0 = synth.random_points(200, w, h, 8, seed=52)
    p1 = synth.random_points(150, w, h, 8, seed=53)
    pts = np.concatenate([p0, p1])
    prev_slot = np.concatenate([np.full(200, 0), np.full(150, 2)]).astype(np.int32)
    next_slot = prev_slot + 1
    got_pts, got_st = ctx1280.lk_track_fb(prev_slot, next_slot, pts, pts.copy())
    e0, st0 = oracle.lk_track_fb(oracle.clahe(s0a), oracle.clahe(s0b), p0, p0.copy())
    e1, st1 = oracle.lk_track_fb(oracle.clahe(s1a), oracle.clahe(s1b), p1, p1.copy())
    assert np.array_equal(got_st, np.concatenate([st0, st1]))
    assert np.array_equal(got_pts.view(np.uint32), np.concatenate([e0, e1]).view(np.uint32))


def test_lk_unrelated_images_all_culled(oracle, ctx640):
    w, h = 640, 480
    a, b = synth.texture(w, h, seed=60), synth.texture(w, h, seed=61)
    ctx640.preprocess([0, 1], [a, b])
    pts = synth.random_points(120, w, h, 10, seed=62)
    got_pts, got_st = ctx640.lk_track_fb(0, 1, pts, pts.copy())
    exp_pts, exp_st = oracle.lk_track_fb(oracle.clahe(a), oracle.clahe(b), pts, pts.copy())
    assert np.array_equal(got_st, exp_st)
    assert np.array_equal(got_pts.view(np.uint32), exp_pts.view(np.uint32))


def test_empty_batches(ctx640):
    out, st = ctx640.lk_track_fb(0, 1, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    assert out.shape == (0, 2) and st.shape == (0,)
    assert ctx640.undistort(np.zeros((0, 2), np.float32)).shape == (0, 2)


def test_camera_point_ops_bit_exact(oracle, ctx1280):
    cam = synth.CAM_1280
    pts = synth.random_points(1000, 1280, 720, 0, seed=70)
    assert np.array_equal(ctx1280.undistort(pts).view(np.uint32), oracle.undistort(cam, pts).view(np.uint32))
    assert np.array_equal(ctx1280.distort(pts).view(np.uint32), oracle.distort(cam, pts).view(np.uint32))
    # INS predictions
    rng = np.random.RandomState(71)
    ang = 0.05
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
    pose = np.concatenate([R.ravel(), [0.3, -0.2, 0.1]])
    pw = np.stack([rng.uniform(-8, 8, 400), rng.uniform(-5, 5, 400), rng.uniform(6, 40, 400)], 1)
    exp = oracle.distort(cam, oracle.world2pixel(cam, pose, pw))
    got = ctx1280.predict_mappoints(pw, 0, pose)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    R_pre = np.eye(3)
    r_cur_pre = R.T @ R_pre
    exp = oracle.predict_rotation(cam, np.eye(3), r_cur_pre, pts)
    got = ctx1280.predict_rotation(pts, 0, r_cur_pre.ravel())
    # the oracle forms I^T r_cur_pre, which is r_cur_pre exactly: both sides rotate by the same matrix -> same bits
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_camera_point_kernels_match_reference_golden():
    """icg_distort_points and icg_predict_mappoints (world2pixel + distort, tracking.cc:367-378) against outputs of the
    REFERENCE's own Camera class (tests/golden/camera_ref_golden.npz): float bit patterns."""
    import os
    import icgvins
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_ref_golden.npz"))
    c = icgvins.Context(int(g["w"]), int(g["h"]), n_slots=1, max_batch=1, max_points=1024)
    try:
        c.set_camera(g["cam"])
        same = lambda a, b: np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
        assert same(c.distort(g["pts"]), g["distorted"])
        assert same(c.predict_mappoints(g["pw"], 0, g["pose12"][None, :]), g["predicted"])
    finally:
        c.close()


def test_lk_survives_a_growing_staging_arena(oracle):
    """icg_arena_reserve replaces the staging arena pair when a call needs more than the context was created with; the
    frame slots and everything else resident must survive it.  Here the arena of a small context is forced to grow between two LK calls
    (a long INS series needs more staging than the context was created with); the second call must still return the oracle's bit patterns."""
    import icgvins
    w, h = 640, 480
    c = icgvins.Context(w, h, n_slots=4, max_batch=2, max_points=512, max_factors=16)
    c.set_camera(synth.CAM_640)
    try:
        A = synth.texture(w, h, seed=70)
        B = synth.shift_image(A, 1.7, -2.1)
        Cc = synth.shift_image(B, -1.2, 1.6)
        c.preprocess([0, 1], [A, B])
        c.preprocess([2], [Cc])
        b_img, c_img = oracle.clahe(B), oracle.clahe(Cc)
        pts = synth.random_points(200, w, h, 12, seed=71)
        n = len(pts)
        s0, s1, s2 = np.zeros(n, np.int32), np.ones(n, np.int32), np.full(n, 2, np.int32)
        out1, st1 = c.lk_track_fb(s0, s1, pts, pts + np.float32([1.5, -2.0]))
        # ~6 MB of staging for one call: several times the arena of this context (512 points, 16 factors -> ~1.6 MB)
        n_streams, n_samples = 64, 400
        offsets = np.arange(n_streams + 1, dtype=np.int32) * n_samples
        imu = np.zeros((n_streams * n_samples, 8))
        imu[:, 0] = np.tile(np.arange(1, n_samples + 1) * 0.005, n_streams)
        imu[:, 1] = 0.005
        states = np.zeros((n_streams, 23))
        states[:, 9] = 1.0  # a valid state layout is not needed for this test beyond finite numbers
        try:
            c.ins_mechanize_batch(offsets, imu, np.zeros(8), states, want_traj=True)
        except RuntimeError:
            pass  # (whatever the INS entry point thinks of these numbers, the arena has grown by then)
        guess2 = out1 + np.float32([-1.0, 1.5])
        exp_pts, exp_st = oracle.lk_track_fb(b_img, c_img, out1, guess2)
        got_pts, got_st = c.lk_track_fb(s1, s2, out1, guess2)
        assert np.array_equal(got_st, exp_st)
        assert np.array_equal(got_pts.view(np.uint32), exp_pts.view(np.uint32))
    finally:
        c.close()
