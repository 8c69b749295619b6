"""Per-stream camera calibration through the host layer on the MI355X: one batch, a camera per stream.  The reference of every stream is
the oracle-backed table engine (CPU, the existing single-camera constructor) run on that stream ALONE with its own camera
(camera_table_utils.reference); every comparison is for equality — states per frame, statistics with the digest, features (ids and pixel bit
patterns) per frame and the canonical dumps after frames 2, 8 and 15.  Frames are rendered through each stream's own camera, and tracking
the wide camera's frames with the base calibration changes its digest (asserted below): a path that picks the wrong camera cannot pass."""
import ctypes as C

import numpy as np
import pytest

import camera_table_utils as ct
import cull_utils as cu
import harness as H

pytestmark = pytest.mark.gpu

FOUR = ("base", "wide", "tele", "skew")


def _check(got, refs, names, dumps=True, full_stats=True):
    for s, (g, r) in enumerate(zip(got, refs)):
        assert r["stats"]["mappoints_created"] > 40, (s, names[s], r["stats"])
        if not dumps or not full_stats:
            g, r = dict(g), dict(r)
            if not dumps:
                g["dumps"], r["dumps"] = {}, {}
            if not full_stats:  # engines that keep their own counters: the digest, the frame / keyframe counts and the tracked sum
                keys = ("frames", "keyframes", "tracked_sum", "digest", "mappoints_created", "last_state")
                g["stats"], r["stats"] = {k: g["stats"][k] for k in keys}, {k: r["stats"][k] for k in keys}
        ct.assert_stream_equal(g, r, f"stream {s} ({names[s]})")


@pytest.mark.parametrize("names", [FOUR, ("tele", "base", "skew", "wide")], ids=["in_order", "reordered"])
def test_device_tracker_heterogeneous_batch(names):
    """four cameras in ONE tracker; the second order shows that the camera follows the stream, not the position"""
    fr, po, cams, refs = ct.batch_inputs(names)
    got = ct.drive(H.HOST_LIB, "device", fr, po, cams=cams)
    _check(got, refs, names)
    # negative control: the wide camera's frames tracked with the base calibration give another digest
    s = names.index("wide")
    assert ct.reference("wide", ct.SCENE0 + s, (), "base")["stats"]["digest"] != refs[s]["stats"]["digest"]


def test_device_tracker_groups_index_their_own_cameras():
    """cameras differ within and across groups: a table indexed by the global instead of the local stream index fails here"""
    names = ("wide", "base", "tele", "skew", "base", "wide")
    fr, po, cams, refs = ct.batch_inputs(names)
    got = ct.drive(H.HOST_LIB, "device", fr, po, cams=cams, groups=3)
    _check(got, refs, names)


def test_device_tracker_idle_stream_keeps_its_camera():
    """stream 1 receives no frame in steps 5 to 7; every stream equals its reference driven with the same gaps"""
    gaps = {1: {5, 6, 7}}
    fr, po, cams, refs = ct.batch_inputs(FOUR, gaps)
    got = ct.drive(H.HOST_LIB, "device", fr, po, cams=cams, gaps=gaps)
    _check(got, refs, FOUR)
    assert got[1]["states"][5:8] == [3, 3, 3]  # PASSED


@pytest.mark.parametrize("engine", ["table", "object", "core"])
def test_host_engines_on_the_hip_library(engine):
    """the host engines hold a Camera per stream; the device calls between their stages take the indexed LK entry"""
    fr, po, cams, refs = ct.batch_inputs(FOUR)
    got = ct.drive(H.HOST_LIB, engine, fr, po, cams=cams)
    _check(got, refs, FOUR, dumps=engine != "object", full_stats=engine != "object")


def test_homogeneous_table_equals_the_existing_constructor():
    names = ("base",) * 4
    fr, po, cams, refs = ct.batch_inputs(names)
    a = ct.drive(H.HOST_LIB, "device", fr, po, cam10=ct.cameras()["base"])
    b = ct.drive(H.HOST_LIB, "device", fr, po, cams=cams)
    _check(b, a, names)
    _check(b, refs, names)


# ---- culling ------------------------------------------------------------------------------------------------------------------------------
def _cull(sb, seeds, frames20, poses20):
    """mode and arguments as tests/cull_checks.py: an optimizer write-back stand-in, statistics, culling, then four more frames"""
    n = sb.n
    tables = [cu.landmark_table(sb, s) for s in range(n)]
    assert all(len(T["id"]) > 40 for T in tables), [len(T["id"]) for T in tables]
    for s, T in enumerate(tables):
        rng = np.random.RandomState(seeds[s])
        sel = np.arange(len(T["id"]))[::4]
        newpos = T["pos"][sel] + rng.normal(0, 1, (len(sel), 3)) * rng.choice([0.05, 0.3, 2.0], (len(sel), 1))
        newpos[::3] += np.array([0.0, 0.0, 400.0])
        ids = np.ascontiguousarray(T["id"][sel])
        assert sb.lib.icgh_batch_set_landmark_pos(C.c_void_p(sb.h_), s, len(sel), ids.ctypes.data_as(C.c_void_p),
                                                  np.ascontiguousarray(newpos).ctypes.data_as(C.c_void_p)) == 0
    tables = [cu.landmark_table(sb, s) for s in range(n)]
    lists = [T["id"][T["id"] % 5 != 0] for T in tables]
    stats = cu.run_culling(sb, 1, lists)
    out = cu.run_culling(sb, 0, lists)
    after = [cu.landmark_table(sb, s) for s in range(n)]
    states = []
    for k in range(ct.NFRAMES, ct.NFRAMES + 4):
        st = sb.step([frames20[s][k].ctypes.data for s in range(n)], ct.W, np.full(n, 100.0 + k / 20.0), np.stack([poses20[s][k] for s in range(n)]))
        states.append([int(v) for v in st])
    res = []
    for s in range(n):
        res.append(dict(out=[int(v) for v in out[s]], stats=stats[s].tobytes(), ids=after[s]["id"].tobytes(), flags=after[s]["obs_flags"].tobytes(),
                        off=after[s]["off"].tobytes(), states=[row[s] for row in states], final=sb.dump(s, 0), digest=sb.stats(s)["digest"]))
    return res


def test_culling_uses_every_streams_camera():
    """icgh_batch_culling on the heterogeneous batch against four single-stream batches of the existing constructor, each with its camera"""
    fr, po, cams, refs = ct.batch_inputs(FOUR)
    long = [ct.rendered(nm, ct.SCENE0 + s, ct.NFRAMES + 4) for s, nm in enumerate(FOUR)]
    f20, p20 = [x[0] for x in long], [x[1] for x in long]
    got, sb = ct.drive(H.HOST_LIB, "device", fr, po, cams=cams, keep=True)
    try:
        _check(got, refs, FOUR)
        het = _cull(sb, [11 + s for s in range(4)], f20, p20)
    finally:
        sb.close()
    # the same batch in two groups: every group's streams are culled on the group's own context, with its table's local indices
    _, sb2 = ct.drive(H.HOST_LIB, "device", fr, po, cams=cams, groups=2, keep=True)
    try:
        het2 = _cull(sb2, [11 + s for s in range(4)], f20, p20)
    finally:
        sb2.close()
    assert het2 == het
    total = np.zeros(5, int)
    for s, nm in enumerate(FOUR):
        one, sb1 = ct.drive(H.HOST_LIB, "device", [fr[s]], [po[s]], cam10=ct.cameras()[nm], keep=True)
        try:
            exp = _cull(sb1, [11 + s], [f20[s]], [p20[s]])[0]
        finally:
            sb1.close()
        for key in ("out", "stats", "ids", "off", "flags", "states", "digest", "final"):
            assert het[s][key] == exp[key], (s, nm, key)
        total += np.array(exp["out"])
    assert total[0] > 5 and total[1] > 0, total  # map points and features were culled
