"""The stage kernels of the device-resident tracker (csrc/tracker.hip, k_trk_stage<STAGE>: one instance per stage) where a per-stage
instance can go wrong: which instance a step launches, and the branches of a stream that has no frame in a step.  Three streams in ONE
tracker, so one launch chain serves streams in different situations; states, statistics and full state dumps downloaded from HBM against
the oracle-backed table engine on the same frames.  Which chain a step took is read from the launch counts of the profiling scopes:
`trk_stage_pre` is launched by the detection-first chain only (instances 0, 1, 2), `trk_begin` without it by the histogram-gate chain
(0, 12), neither by the steady chain (120)."""
import ctypes as C

import numpy as np
import pytest

import harness as H
from stream_utils import ensure_oracle_host

pytestmark = pytest.mark.gpu

W, HGT, NFEAT, NFRAMES, NS = 640, 480, 100, 14, 3
DUMP_AT = (2, NFRAMES // 2, NFRAMES - 1)
TRACKING = H.TRACK_STATES.index("TRACKING")


@pytest.fixture(scope="module")
def frames_and_poses():
    cam = H.camera_for(W, HGT)
    scene = H.SynthScene(C.CDLL(ensure_oracle_host()), W, HGT, cam, tex_size=1024, threads=4)
    frames = [[scene.render(k, stream=40 + s) for k in range(NFRAMES)] for s in range(NS)]
    poses = [[H.pose12(*scene.ins_pose(k, stream=40 + s)) for k in range(NFRAMES)] for s in range(NS)]
    for row in frames:
        for f in row:
            f.setflags(write=False)
    return frames, poses


def _launches(hip, ctx, name):
    n = C.c_int()
    assert hip.icg_prof_get(C.c_void_p(ctx), name.encode(), C.byref(n), None) == 0
    return n.value


def _drive(lib, engine, frames, poses, has_frame, check_hist=False, chains=False):
    """has_frame(s, k): stream s gets frame k (else None: the stream idles in that step).  Returns states per step, dumps at DUMP_AT,
    statistics and — chains=True, device engine — the chain each step took."""
    sb = H.StreamBatch(lib, NS, W, HGT, H.camera_for(W, HGT), max_features=NFEAT, engine=engine, check_hist=check_hist)
    assert sb.engine() == engine
    hip = ctx = None
    if chains:
        import icgvins
        hip, ctx = icgvins.load_library(), sb.ctx_handle(0)
        assert hip.icg_prof_enable(C.c_void_p(ctx), 1) == 0
    states, dumps, chain = [], {}, []
    seen = {"trk_stage_pre": 0, "trk_begin": 0}
    for k in range(NFRAMES):
        ptrs = [frames[s][k].ctypes.data if has_frame(s, k) else None for s in range(NS)]
        st = sb.step(ptrs, W, np.full(NS, 100.0 + k / 20.0), np.stack([poses[s][k] for s in range(NS)]))
        states.append([int(v) for v in st])
        if k in DUMP_AT:
            dumps[k] = [sb.dump(s, 0) for s in range(NS)]
        if chains:
            now = {name: _launches(hip, ctx, name) for name in seen}
            chain.append("detect_first" if now["trk_stage_pre"] > seen["trk_stage_pre"] else "gate" if now["trk_begin"] > seen["trk_begin"] else "steady")
            seen = now
    stats = [sb.stats(s) for s in range(NS)]
    sb.close()
    return states, dumps, stats, chain


def _compare(frames_and_poses, has_frame, check_hist=False):
    frames, poses = frames_and_poses
    st_t, d_t, stats_t, _ = _drive(ensure_oracle_host(), "table", frames, poses, has_frame, check_hist)
    st_d, d_d, stats_d, chain = _drive(H.HOST_LIB, "device", frames, poses, has_frame, check_hist, chains=True)
    assert st_t == st_d
    assert stats_t == stats_d
    for k in DUMP_AT:
        for s in range(NS):
            if d_t[k][s] != d_d[k][s]:
                la, lb = d_t[k][s].splitlines(), d_d[k][s].splitlines()
                i = next((i for i in range(min(len(la), len(lb))) if la[i] != lb[i]), min(len(la), len(lb)))
                raise AssertionError(f"stream {s} after frame {k}, dump line {i}:\n table : {la[i] if i < len(la) else '<end>'}\n device: {lb[i] if i < len(lb) else '<end>'}")
    return st_d, stats_d, chain


def test_idle_streams_in_every_chain(frames_and_poses):
    """stream 1 has no frame in the first step and in two later ones: begin-frame's idle path in instances 0 and 120, build_rois for an
    inactive stream in instances 1 (first steps, detection-first chain) and 5 (every chain)"""
    idle = {0, 6, 9}
    states, stats, chain = _compare(frames_and_poses, lambda s, k: not (s == 1 and k in idle))
    assert chain[0] == "detect_first" and chain[1] == "detect_first"  # (step 1: stream 1 has not seen a frame yet)
    assert chain[6] == "steady" and chain[9] == "steady"
    assert stats[1]["frames"] == NFRAMES - len(idle) and stats[0]["frames"] == NFRAMES
    assert all(s["mappoints_created"] > 40 for s in stats)


def test_late_stream_switches_the_chain(frames_and_poses):
    """stream 2 starts five frames after the others: until it has started, every step of the tracker takes the detection-first chain
    (instances 0, 1, 2) — with the two other streams already tracking, which the steady chain serves otherwise — and from then on 120"""
    start = 5
    states, stats, chain = _compare(frames_and_poses, lambda s, k: s != 2 or k >= start)
    assert all(c == "detect_first" for c in chain[:start + 1])
    assert states[start][0] == TRACKING and states[start][1] == TRACKING
    assert "steady" in chain[start + 1:]
    assert stats[2]["frames"] == NFRAMES - start


def test_histogram_gate_chain(frames_and_poses):
    """the histogram gate on: the prediction waits for the preprocessing, so a step launches instance 0, then 12 (or 1 and 2) and never
    120; stream 1 idles in two steps as above"""
    idle = {6, 9}
    states, stats, chain = _compare(frames_and_poses, lambda s, k: not (s == 1 and k in idle), check_hist=True)
    assert chain[0] == "detect_first"
    assert "steady" not in chain and chain.count("gate") >= NFRAMES // 2
    assert chain[6] == "gate" and chain[9] == "gate"
    assert all(s["mappoints_created"] > 40 for s in stats)
