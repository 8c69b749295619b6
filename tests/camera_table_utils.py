"""Shared data and drivers of the per-stream camera calibration tests: four calibrations at 640x480, frames rendered through each stream's
own camera, and the per-stream references — the oracle-backed table engine (CPU) run on ONE stream with the existing single-camera
constructor.  References are computed once per (camera, scene stream, gaps) and shared by every test of the session."""
import ctypes as C
import functools

import numpy as np

import harness as H
from stream_utils import ensure_oracle_host

W, HGT, NFEAT, NFRAMES = 640, 480, 100, 16
SCENE0 = 40  # the stream at position s of a batch flies scene stream SCENE0 + s
DUMP_AT = (2, 8, 15)


def cameras():
    b = H.camera_for(W, HGT)
    fx, fy = b[0], b[1]
    return {
        "base": list(b),
        "wide": [0.8 * fx, 0.8 * fy, W / 2 + 11.5, HGT / 2 - 7.25, 0.0, -0.28, 0.07, 0.0004, -0.0003, 0.0],
        "tele": [1.25 * fx, 1.25 * fy, W / 2 - 9.0, HGT / 2 + 6.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
        "skew": [fx, 1.02 * fy, W / 2, HGT / 2, 1.5, -0.09, 0.08, 0.0002, 0.0002, 0.01],
    }


@functools.lru_cache(maxsize=None)
def _scene(name):
    return H.SynthScene(C.CDLL(ensure_oracle_host()), W, HGT, cameras()[name], tex_size=1024, threads=4)


@functools.lru_cache(maxsize=None)
def rendered(name, scene_stream, n_frames=NFRAMES):
    """(frames, poses12) of scene stream `scene_stream` seen through camera `name`"""
    sc = _scene(name)
    frames = tuple(sc.render(k, stream=scene_stream) for k in range(n_frames))
    poses = tuple(H.pose12(*sc.ins_pose(k, stream=scene_stream)) for k in range(n_frames))
    return frames, poses


def drive(lib, engine, frames, poses, cam10=None, cams=None, groups=1, gaps=None, dump_at=DUMP_AT, keep=False):
    """frames[s][k], poses[s][k]; gaps: {stream: set of steps without a frame}.  Returns per stream: states, features (ids, pixel bits) per
    frame, dumps at dump_at, stats; with keep=True also the open batch (the caller closes it)."""
    n = len(frames)
    gaps = gaps or {}
    sb = H.StreamBatch(lib, n, W, HGT, cam10 if cam10 is not None else cams[0], max_features=NFEAT, engine=engine, groups=groups, cams=cams)
    out = [dict(states=[], feats=[], dumps={}) for _ in range(n)]
    for k in range(len(frames[0])):
        ptrs = [None if k in gaps.get(s, ()) else frames[s][k].ctypes.data for s in range(n)]
        st = sb.step(ptrs, W, np.full(n, 100.0 + k / 20.0), np.stack([poses[s][k] for s in range(n)]))
        for s in range(n):
            ids, px = sb.features(s)
            out[s]["states"].append(int(st[s]))
            out[s]["feats"].append((ids.tobytes(), px.view(np.uint32).tobytes()))
            if k in dump_at:
                out[s]["dumps"][k] = sb.dump(s, 0)
    for s in range(n):
        out[s]["stats"] = sb.stats(s)
    if keep:
        return out, sb
    sb.close()
    return out


@functools.lru_cache(maxsize=None)
def reference(name, scene_stream, gaps=(), calib=None):
    """the stream alone on the oracle-backed table engine, existing constructor, calibration `calib` (default: its own camera)"""
    frames, poses = rendered(name, scene_stream)
    r = drive(ensure_oracle_host(), "table", [frames], [poses], cam10=cameras()[calib or name], gaps={0: set(gaps)} if gaps else None)[0]
    return r


def assert_stream_equal(got, ref, what):
    assert got["states"] == ref["states"], (what, got["states"], ref["states"])
    assert got["stats"] == ref["stats"], (what, got["stats"], ref["stats"])
    for k, (a, b) in enumerate(zip(got["feats"], ref["feats"])):
        assert a == b, f"{what}: features of frame {k} differ"
    for k in ref["dumps"]:
        if got["dumps"][k] != ref["dumps"][k]:
            la, lb = ref["dumps"][k].splitlines(), got["dumps"][k].splitlines()
            i = next((i for i in range(min(len(la), len(lb))) if la[i] != lb[i]), min(len(la), len(lb)))
            raise AssertionError(f"{what} after frame {k}, dump line {i}:\n reference: {la[i] if i < len(la) else '<end>'}\n got      : {lb[i] if i < len(lb) else '<end>'}")


def batch_inputs(names, gaps=None):
    """frames, poses, cams rows and references for a batch whose stream s has camera names[s] and flies scene stream SCENE0 + s"""
    fr, po, refs = [], [], []
    for s, nm in enumerate(names):
        f, p = rendered(nm, SCENE0 + s)
        fr.append(f), po.append(p)
        refs.append(reference(nm, SCENE0 + s, tuple(sorted((gaps or {}).get(s, ())))))
    cams = np.array([cameras()[nm] for nm in names], np.float64)
    return fr, po, cams, refs
