"""Cost of per-stream camera calibration in the device-resident tracker: N streams at C2 (1280x720, 300 features) through ONE tracker
(harness.StreamBatch, engine="device", one group), once with one shared camera (the existing constructor) and once with four cameras assigned
round robin (cams=).  Both runs get the same frames — stream s sees the scene through camera s % 4 — resident in HBM; the two runs alternate
`--reps` times.  Prints one JSON line and writes it to --out.

    python profiles/camera_table_probe.py --streams 96 --steps 40 --warmup 10 --reps 3 --out profiles/camera_table_probe.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ic-gvins_amd"))
import harness as H  # noqa: E402
import icgvins  # noqa: E402

W, HGT, NFEAT = 1280, 720, 300


def cameras():
    b = H.camera_for(W, HGT)
    fx, fy = b[0], b[1]
    return np.array([list(b),
                     [0.8 * fx, 0.8 * fy, W / 2 + 23.0, HGT / 2 - 14.5, 0.0, -0.28, 0.07, 0.0004, -0.0003, 0.0],
                     [1.25 * fx, 1.25 * fy, W / 2 - 18.0, HGT / 2 + 13.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                     [fx, 1.02 * fy, W / 2, HGT / 2, 1.5, -0.09, 0.08, 0.0002, 0.0002, 0.01]], np.float64)


def run(n, cams, ring, poses, steps, warmup, per_stream):
    kw = dict(cams=cams[np.arange(n) % 4]) if per_stream else {}
    sb = H.StreamBatch(H.HOST_LIB, n, W, HGT, cams[0], max_features=NFEAT, engine="device", groups=1, **kw)
    lib = icgvins.load_library()
    ctx = C.c_void_p(sb.ctx_handle(0))
    dev = []
    try:
        for c in range(4):  # the ring of every camera once in HBM; streams of one camera share it
            row = []
            for f in ring[c]:
                p = C.c_void_p()
                assert lib.icg_dev_alloc(ctx, C.c_size_t(f.nbytes + 16), C.byref(p)) == 0
                assert lib.icg_dev_upload(ctx, p, f.ctypes.data_as(C.c_void_p), C.c_size_t(f.nbytes)) == 0
                row.append(p.value)
            dev.append(row)
        R = len(ring[0])

        def block(k0, K):
            idx = [H.pingpong(k, R) for k in range(k0, k0 + K)]
            ptrs = [[dev[s % 4][i] for s in range(n)] for i in idx]
            stamps = np.array([[100.0 + k / 20.0] * n for k in range(k0, k0 + K)])
            p12 = np.stack([np.stack([poses[i]] * n) for i in idx])
            t0 = time.perf_counter()
            sb.run(ptrs, W, stamps, p12, on_device=True)
            return time.perf_counter() - t0

        block(0, warmup)
        dt = block(warmup, steps)
        tracking = sum(1 for s in sb.stats_all() if s["last_state"] == 2)
        return n * steps / dt, tracking
    finally:
        for row in dev:
            for p in row:
                lib.icg_dev_free(ctx, C.c_void_p(p))
        sb.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=96)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ring", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cams = cameras()
    tools = C.CDLL(H.TOOLS_LIB)
    scenes = [H.SynthScene(tools, W, HGT, cams[c], tex_size=2048, threads=8) for c in range(4)]
    ring = [[sc.render(k) for k in range(a.ring)] for sc in scenes]
    poses = [H.pose12(*scenes[0].ins_pose(k)) for k in range(a.ring)]
    res = {"shared": [], "per_stream": []}
    states = {}
    for _ in range(a.reps):
        for key in ("shared", "per_stream"):
            fps, tracking = run(a.streams, cams, ring, poses, a.steps, a.warmup, key == "per_stream")
            res[key].append(round(fps, 1))
            states[key] = tracking
    out = {"workload": f"C2 {W}x{HGT}, {NFEAT} features, {a.streams} streams in one device tracker (one group), frames in HBM",
           "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "unit": "frames/s"}
    for key, v in res.items():
        out[key] = {"runs": v, "best": max(v), "median": statistics.median(v), "scatter": round((max(v) - min(v)) / statistics.median(v), 4),
                    "streams_in_tracking_state_at_end": states[key]}
    out["per_stream_over_shared_median"] = round(out["per_stream"]["median"] / out["shared"]["median"], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
