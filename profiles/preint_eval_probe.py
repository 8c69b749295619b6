"""P2 (PreintegrationFactor::Evaluate) batched on the device against the same evaluations on the host pool, on the product libraries:
bench.py's C4 preintegration shape (256 streams x 15 intervals x 40 samples, Earth variant) is integrated once, then every factor is
evaluated (a) by one icg_preint_evaluate_batch call (device time of its two kernels from the context's profiler; wall time of the call
including packing and transfers) and (b) by one PreintegrationFactor::Evaluate per factor on a HostPool.
`python profiles/preint_eval_probe.py [out.json] [--threads 16] [--cpus 2] [--reps 5]`; --cpus N confines the process to N of the CPUs it
may run on (one rank's share of a node) before any library is loaded.  The one shape is one leg: a child process under a time limit.
Run by hand; not part of bench.py."""
import ctypes as C
import os
import time

import numpy as np

import probe_common as pc
from ctypes_util import ErrBuf, ptr

LEG_LIMIT_S = 60  # the whole probe at its defaults took 0.9 s: twice that, rounded up to a full minute


def measure(threads=16, reps=5, n_streams=256, n_int=15, n_samples=40):
    import harness as H
    import icgvins
    import preint_data as pd
    import reproj_data as rd
    n = n_streams * n_int
    base = [pd.make_interval(n_samples + 1, seed=s) for s in range(n_int)]
    imu = np.ascontiguousarray(np.concatenate(base * n_streams))
    off = (np.arange(n + 1) * (n_samples + 1)).astype(np.int32)
    s0 = np.ascontiguousarray(np.tile(pd.state(), (n, 1)))
    params = np.ascontiguousarray(pd.PARAMS)
    # --- the C ABI alone: integrate, evaluate
    ctx = icgvins.Context(640, 480, n_slots=1, max_batch=1, max_points=64)
    cur, delta, jac, cov, dt, pn = ctx.preint_batch(1, off, imu, s0, params)
    rng = np.random.RandomState(11)
    scale = np.array([0.02, 0.02, 0.02, 0.002, 0.002, 0.002])
    points = np.zeros((n, 32))
    for k in range(n):
        pose1 = rd.pose_plus(cur[k, :7], rng.normal(0, 1, 6) * scale)
        points[k] = np.concatenate([s0[k], pose1, cur[k, 7:]])
    pn_rows = np.ascontiguousarray(pn.reshape(n, n_samples + 1, 4)[:, :n_samples].reshape(-1, 4))
    pn_off = (np.arange(n + 1) * n_samples).astype(np.int32)
    env = np.tile(params[5:9], (n, 1))
    args = (1, delta, jac, cov, dt, env, points, pn_off, pn_rows)
    for _ in range(2):
        ctx.preint_evaluate_batch(*args)
    ctx.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        _, _, _, status = ctx.preint_evaluate_batch(*args)
    wall = (time.perf_counter() - t0) / reps
    launches, ms = ctx.prof()["preint_eval"]
    ctx.close()
    out = {"shape": f"{n_streams} streams x {n_int} intervals x {n_samples} samples, Earth", "factors": n, "cpus": len(os.sched_getaffinity(0)),
           "c_abi": {"kernels_us_per_call": round(ms * 1e3 / launches, 1), "call_wall_us_incl_transfers": round(wall * 1e6, 1),
                     "factors_per_s_kernels": round(n / (ms * 1e-3 / launches), 1), "singular": int(status.sum())}}
    # --- the host layer: the same objects on both paths
    hl = C.CDLL(H.HOST_LIB)
    out6, err = np.zeros(6), ErrBuf()
    rc = hl.icgh_backend_preint_eval_time(1, n, ptr(off), ptr(imu), ptr(s0), ptr(params), ptr(points), int(threads), int(reps), ptr(out6), *err.args)
    if rc != 0:
        raise RuntimeError(f"icgh_backend_preint_eval_time rc={rc}: {err.text()}")
    out["host_layer"] = {"host_pool_threads": int(threads), "host_evaluate_us": round(out6[0] * 1e6, 1),
                         "host_factors_per_s": round(n / out6[0], 1), "evaluate_batch_wall_us_incl_packing_and_transfers": round(out6[1] * 1e6, 1),
                         "evaluate_batch_kernels_us": round(out6[2] * 1e3, 1), "max_abs_diff_residual": float(out6[3]),
                         "max_abs_diff_jacobian": float(out6[4]), "evaluated": int(out6[5])}
    return out


if __name__ == "__main__":
    pc.main(__file__, {"--threads": 16, "--cpus": 0, "--reps": 5}, ["all"], LEG_LIMIT_S, lambda leg, opt: measure(threads=opt["--threads"], reps=opt["--reps"]),
            lambda opt, cpus, legs: legs["all"])
