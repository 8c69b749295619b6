"""The 19-state odometer preintegration kernels beside their 15-state siblings, in one run on the product libraries: bench.py's C4
preintegration shape (256 streams x 15 intervals = 3 840 intervals x 41 samples) is integrated with all four variants (0 Normal, 1 Earth
through icg_preint_batch; 2 Odo, 3 EarthOdo through icg_preint_odo_batch), and the 3 840 factors of variants 1 and 3 are evaluated on the
device (icg_preint_evaluate_batch / icg_preint_odo_evaluate_batch: device time of the two kernels from the context's profiler) and on the
host (one Evaluate per factor on a HostPool).  Both kernel families are latency bound: intervals/s and factors/s, not against the HBM roof.
`python profiles/preint_odo_probe.py [out.json] [--threads 16] [--cpus 0] [--reps 5]`; the one shape is one leg: a child process under a
time limit.  Run by hand; not part of bench.py."""
import ctypes as C
import os

import numpy as np

import probe_common as pc
from ctypes_util import ErrBuf, ptr

LEG_LIMIT_S = 120


def measure(threads=16, reps=5, n_streams=256, n_int=15, n_samples=40):
    import harness as H
    import icgvins
    import preint_data as pd
    import preint_odo_data as od
    import reproj_data as rd
    n = n_streams * n_int
    base = [od._imu9(n_samples + 1, seed=s) for s in range(n_int)]
    imu9 = np.ascontiguousarray(np.concatenate(base * n_streams))
    imu8 = np.ascontiguousarray(imu9[:, :8])
    off = (np.arange(n + 1) * (n_samples + 1)).astype(np.int32)
    s17 = np.ascontiguousarray(np.tile(od.state17(), (n, 1)))
    s16 = np.ascontiguousarray(s17[:, :16])
    par25 = od.params25()
    par9, par19 = np.ascontiguousarray(par25[:9]), np.ascontiguousarray(od.params19(par25, od.ABV))
    ctx = icgvins.Context(640, 480, n_slots=1, max_batch=1, max_points=64)
    out = {"shape": f"{n_streams} streams x {n_int} intervals x {n_samples + 1} samples", "intervals": n, "cpus": len(os.sched_getaffinity(0)), "p1": {}, "p2": {}}
    res = {}
    for variant, name in ((0, "normal"), (1, "earth"), (2, "odo"), (3, "earth_odo")):
        if variant < 2:
            call, scope = (lambda v=variant: res.__setitem__(v, ctx.preint_batch(v, off, imu8, s16, par9))), "preint"
        else:
            call, scope = (lambda v=variant: res.__setitem__(v, ctx.preint_odo_batch(v, off, imu9, s17, par25))), "preint_odo"
        t = pc.timed_call(ctx, reps, call, [scope])
        ms = t[scope + "_ms"]
        out["p1"][name] = {"kernel_us": round(ms * 1e3, 1), "call_wall_us_incl_transfers": round(t["python_call_ms"] * 1e3, 1),
                           "intervals_per_s": round(n / (ms * 1e-3), 1), "samples_per_s": round(n * n_samples / (ms * 1e-3), 1)}
    out["p1"]["odo_over_normal"] = round(out["p1"]["odo"]["kernel_us"] / out["p1"]["normal"]["kernel_us"], 3)
    out["p1"]["earth_odo_over_earth"] = round(out["p1"]["earth_odo"]["kernel_us"] / out["p1"]["earth"]["kernel_us"], 3)
    # P2 on the device, Earth and EarthOdo, at points off the integrated states
    rng = np.random.RandomState(11)
    scale = np.array([0.02, 0.02, 0.02, 0.002, 0.002, 0.002])
    pose1 = np.stack([rd.pose_plus(res[1][0][k, :7], rng.normal(0, 1, 6) * scale) for k in range(n)])
    pts32 = np.concatenate([s16, pose1, res[1][0][:, 7:]], axis=1)
    pts34 = np.concatenate([s17, pose1, res[3][0][:, 7:], s17[:, 16:17] + 1e-3], axis=1)
    pn_off = (np.arange(n + 1) * n_samples).astype(np.int32)
    env = np.tile(par25[5:9], (n, 1))
    status = {}
    for variant, name, pts, fn, scope in ((1, "earth", pts32, ctx.preint_evaluate_batch, "preint_eval"),
                                          (3, "earth_odo", pts34, ctx.preint_odo_evaluate_batch, "preint_odo_eval")):
        cur, delta, jac, cov, dt, pn = res[variant]
        pn_rows = np.ascontiguousarray(pn.reshape(n, n_samples + 1, 4)[:, :n_samples].reshape(-1, 4))
        t = pc.timed_call(ctx, reps, lambda: status.__setitem__(variant, fn(variant, delta, jac, cov, dt, env, pts, pn_off, pn_rows)[3]), [scope])
        ms = t[scope + "_ms"]
        out["p2"][name] = {"device_kernels_us": round(ms * 1e3, 1), "call_wall_us_incl_transfers": round(t["python_call_ms"] * 1e3, 1),
                           "device_factors_per_s": round(n / (ms * 1e-3), 1), "singular": int(status[variant].sum())}
    ctx.close()
    out["p2"]["earth_odo_over_earth_device"] = round(out["p2"]["earth_odo"]["device_kernels_us"] / out["p2"]["earth"]["device_kernels_us"], 3)
    # P2 on the host, the same evaluations one factor at a time on a HostPool (the host layer's entries integrate on the device themselves)
    hl = C.CDLL(H.HOST_LIB)
    out6, err = np.zeros(6), ErrBuf()
    rc = hl.icgh_backend_preint_eval_time(1, n, ptr(off), ptr(imu8), ptr(s16), ptr(par9), ptr(np.ascontiguousarray(pts32)), int(threads), int(reps), ptr(out6),
                                          *err.args)
    if rc != 0:
        raise RuntimeError(f"icgh_backend_preint_eval_time rc={rc}: {err.text()}")
    out8 = np.zeros(8)
    rc = hl.icgh_backend_preint_odo_time(3, n, ptr(off), ptr(imu9), ptr(s17), ptr(par19), ptr(np.ascontiguousarray(pts34)), int(threads), int(reps), ptr(out8),
                                         *err.args)
    if rc != 0:
        raise RuntimeError(f"icgh_backend_preint_odo_time rc={rc}: {err.text()}")
    out["p2"]["earth"].update({"host_pool_threads": int(threads), "host_evaluate_us": round(out6[0] * 1e6, 1), "host_factors_per_s": round(n / out6[0], 1),
                               "max_abs_diff_residual": float(out6[3]), "max_abs_diff_jacobian": float(out6[4]), "evaluated": int(out6[5])})
    out["p2"]["earth_odo"].update({"host_pool_threads": int(threads), "host_evaluate_us": round(out8[2] * 1e6, 1), "host_factors_per_s": round(n / out8[2], 1),
                                   "max_abs_diff_residual": float(out8[5]), "max_abs_diff_jacobian": float(out8[6]), "evaluated": int(out8[7]),
                                   "host_layer_integrate_wall_us": round(out8[1] * 1e6, 1), "host_layer_p1_kernel_us": round(out8[0] * 1e3, 1)})
    out["p2"]["earth_odo_over_earth_host"] = round(out["p2"]["earth_odo"]["host_evaluate_us"] / out["p2"]["earth"]["host_evaluate_us"], 3)
    return out


if __name__ == "__main__":
    pc.main(__file__, {"--threads": 16, "--cpus": 0, "--reps": 5}, ["all"], LEG_LIMIT_S, lambda leg, opt: measure(threads=opt["--threads"], reps=opt["--reps"]),
            lambda opt, cpus, legs: legs["all"])
