"""The reduced camera solve of WindowSolverBatch on the device (mode 1: icg_reproj_schur_windows_resident + icg_reproj_solve_windows, one wave
per window in k_chol_solve) against the host pool (mode 0), on the product libraries, 256 windows per shape: the bench's C2 solve problem
(300 landmarks, 10 keyframes: P = 67), a window as wide as the estimator's (25 keyframes: P = 157, the packed triangle still in LDS) and a C4
width above the LDS limit (34 keyframes: P = 211, global scratch).  Per shape, in one process: the device time of k_chol_solve (the
context's profiler: HIP events around the launch) and the wall time of an icg_reproj_solve_windows call with its transfers, beside the
icg_reproj_backsub_windows call it replaces; then the whole two-solve flow of icgh_backend_solve_batch_mode in mode 0 and in mode 1 (its
own timer around solve + culling + solve), results compared bit for bit.
`python profiles/reduced_solve_probe.py [out.json] [--cpus 2] [--reps 3]`; --cpus N confines the legs to N of the CPUs the process may run on
(one rank's share of a node; the host pool then has N threads).  Every leg is a child process of its own under a time limit; the first leg
that fails ends the run.  Run by hand; not part of bench.py."""
import ctypes as C

import numpy as np

import probe_common as pc

SHAPES = {"C2": (300, 10), "estimator": (300, 25), "C4": (300, 34)}  # landmarks, keyframes: P = 6 keyframes + 7
LEG_LIMIT_S = 300


def measure_call(n_lm, n_kf, n_windows, reps):
    """the C entries on n_windows copies of one window's factor set: kernel time and call wall time"""
    import reproj_data as rd
    w = rd.make_window(n_lm, n_kf, seed=0, pixel_noise=0.3)
    K, L = w["poses"].shape[0], len(w["invdepth"])
    W, P = n_windows, 6 * K + 7
    best_of = lambda reps, fn: round(pc.best_of(reps, fn) * 1e3, 3)
    ctx = pc.resident_windows(w, W)
    ctx.reproj_eval_windows(np.tile(w["poses"], (W, 1)), np.tile(w["ext"], (W, 1)), np.tile(w["invdepth"], W), np.full(W, w["td"]), huber=1.0)
    cols = (np.tile(6 * np.arange(K), W), np.full(W, 6 * K), np.full(W, 6 * K + 6))
    s, dg, _ = ctx.reproj_schur_windows_resident(P, *cols, damp=np.full(W, 1e-4))
    # the host part of a window whose poses carry priors, the damping of radius 1e4
    part = np.concatenate([np.where(np.arange(i + 1) == i, 900.0, 0.0) for i in range(P)])
    dd = np.clip(dg + 900.0, 1e-6, 1e32) / 1e4
    Pw, ones = np.full(W, P, np.int32), np.ones(W, np.uint8)
    parts = np.tile(part, W)
    dc, st, _, _ = ctx.reproj_solve_windows(P, Pw, ones, dd, s, W * L, host_part_new=ones, host_S=parts)
    assert not st.any(), "the probe's systems must factor"
    ctx.prof_enable(True)
    out = {"solve_windows_call_ms_host_parts_resident": best_of(reps, lambda: ctx.reproj_solve_windows(P, Pw, ones, dd, s, W * L)),
           "solve_windows_call_ms_host_parts_shipped": best_of(reps, lambda: ctx.reproj_solve_windows(P, Pw, ones, dd, s, W * L, host_part_new=ones,
                                                                                                       host_S=parts))}
    out.update({key + "_kernel_ms": round(ms / k, 3) for key, (k, ms) in ctx.prof().items() if key.startswith("chol_solve") and k})
    ctx.prof_enable(False)
    out["backsub_windows_call_ms"] = best_of(reps, lambda: ctx.reproj_backsub_windows(P, dc, W * L))
    out["schur_windows_view_call_ms"] = best_of(reps, lambda: ctx.reproj_schur_windows_view(P, *cols, damp=np.full(W, 1e-4)))
    out["schur_windows_resident_call_ms"] = best_of(reps, lambda: ctx.reproj_schur_windows_resident(P, *cols, damp=np.full(W, 1e-4)))
    ctx.close()
    return P, out


def measure_shape(name, reps, n_windows=256):
    import harness as H
    import reduced_solve_utils as ru
    import solve_utils as su
    n_lm, n_kf = SHAPES[name]
    P, call = measure_call(n_lm, n_kf, n_windows, reps)
    lib = C.CDLL(H.HOST_LIB)
    probs = [su.make_problem(n_lm, n_kf, seed=w % 8, n_outliers=10) for w in range(n_windows)]
    ms = {0: [], 1: []}

    def run(mode, counted):
        rc, msg, res = ru.solve_batch_mode(lib, probs, mode, solve_ms=ms[mode] if counted else None)
        if rc != 0:
            raise RuntimeError(f"icgh_backend_solve_batch_mode {mode} rc={rc}: {msg}")
        return res

    pc.alternate_modes((0, 1), reps, run, lambda mode, got, ref: ru.assert_same_results(got, ref))
    return {"shape": f"{name}: {n_lm} landmarks, {n_kf} keyframes, P = {P}", "windows": n_windows, "c_abi": call,
            "two_solves_ms": {"mode0_host": [round(t, 3) for t in ms[0]], "mode1_device": [round(t, 3) for t in ms[1]]},
            "two_solves_ms_best": {"mode0_host": round(min(ms[0]), 3), "mode1_device": round(min(ms[1]), 3)},
            "two_solves_ms_median": {"mode0_host": round(float(np.median(ms[0])), 3), "mode1_device": round(float(np.median(ms[1])), 3)},
            "results_bit_identical": True}


def assemble(opt, cpus, legs):
    return {"cpus": cpus, "host_pool_threads": min(16, cpus), "shapes": list(legs.values())}


if __name__ == "__main__":
    pc.main(__file__, {"--cpus": 0, "--reps": 3}, list(SHAPES), LEG_LIMIT_S, lambda leg, opt: measure_shape(leg, opt["--reps"]), assemble,
            solver_threads=True)
