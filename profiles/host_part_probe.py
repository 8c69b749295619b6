"""The host-factor part of WindowSolverBatch's reduced systems on the device (mode 2: icg_reproj_host_parts_build after the device
reduction, nothing but residuals and changed Jacobians crossing the link) against the device reduced solve alone (mode 1: the parts formed on
the host pool and shipped as packed triangles) and the host solve (mode 0), on the product libraries, 256 visual-inertial windows per shape
through icgh_backend_solve_vio_batch: small (4 states, preintegration + pose and mix priors: P = 60) and estimator-like (10 states and a
dense linear factor over all mix blocks, 90 rows and columns, in the place of the marginalization prior: P = 150).  The three modes
alternate in one process; per mode the entry's own solve time, best and median of the repetitions, results compared bit for bit.  Beside
it the kernel's own time (the context's profiler around k_host_part and the copy of the shipped Jacobians) for one
icg_reproj_host_parts_build call on 256 windows of the shape's blocks, with every Jacobian shipped and with the dense block kept.
`python profiles/host_part_probe.py [out.json] [--cpus 2] [--reps 3]`; --cpus N confines the legs to N of the CPUs the process may run on
(one rank's share of a node; the host pool then has N threads).  Every leg is a child process of its own under a time limit; the first leg
that fails ends the run.  Run by hand; not part of bench.py."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "ic-gvins_amd"), ROOT]

SHAPES = {"small": (4, False), "estimator": (10, True)}  # states, dense factor over the mix blocks
LEG_LIMIT_S = 400


def measure_kernel(states, dense, n_windows, reps):
    """one icg_reproj_host_parts_build call on n_windows windows with the block structure of the shape: profiler time and call wall time"""
    import icgvins
    import reproj_data as rd
    rng = np.random.RandomState(1)
    mk = lambda nr, cols: (rng.normal(0, 1.0, (nr, len(cols))), rng.normal(0, 1.0, nr), np.asarray(cols, np.int32))
    P = 15 * states
    blocks = [mk(15, range(15 * k, 15 * k + 30)) for k in range(states - 1)] + [mk(6, range(0, 6)), mk(9, range(6, 15))]
    if dense:
        blocks.append(mk(9 * states, [15 * k + 6 + x for k in range(states) for x in range(9)]))
    w = rd.make_window(3, 2, seed=5)
    n, K, L, W = w["obs_soa"].shape[1], w["poses"].shape[0], len(w["invdepth"]), n_windows
    rep = lambda a, step: np.concatenate([a + k * step for k in range(W)]).astype(np.int32)
    ctx = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64, max_factors=W * n)
    ctx.reproj_set_factors(np.tile(w["obs_soa"], (1, W)), rep(w["idx_i"], K), rep(w["idx_j"], K), rep(w["idx_lm"], L))
    ctx.reproj_set_windows(np.arange(W + 1, dtype=np.int32) * n, np.arange(W + 1, dtype=np.int32) * L)
    out = {}
    for name, keep_last in (("all_shipped", False), ("dense_kept", True)):
        if keep_last and not dense:
            continue
        wins = [[(J, r, cols, keep_last and b == len(blocks) - 1) for b, (J, r, cols) in enumerate(blocks)]] * W
        call = lambda: ctx.reproj_host_parts_build(P, np.full(W, P), wins)
        call()  # (sizes the buffers; the kept Jacobians of the second variant come from here)
        ctx.prof_enable(True)
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.lib.icg_ctx_sync(ctx.h)
            call()
            best = min(best or 1e9, time.perf_counter() - t0)
        k, ms = ctx.prof().get("host_part", (0, 0.0))
        ctx.prof_enable(False)
        out[name] = {"kernel_ms": round(ms / max(k, 1), 3), "python_call_ms": round(best * 1e3, 3)}
    ctx.close()
    return P, out


def measure_shape(name, reps, n_windows=256):
    import harness as H
    import host_part_data as hp
    import oracle_lib
    import vio_data as vd
    states, dense = SHAPES[name]
    P, kernel = measure_kernel(states, dense, n_windows, reps)
    lib, orc = C.CDLL(H.HOST_LIB), oracle_lib.load()
    base = [vd.make_vio_window(orc, n_intervals=states - 1, per=20, n_lm=60, seed=40 + k) for k in range(8)]
    wins = [base[w % 8] for w in range(n_windows)]
    starts = [vd.perturbed_start(wins[w], seed=w % 8) for w in range(n_windows)]
    ms, res = {0: [], 1: [], 2: []}, {}
    for _ in range(reps + 1):  # (the first round also sizes the context's buffers: it is not counted)
        for mode in (0, 1, 2):
            t0 = time.perf_counter()
            rc, msg, st, inv, summ = hp.solve_vio_batch(lib, wins, starts, [int(dense)] * n_windows, mode, iters=12, timer=ms[mode])
            if rc != 0:
                raise RuntimeError(f"icgh_backend_solve_vio_batch mode {mode} rc={rc}: {msg}")
            res[mode] = (st, inv, summ)
    for mode in (1, 2):
        for a, b in zip(res[mode][0] + res[mode][1] + [res[mode][2]], res[0][0] + res[0][1] + [res[0][2]]):
            assert np.array_equal(hp.bits(a), hp.bits(b)), f"mode {mode} differs from mode 0"
    names = {0: "mode0_host", 1: "mode1_device_solve", 2: "mode2_device_solve_and_host_part"}
    return {"shape": f"{name}: {states} states, {'a dense factor of width ' + str(9 * states) if dense else 'no dense factor'}, P = {P}", "windows": n_windows,
            "lm_steps": [float(res[0][2][:, 2].mean()), float(res[0][2][:, 3].mean())], "host_parts_build": kernel,
            "solve_ms": {names[m]: [round(t, 3) for t in ms[m][1:]] for m in ms},
            "solve_ms_best": {names[m]: round(min(ms[m][1:]), 3) for m in ms},
            "solve_ms_median": {names[m]: round(float(np.median(ms[m][1:])), 3) for m in ms}, "results_bit_identical": True}


if __name__ == "__main__":
    argv = sys.argv[1:]
    opt = {"--cpus": 0, "--reps": 3}
    leg = None
    if "--leg" in argv:
        k = argv.index("--leg")
        leg = argv[k + 1]
        del argv[k:k + 2]
    for flag in list(opt):
        if flag in argv:
            k = argv.index(flag)
            opt[flag] = int(argv[k + 1])
            del argv[k:k + 2]
    if opt["--cpus"] > 0:
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:opt["--cpus"]])
    cpus = len(os.sched_getaffinity(0))
    os.environ["ICG_SOLVER_THREADS"] = str(min(16, cpus))  # the host pool of every mode: one thread per CPU the process may use
    if leg is not None:  # a child: one leg, its result on the last line
        print(json.dumps(measure_shape(leg, opt["--reps"])))
        sys.exit(0)
    result = {"cpus": cpus, "host_pool_threads": min(16, cpus), "shapes": []}
    for name in SHAPES:
        cmd = ["timeout", "-k", "10", str(LEG_LIMIT_S), sys.executable, os.path.abspath(__file__), "--leg", name, "--reps", str(opt["--reps"])]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(f"leg {name} ended with status {r.returncode}; nothing further is started\n{r.stdout[-2000:]}\n")
            sys.exit(r.returncode)
        result["shapes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        sys.stderr.write(f"leg {name} done\n")
        sys.stderr.flush()
    txt = json.dumps(result)
    print(txt)
    if argv:
        open(argv[0], "w").write(txt + "\n")
