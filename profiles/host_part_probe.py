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

import numpy as np

import probe_common as pc
from ctypes_util import bits

SHAPES = {"small": (4, False), "estimator": (10, True)}  # states, dense factor over the mix blocks
LEG_LIMIT_S = 400


def measure_kernel(states, dense, n_windows, reps):
    """one icg_reproj_host_parts_build call on n_windows windows with the block structure of the shape: profiler time and call wall time"""
    import reproj_data as rd
    rng = np.random.RandomState(1)
    mk = lambda nr, cols: (rng.normal(0, 1.0, (nr, len(cols))), rng.normal(0, 1.0, nr), np.asarray(cols, np.int32))
    P = 15 * states
    blocks = [mk(15, range(15 * k, 15 * k + 30)) for k in range(states - 1)] + [mk(6, range(0, 6)), mk(9, range(6, 15))]
    if dense:
        blocks.append(mk(9 * states, [15 * k + 6 + x for k in range(states) for x in range(9)]))
    W = n_windows
    ctx = pc.resident_windows(rd.make_window(3, 2, seed=5), W)
    out = {}
    for name, keep_last in (("all_shipped", False), ("dense_kept", True)):
        if keep_last and not dense:
            continue
        wins = [[(J, r, cols, keep_last and b == len(blocks) - 1) for b, (J, r, cols) in enumerate(blocks)]] * W
        call = lambda: ctx.reproj_host_parts_build(P, np.full(W, P), wins)
        call()  # (sizes the buffers; the kept Jacobians of the second variant come from here)
        ctx.prof_enable(True)
        best = pc.best_of(reps, lambda: (ctx.lib.icg_ctx_sync(ctx.h), call()))
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
    ms = {0: [], 1: [], 2: []}

    def run(mode, counted):
        rc, msg, st, inv, summ = hp.solve_vio_batch(lib, wins, starts, [int(dense)] * n_windows, mode, iters=12, timer=ms[mode] if counted else None)
        if rc != 0:
            raise RuntimeError(f"icgh_backend_solve_vio_batch mode {mode} rc={rc}: {msg}")
        return st + inv + [summ]

    def compare(mode, got, ref):
        for a, b in zip(got, ref):
            assert np.array_equal(bits(a), bits(b)), f"mode {mode} differs from mode 0"

    summ = pc.alternate_modes((0, 1, 2), reps, run, compare)[0][-1]
    names = {0: "mode0_host", 1: "mode1_device_solve", 2: "mode2_device_solve_and_host_part"}
    return {"shape": f"{name}: {states} states, {'a dense factor of width ' + str(9 * states) if dense else 'no dense factor'}, P = {P}", "windows": n_windows,
            "lm_steps": [float(summ[:, 2].mean()), float(summ[:, 3].mean())], "host_parts_build": kernel,
            "solve_ms": {names[m]: [round(t, 3) for t in ms[m]] for m in ms},
            "solve_ms_best": {names[m]: round(min(ms[m]), 3) for m in ms},
            "solve_ms_median": {names[m]: round(float(np.median(ms[m])), 3) for m in ms}, "results_bit_identical": True}


def assemble(opt, cpus, legs):
    return {"cpus": cpus, "host_pool_threads": min(16, cpus), "shapes": list(legs.values())}


if __name__ == "__main__":
    pc.main(__file__, {"--cpus": 0, "--reps": 3}, list(SHAPES), LEG_LIMIT_S, lambda leg, opt: measure_shape(leg, opt["--reps"]), assemble, solver_threads=True)
