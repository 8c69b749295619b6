"""WindowSolverBatch with every window's marginalization prior resident on the device (mode 3: setDevicePrior — the prior evaluated by
icg_marg_prior_evaluate_resident at every linearization and trial point, its residual and Jacobian handed to the host-part kernel on the
device) against mode 2 (device reduced solve and device host part, the prior evaluated on the host pool), mode 1 and mode 0, on the product
libraries: 256 visual-inertial windows per shape through icgh_backend_solve_prior_batch, every window with a full-width prior over the pose
and mix blocks of all its states — small (4 states: r = P = 60) and estimator-like (10 states: r = P = 150).  The four modes alternate in one
process; per mode the entry's own solve time, best and median of the repetitions, results compared bit for bit.  Beside it the kernels' own
times (the context's profiler) for 256 priors of the shape: the resident evaluation (marg_eval) and the gather / residual copy ahead of
k_host_part (host_part_prior), at a window's first rebuild (Jacobian gathered) and at a later one (Jacobian kept).
`python profiles/prior_solve_probe.py [out.json] [--cpus 2] [--reps 3]`; --cpus N confines the legs to N of the CPUs the process may run on
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

SHAPES = {"small": 4, "estimator": 10}  # states
LEG_LIMIT_S = 500


def measure_kernels(states, n_windows, reps):
    """n_windows priors of the shape resident on one context: profiler time of the resident evaluation and of the prior kernel of
    icg_reproj_host_parts_build_prior (with the accumulation kernel's beside it), call wall times from Python"""
    import icgvins
    import marg_factor_data as mf
    import reproj_data as rd
    sizes = [7, 9] * states
    prior = mf.make_prior(sizes, 3)
    r = prior["r"]
    priors = [prior] * n_windows
    x = np.concatenate([mf.make_x(prior, 50)] * n_windows)
    w = rd.make_window(3, 2, seed=5)
    n, K, L, W = w["obs_soa"].shape[1], w["poses"].shape[0], len(w["invdepth"]), n_windows
    rep = lambda a, step: np.concatenate([a + k * step for k in range(W)]).astype(np.int32)
    ctx = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64, max_factors=W * n)
    ctx.reproj_set_factors(np.tile(w["obs_soa"], (1, W)), rep(w["idx_i"], K), rep(w["idx_j"], K), rep(w["idx_lm"], L))
    ctx.reproj_set_windows(np.arange(W + 1, dtype=np.int32) * n, np.arange(W + 1, dtype=np.int32) * L)
    ctx.marg_prior_set(*mf.set_args(priors))
    pc = np.arange(r, dtype=np.int32)
    out = {}

    def timed(name, scopes, call):
        call()
        ctx.prof_enable(True)
        best = None
        for _ in range(reps):
            ctx.lib.icg_ctx_sync(ctx.h)
            t0 = time.perf_counter()
            call()
            best = min(best or 1e9, time.perf_counter() - t0)
        prof = ctx.prof()
        ctx.prof_enable(False)
        out[name] = {"python_call_ms": round(best * 1e3, 3)}
        for scope in scopes:
            k, ms = prof.get(scope, (0, 0.0))
            out[name][scope + "_ms"] = round(ms / max(k, 1), 4)

    timed("evaluate_resident", ["marg_eval"], lambda: ctx.marg_prior_evaluate_resident(x))
    for name, how in (("build_first_rebuild_gather", "gather"), ("build_later_rebuild_keep", "keep")):
        wins = [[("prior", k, pc, pc, how)] for k in range(W)]
        timed(name, ["host_part_prior", "host_part"], lambda: ctx.reproj_host_parts_build_prior(r, np.full(W, r), wins))
    ctx.close()
    return r, out


def measure_shape(name, reps, n_windows=256):
    import harness as H
    import oracle_lib
    import prior_solve_data as ps
    import vio_data as vd
    states = SHAPES[name]
    r, kernels = measure_kernels(states, n_windows, reps)
    lib, orc = C.CDLL(H.HOST_LIB), oracle_lib.load()
    base = [vd.make_vio_window(orc, n_intervals=states - 1, per=20, n_lm=60, seed=40 + k) for k in range(8)]
    base_prior = [ps.make_prior(base[k], range(states), 60 + k) for k in range(8)]
    wins = [base[w % 8] for w in range(n_windows)]
    priors = [base_prior[w % 8] for w in range(n_windows)]
    starts = [vd.perturbed_start(wins[w], seed=w % 8) for w in range(n_windows)]
    modes = (0, 1, 2, 3)
    ms, res = {m: [] for m in modes}, {}
    for _ in range(reps + 1):  # (the first round also sizes the context's buffers: it is not counted)
        for mode in modes:
            rc, msg, st, inv, summ, _ = ps.solve_prior_batch(lib, wins, starts, priors, mode, iters=12, timer=ms[mode])
            if rc != 0:
                raise RuntimeError(f"icgh_backend_solve_prior_batch mode {mode} rc={rc}: {msg}")
            res[mode] = (st, inv, summ)
    for mode in modes[1:]:
        for a, b in zip(res[mode][0] + res[mode][1] + [res[mode][2]], res[0][0] + res[0][1] + [res[0][2]]):
            assert np.array_equal(ps.bits(a), ps.bits(b)), f"mode {mode} differs from mode 0"
    names = {0: "mode0_host", 1: "mode1_device_solve", 2: "mode2_device_solve_and_host_part", 3: "mode3_device_prior"}
    best = {m: min(ms[m][1:]) for m in modes}
    scatter = {m: max(ms[m][1:]) - min(ms[m][1:]) for m in modes}
    margin = best[2] - best[3]
    return {"shape": f"{name}: {states} states, a prior over all of them: r = P = {r}", "windows": n_windows,
            "lm_steps": [float(res[0][2][:, 2].mean()), float(res[0][2][:, 3].mean())], "kernels": kernels,
            "solve_ms": {names[m]: [round(t, 3) for t in ms[m][1:]] for m in modes},
            "solve_ms_best": {names[m]: round(best[m], 3) for m in modes},
            "solve_ms_median": {names[m]: round(float(np.median(ms[m][1:])), 3) for m in modes},
            "mode3_against_mode2": {"best_ms_saved": round(margin, 3), "scatter_ms_mode2": round(scatter[2], 3), "scatter_ms_mode3": round(scatter[3], 3),
                                    "verdict": "mode 3 faster" if margin > max(scatter[2], scatter[3]) else
                                               "mode 3 slower" if -margin > max(scatter[2], scatter[3]) else "not a result: the margin is below the scatter of the repetitions"},
            "results_bit_identical": True}


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
