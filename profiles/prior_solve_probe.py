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

import numpy as np

import probe_common as pc
from ctypes_util import bits

SHAPES = {"small": 4, "estimator": 10}  # states
LEG_LIMIT_S = 500


def measure_kernels(states, n_windows, reps):
    """n_windows priors of the shape resident on one context: profiler time of the resident evaluation and of the prior kernel of
    icg_reproj_host_parts_build_prior (with the accumulation kernel's beside it), call wall times from Python"""
    import marg_factor_data as mf
    import reproj_data as rd
    sizes = [7, 9] * states
    prior = mf.make_prior(sizes, 3)
    r = prior["r"]
    priors = [prior] * n_windows
    x = np.concatenate([mf.make_x(prior, 50)] * n_windows)
    W = n_windows
    ctx = pc.resident_windows(rd.make_window(3, 2, seed=5), W)
    ctx.marg_prior_set(*mf.set_args(priors))
    cols = np.arange(r, dtype=np.int32)
    out = {}

    def timed(name, scopes, call):
        out[name] = pc.timed_call(ctx, reps, call, scopes)

    timed("evaluate_resident", ["marg_eval"], lambda: ctx.marg_prior_evaluate_resident(x))
    for name, how in (("build_first_rebuild_gather", "gather"), ("build_later_rebuild_keep", "keep")):
        wins = [[("prior", k, cols, cols, how)] for k in range(W)]
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
    ms = {m: [] for m in modes}

    def run(mode, counted):
        rc, msg, st, inv, summ, _ = ps.solve_prior_batch(lib, wins, starts, priors, mode, iters=12, timer=ms[mode] if counted else None)
        if rc != 0:
            raise RuntimeError(f"icgh_backend_solve_prior_batch mode {mode} rc={rc}: {msg}")
        return st + inv + [summ]

    def compare(mode, got, ref):
        for a, b in zip(got, ref):
            assert np.array_equal(bits(a), bits(b)), f"mode {mode} differs from mode 0"

    summ = pc.alternate_modes(modes, reps, run, compare)[0][-1]
    names = {0: "mode0_host", 1: "mode1_device_solve", 2: "mode2_device_solve_and_host_part", 3: "mode3_device_prior"}
    best = {m: min(ms[m]) for m in modes}
    scatter = {m: max(ms[m]) - min(ms[m]) for m in modes}
    margin = best[2] - best[3]
    return {"shape": f"{name}: {states} states, a prior over all of them: r = P = {r}", "windows": n_windows,
            "lm_steps": [float(summ[:, 2].mean()), float(summ[:, 3].mean())], "kernels": kernels,
            "solve_ms": {names[m]: [round(t, 3) for t in ms[m]] for m in modes},
            "solve_ms_best": {names[m]: round(best[m], 3) for m in modes},
            "solve_ms_median": {names[m]: round(float(np.median(ms[m])), 3) for m in modes},
            "mode3_against_mode2": {"best_ms_saved": round(margin, 3), "scatter_ms_mode2": round(scatter[2], 3), "scatter_ms_mode3": round(scatter[3], 3),
                                    "verdict": pc.verdict(margin, max(scatter[2], scatter[3]), "mode 3 faster", "mode 3 slower",
                                                          "not a result: the margin is below the scatter of the repetitions")},
            "results_bit_identical": True}


def assemble(opt, cpus, legs):
    return {"cpus": cpus, "host_pool_threads": min(16, cpus), "shapes": list(legs.values())}


if __name__ == "__main__":
    pc.main(__file__, {"--cpus": 0, "--reps": 3}, list(SHAPES), LEG_LIMIT_S, lambda leg, opt: measure_shape(leg, opt["--reps"]), assemble, solver_threads=True)
