"""WindowSolverBatch with every window's ODOMETER preintegration factors resident on the device (mode 5: setDevicePreintegration on top of
mode 3 — the factors evaluated by icg_preint_odo_evaluate_resident at every linearization and trial point, their residuals and 19 x 34
Jacobians handed to the host-part kernel on the device) against mode 3 (device reduced solve, host part and prior; the odometer factors
evaluated on the host pool), and mode 4 against mode 2 (the same pair without the device prior), on the product libraries: 256
visual-inertial windows per shape through icgh_backend_solve_preint_odo_batch (Odo variant, integration results from one
icg_preint_odo_batch call), every window with a full-width prior — small (4 states, 3 odometer factors) and estimator-like (10 states, 9
factors).  The modes alternate in one process; per mode the entry's own solve time, best and median of the repetitions, results compared bit
for bit.  Beside it the kernels' own times (the context's profiler) for the factors of 256 windows of the shape: the resident evaluation with
and without Jacobians (preint_odo_eval_given) and the gather / residual copy ahead of k_host_part (host_part_prior), and the link bytes per
linearization that follow from the shapes.
`python profiles/preint_odo_solve_probe.py [out.json] [--cpus 2] [--reps 3]`; --cpus N confines the legs to N of the CPUs the process may run
on (one rank's share of a node; the host pool then has N threads).  Every leg is a child process of its own under a time limit; the first leg
that fails ends the run.  Run by hand; not part of bench.py."""
import ctypes as C

import numpy as np

import probe_common as pc
from ctypes_util import bits, i32

SHAPES = {"small": 4, "estimator": 10}  # states
LEG_LIMIT_S = 500
ALL = np.array(list(range(0, 6)) + list(range(7, 17)) + list(range(17, 23)) + list(range(24, 34)), np.int32)


def measure_kernels(states, n_windows, reps):
    """the factors of n_windows windows of the shape resident on one context: profiler time of the resident evaluation and of the gather kernel
    of icg_reproj_host_parts_build_preint_odo (with the accumulation kernel's beside it), call wall times from Python"""
    import icgvins
    import preint_odo_data as od
    import preint_odo_split_data as sd
    import reproj_data as rd
    per, W = states - 1, n_windows
    n = per * W
    imus = [od._imu9(21, 80 + i) for i in range(per)]
    st0 = [od.state17(p=(i, 1, 0), v=(2, 0.1 * i, 0)) for i in range(per)]
    par25 = od.params25()
    off = (np.arange(n + 1) * 21).astype(np.int32)
    ctx = pc.resident_windows(rd.make_window(3, 2, seed=5), W)
    cur, delta, jac, cov, dt, pn = ctx.preint_odo_batch(od.ODO, off, np.concatenate(imus * W), np.stack(st0 * W), par25)
    env = np.tile(par25[5:9], (n, 1))
    pts = np.stack([sd.eval_point("perturbed", delta[i], cur[i], (st0 * W)[i]) for i in range(n)])
    S = ctx.preint_odo_evaluate_batch(od.ODO, delta, jac, cov, dt, env, pts)[2]
    ident = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1))
    ctx.preint_odo_set(np.full(n, od.ODO, np.int32), delta, jac, S, dt, env, ident)
    Pw = 16 * states
    cols = i32(np.concatenate([np.arange(16 * k, 16 * k + 32) for k in range(per)] * W))
    s, dg = np.zeros((W, Pw)), np.zeros((W, Pw))
    args = (Pw, i32(np.full(W, Pw)), np.ones(W, np.uint8), i32(np.arange(W + 1) * per), i32(np.full(n, 19)), i32(np.full(n, 32)), cols,
            np.full(n, icgvins.HP_JAC_FROM_PREINT_ODO, np.int64), None, np.full(19 * n, np.nan), s, dg, None, None, None, None, None, i32(np.arange(n)),
            i32(np.tile(ALL, n)))
    out = {}

    def timed(name, scopes, call):
        out[name] = pc.timed_call(ctx, reps, call, scopes)

    def build():
        if ctx.reproj_host_parts_build_preint_odo_raw(*args) != 0:
            raise RuntimeError(ctx.lib.icg_last_error(ctx.h).decode())

    timed("evaluate_resident_residual_only", ["preint_odo_eval_given"], lambda: ctx.preint_odo_evaluate_resident(pts, ident, want_jac=False))
    timed("evaluate_resident_with_jacobians", ["preint_odo_eval_given"], lambda: ctx.preint_odo_evaluate_resident(pts, ident, want_jac=True))
    timed("build_gather", ["host_part_prior", "host_part"], build)
    ctx.close()
    return n, out


def measure_shape(name, reps, n_windows=256):
    import harness as H
    import icgvins
    import oracle_lib
    import preint_odo_solve_data as os_
    import vio_data as vd
    states = SHAPES[name]
    n_fac, kernels = measure_kernels(states, n_windows, reps)
    lib, orc = C.CDLL(H.HOST_LIB), oracle_lib.load()
    base = [vd.make_vio_window(orc, n_intervals=states - 1, per=20, n_lm=60, seed=40 + k) for k in range(8)]
    base_prior = [os_.make_prior(base[k], range(states), 60 + k) for k in range(8)]
    base_start = [vd.perturbed_start(base[k], seed=k) for k in range(8)]
    ctx = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    base_res = [os_.integrate_on_device(ctx, 2, [base[k]], [base_start[k]]) for k in range(8)]
    ctx.close()
    wins = [base[w % 8] for w in range(n_windows)]
    priors = [base_prior[w % 8] for w in range(n_windows)]
    starts = [base_start[w % 8] for w in range(n_windows)]
    results = [r for w in range(n_windows) for r in base_res[w % 8]]
    modes = (2, 4, 3, 5)
    ms = {m: [] for m in modes}

    def run(mode, counted):
        rc, msg, st, inv, summ, _, n_dev = os_.solve_preint_odo_batch(lib, wins, starts, results, priors, mode, iters=12, timer=ms[mode] if counted else None)
        if rc != 0:
            raise RuntimeError(f"icgh_backend_solve_preint_odo_batch mode {mode} rc={rc}: {msg}")
        assert n_dev == (n_fac if mode >= 4 else 0), (mode, n_dev)
        return st + inv + [summ]

    def compare(mode, got, ref):
        for a, b in zip(got, ref):
            assert np.array_equal(bits(a), bits(b)), f"mode {mode} differs from mode 2"

    summ = pc.alternate_modes(modes, reps, run, compare)[2][-1]
    names = {2: "mode2_device_solve_and_host_part", 3: "mode3_device_prior", 4: "mode4_mode2_and_device_preintegration", 5: "mode5_mode3_and_device_preintegration"}
    best = {m: min(ms[m]) for m in modes}
    scatter = {m: max(ms[m]) - min(ms[m]) for m in modes}

    def pair(with_, without):
        margin = best[without] - best[with_]
        worst  = max(scatter[with_], scatter[without])
        return {"best_ms_saved": round(margin, 3), f"scatter_ms_mode{without}": round(scatter[without], 3), f"scatter_ms_mode{with_}": round(scatter[with_], 3),
                "verdict": pc.verdict(margin, worst, f"mode {with_} faster", f"mode {with_} slower",
                                      "not a result: the margin is below the scatter of the repetitions")}

    per = states - 1
    return {"shape": f"{name}: {states} states, {per} odometer preintegration factors per window, a prior over all states", "windows": n_windows,
            "lm_steps": [float(summ[:, 2].mean()), float(summ[:, 3].mean())], "kernels": kernels,
            "link_bytes_per_linearization_from_the_shapes": {
                "pool_path_up": n_windows * per * (19 * 32 + 19) * 8,  # every factor's gathered 19 x 32 Jacobian and its residual
                "resident_path_up": n_windows * per * (34 + 4) * 8,  # evaluation point and correction quaternion
                "resident_path_down": n_windows * per * 8},  # one squared norm
            "solve_ms": {names[m]: [round(t, 3) for t in ms[m]] for m in modes},
            "solve_ms_best": {names[m]: round(best[m], 3) for m in modes},
            "solve_ms_median": {names[m]: round(float(np.median(ms[m])), 3) for m in modes},
            "mode5_against_mode3": pair(5, 3), "mode4_against_mode2": pair(4, 2), "results_bit_identical": True}


def assemble(opt, cpus, legs):
    return {"cpus": cpus, "host_pool_threads": min(16, cpus), "shapes": list(legs.values())}


if __name__ == "__main__":
    pc.main(__file__, {"--cpus": 0, "--reps": 3}, list(SHAPES), LEG_LIMIT_S, lambda leg, opt: measure_shape(leg, opt["--reps"]), assemble, solver_threads=True)
