"""WindowSolverBatch with every window's NAVIGATION factors resident on the device (mode 5 + setDeviceNavFactors: ImuPosePriorFactor,
ImuMixPriorFactor, ImuErrorFactor and a GnssFactor on every state evaluated by icg_nav_evaluate_resident at every linearization and trial
point, the Huber loss of the GNSS factors corrected by icg_nav_correct_resident, residuals and Jacobians handed to the host-part kernel on the
device) against mode 5 alone (device reduced solve, host part, prior and preintegration; the navigation factors evaluated, gathered and
costed on the host pool), on the product libraries: 256 visual-inertial windows per shape through icgh_backend_solve_nav_batch (Odo width,
integration results from one icg_preint_odo_batch call, HuberLoss(1.0) on the GNSS factors), every window with a full-width prior — small
(4 states) and estimator-like (10 states).  With the switch a window's host factors are all evaluated on the device in every LM step.  The
two modes alternate in one process; per mode the entry's own solve time, best and median of the repetitions, results compared bit for bit.
Beside it the kernels' own times (the context's profiler) for the factors of 256 windows of the shape: the resident evaluation with and
without Jacobians (nav_eval), the correction (nav_correct) and the gather / residual copy ahead of k_host_part (host_part_prior), and the link
bytes per linearization that follow from the shapes.
`python profiles/nav_solve_probe.py [out.json] [--cpus 2] [--reps 3]`; --cpus N confines the legs to N of the CPUs the process may run on (one
rank's share of a node; the host pool then has N threads).  Every leg is a child process of its own under a time limit; the first leg that
fails ends the run.  Run by hand; not part of bench.py."""
import ctypes as C

import numpy as np

import probe_common as pc
from ctypes_util import bits, i32

SHAPES = {"small": 4, "estimator": 10}  # states
LEG_LIMIT_S = 500


def window_members(states):
    """the navigation factors of one window of the shape at the Odo width as nav_product_data cases, with the system columns each takes:
    pose prior and mix prior on state 0, the error factor on the last state, a GNSS factor on every state"""
    import nav_product_data as nd
    by = nd.one_of_each()
    pose, mix, err, gnss = by[2], by[5], by[4], by[0]
    members = [(pose, np.arange(0, 6)), (mix, np.arange(6, 16)), (err, np.arange(16 * (states - 1) + 6, 16 * states))]
    return members + [(gnss, np.arange(16 * k, 16 * k + 6)) for k in range(states)]


def measure_kernels(states, n_windows, reps):
    """the navigation factors of n_windows windows of the shape resident on one context: profiler time of the resident evaluation, of the
    correction of the GNSS members and of the gather kernel of icg_reproj_host_parts_build_nav (the accumulation kernel's beside it)"""
    import icgvins
    import nav_product_data as nd
    import reproj_data as rd
    W = n_windows
    members = window_members(states)
    per = len(members)
    n = per * W
    cases = [m[0] for m in members] * W
    kind, aux_off, aux, points, point_off = nd.pack(cases)
    ctx = pc.resident_windows(rd.make_window(3, 2, seed=5), W)
    ctx.nav_set(kind, aux_off, aux)
    robust = (kind == 0).astype(np.uint8)
    corr = np.tile([0.7, 0.0, 0.7], (n, 1))
    Pw = 16 * states
    cols = i32(np.concatenate([m[1] for m in members] * W))
    nav_cols = i32(np.concatenate([np.arange(len(m[1])) for m in members] * W))
    nr = i32([nd.SHAPES[int(k)][0] for k in kind])
    nf = i32([len(m[1]) for m in members] * W)
    s, dg = np.zeros((W, Pw)), np.zeros((W, Pw))
    args = (Pw, i32(np.full(W, Pw)), np.ones(W, np.uint8), i32(np.arange(W + 1) * per), nr, nf, cols, np.full(n, icgvins.HP_JAC_FROM_NAV, np.int64), None,
            np.full(int(nr.sum()), np.nan), s, dg, None, None, None, None, None, None, None, i32(np.arange(n)), nav_cols)
    out = {}

    def timed(name, scopes, call):
        out[name] = pc.timed_call(ctx, reps, call, scopes)

    def evaluate_and_correct():
        ctx.nav_evaluate_resident(points, point_off, want_jac=True)
        ctx.nav_correct_resident(robust, corr)

    def build():
        evaluate_and_correct()
        if ctx.reproj_host_parts_build_nav_raw(*args) != 0:
            raise RuntimeError(ctx.lib.icg_last_error(ctx.h).decode())

    timed("evaluate_resident_residual_only", ["nav_eval"], lambda: ctx.nav_evaluate_resident(points, point_off, want_jac=False))
    timed("evaluate_resident_with_jacobians", ["nav_eval"], lambda: ctx.nav_evaluate_resident(points, point_off, want_jac=True))
    timed("evaluate_and_correct", ["nav_eval", "nav_correct"], evaluate_and_correct)
    timed("evaluate_correct_and_build_gather", ["nav_eval", "nav_correct", "host_part_prior", "host_part"], build)
    ctx.close()
    return n, out, int(nr.sum()), int((nr * nf).sum())


def measure_shape(name, reps, n_windows=256):
    import harness as H
    import icgvins
    import nav_solve_data as nsd
    import oracle_lib
    import preint_odo_solve_data as os_
    import vio_data as vd
    states = SHAPES[name]
    n_nav, kernels, total_r, total_j = measure_kernels(states, n_windows, reps)
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
    modes = ("mode5", "mode5_nav")
    ms = {m: [] for m in modes}

    def run(mode, counted):
        nav = mode == "mode5_nav"
        rc, msg, st, inv, summ, _, n_dev = nsd.solve_nav_batch(lib, wins, starts, priors, 5, variant=2, device_nav=1 if nav else 0, gnss_huber=1.0, results=results,
                                                               iters=12, timer=ms[mode] if counted else None)
        if rc != 0:
            raise RuntimeError(f"icgh_backend_solve_nav_batch {mode} rc={rc}: {msg}")
        assert n_dev == (n_nav if nav else 0), (mode, n_dev, n_nav)
        return st + inv + [summ]

    def compare(mode, got, ref):
        for a, b in zip(got, ref):
            assert np.array_equal(bits(a), bits(b)), f"{mode} differs from mode5"

    summ = pc.alternate_modes(modes, reps, run, compare)["mode5"][-1]
    best = {m: min(ms[m]) for m in modes}
    scatter = {m: max(ms[m]) - min(ms[m]) for m in modes}
    margin, worst = best["mode5"] - best["mode5_nav"], max(scatter.values())
    return {"shape": f"{name}: {states} states, {3 + states} navigation factors per window (Huber on the {states} GNSS factors), {states - 1} odometer "
                     "preintegration factors, a prior over all states",
            "windows": n_windows, "navigation_factors": n_nav, "lm_steps": [float(summ[:, 2].mean()), float(summ[:, 3].mean())], "kernels": kernels,
            "link_bytes_per_linearization_from_the_shapes": {
                "pool_path_up": (total_j + total_r) * 8,  # every factor's gathered Jacobian (its free columns: all but the seventh pose column) and residual
                "resident_path_up": sum(7 if len(m[1]) == 6 else 10 for m in window_members(states)) * n_windows * 8
                + n_nav * (3 * 8 + 1),  # the parameter blocks (7 or 10 wide), then three scalars and a mark per member for the correction
                "resident_path_down": n_nav * 8},  # one squared norm
            "solve_ms": {m: [round(t, 3) for t in ms[m]] for m in modes},
            "solve_ms_best": {m: round(best[m], 3) for m in modes},
            "solve_ms_median": {m: round(float(np.median(ms[m])), 3) for m in modes},
            "mode5_nav_against_mode5": {"best_ms_saved": round(margin, 3), "scatter_ms_mode5": round(scatter["mode5"], 3),
                                        "scatter_ms_mode5_nav": round(scatter["mode5_nav"], 3),
                                        "verdict": pc.verdict(margin, worst, "mode 5 + nav faster", "mode 5 + nav slower",
                                                              "not a result: the margin is below the scatter of the repetitions")},
            "results_bit_identical": True}


def assemble(opt, cpus, legs):
    return {"cpus": cpus, "host_pool_threads": min(16, cpus), "shapes": list(legs.values())}


if __name__ == "__main__":
    pc.main(__file__, {"--cpus": 0, "--reps": 3}, list(SHAPES), LEG_LIMIT_S, lambda leg, opt: measure_shape(leg, opt["--reps"]), assemble, solver_threads=True)
