"""M4 (MarginalizationFactor::Evaluate) resident and batched on the device against the same evaluations on the host pool, on the product
libraries: 256 priors of the C2 estimator shape (9 x (7, 9) + 7 + 1, r = 142) and 256 of the C4 shape (14 x (7, 9) + 7 + 1, r = 217).
Per shape: icg_marg_prior_set once, then icg_marg_prior_evaluate in three forms — residual only; residual + gradient + squared norm; the
same with the Jacobian blocks — each with the device time of its kernels (the context's profiler: HIP events around the launches) and the
wall time of the call including its transfers; then the host layer's entry (icgh_backend_marg_factor mode 1: packing + the call) and
mode 0 (evaluateMargPrior per window on a HostPool).
`python profiles/marg_factor_probe.py [out.json] [--threads 16] [--cpus 2] [--reps 10]`; --cpus N confines the process to N of the CPUs it
may run on (one rank's share of a node) before any library is loaded.  Every shape is a leg: a child process of its own under a time
limit; the first leg that fails ends the run.  Run by hand; not part of bench.py."""
import ctypes as C

import numpy as np

import probe_common as pc
from ctypes_util import same_bits

SHAPES = {"C2": ("C2: 9 x (7, 9) + 7 + 1", "C2_SIZES"), "C4": ("C4: 14 x (7, 9) + 7 + 1", "C4_SIZES")}
LEG_LIMIT_S = 60  # the whole probe, both shapes in one process at its defaults, took 2.0 s: twice that, rounded up to a full minute
FORMS = {"residual": (False, False, False), "residual_gradient_sq_norm": (False, True, True), "with_jacobians": (True, True, True)}


def measure_shape(name, sizes, threads, reps, n_windows=256):
    import harness as H
    import icgvins
    import marg_factor_data as mf
    priors = [mf.make_prior(sizes, 7000 + w) for w in range(n_windows)]
    points = [[mf.make_x(p, 9000 + 1000 * k + w, negate=(k,)) for w, p in enumerate(priors)] for k in range(2)]
    x = [np.concatenate(pt) for pt in points]
    r, xs = priors[0]["r"], int(priors[0]["size"].sum())
    out = {"shape": name, "windows": n_windows, "r": r, "J0_MB": round(n_windows * r * r * 8 / 1e6, 1),
           "jacobians_MB_per_evaluation": round(n_windows * r * xs * 8 / 1e6, 1)}
    # --- the C ABI alone
    ctx = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    args = mf.set_args(priors)
    ctx.marg_prior_set(*args)  # (the first call also grows the staging arena and the resident buffers)
    out["c_abi"] = {"set_wall_us": round(pc.best_of(1, lambda: ctx.marg_prior_set(*args)) * 1e6, 1)}
    for form, (wj, wg, ws) in FORMS.items():
        for k in range(2):
            ctx.marg_prior_evaluate(x[k], want_jac=wj, want_grad=wg, want_sq_norm=ws)
        ctx.prof_enable(True)  # (clears the profiler's records)
        turn = iter(range(reps))
        best = pc.best_of(reps, lambda: ctx.marg_prior_evaluate(x[next(turn) & 1], want_jac=wj, want_grad=wg, want_sq_norm=ws))
        kern = {key + "_us": round(ms * 1e3 / n, 1) for key, (n, ms) in ctx.prof().items() if key in ("marg_eval", "marg_jac") and n}
        ctx.prof_enable(False)
        out["c_abi"][form] = dict(kern, call_wall_us_incl_transfers_best=round(best * 1e6, 1))
    ctx.close()
    # --- the host layer: device mode (packing + call) and the host pool, the same inputs
    hl = C.CDLL(H.HOST_LIB)
    out["host_layer"] = {"host_pool_threads": int(threads)}
    for form, want in FORMS.items():
        rc, msg, res1, jac1, grad1, sq1, sec1 = mf.backend_marg_factor(hl, 1, priors, points, want=want, reps=reps)
        if rc != 0:
            raise RuntimeError(f"icgh_backend_marg_factor mode 1 rc={rc}: {msg}")
        rc, msg, res0, jac0, grad0, sq0, sec0 = mf.backend_marg_factor(hl, 0, priors, points, want=want, host_threads=threads, reps=reps)
        if rc != 0:
            raise RuntimeError(f"icgh_backend_marg_factor mode 0 rc={rc}: {msg}")
        same = all(a is None or same_bits(a, b) for a, b in ((res1, res0), (jac1, jac0), (grad1, grad0), (sq1, sq0)))
        out["host_layer"][form] = {"device_set_us": round(sec1[0] * 1e6, 1), "device_evaluate_us_incl_packing_and_transfers": round(sec1[1] * 1e6, 1),
                                   "host_pool_evaluate_us": round(sec0[1] * 1e6, 1), "bit_identical": bool(same)}
    return out


def run_leg(leg, opt):
    import marg_factor_data as mf
    name, sizes = SHAPES[leg]
    return measure_shape(name, getattr(mf, sizes), opt["--threads"], opt["--reps"])


def assemble(opt, cpus, legs):
    return {"cpus": cpus, "shapes": list(legs.values())}


if __name__ == "__main__":
    pc.main(__file__, {"--threads": 16, "--cpus": 0, "--reps": 10}, list(SHAPES), LEG_LIMIT_S, run_leg, assemble)
