"""The previous marginalization's prior read from the device (MarginalizationBatch::setDevicePrior) against evaluating it on the pool and
shipping its r x r Jacobian as an ordinary block (setDeviceReducedSystem alone), on the product libraries: 256 SECOND-GENERATION windows —
each carries the prior its first marginalization left — at the bench's marginalization shape (marg_data.make_problem(300, 10): the prior
has r = 61) and at the estimator's width (make_problem(300, 25): visual windows of 25 keyframes, the prior has r = 151; the estimator's
visual-inertial window has r = 142).  Both generations run on ONE batch object with setKeepLinearized (chain A of
icgh_backend_marg_prior_resident: the resident set comes from the kept linearization), mode 2 (switch off) and mode 3 (on) ALTERNATING in
one process, `--runs` runs each (default 3), the timed generation-2 marginalize() of a second pass on the same object; per phase and for
the whole call best, median and scatter (max - min) over the runs, the device time of marg_eval, host_part_prior, host_part and lm_min from
the context's profiler in a pass of its own, and the bytes each mode moves for the prior and the first guard, computed from the shapes.
Every output of the two modes is compared bit for bit.  By the project's rule a margin below the scatter of either mode's repetitions is
"not a result".
`python profiles/marg_prior_resident_probe.py [out.json] [--cpus 2] [--runs 3] [--windows 256]`; --cpus N confines the process to N of the
CPUs it may run on before any library is loaded (the pool is sized to them).  Run by hand; not part of bench.py."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "ic-gvins_amd"), ROOT]

PHASES = ("evaluate_ms", "bookkeeping_host_factors_ms", "assemble_eliminate_ms", "m3_linearize_ms", "marginalize_ms")
KERNELS = ("marg_eval", "host_part_prior", "host_part", "lm_min")


def bytes_moved(n, r, n_lm, x_doubles):
    """what crosses the link for the previous prior and the first guard, per mode; everything else is the same in both"""
    off = {"up": n * (r * r + r) * 8, "down": n_lm * 8}  # the prior's Jacobian block and residual; every landmark diagonal
    on = {"up": n * x_doubles * 8, "down": n * 2 * 8}  # x; one squared norm and one minimum per window (the set comes from the kept buffer)
    for d in (off, on):
        d["total_MB"] = round((d["up"] + d["down"]) / 1e6, 3)
    return {"off": off, "on": on}


def measure_shape(lib, name, P, n, runs, threads):
    import marg_prior_data as mp
    import marg_resident_data as mr
    rec, ref, shape = {2: [], 3: []}, None, None
    for _ in range(runs):
        for mode in (2, 3):
            rc, msg, got = mp.backend_marg_prior_resident(lib, mode, mp.CHAIN_A, n, P, host_threads=threads, passes=2)
            if rc != 0:
                raise RuntimeError(f"icgh_backend_marg_prior_resident mode {mode} rc={rc}: {msg}")
            assert got["structured"] == n and got["dense"] == 0 and got["deferred"] == 0, (got["structured"], got["dense"], got["deferred"])
            assert (got["device_priors"], got["from_kept"]) == ((n, n) if mode == 3 else (0, 0)), (mode, got["device_priors"], got["from_kept"])
            ref = got if ref is None else ref
            for k in ("Hp", "bp", "J0", "e0", "residuals"):
                assert np.array_equal(mr.bits(got[k]), mr.bits(ref[k])), (mode, k)  # the same priors wherever the previous one was read
            rec[mode].append(dict(zip(PHASES, list(got["phase_ms"]) + [float(got["wall_ms"][1])])))
            print(f"{name}: mode {mode}: {rec[mode][-1]['marginalize_ms']:.2f} ms", file=sys.stderr, flush=True)
            shape = int(got["r"][0])
    K, L = P["w"]["poses"].shape[0], len(P["w"]["invdepth"])
    r_prior = 6 * (K - 1) + 7
    n2 = int((P["w"]["idx_i"] == 1).sum())
    out = {"shape": name, "windows": n, "prior_r": r_prior, "r_after": shape, "second_table_factors_per_window": n2,
           "bytes": bytes_moved(n, r_prior, n * len(set(P["w"]["idx_lm"][P["w"]["idx_i"] == 1])), 7 * (K - 1) + 7 + 1)}
    for mode, key in ((2, "off"), (3, "on")):
        out[key] = {k: {"best": round(min(v), 3), "median": round(statistics.median(v), 3), "scatter": round(max(v) - min(v), 3)}
                    for k in PHASES for v in [[row[k] for row in rec[mode]]]}
    out["kernel_ms"] = {}
    for mode, key in ((2, "off"), (3, "on")):
        rc, msg, got = mp.backend_marg_prior_resident(lib, mode, mp.CHAIN_A, n, P, host_threads=threads, passes=2, profile=True)
        if rc != 0:
            raise RuntimeError(msg)
        out["kernel_ms"][key] = {k: round(float(v), 4) for k, v in zip(KERNELS, got["kernel_ms"])}
    verdict = {}
    for k in ("bookkeeping_host_factors_ms", "assemble_eliminate_ms", "marginalize_ms"):
        a, b = out["off"][k], out["on"][k]
        margin, noise = a["median"] - b["median"], max(a["scatter"], b["scatter"])
        verdict[k] = {"margin_ms_median": round(margin, 3), "best_ratio_off_over_on": round(a["best"] / b["best"], 3),
                      "result": "device prior is faster" if margin > noise else ("pool prior is faster" if -margin > noise else "not a result")}
    out["off_minus_on"] = verdict
    return out


def measure(runs=3, n=256):
    import harness as H
    import marg_data as md
    lib = C.CDLL(H.HOST_LIB)
    threads = min(16, len(os.sched_getaffinity(0)))
    return {"cpus": len(os.sched_getaffinity(0)), "pool_threads": threads, "runs_per_mode": runs,
            "shapes": [measure_shape(lib, "bench marginalization shape, second generation: prior r = 61", md.make_problem(n_lm=300, n_kf=10, seed=2), n, runs, threads),
                       measure_shape(lib, "estimator width, second generation: prior r = 151", md.make_problem(n_lm=300, n_kf=25, seed=2), n, runs, threads)]}


if __name__ == "__main__":
    argv = sys.argv[1:]
    opt = {"--cpus": 0, "--runs": 3, "--windows": 256}
    for flag in list(opt):
        if flag in argv:
            k = argv.index(flag)
            opt[flag] = int(argv[k + 1])
            del argv[k:k + 2]
    if opt["--cpus"] > 0:
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:opt["--cpus"]])
    txt = json.dumps(measure(runs=opt["--runs"], n=opt["--windows"]))
    print(txt)
    if argv:
        open(argv[0], "w").write(txt + "\n")
