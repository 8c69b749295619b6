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
CPUs it may run on before any library is loaded (the pool is sized to them).  Every shape is a leg: a child process of its own under a
time limit; the first leg that fails ends the run.  Run by hand; not part of bench.py."""
import ctypes as C
import os
import sys

import numpy as np

import probe_common as pc
from ctypes_util import bits

PHASES = ("evaluate_ms", "bookkeeping_host_factors_ms", "assemble_eliminate_ms", "m3_linearize_ms", "marginalize_ms")
KERNELS = ("marg_eval", "host_part_prior", "host_part", "lm_min")
SHAPES = {"bench": ("bench marginalization shape, second generation: prior r = 61", 10), "estimator": ("estimator width, second generation: prior r = 151", 25)}  # keyframes
LEG_LIMIT_S = 60  # the whole probe, both shapes in one process at its defaults, took 16.2 s: twice that, rounded up to a full minute


def bytes_moved(n, r, n_lm, x_doubles):
    """what crosses the link for the previous prior and the first guard, per mode; everything else is the same in both"""
    off = {"up": n * (r * r + r) * 8, "down": n_lm * 8}  # the prior's Jacobian block and residual; every landmark diagonal
    on = {"up": n * x_doubles * 8, "down": n * 2 * 8}  # x; one squared norm and one minimum per window (the set comes from the kept buffer)
    for d in (off, on):
        d["total_MB"] = round((d["up"] + d["down"]) / 1e6, 3)
    return {"off": off, "on": on}


def measure_shape(lib, name, P, n, runs, threads):
    import marg_prior_data as mp
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
                assert np.array_equal(bits(got[k]), bits(ref[k])), (mode, k)  # the same priors wherever the previous one was read
            rec[mode].append(dict(zip(PHASES, list(got["phase_ms"]) + [float(got["wall_ms"][1])])))
            print(f"{name}: mode {mode}: {rec[mode][-1]['marginalize_ms']:.2f} ms", file=sys.stderr, flush=True)
            shape = int(got["r"][0])
    K, L = P["w"]["poses"].shape[0], len(P["w"]["invdepth"])
    r_prior = 6 * (K - 1) + 7
    n2 = int((P["w"]["idx_i"] == 1).sum())
    out = {"shape": name, "windows": n, "prior_r": r_prior, "r_after": shape, "second_table_factors_per_window": n2,
           "bytes": bytes_moved(n, r_prior, n * len(set(P["w"]["idx_lm"][P["w"]["idx_i"] == 1])), 7 * (K - 1) + 7 + 1)}
    for mode, key in ((2, "off"), (3, "on")):
        out[key] = {k: pc.stats([row[k] for row in rec[mode]]) for k in PHASES}
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
                      "result": pc.verdict(margin, noise, "device prior is faster", "pool prior is faster", "not a result")}
    out["off_minus_on"] = verdict
    return out


def run_leg(leg, opt):
    import harness as H
    import marg_data as md
    name, n_kf = SHAPES[leg]
    return measure_shape(C.CDLL(H.HOST_LIB), name, md.make_problem(n_lm=300, n_kf=n_kf, seed=2), opt["--windows"], opt["--runs"], min(16, len(os.sched_getaffinity(0))))


def assemble(opt, cpus, legs):
    return {"cpus": cpus, "pool_threads": min(16, cpus), "runs_per_mode": opt["--runs"], "shapes": list(legs.values())}


if __name__ == "__main__":
    pc.main(__file__, {"--cpus": 0, "--runs": 3, "--windows": 256}, list(SHAPES), LEG_LIMIT_S, run_leg, assemble)
