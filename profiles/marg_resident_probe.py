"""The reduced systems of a batched marginalization kept on the device between M2 and M3 (MarginalizationBatch::setDeviceReducedSystem)
against shipping them down and up again (setDeviceLinearization alone), on the product libraries: 256 windows of the bench's
marginalization shape (marg_data.make_problem(300, 10): P = 67, m = 6, r = 61, one 6-column host block) and 256 visual-inertial windows at
the estimator's width (10 states: P = 157, m = 15, r = 142; nine 15 x 30 preintegration blocks, a pose and a mix prior).
Per shape icgh_backend_marg_resident, mode 0 (device linearization) and mode 1 (+ device reduced system) ALTERNATING in one process,
`--runs` runs each (default 3), one timed marginalize() per run behind an untimed one on the same batch object; per phase and for the whole
call best, median and scatter (max - min) over the runs, the device time of marg_form_h and host_part from the context's profiler in a
pass of its own, and the bytes each mode moves for the reduced systems, computed from the shapes.  Every output of the two modes is
compared bit for bit.  By the project's rule a margin below the scatter of either mode's repetitions is "not a result".
`python profiles/marg_resident_probe.py [out.json] [--cpus 2] [--runs 3] [--windows 256]`; --cpus N confines the process to N of the CPUs
it may run on before any library is loaded (the pool is sized to them).  Every shape is a leg: a child process of its own under a time
limit; the first leg that fails ends the run.  Run by hand; not part of bench.py."""
import ctypes as C
import os

import numpy as np

import probe_common as pc
from ctypes_util import bits

PHASES = ("evaluate_ms", "bookkeeping_host_factors_ms", "assemble_eliminate_ms", "m3_linearize_ms", "marginalize_ms")
LEGS = ("bench", "estimator")
LEG_LIMIT_S = 60  # the whole probe, both shapes in one process at its defaults, took 7.4 s: twice that, rounded up to a full minute


def bytes_moved(n, P, m, blocks):
    """what crosses the link for the reduced systems and their right-hand sides, per mode (the factor upload, the evaluation and the prior
    coming down — Hp, bp, J0, e0 — are the same in both); blocks: (nr, nf) of a window's host factors"""
    r = P - m
    prior = n * (2 * r * r + 2 * r + 2) * 8
    mode0 = {"down": n * (P * P + 2 * P + 1) * 8, "up": n * (P * P + P) * 8}
    blk = sum(a * f * 8 + a * 8 + f * 4 for a, f in blocks)
    mode1 = {"down": n * (4 * P + 1) * 8, "up": n * (blk + P * 8)}
    for d in (mode0, mode1):
        d["prior_down"] = prior
        d["total_MB"] = round((d["down"] + d["up"] + prior) / 1e6, 2)
    return {"mode0": mode0, "mode1": mode1}


def measure_shape(lib, name, family, n, runs, threads, width, m, blocks, **kw):
    """kw: P = the visual problem (family 0) or vio = the windows (family 1), as marg_resident_data.backend_marg_resident takes them"""
    import marg_resident_data as mr
    out = {"shape": name, "windows": n, "P": width, "m": m, "r": width - m, "host_blocks_per_window": blocks, "bytes": bytes_moved(n, width, m, blocks)}
    rec, ref = {0: [], 1: []}, None
    for _ in range(runs):
        for mode in (0, 1):
            rc, msg, got = mr.backend_marg_resident(lib, mode, family, n, host_threads=threads, passes=2, **kw)
            if rc != 0:
                raise RuntimeError(f"icgh_backend_marg_resident mode {mode} rc={rc}: {msg}")
            assert got["structured"] == n and got["dense"] == 0 and (got["r"] == width - m).all(), (got["structured"], got["dense"])
            ref = got if ref is None else ref
            for k in ("Hp", "bp", "J0", "e0", "residuals"):
                assert np.array_equal(bits(got[k]), bits(ref[k])), (mode, k)  # the same priors whichever way H travelled
            rec[mode].append(dict(zip(PHASES, got["pass_ms"][1])))
    for mode in (0, 1):
        out[f"mode{mode}"] = {k: pc.stats([row[k] for row in rec[mode]]) for k in PHASES}
    rc, msg, got = mr.backend_marg_resident(lib, 1, family, n, host_threads=threads, passes=2, profile=True, **kw)
    if rc != 0:
        raise RuntimeError(msg)
    out["kernel_ms"] = {"marg_form_h": round(float(got["kernel_ms"][0]), 4), "host_part": round(float(got["kernel_ms"][1]), 4)}
    verdict = {}
    for k in ("m3_linearize_ms", "marginalize_ms"):
        a, b = out["mode0"][k], out["mode1"][k]
        margin, noise = a["median"] - b["median"], max(a["scatter"], b["scatter"])
        verdict[k] = {"margin_ms_median": round(margin, 3), "best_ratio_mode0_over_mode1": round(a["best"] / b["best"], 3),
                      "result": pc.verdict(margin, noise, "resident is faster", "shipping is faster", "not a result")}
    out["mode0_minus_mode1"] = verdict
    return out


def run_leg(leg, opt):
    import harness as H
    import marg_data as md
    import oracle_lib
    import vio_data as vd
    lib, n, runs = C.CDLL(H.HOST_LIB), opt["--windows"], opt["--runs"]
    threads = min(16, len(os.sched_getaffinity(0)))
    if leg == "bench":
        return measure_shape(lib, "bench marginalization shape: P = 67, m = 6", 0, n, runs, threads, 67, 6, [(6, 6)], P=md.make_problem(n_lm=300, n_kf=10, seed=2))
    base = [vd.make_vio_window(oracle_lib.load(), n_intervals=9, per=20, n_lm=120, seed=40 + k) for k in range(4)]
    return measure_shape(lib, "visual-inertial, estimator width: P = 157, m = 15", 1, n, runs, threads, 157, 15, [(15, 30)] * 9 + [(6, 6), (9, 9)],
                         vio=[base[w % len(base)] for w in range(n)])


def assemble(opt, cpus, legs):
    return {"cpus": cpus, "pool_threads": min(16, cpus), "runs_per_mode": opt["--runs"], "shapes": list(legs.values())}


if __name__ == "__main__":
    pc.main(__file__, {"--cpus": 0, "--runs": 3, "--windows": 256}, LEGS, LEG_LIMIT_S, run_leg, assemble)
