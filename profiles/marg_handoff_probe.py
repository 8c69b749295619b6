"""The M3 -> M4 hand-off on the device against shipping, on the product libraries: 256 priors of the C2 estimator shape (P = 157, m = 15,
r = 142; 9 x (7, 9) + 7 + 1) and 256 of the C4 shape (P = 232, m = 15, r = 217; 14 x (7, 9) + 7 + 1).
Per shape the host layer's chain (icgh_backend_marg_handoff_chain): the M3 of all windows in one device call — the device half of a
batched marginalization, the part that produces J0 / e0 — then MarginalizationPriorSet::set on a second context, then one resident
evaluation.  Mode "shipped": icg_marg_linearize_batch, set packs and uploads every J0.  Mode "handed_off": icg_marg_linearize_batch_keep,
set goes through icg_marg_prior_set_from_kept.  The two modes ALTERNATE in one process, `--runs` runs each (default 3), one timed pass per
run behind an untimed one; per phase best and median over the runs, and the device time of the set's store kernel from the context's
profiler.  By the project's rule a margin below the scatter (max - min over the runs) of either mode is "not a result".
`python profiles/marg_handoff_probe.py [out.json] [--cpus 2] [--runs 3]`; --cpus N confines the process to N of the CPUs it may run on
before any library is loaded.  Every shape is a leg: a child process of its own under a time limit; the first leg that fails ends the run.
Run by hand; not part of bench.py."""
import ctypes as C

import numpy as np

import probe_common as pc
from ctypes_util import ErrBuf, bits, ptr

PHASES = ("linearize_ms", "set_ms", "resident_evaluate_ms")
SHAPES = {"C2": ("C2: P = 157, m = 15; 9 x (7, 9) + 7 + 1", 157, 15, "C2_SIZES"), "C4": ("C4: P = 232, m = 15; 14 x (7, 9) + 7 + 1", 232, 15, "C4_SIZES")}
LEG_LIMIT_S = 60  # the whole probe, both shapes in one process at its defaults, took 4.7 s: twice that, rounded up to a full minute


def chain(lib, mode, lin_args, set_args, x, n):
    P, m, H, b = lin_args
    block_off, block_size, block_index, x0 = set_args
    sq, handed, ms, kern = np.zeros(n), np.zeros(1, np.int32), np.zeros(3), np.zeros(1)
    err = ErrBuf()
    rc = lib.icgh_backend_marg_handoff_chain(mode, n, ptr(P), ptr(m), ptr(H), ptr(b), C.c_double(1e-8), ptr(block_off), ptr(block_size), ptr(block_index),
                                             ptr(x0), ptr(x), 1, ptr(sq), ptr(handed), ptr(ms), ptr(kern), *err.args)
    if rc != 0:
        raise RuntimeError(f"icgh_backend_marg_handoff_chain mode {mode} rc={rc}: {err.text()}")
    return sq, int(handed[0]), ms, float(kern[0])


def measure_shape(lib, name, P, m, sizes, runs, n_windows=256):
    import marg_factor_data as mf
    import marg_linearize_data as ml
    systems = [ml.spd_system(P, m, 5000 + w) for w in range(n_windows)]
    priors = [mf.make_prior(sizes, 7000 + w) for w in range(n_windows)]
    assert priors[0]["r"] == P - m
    a = mf.pack(priors)
    x = np.concatenate([mf.make_x(p, 9000 + w, negate=(0,)) for w, p in enumerate(priors)])
    lin_args, set_args = ml.pack(systems), (a["block_off"], a["block_size"], a["block_index"], a["x0"])
    r = P - m
    out = {"shape": name, "windows": n_windows, "r": r, "J0_MB": round(n_windows * r * r * 8 / 1e6, 1)}
    rec = {"shipped": [], "handed_off": []}
    sq_ref = None
    for _ in range(runs):
        for mode, key in ((0, "shipped"), (1, "handed_off")):
            sq, handed, ms, kern = chain(lib, mode, lin_args, set_args, x, n_windows)
            assert handed == (n_windows if mode else 0), (key, handed)
            sq_ref = sq if sq_ref is None else sq_ref
            assert np.array_equal(bits(sq), bits(sq_ref)), key  # the same priors whichever way they came
            rec[key].append(dict(zip(PHASES, ms), chain_ms=float(ms.sum()), store_kernel_ms=kern))
    for key, rows in rec.items():
        out[key] = {k: pc.stats([row[k] for row in rows]) for k in PHASES + ("chain_ms", "store_kernel_ms")}
    verdict = {}
    for k in ("set_ms", "chain_ms"):
        s, h = out["shipped"][k], out["handed_off"][k]
        margin = s["median"] - h["median"]
        verdict[k] = {"margin_ms_median": round(margin, 3),
                      "result": pc.verdict(margin, max(s["scatter"], h["scatter"]), "handed off is faster", "shipped is faster", "not a result")}
    out["shipped_minus_handed_off"] = verdict
    return out


def run_leg(leg, opt):
    import harness as H
    import marg_factor_data as mf
    name, P, m, sizes = SHAPES[leg]
    return measure_shape(C.CDLL(H.HOST_LIB), name, P, m, getattr(mf, sizes), opt["--runs"])


def assemble(opt, cpus, legs):
    return {"cpus": cpus, "runs_per_mode": opt["--runs"], "shapes": list(legs.values())}


if __name__ == "__main__":
    pc.main(__file__, {"--cpus": 0, "--runs": 3}, list(SHAPES), LEG_LIMIT_S, run_leg, assemble)
