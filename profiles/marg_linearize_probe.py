"""M3 (Schur step on the pose / mix block + linearization, marginalization_info.h:153-192) for many windows in one device call against
the same systems on the host pool, on the product libraries: 256 reduced systems of the C2 shape (P = 157, m = 15, r = 142: the working
matrix lives in LDS) and 256 of the C4 shape (P = 232, m = 15, r = 217: global scratch).  Per shape: icg_marg_linearize_batch with J0 / e0
only and with every output — device time of the kernels (the context's profiler: HIP events around the launches) and wall time of the call
including its transfers — then the host layer's entry (icgh_backend_marg_linearize mode 1) and mode 0 (linearizeReduced per window on a
HostPool).  Last leg: icgh_backend_marginalize_batch on 256 C2 windows, mode 0 (host step 4) against mode 2 (setDeviceLinearization).
`python profiles/marg_linearize_probe.py [out.json] [--threads 16] [--cpus 2] [--reps 5]`; --cpus N confines the legs to N of the CPUs the
process may run on (one rank's share of a node).  Every leg is a child process of its own under a time limit; the first leg that fails
ends the run.  ICG_PROBE_HOST_LIB: another build of the host layer (as in marg_batch_probe.py; the
c_abi leg is the device library's own and does not depend on it).  Run by hand; not part of bench.py."""
import ctypes as C
import os

import numpy as np

import probe_common as pc

SHAPES = {"C2": (157, 15), "C4": (232, 15)}
LEG_LIMIT_S = {"C2": 240, "C4": 300, "batch": 240}


def measure_shape(name, threads, reps, n_windows=256):
    import harness as H
    import icgvins
    import marg_linearize_data as ml
    P, m = SHAPES[name]
    systems = [ml.spd_system(P, m, 7000 + w) for w in range(n_windows)]
    packed = ml.pack(systems)
    r = P - m
    out = {"shape": f"{name}: P = {P}, m = {m}, r = {r}", "windows": n_windows, "H_MB": round(n_windows * P * P * 8 / 1e6, 1),
           "J0_MB": round(n_windows * r * r * 8 / 1e6, 1)}
    ctx = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    out["c_abi"] = {}
    for form, want in (("J0_e0", False), ("all_outputs", True)):
        kw = dict(want_Hp=want, want_bp=want, want_evals=want, want_min_ev=want, want_status=True)
        res = ctx.marg_linearize_batch(*packed, **kw)  # (the first call also grows the staging arena and the scratch)
        ctx.prof_enable(True)
        best = pc.best_of(reps, lambda: ctx.marg_linearize_batch(*packed, **kw))
        kern = {key + "_ms": round(ms / n, 3) for key, (n, ms) in ctx.prof().items() if key.startswith("marg_lin") and n}
        ctx.prof_enable(False)
        out["c_abi"][form] = dict(kern, call_wall_ms_incl_transfers_best=round(best * 1e3, 3), status_or=int(np.bitwise_or.reduce(res["status"])))
    ctx.close()
    hl = C.CDLL(os.environ.get("ICG_PROBE_HOST_LIB") or H.HOST_LIB)
    rc, msg, o1, s1 = ml.backend_marg_linearize(hl, 1, systems, reps=reps)
    if rc != 0:
        raise RuntimeError(f"icgh_backend_marg_linearize mode 1 rc={rc}: {msg}")
    rc, msg, o0, s0 = ml.backend_marg_linearize(hl, 0, systems, host_threads=threads, reps=reps)
    if rc != 0:
        raise RuntimeError(f"icgh_backend_marg_linearize mode 0 rc={rc}: {msg}")
    scale = float(np.abs(o0["Hp"]).max())
    out["host_layer"] = {"host_pool_threads": int(threads), "device_call_ms": round(s1[0] * 1e3, 3), "device_kernel_ms": round(s1[1] * 1e3, 3),
                         "host_pool_ms": round(s0[0] * 1e3, 3), "max_abs_Hp_difference_over_scale": float(np.abs(o1["Hp"] - o0["Hp"]).max() / scale),
                         "J0_e0_bit_identical": bool(ml.same_bits(o1["J0"], o0["J0"]) and ml.same_bits(o1["e0"], o0["e0"]))}
    return out


def measure_batch(threads, reps, n_windows=256):
    import backend_utils as bu
    import harness as H
    import marg_data as md
    hl = C.CDLL(os.environ.get("ICG_PROBE_HOST_LIB") or H.HOST_LIB)
    Pm = md.make_problem(n_lm=300, n_kf=10, seed=2)  # the C2 window of the bench's marginalization block
    bu.backend_marginalize_batch(hl, Pm, 8, 0)
    bu.backend_marginalize_batch(hl, Pm, 8, 2)
    a = bu.backend_marginalize_batch(hl, Pm, n_windows, 0, host_threads=threads, reps=reps)
    b = bu.backend_marginalize_batch(hl, Pm, n_windows, 2, host_threads=threads, reps=reps)
    return {"windows": n_windows, "reduced_system": f"P = {a['r'] + 6}, m = 6, r = {a['r']}", "host_pool_threads": int(threads),
            "mode0_host_step4_ms": round(a["seconds"] * 1e3, 3), "mode2_device_linearization_ms": round(b["seconds"] * 1e3, 3),
            "structured_dense": [[a["structured"], a["dense"]], [b["structured"], b["dense"]]],
            "max_abs_Hp_difference_over_scale": float(np.abs(a["Hp"] - b["Hp"]).max() / np.abs(a["Hp"]).max())}


def run_leg(leg, opt):
    return measure_batch(opt["--threads"], opt["--reps"]) if leg == "batch" else measure_shape(leg, opt["--threads"], opt["--reps"])


def assemble(opt, cpus, legs):
    return {"cpus": cpus, "host_pool_threads": opt["--threads"], "shapes": [legs[name] for name in SHAPES], "marginalize_batch": legs["batch"]}


if __name__ == "__main__":
    pc.main(__file__, {"--threads": 16, "--cpus": 0, "--reps": 5}, list(LEG_LIMIT_S), LEG_LIMIT_S, run_leg, assemble)
