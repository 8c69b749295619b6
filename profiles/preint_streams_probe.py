"""What the re-integration of many streams costs through Preintegration::integrateBatch (mode 0: one icg_preint_batch launch per (variant,
parameter values) group, which with a station per stream is one launch per interval, and the square-root information of every result formed
serially on the calling thread) and through ::integrateStreams (mode 1: one icg_preint_batch_params call per variant, the square-root
information formed on the device behind the integration).  Shape: 256 streams, each with its own station, x 10 intervals x 41 samples;
Earth (15 states) and EarthOdo (19 states), one leg each: a child process under a time limit.
In a leg both modes run once untimed, then alternate `--reps` times; every run is an entry call that integrates all intervals twice on a
context of its own and reports the wall time around the second integrate call (the first pages the context's arena in), with the profiler
off.  One more run per mode with the profiler on gives the launch counts and the kernel times; mode 0's last run also times one host loop
that forms every square-root information again: the share of mode 0 that integrateBatch spends on it.
The yardstick is mode 0 on the same build: it is the path the callers have today.  A margin below the scatter of either mode is not a result.
`python profiles/preint_streams_probe.py [out.json] [--cpus 0] [--reps 3]`.  Run by hand; not part of bench.py."""
import ctypes as C

import numpy as np

import probe_common as pc

LEG_LIMIT_S = 240
N_STREAMS, N_INT, N_SAMPLES = 256, 10, 41


def measure(family, reps):
    import harness as H
    import preint_streams_data as sd
    fam = sd.FAMILIES[family]
    lib = C.CDLL(H.HOST_LIB)
    base = [fam.interval(N_SAMPLES, 200 + j) for j in range(N_INT)]
    items, stations = [], []
    for s in range(N_STREAMS):
        for j in range(N_INT):
            items.append((base[j], fam.state(0.05 * s + j)))
            stations.append([0.1 + 0.004 * s, 0.3 + 0.01 * s, 20.0 + s])
    n = len(items)
    rows = np.tile(fam.rows(1), (n, 1))
    hostrows = sd.host_rows(fam, rows, abv=np.tile(fam.abv(1), (n, 1)), stations=np.array(stations))

    def run(mode, profile):
        r = sd.streams(lib, fam, fam.earth, items, hostrows, mode, passes=2, profile=profile)
        if r["rc"] != 0:
            raise RuntimeError(f"{fam.host_entry} mode {mode} rc={r['rc']}: {r['msg']}")
        return r

    first = {mode: run(mode, False) for mode in (0, 1)}  # untimed; and the two modes agree
    f = sd.member_fields(fam)
    from ctypes_util import same_bits
    equal = all(same_bits(first[0]["members"][0][:, sl], first[1]["members"][0][:, sl]) for sl in f.values()) and \
        np.array_equal(first[0]["ready"][0], first[1]["ready"][0])
    ms = {0: [], 1: []}
    for _ in range(reps):
        for mode in (0, 1):
            ms[mode].append(run(mode, False)["seconds"][1] * 1e3)
    prof = {mode: run(mode, True) for mode in (0, 1)}
    out = {"shape": f"{N_STREAMS} streams x {N_INT} intervals x {N_SAMPLES} samples, a station per stream", "intervals": n, "variant": fam.earth,
           "members_equal_bit_for_bit": bool(equal), "ready": int(first[1]["ready"][0].sum())}
    for mode, name in ((0, "integrateBatch"), (1, "integrateStreams")):
        p = prof[mode]["prof"][0]  # after the two passes
        out[name] = {"integrate_call_ms": pc.stats(ms[mode]), "runs_ms": [round(v, 3) for v in ms[mode]],
                     "profiled_run": {"integrate_call_ms": round(prof[mode]["seconds"][1] * 1e3, 3), "launches_per_pass": {fam.p1: int(p[0]) // 2, fam.s: int(p[2]) // 2},
                                      "kernel_ms_per_pass": {fam.p1: round(p[1] / 2, 4), fam.s: round(p[3] / 2, 4)}}}
    s_loop = prof[0]["seconds"][-1] * 1e3
    b0, b1 = out["integrateBatch"]["integrate_call_ms"], out["integrateStreams"]["integrate_call_ms"]
    out["integrateBatch"]["host_sqrt_information_loop_ms"] = round(s_loop, 3)
    out["integrateBatch"]["host_sqrt_information_share_of_median"] = round(s_loop / b0["median"], 3)
    margin, scatter = b0["median"] - b1["median"], max(b0["scatter"], b1["scatter"])
    out["margin_ms_median"] = round(margin, 3)
    out["scatter_ms"] = round(scatter, 3)
    out["verdict"] = pc.verdict(margin, scatter, "integrateStreams is faster", "integrateStreams is slower", "not a result: the margin is inside the scatter")
    return out


if __name__ == "__main__":
    pc.main(__file__, {"--cpus": 0, "--reps": 3}, ["imu", "odo"], LEG_LIMIT_S, lambda leg, opt: measure(leg, opt["--reps"]),
            lambda opt, cpus, legs: {"cpus": cpus, "reps": opt["--reps"], "earth": legs["imu"], "earth_odo": legs["odo"]})
