"""What the probes of this directory share: the command line, the confinement to a rank's share of the CPUs, the runner that gives every
leg a child process of its own under a time limit and starts nothing after a failure, the result's way out, and the few measuring
helpers they all had copies of."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "ic-gvins_amd"), ROOT]


def parse_options(argv, defaults):
    """flags with integer values (defaults: flag -> value), `--leg NAME`, and what is left over: the optional output path -> (opt, leg, rest)"""
    argv, opt, leg = list(argv), dict(defaults), None
    if "--leg" in argv:
        k = argv.index("--leg")
        leg = argv[k + 1]
        del argv[k:k + 2]
    for flag in opt:
        if flag in argv:
            k = argv.index(flag)
            opt[flag] = int(argv[k + 1])
            del argv[k:k + 2]
    return opt, leg, argv


def confine(cpus, solver_threads=False):
    """the process (and its children) on the first `cpus` of the CPUs it may run on (0: all of them); solver_threads: the host pool of
    WindowSolverBatch gets one thread per CPU, 16 at the most -> the number of CPUs"""
    if cpus > 0:
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:cpus])
    n = len(os.sched_getaffinity(0))
    if solver_threads:
        os.environ["ICG_SOLVER_THREADS"] = str(min(16, n))
    return n


def run_legs(script, legs, limit_s, args):
    """every leg a child `python script --leg NAME args...` under `timeout -k 10 <limit>` (limit_s: seconds, or leg -> seconds), its stderr
    passed through, its result the last line of its stdout -> {leg: result}.  The first leg that ends with a non-zero status ends the
    run with that status: nothing further is started."""
    out = {}
    for name in legs:
        limit = limit_s[name] if isinstance(limit_s, dict) else limit_s
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(script), "--leg", name] + [str(a) for a in args]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(f"leg {name} ended with status {r.returncode}; nothing further is started\n{r.stdout[-2000:]}\n")
            sys.exit(r.returncode)
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
        sys.stderr.write(f"leg {name} done\n")
        sys.stderr.flush()
    return out


def emit(result, rest):
    """the result as one JSON line on stdout and, if a path was left on the command line, in that file"""
    txt = json.dumps(result)
    print(txt)
    if rest:
        open(rest[0], "w").write(txt + "\n")


def main(script, defaults, legs, limit_s, run_leg, assemble, solver_threads=False):
    """a probe's __main__.  As a child (--leg NAME): run_leg(NAME, opt) -> that leg's result.  Otherwise the runner: the legs one after
    the other with every option but --cpus handed on (the children inherit the confinement), then assemble(opt, cpus, {leg: result})"""
    opt, leg, rest = parse_options(sys.argv[1:], defaults)
    cpus = confine(opt["--cpus"], solver_threads)
    if leg is not None:
        print(json.dumps(run_leg(leg, opt)))
        return
    args = [a for flag in opt if flag != "--cpus" for a in (flag, opt[flag])]
    emit(assemble(opt, cpus, run_legs(script, legs, limit_s, args)), rest)


def stats(values):
    return {"best": round(min(values), 3), "median": round(statistics.median(values), 3), "scatter": round(max(values) - min(values), 3)}


def verdict(margin, scatter, won, lost, neither):
    """the project's rule: a margin that does not exceed the scatter of the repetitions (of either side) is not a result"""
    return won if margin > scatter else lost if -margin > scatter else neither


def best_of(reps, fn):
    """the shortest of reps calls, seconds"""
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return best


def timed_call(ctx, reps, call, scopes):
    """one untimed call, then reps calls each behind a sync: the shortest wall time and the profiler's time per launch of every scope"""
    call()
    ctx.prof_enable(True)
    best = None
    for _ in range(reps):
        ctx.lib.icg_ctx_sync(ctx.h)
        t0 = time.perf_counter()
        call()
        best = min(best or 1e9, time.perf_counter() - t0)
    prof = ctx.prof()
    ctx.prof_enable(False)
    out = {"python_call_ms": round(best * 1e3, 3)}
    for scope in scopes:
        k, ms = prof.get(scope, (0, 0.0))
        out[scope + "_ms"] = round(ms / max(k, 1), 4)
    return out


def resident_windows(window, W):
    """a context with W copies of one reproj_data window resident as W windows of one partition"""
    import icgvins
    w = window
    n, K, L = w["obs_soa"].shape[1], w["poses"].shape[0], len(w["invdepth"])
    rep = lambda a, step: np.concatenate([a + k * step for k in range(W)]).astype(np.int32)
    ctx = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64, max_factors=W * n)
    ctx.reproj_set_factors(np.tile(w["obs_soa"], (1, W)), rep(w["idx_i"], K), rep(w["idx_j"], K), rep(w["idx_lm"], L))
    ctx.reproj_set_windows(np.arange(W + 1, dtype=np.int32) * n, np.arange(W + 1, dtype=np.int32) * L)
    return ctx


def alternate_modes(modes, rounds, run, compare):
    """rounds + 1 passes over the modes, run(mode, counted) -> that mode's outputs; the first pass also sizes the buffers and is not
    counted.  compare(mode, outputs, outputs of modes[0]) for every other mode -> {mode: last outputs}"""
    last = {}
    for k in range(rounds + 1):
        for mode in modes:
            last[mode] = run(mode, k > 0)
    for mode in modes[1:]:
        compare(mode, last[mode], last[modes[0]])
    return last
