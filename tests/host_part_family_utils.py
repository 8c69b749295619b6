"""Shared by the GPU tests of the host-part entries with device-resident blocks (test_gpu_marg_prior_resident.py and
test_gpu_host_part_{preint,preint_odo,nav}.py): the block description, the raw arguments and the call of any of the five entries, the
reference built from fetched values, and the resident sets and layouts that more than one of those files runs.

A layout is a list of windows, a window a list of blocks, a block ("ord", J, r, cols) or (family, member, member_cols, cols, how[, nr]) with
family "prior" / "preint" / "odo" / "nav" and how = "gather" / "keep"."""
import numpy as np

import marg_factor_data as mf
import preint_data as pd
import preint_odo_data as od
import preint_odo_split_data as osd
import preint_split_data as sd
import reproj_data as rd
from ctypes_util import bits, i32

FILL = 7.0
CODE = {"prior": -2, "preint": -3, "odo": -4, "nav": -5}  # ICG_HP_JAC_FROM_*; the families in the order the entries take their tables
ENTRIES = {"plain": 0, "prior": 1, "preint": 2, "odo": 3, "nav": 4}  # an entry -> how many families' tables it takes
ALL15 = np.array(list(range(0, 6)) + list(range(7, 16)) + list(range(16, 22)) + list(range(23, 32)), np.int32)  # all four blocks free
ALL34 = np.array(list(range(0, 6)) + list(range(7, 17)) + list(range(17, 23)) + list(range(24, 34)), np.int32)  # all four blocks free: 32 columns


# ---- the resident prior's columns and the partition (test_gpu_marg_prior_resident.py and the three family tests) -------------------------
def _columns(prior, drop=()):
    """the local columns of the prior's blocks in block order, without the blocks listed in drop -> (columns of J0, (block, local column) pairs)"""
    pc, src = [], []
    for b, (size, index) in enumerate(zip(prior["size"], prior["index"])):
        if b in drop:
            continue
        for x in range(mf.local(int(size))):
            pc.append(int(index) + x), src.append((b, x))
    return np.array(pc, np.int32), src


def _gathered(prior, jac, src):
    """the dense Jacobian of those columns from the blocks icg_marg_prior_evaluate ships (block b: r x size[b] row-major, blocks concatenated)"""
    r, off, blocks = prior["r"], 0, []
    for size in prior["size"]:
        blocks.append(jac[off:off + r * int(size)].reshape(r, int(size)))
        off += r * int(size)
    return np.ascontiguousarray(np.stack([blocks[b][:, x] for b, x in src], axis=1))


def _partition(ctx, W):
    w = rd.make_window(3, 2, seed=5)
    n, K, L = w["obs_soa"].shape[1], w["poses"].shape[0], len(w["invdepth"])
    ctx.reproj_set_factors(np.tile(w["obs_soa"], (1, W)), np.concatenate([w["idx_i"] + K * k for k in range(W)]),
                           np.concatenate([w["idx_j"] + K * k for k in range(W)]), np.concatenate([w["idx_lm"] + L * k for k in range(W)]))
    ctx.reproj_set_windows(n * np.arange(W + 1), L * np.arange(W + 1))


# ---- arguments, call, comparison, reference ------------------------------------------------------------------------------------------------
def nr_of(b):
    """the residuals of a resident block of the families whose count does not depend on the member"""
    return b[5] if b[0] == "prior" else {"preint": 15, "odo": 19}[b[0]]


def arrays(layout, Pw, rebuild, nr_of=nr_of):
    """the raw arguments of the host-part entries: every family's <family>_of and <family>_cols (None without a block of it); the resident
    blocks' slots in r are NaN"""
    blocks = [b for win in layout for b in win]
    a = dict(Pw=i32(Pw), rebuild=np.ascontiguousarray(rebuild, np.uint8), blk_off=i32(np.concatenate([[0], np.cumsum([len(w) for w in layout])])))
    nr, nf, cols, r, jac_off, Js, at = [], [], [], [], [], [], 0
    of = {f: [] for f in CODE}
    fc = {f: [] for f in CODE}
    for b in blocks:
        for f in CODE:
            of[f].append(b[1] if b[0] == f else -1)
        if b[0] == "ord":
            nr.append(b[1].shape[0]), nf.append(b[1].shape[1]), cols.append(b[3]), r.append(b[2])
            jac_off.append(at), Js.append(b[1].ravel())
            at += b[1].size
        else:
            nr.append(nr_of(b)), nf.append(len(b[3])), cols.append(b[3]), r.append(np.full(nr[-1], np.nan))
            fc[b[0]].append(b[2])
            jac_off.append(-1 if b[4] == "keep" else CODE[b[0]])
    cat = lambda xs, t: np.ascontiguousarray(np.concatenate(xs), t) if xs else None
    a.update(nr=i32(nr), nf=i32(nf), cols=cat(cols, np.int32), r=cat(r, np.float64), jac_off=np.ascontiguousarray(jac_off, np.int64), J=cat(Js, np.float64))
    for f in CODE:
        a[f + "_of"], a[f + "_cols"] = i32(of[f]), cat(fc[f], np.int32)
    return a


def call(ctx, a, W, entry, P=64, **over):
    """entry: "plain" / "prior" / "preint" / "odo" / "nav" with the tables it takes; over: arguments replaced for this call
    -> (rc, message, (s, diag, part per window or None), the whole part buffer)"""
    a = dict(a)
    a.update(over)
    sizes = [int(a["Pw"][w]) * (int(a["Pw"][w]) + 1) // 2 if a["rebuild"][w] else 0 for w in range(W)]
    s, dg, part = np.full((W, P), FILL), np.full((W, P), FILL), np.full(max(1, sum(sizes)), FILL)
    raw = getattr(ctx, {"plain": "reproj_host_parts_build_raw", "odo": "reproj_host_parts_build_preint_odo_raw"}.get(entry, f"reproj_host_parts_build_{entry}_raw"))
    tables = [a[f + key] for f in list(CODE)[:ENTRIES[entry]] for key in ("_of", "_cols")]
    rc = raw(P, a["Pw"], a["rebuild"], a["blk_off"], a["nr"], a["nf"], a["cols"], a["jac_off"], a["J"], a["r"], s, dg, part, *tables)
    parts, at = [], 0
    for w in range(W):
        parts.append(part[at:at + sizes[w]].copy() if a["rebuild"][w] else None)
        at += sizes[w]
    return rc, ctx.lib.icg_last_error(ctx.h).decode(), (s, dg, parts), part


def same(got, ref, rebuilt):
    (gs, gd, gp), (rs, rdg, rp) = got, ref
    for w in rebuilt:
        assert np.array_equal(bits(gp[w]), bits(rp[w])), ("part", w)
        assert np.array_equal(bits(gs[w]), bits(rs[w])) and np.array_equal(bits(gd[w]), bits(rdg[w])), ("s / diag", w)


def reference(ctx, layout, Pw, rebuild, sources, P=64):
    """icg_reproj_host_parts_build fed what the resident blocks hold: sources[family](block) -> (the numpy-gathered columns of the member's
    fetched Jacobian, its fetched residuals)"""
    wins = []
    for win in layout:
        out = []
        for b in win:
            J, r = (b[1], b[2]) if b[0] == "ord" else sources[b[0]](b)
            out.append((np.ascontiguousarray(J), r, b[3], False))
        wins.append(out)
    s, dg = np.full((len(layout), P), FILL), np.full((len(layout), P), FILL)
    return ctx.reproj_host_parts_build(P, Pw, wins, rebuild=rebuild, host_s=s, host_diag=dg)


def j32(J480):
    return np.concatenate([J480[0:105].reshape(15, 7), J480[105:240].reshape(15, 9), J480[240:345].reshape(15, 7), J480[345:480].reshape(15, 9)], axis=1)


def j34(J646):
    return np.concatenate([J646[0:133].reshape(19, 7), J646[133:323].reshape(19, 10), J646[323:456].reshape(19, 7), J646[456:646].reshape(19, 10)], axis=1)


def sources(prior=None, prior_res=None, prior_jac=None, fifteen=None, odo=None):
    """the sources of the families whose fetched values have one shape per family: fifteen, odo = (residuals, Jacobians) per factor"""
    return {"prior": lambda b: (_gathered(prior, prior_jac, _columns(prior)[1]), prior_res),
            "preint": lambda b: (j32(fifteen[1][b[1]])[:, b[2]], fifteen[0][b[1]]),
            "odo": lambda b: (j34(odo[1][b[1]])[:, b[2]], odo[0][b[1]])}


# ---- resident sets and layouts that more than one file runs --------------------------------------------------------------------------------
def unit(rng, n, scale):
    q = np.concatenate([rng.normal(0, scale, (n, 3)), np.ones((n, 1))], axis=1)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def resident_set15(ctx):
    """six factors (N E N E E N) of 21-sample intervals -> the two evaluations' arguments"""
    n = 6
    imus, states = sd.intervals([21] * n, seed0=70)
    off = (np.arange(n + 1) * 21).astype(np.int32)
    cur, delta, jac, cov, dt, pn = ctx.preint_batch(1, off, np.concatenate(imus), np.stack(states), pd.PARAMS)
    pn_rows = pn.reshape(n, 21, 4)[:, :20].reshape(-1, 4)
    pn_off = (np.arange(n + 1) * 20).astype(np.int32)
    env = np.tile(pd.PARAMS[5:9], (n, 1))
    pts = [np.stack([sd.eval_point(kind, states[i], cur[i]) for i in range(n)]) for kind in ("perturbed", "large_bias_step")]
    _, _, S, status = ctx.preint_evaluate_batch(1, delta, jac, cov, dt, env, pts[0], pn_off, pn_rows)
    assert np.all(status == 0)
    rng = np.random.RandomState(3)
    ctx.preint_set([0, 1, 0, 1, 1, 0], delta, jac, S, dt, env, unit(rng, n, 1e-5), pn_off, pn_rows)
    return pts, [unit(rng, n, 1e-3), unit(rng, n, 3e-2)]


def resident_set_odo(ctx):
    """six odometer factors (O E O E E O) of 21-sample intervals resident -> the two evaluations' (points, correction quaternions)"""
    n = 6
    variants = [2, 3, 2, 3, 3, 2]
    imus = [od._imu9(21, 80 + i) for i in range(n)]
    states = [od.state17(p=(i, 1, 0), v=(2, 0.1 * i, 0)) for i in range(n)]
    par25 = od.params25()
    off = (np.arange(n + 1) * 21).astype(np.int32)
    cur, delta, jac, cov, dt, pn = ctx.preint_odo_batch(3, off, np.concatenate(imus), np.stack(states), par25)
    pn_rows = pn.reshape(n, 21, 4)[:, :20].reshape(-1, 4)
    pn_off = (np.arange(n + 1) * 20).astype(np.int32)
    env = np.tile(par25[5:9], (n, 1))
    pts = [np.stack([osd.eval_point(kind, delta[i], cur[i], states[i]) for i in range(n)]) for kind in ("perturbed", "large_bias_step")]
    _, _, S, status = ctx.preint_odo_evaluate_batch(3, delta, jac, cov, dt, env, pts[0], pn_off, pn_rows)
    assert np.all(status == 0)
    rng = np.random.RandomState(4)
    ctx.preint_odo_set(variants, delta, jac, S, dt, env, unit(rng, n, 1e-5), pn_off, pn_rows)
    return pts, [unit(rng, n, 1e-3), unit(rng, n, 3e-2)]


def everything_resident(ctx):
    """the odometer set, a 15-state set and a prior set resident in one context, all evaluated at their first point"""
    pts, qcs = resident_set_odo(ctx)
    pts15, qcs15 = resident_set15(ctx)
    prior = mf.make_prior([7], 42)
    ctx.marg_prior_set(*mf.set_args([prior]))
    x = mf.make_x(prior, 100)
    ctx.marg_prior_evaluate_resident(x)
    ctx.preint_evaluate_resident(pts15[0], qcs15[0])
    ctx.preint_odo_evaluate_resident(pts[0], qcs[0])
    return pts, qcs, prior, x


def _ord(rng):
    return lambda nr, cols, scale=1.0: ("ord", rng.normal(0, scale, (nr, len(cols))), rng.normal(0, 1.0, nr), np.asarray(cols, np.int32))


def layout15(rng, prior, how):
    """the 15-state test's input: priors and 15-state factors -> (layout, Pw, rebuild)"""
    mk, pc, SECOND = _ord(rng), _columns(prior)[0], ALL15[15:]  # (SECOND: the first state constant)
    layout = [[("preint", 3, ALL15, np.arange(0, 30), how), ("preint", 1, ALL15, np.arange(15, 45), how)],  # two factors sharing the middle state's columns
              [("preint", 0, SECOND, np.arange(0, 15), how), mk(9, range(6, 15), 10.0)],  # the first state constant: nf = 15
              [mk(6, range(0, 6), 30.0), ("preint", 4, ALL15, 3 + rng.permutation(30), how), ("prior", 0, pc, np.arange(34, 40), how, prior["r"])],
              [],  # rebuilt, no host block
              [mk(3, [1, 5, 2]), ("preint", 5, ALL15, np.arange(30), how)],  # not rebuilt: its block only places the others' columns
              [("preint", 2, ALL15, rng.permutation(30), how)]]
    return layout, [45, 20, 40, 10, 30, 30], [1, 1, 1, 1, 0, 1]


def layout_odo(rng, prior, how):
    """the odometer test's input: priors, 15-state and odometer factors -> (layout, Pw, rebuild)"""
    mk, pc, SECOND = _ord(rng), _columns(prior)[0], ALL34[16:]
    layout = [[("odo", 3, ALL34, np.arange(0, 32), how), ("odo", 1, ALL34, np.arange(16, 48), how)],  # two factors sharing the middle state's columns
              [("odo", 0, SECOND, np.arange(0, 16), how), mk(9, range(6, 15), 10.0)],  # the first state constant: nf = 16
              [mk(6, range(0, 6), 30.0), ("odo", 4, ALL34, 3 + rng.permutation(32), how), ("prior", 0, pc, np.arange(36, 42), how, prior["r"])],
              [],  # rebuilt, no host block
              [mk(3, [1, 5, 2]), ("odo", 5, ALL34, np.arange(32), how)],  # not rebuilt: its block only places the others' columns
              [("preint", 2, ALL15, rng.permutation(30), how), ("odo", 2, ALL34, 30 + rng.permutation(32), how)]]  # a 15-state and an odometer factor
    return layout, [48, 20, 42, 10, 32, 62], [1, 1, 1, 1, 0, 1]
