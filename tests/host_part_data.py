"""Shared by the host-part tests (test_host_part_cpu.py, test_gpu_host_part.py): the heterogeneous batch of windows, the flat arrays of
icg_reproj_host_parts_build / icgh_host_part_from_blocks, the host twin, and the restatement of the arithmetic contract in plain loops.

A window is dict(Pw=columns, blocks=[(J nr x nf, r nr, cols nf), ...]); a batch shares one P."""
import ctypes as C

import numpy as np

from ctypes_util import ErrBuf, i32, ptr, ptr_or_null as p
from prior_solve_data import call_batch

P_BATCH = 157


def _block(rng, nr, cols, scale=1.0):
    cols = np.asarray(cols, np.int32)
    return rng.normal(0, scale, (nr, len(cols))), rng.normal(0, 1.0, nr), cols


def order_window():
    """three blocks (and a small fourth) on the same cells whose sums see the order: cell (1, 0) receives +1e16, +1, -1e16, +1e-16 and
    (1e16 + 1) - 1e16 = 0 while (1e16 - 1e16) + 1 = 1"""
    cols = np.array([0, 1, 2], np.int32)
    mk = lambda rows, r: (np.array(rows, np.float64), np.array(r, np.float64), cols)
    return dict(Pw=5, blocks=[mk([[1e8, 1e8, -1.0]], [1.0]), mk([[1.0, 1.0, 1e-8], [-1e-8, 1e-8, 1.0]], [-2.0, 1e8]), mk([[1e8, -1e8, 1.0]], [1e-8]),
                              mk([[1e-8, 1e-8, -1e8]], [3.0])])


def batch():
    """the windows the kernel can go wrong at, under the common P_BATCH; the order of the list is the order of the tests' one call"""
    rng = np.random.RandomState(2024)
    wins = []
    # Pw < P; a block whose columns descend and interleave two parameter blocks (6 .. 11 and 20 .. 28), and a 6-column block
    inter = [28, 11, 27, 10, 26, 9, 25, 8, 24, 7, 23, 6, 22, 21, 20]
    wins.append(dict(Pw=31, blocks=[_block(rng, 15, inter), _block(rng, 6, range(0, 6), 30.0)]))
    wins.append(dict(Pw=12, blocks=[]))  # no host factor at all: the part is zero
    wins.append(order_window())
    # products that are -0.0 only: cell (1, 0) = (-0.0 * 3) + (0.0 * -2) must be +0.0, and so must s[0] = -(-0.0 * 1 + 0.0 * -1)
    wins.append(dict(Pw=2, blocks=[(np.array([[-0.0, 3.0], [0.0, -2.0]]), np.array([1.0, -1.0]), np.array([0, 1], np.int32))]))
    wins.append(dict(Pw=70, blocks=[_block(rng, 1, rng.permutation(70)[:65])]))  # nr = 1, nf = 65: past one wave of columns
    wins.append(dict(Pw=9, blocks=[_block(rng, 257, [7, 2, 5])]))  # nr = 257: more rows than one staging pass and than threads
    # a chain of nine 15 x 30 blocks over overlapping column groups (ten states of 15 columns), a 6- and a 9-column block on state 0
    chain = [_block(rng, 15, range(15 * k, 15 * k + 30), 10.0) for k in range(9)]
    wins.append(dict(Pw=150, blocks=chain + [_block(rng, 6, range(0, 6), 100.0), _block(rng, 9, range(6, 15), 100.0)]))
    # the estimator's width: a dense 142 x 142 block (a marginalization prior) in a system of 157 columns, and a pose prior
    wins.append(dict(Pw=157, blocks=[_block(rng, 142, range(15, 157)), _block(rng, 6, range(0, 6), 30.0)]))
    return wins


def flat(P, wins):
    """-> dict of the C entry's arrays for a list of windows (every Jacobian shipped)"""
    blocks = [b for w in wins for b in w["blocks"]]
    f = dict(P=P, W=len(wins), Pw=np.array([w["Pw"] for w in wins], np.int32),
             blk_off=np.concatenate([[0], np.cumsum([len(w["blocks"]) for w in wins])]).astype(np.int32),
             nr=np.array([b[0].shape[0] for b in blocks], np.int32), nf=np.array([b[0].shape[1] for b in blocks], np.int32))
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts), dt) if parts else np.zeros(0, dt)
    f["cols"] = cat([np.asarray(b[2]).reshape(-1) for b in blocks], np.int32)
    f["r"] = cat([np.asarray(b[1]).reshape(-1) for b in blocks], np.float64)
    f["J"] = cat([np.asarray(b[0]).reshape(-1) for b in blocks], np.float64)
    f["jac_off"] = np.concatenate([[0], np.cumsum([b[0].size for b in blocks])])[:len(blocks)].astype(np.int64)
    f["cells"] = [int(w["Pw"]) * (int(w["Pw"]) + 1) // 2 for w in wins]
    return f


def twin(lib, P, wins):
    """icgh_host_part_from_blocks -> (rc, message, packed parts as a list, s W x P, diag W x P)"""
    f = flat(P, wins)
    part, s, dg = np.zeros(max(1, sum(f["cells"]))), np.full((f["W"], P), 7.0), np.full((f["W"], P), 7.0)
    err = ErrBuf()
    rc = lib.icgh_host_part_from_blocks(f["W"], int(P), p(f["Pw"]), p(f["blk_off"]), p(f["nr"]), p(f["nf"]), p(f["cols"]), p(f["jac_off"]), p(f["J"]),
                                        p(f["r"]), p(part), p(s), p(dg), *err.args)
    off = np.concatenate([[0], np.cumsum(f["cells"])])
    return rc, err.text(), [part[off[w]:off[w + 1]].copy() for w in range(f["W"])], s, dg


def restate(P, win):
    """The arithmetic contract in plain loops over numpy.float64 scalars, one multiply and one add per term: block values summed over k
    ascending from +0.0, cells / s / diag receiving them in block order.  -> (packed part, s, diag) of one window"""
    zero = np.float64(0.0)
    Pw = win["Pw"]
    part = [[zero] * (a + 1) for a in range(Pw)]
    s, dg = [zero] * P, [zero] * P
    for J, r, cols in win["blocks"]:
        nr, nf = J.shape
        Jl = [[np.float64(v) for v in row] for row in np.asarray(J, np.float64)]
        rl = [np.float64(v) for v in r]
        cols = [int(c) for c in cols]
        for x in range(nf):
            g = zero
            for k in range(nr):
                g = g + Jl[k][x] * rl[k]
            s[cols[x]] = s[cols[x]] - g
            for y in range(nf):
                a, b = cols[x], cols[y]
                if a < b:
                    continue
                t = zero
                for k in range(nr):
                    t = t + Jl[k][x] * Jl[k][y]
                part[a][b] = part[a][b] + t
                if a == b:
                    dg[a] = dg[a] + t
    return np.array([v for row in part for v in row], np.float64), np.array(s, np.float64), np.array(dg, np.float64)


def solve_vio_batch(lib, wins, starts, dense, mode, iters=25, prior_weight=100.0, huber=1.0, dense_weight=1.0, dense_seed=7, timer=None):
    """icgh_backend_solve_vio_batch on vio_data windows from the given (states, invdepth) starts -> (rc, message, states, invdepth, summary W x 4);
    a list given as timer receives the entry's own time of the solve in ms"""
    return call_batch(lib.icgh_backend_solve_vio_batch, wins, starts, mode, iters, prior_weight, huber, timer,
                      before=[ptr(i32(dense)), C.c_double(dense_weight), C.c_uint32(dense_seed)])[:5]
