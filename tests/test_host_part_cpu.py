"""The host-factor part of a window's reduced system without a GPU: the new C entry is exported, the host twin of the device kernel
(icgh_host_part_from_blocks) equals a restatement of the arithmetic contract bit for bit, the split of hostFactors moved nothing, and a
build of the host layer without the device entry says so by name."""
import ctypes as C

import numpy as np

import host_part_data as hp
import reduced_solve_utils as ru
import test_host_solver_cpu as ths
from ctypes_util import bits, ErrBuf, ptr

NOT_BUILT = "icg_reproj_host_parts_build is not in this build"


def test_entry_is_exported_and_listed(hiplib):
    import icgvins
    assert "icg_reproj_host_parts_build" in icgvins.EXPORTS
    assert hasattr(hiplib, "icg_reproj_host_parts_build")
    assert icgvins.HOST_PART_MAX_NR == icgvins.MARG_MAX_R == 1024


def test_twin_equals_the_contract_restated():
    import harness
    lib = C.CDLL(harness.HOST_LIB)
    wins = hp.batch()
    rc, msg, parts, s, dg = hp.twin(lib, hp.P_BATCH, wins)
    assert rc == 0, msg
    for w, win in enumerate(wins):
        part, sr, dr = hp.restate(hp.P_BATCH, win)
        assert np.array_equal(bits(parts[w]), bits(part)), w
        assert np.array_equal(bits(s[w]), bits(sr)) and np.array_equal(bits(dg[w]), bits(dr)), w
    # the batch sees the order of the blocks: the window built for it changes its bits when its blocks are permuted
    ow = hp.order_window()
    _, _, (a,), sa, _ = hp.twin(lib, 5, [ow])
    _, _, (b,), sb, _ = hp.twin(lib, 5, [dict(Pw=5, blocks=[ow["blocks"][k] for k in (0, 2, 1, 3)])])
    assert not np.array_equal(bits(a), bits(b))
    assert 0.0 < a[1] < 1e-15 and 0.9 < b[1] < 1.1  # cell (1, 0): ((1e16 + ~1) - 1e16) + 1e-16 against ((1e16 - 1e16) + ~1) + 1e-16
    # -0.0 products leave +0.0 (bit pattern 0) in the cell and in s
    rc, _, parts, s, _ = hp.twin(lib, 2, [wins[3]])
    assert bits(parts[0])[1] == 0 and bits(s[0])[0] == 0


def _parts(lib, problems, reduced_mode, part_mode):
    """icgh_backend_solve_batch_parts on solve_utils problems -> (rc, message, results as reduced_solve_utils.solve_batch_mode gives them)"""
    W = len(problems)
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    fac_off = off([P["obs"].shape[1] for P in problems])
    pose_off = off([P["start"]["poses"].shape[0] for P in problems])
    lm_off = off([len(P["start"]["invdepth"]) for P in problems])
    obs = np.ascontiguousarray(np.concatenate([P["obs"] for P in problems], axis=1))
    ii, jj, ll = (np.ascontiguousarray(np.concatenate([P[k] for P in problems]), np.int32) for k in ("ii", "jj", "ll"))
    poses = np.ascontiguousarray(np.concatenate([P["start"]["poses"] for P in problems]))
    ext = np.ascontiguousarray(np.stack([P["start"]["ext"] for P in problems]))
    inv = np.ascontiguousarray(np.concatenate([P["start"]["invdepth"] for P in problems]))
    td = np.array([P["start"]["td"] for P in problems], np.float64)
    prior = np.ascontiguousarray(np.concatenate([P["prior"] for P in problems]))
    summ, ms, err = np.zeros((W, 8)), C.c_double(0), ErrBuf()
    rc = lib.icgh_backend_solve_batch_parts(W, ptr(fac_off), ptr(pose_off), ptr(lm_off), ptr(obs), ptr(ii), ptr(jj), ptr(ll), ptr(poses), ptr(ext), ptr(inv), ptr(td),
                                            ptr(prior), C.c_double(30.0), C.c_double(1.0), 0, 0, 6, 18, C.c_double(5.991), ptr(summ), C.byref(ms), *err.args,
                                            int(reduced_mode), int(part_mode))
    out = [dict(poses=poses[pose_off[w]:pose_off[w + 1]], ext=ext[w], invdepth=inv[lm_off[w]:lm_off[w + 1]], td=td[w:w + 1], summary=summ[w])
           for w in range(W)]
    return rc, err.text(), out


def test_split_of_host_factors_moved_nothing_and_missing_entry_is_named():
    from stream_utils import ensure_oracle_host
    lib = C.CDLL(ensure_oracle_host())
    probs = ths._batch_problems()
    rc, msg, plain = ru.solve_batch_mode(lib, probs, None)
    assert rc == 0, msg
    rc, msg, parts = _parts(lib, probs, 0, 0)
    assert rc == 0, msg
    ru.assert_same_results(parts, plain)
    # the oracle-backed build has no icg_reproj_host_parts_build: nothing is computed, the entry is named
    rc, msg, _ = _parts(lib, probs, 0, 1)
    assert rc == -4 and NOT_BUILT in msg, (rc, msg)
    rc, msg, _, _, _ = hp.twin(lib, 5, [hp.order_window()])
    assert rc == -4 and NOT_BUILT in msg, (rc, msg)
