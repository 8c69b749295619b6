"""GPU: MarginalizationBatch::setDevicePrior (host/marg_batch.h) — the previous marginalization's prior is evaluated and gathered on the
device, the first guard's minimum is reduced there — gives every output bit, ok, r, the tags and the structured / dense counts of
setDeviceReducedSystem alone, on six jittered second-generation windows (the prior is evaluated away from its linearization point):
chain A, both generations on one batch object (with keeping on, the resident set comes from the kept linearization), and chain B, a
default-path first generation (every prior is shipped once); a mixed batch with a window without a prior, a dense window, a robustified
prior and a first-guard failure; the chain twice on one object; the prerequisites.  No tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

import marg_prior_data as mp
import marg_resident_data as mr

pytestmark = pytest.mark.gpu

W = 6


@pytest.fixture(scope="module")
def lib():
    import harness
    return C.CDLL(harness.HOST_LIB)


@pytest.fixture(scope="module")
def runs(lib):
    """every (mode, chain, mixed) run the tests compare, computed once"""
    P, cache = mr.visual_problem(), {}

    def get(mode, chain, mixed=False, passes=1):
        key = (mode, chain, mixed, passes)
        if key not in cache:
            rc, msg, out = mp.backend_marg_prior_resident(lib, mode, chain, W, P, mixed=mixed, passes=passes)
            assert rc == 0, (key, rc, msg)
            cache[key] = out
        return cache[key]
    return get


def _same(a, b, what):
    assert np.array_equal(a["ok"], b["ok"]) and np.array_equal(a["r"], b["r"]), what
    assert (a["structured"], a["dense"]) == (b["structured"], b["dense"]), what
    assert np.array_equal(a["tag_slot"], b["tag_slot"]) and a["tagged"] == b["tagged"] and a["handed_off"] == b["handed_off"], what
    for w, (x, y) in enumerate(zip(mr.split(a), mr.split(b))):
        assert (x is None) == (y is None), (what, w)
        if x is not None:
            for k in x:  # Hp, bp, J0, e0 and the second context's residuals, as bit patterns
                assert np.array_equal(x[k], y[k]), (what, w, k)


@pytest.mark.parametrize("chain", [mp.CHAIN_A, mp.CHAIN_B])
def test_device_prior_equals_the_resident_reduced_system_bit_for_bit(lib, runs, chain):
    assert lib.icgh_backend_marg_prior_available() == 1
    ref, got = runs(0, chain), runs(1, chain)
    assert int(ref["ok"].sum()) == W and (ref["structured"], ref["dense"]) == (W, 0), ref
    assert ref["device_priors"] == ref["from_kept"] == ref["deferred"] == 0
    _same(got, ref, (chain, "mode 1 against mode 0"))
    parts = mr.split(ref)
    assert not np.array_equal(parts[0]["e0"], parts[-1]["e0"])  # (the windows are different problems)
    # every window has a plain prior and stays structured: all are taken, none is evaluated on the pool; nothing was kept
    assert (got["device_priors"], got["from_kept"], got["deferred"]) == (W, 0, 0)
    kept_ref, kept = runs(2, chain), runs(3, chain)
    _same(kept, kept_ref, (chain, "mode 3 against mode 2"))
    assert kept["tagged"] == W and sorted(kept["tag_slot"]) == list(range(W))
    for w, (x, y) in enumerate(zip(mr.split(kept), mr.split(ref))):  # keeping changes no bit either
        for k in x:
            assert np.array_equal(x[k], y[k]), (chain, "keep", w, k)
    # chain A: generation 1 was kept on the same object, its priors carry live tags and the set takes all of them from the kept buffer;
    # chain B: generation 1 ran on a default-path batch, every prior is shipped
    assert (kept["device_priors"], kept["from_kept"], kept["deferred"]) == (W, W if chain == mp.CHAIN_A else 0, 0)
    assert kept_ref["device_priors"] == kept_ref["from_kept"] == 0


@pytest.mark.parametrize("chain", [mp.CHAIN_A, mp.CHAIN_B])
def test_mixed_batch(runs, chain):
    ref = runs(0, chain, mixed=True)
    assert int(ref["ok"].sum()) == W
    # the window with a host factor on a leaving inverse depth and the one whose weak landmark fails the first guard take the dense path
    assert (ref["structured"], ref["dense"]) == (W - 2, 2), ref
    for keep in (0, 2):
        got = runs(keep | 1, chain, mixed=True)
        _same(got, runs(keep, chain, mixed=True), (chain, keep, "mixed"))
        for w, (x, y) in enumerate(zip(mr.split(got), mr.split(ref))):
            for k in x:
                assert np.array_equal(x[k], y[k]), (chain, keep, "mixed against mode 0", w, k)
        # taken: every window but the one without a prior and the one whose prior is robustified; of those the dense window and the
        # first-guard failure left the structured path and evaluated their prior on the pool after all
        assert got["device_priors"] == W - 2 and got["deferred"] == 2, got
        assert got["from_kept"] == (W - 2 if keep and chain == mp.CHAIN_A else 0), got


def test_chain_a_twice_on_one_batch_object(runs):
    for mode in (1, 3):
        once, twice = runs(mode, mp.CHAIN_A), runs(mode, mp.CHAIN_A, passes=2)
        _same(twice, once, ("two passes", mode))
        assert (twice["device_priors"], twice["from_kept"], twice["deferred"]) == (once["device_priors"], once["from_kept"], once["deferred"])


def test_device_prior_without_the_reduced_system_is_refused_and_launches_nothing(lib):
    rc, msg, launches = mp.switch_alone(lib, mr.visual_problem())
    assert rc == 1 and "setDevicePrior(true) needs setDeviceReducedSystem(true)" in msg, (rc, msg)
    assert launches == 0
