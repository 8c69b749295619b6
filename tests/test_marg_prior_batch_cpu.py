"""MarginalizationBatch::setDevicePrior (host/marg_batch.h) as far as it can be checked without a GPU, on a second-generation window built on
the oracle-backed host layer: the gather form with the prior deferred yields gatherHostBlocks' block list — the same nr, nf, columns and
places in r and cols for every block, the same Jacobian for every other block — with no Jacobian and no residual for the prior; what the
device gathers instead, J0[k][prior_cols[y]], holds the bytes gatherHostBlocks packs for the prior's block, and evaluateMargPrior's residual
is that block's r; the deferred evaluation leaves the factor as an eager Evaluate() does.  The switch's prerequisites are refused by
message, and a build without the entries says so by name.

Jacobian offsets: the deferred form keeps no room in J for the prior (its r x r Jacobian is what must not be shipped), so the blocks behind
the prior sit r * nf doubles earlier in J than in the eager form; their offsets are compared after that shift, their contents bit for bit."""
import ctypes as C

import numpy as np
import pytest

import marg_prior_data as mp
import marg_resident_data as mr
from ctypes_util import bits


def _oracle_host():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


def _product_host():
    import harness
    return C.CDLL(harness.HOST_LIB)


@pytest.fixture(scope="module")
def gathered():
    """windows 0 (as given) and 2 (jittered: the prior is evaluated away from x0) of the second generation"""
    lib, P, out = _oracle_host(), mr.visual_problem(), {}
    for which in (0, 2):
        rc, msg, got = mp.gather(lib, which, P)
        assert rc == 0, (which, rc, msg)
        out[which] = got
    return out


@pytest.mark.parametrize("which", [0, 2])
def test_deferred_gather_yields_the_block_list_of_gather_host_blocks(gathered, which):
    g = gathered[which]
    D, E, pb = g["deferred"], g["eager"], g["prior_block"]
    assert len(D) == len(E) >= 1 and 0 <= pb < len(D)
    assert D[pb]["nr"] == g["r"] and D[pb]["jac_off"] == -2 and D[pb]["J"] is None  # ICG_HP_JAC_FROM_PRIOR: no Jacobian was written
    assert not D[pb]["r"].any()  # the slots in r are reserved, nothing was evaluated into them
    shift = 0
    for k, (d, e) in enumerate(zip(D, E)):
        assert (d["nr"], d["nf"], d["c_at"], d["r_at"]) == (e["nr"], e["nf"], e["c_at"], e["r_at"]), k
        assert np.array_equal(d["cols"], e["cols"]), k
        if k == pb:
            shift = e["nr"] * e["nf"]
            continue
        assert d["jac_off"] == e["jac_off"] - shift, k
        assert np.array_equal(bits(d["J"]), bits(e["J"])) and np.array_equal(bits(d["r"]), bits(e["r"])), k
    assert g["sizes"][2] == g["sizes"][3] - E[pb]["nr"] * E[pb]["nf"]  # J is shorter by exactly the prior's Jacobian


@pytest.mark.parametrize("which", [0, 2])
def test_j0_gathered_by_prior_cols_is_the_prior_block_and_its_residual_is_evaluate_marg_prior(gathered, which):
    g = gathered[which]
    e = g["eager"][g["prior_block"]]
    pc = g["prior_cols"]
    assert len(pc) == e["nf"] and len(set(pc)) == len(pc) and pc.min() >= 0 and pc.max() < g["r"]
    assert np.array_equal(bits(g["J0"][:, pc]), bits(e["J"]))  # Jd[k][y] = J0[k][prior_cols[y]]: a copy
    assert np.array_equal(bits(g["prior_res"]), bits(e["r"]))
    assert e["J"].any() and e["r"].any()
    if which == 2:
        assert not np.array_equal(bits(gathered[0]["prior_res"]), bits(g["prior_res"]))  # (another window, another point)


@pytest.mark.parametrize("which", [0, 2])
def test_deferred_evaluation_equals_an_eager_evaluate(gathered, which):
    g = gathered[which]
    r = g["r"]
    assert len(g["def_eval"]) == len(g["eag_eval"]) > r + r * r  # residuals, then a Jacobian block per parameter block (a pose block is 7 wide)
    assert np.array_equal(bits(g["def_eval"]), bits(g["eag_eval"]))
    assert np.array_equal(bits(g["def_eval"][:r]), bits(g["prior_res"]))


def test_prerequisites_are_refused_by_message_and_a_build_without_the_entries_says_so():
    lib, P = _oracle_host(), mr.visual_problem()
    assert lib.icgh_backend_marg_prior_available() == 0 and _product_host().icgh_backend_marg_prior_available() == 1
    rc, msg, launches = mp.switch_alone(lib, P)
    assert rc == 1 and "setDevicePrior(true) needs setDeviceReducedSystem(true)" in msg, (rc, msg)
    for mode in range(4):  # the device linearization itself is what this build lacks: nothing is computed
        rc, msg, out = mp.backend_marg_prior_resident(lib, mode, mp.CHAIN_B, 3, P)
        assert rc == -4 and "icg_marg_linearize_batch is not in this build" in msg, (mode, rc, msg)
        assert not out["ok"].any() and out["device_priors"] == 0
    rc, msg, _ = mp.backend_marg_prior_resident(lib, 4, mp.CHAIN_A, 3, P)
    assert rc == -1 and "mode" in msg
    rc, msg, _ = mp.backend_marg_prior_resident(lib, 1, mp.CHAIN_A, 5, P, mixed=True)
    assert rc == -1 and "mixed" in msg
