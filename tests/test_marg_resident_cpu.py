"""The device-resident reduced system of the batched marginalization (icg_marg_linearize_resident,
MarginalizationBatch::setDeviceReducedSystem) as far as it can be checked without a GPU: the entry is declared with the reference code it
restates, exported and wrapped; a build of the host layer WITHOUT it (the oracle-backed checker library) says so and refuses by name; the
switch needs the device linearization; and the claim the whole mode rests on — the blocks a window ships, accumulated by the host twin of
icg_reproj_host_parts_build and mirrored, ARE planStructured's H and b, bit for bit."""
import ctypes as C
import os
import re

import numpy as np

import host_part_data as hp
import marg_resident_data as mr
from ctypes_util import bits, ErrBuf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "icg_marg_linearize_resident"


def _oracle_host():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


def _product_host():
    import harness
    return C.CDLL(harness.HOST_LIB)


def test_entry_is_declared_exported_listed_and_wrapped(hiplib):
    import icgvins
    txt = open(os.path.join(ROOT, "include", "icgvins_hip.h")).read()
    at = txt.index("int " + ENTRY + "(")
    comment = txt[txt.rindex("/*", 0, at):at]
    assert "factors/marginalization_info.h:195-230" in comment and "factors/marginalization_info.h:153-192" in comment
    assert "part[i (i + 1) / 2 + j] + S_w[i * P + j]" in comment  # the arithmetic is stated
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", code)
    assert hasattr(hiplib, ENTRY) and ENTRY in icgvins.EXPORTS
    assert hasattr(icgvins.Context, "marg_linearize_resident")
    src = open(os.path.join(ROOT, "ic-gvins_amd", "csrc", "marg_linearize.hip")).read()
    head = src[:src.index("#include")]
    assert "factors/marginalization_info.h:195-230" in head and "k_marg_form_h" in head
    host = _product_host()
    assert hasattr(host, "icgh_backend_marg_resident") and hasattr(host, "icgh_backend_marg_plan_blocks")
    assert host.icgh_backend_marg_resident_available() == 1  # the product library links the C ABI that has the three entries


def test_host_layer_without_the_entry_loads_and_refuses_by_name():
    lib = _oracle_host()
    assert lib.icgh_backend_marg_resident_available() == 0
    P = mr.visual_problem()
    for mode in (1, 3):
        rc, msg, out = mr.backend_marg_resident(lib, mode, 0, 3, P=P)
        assert rc == -4 and msg.startswith(ENTRY + " is not in this build"), (mode, rc, msg)
        assert not out["ok"].any() and not out["r"].any() and not out["phase_ms"].any() and out["structured"] == out["dense"] == 0  # nothing was computed
    # the switch off: what this build lacks is the device linearization itself
    rc, msg, _ = mr.backend_marg_resident(lib, 0, 0, 3, P=P)
    assert rc == -4 and "icg_marg_linearize_batch is not in this build" in msg, (rc, msg)
    rc, msg, _ = mr.backend_marg_resident(lib, 4, 0, 3, P=P)
    assert rc == -1 and "mode" in msg, (rc, msg)


def test_switch_without_the_device_linearization_is_refused_by_message():
    lib = _oracle_host()  # (a batch owns a context: on the product library this is checked with the GPU tests)
    err = ErrBuf()
    assert lib.icgh_backend_marg_resident_switch_alone(*err.args) == 1, err.value
    msg = err.text()
    assert "setDeviceReducedSystem(true) needs setDeviceLinearization(true)" in msg, msg


def _mirror(part, n):
    H = np.zeros((n, n))
    for i in range(n):
        H[i, :i + 1] = part[i * (i + 1) // 2:i * (i + 1) // 2 + i + 1]
        H[:i + 1, i] = H[i, :i + 1]
    return H


def _check_blocks_form_the_plan(got, twin_lib):
    n, win = got["P"], got["window"]
    assert win["blocks"], "the window has host factors"
    rc, msg, (part,), s, _ = hp.twin(twin_lib, n, [win])
    assert rc == 0, msg
    assert np.array_equal(bits(_mirror(part, n)), bits(got["H"]))
    assert np.array_equal(bits(s[0]), bits(got["b"]))
    assert np.array_equal(bits(got["H"]), bits(got["H"].T)) and got["H"].any() and got["b"].any()


def test_gathered_blocks_form_plan_h_and_b_bit_for_bit_visual():
    got = mr.plan_blocks(_oracle_host(), 0, 0, P=mr.visual_problem())
    assert got[0] == 0, got[1]
    got = got[2]
    assert got["m"] == 6 and [b[0].shape for b in got["window"]["blocks"]] == [(6, 6)]  # the pose prior on keyframe 0
    assert list(got["window"]["blocks"][0][2]) == list(range(6))
    _check_blocks_form_the_plan(got, _product_host())


def test_gathered_blocks_form_plan_h_and_b_bit_for_bit_visual_inertial(oracle):
    wins = mr.vio_windows(oracle)
    for which in (1, 3):  # four states and two
        got = mr.plan_blocks(_oracle_host(), 1, which, vio=wins)
        assert got[0] == 0, got[1]
        got = got[2]
        K = len(wins[which]["states"])
        assert got["m"] == 15 and got["P"] == 15 * K + 7
        # K - 1 preintegration factors over two (pose, mix) pairs, the pose prior and the mix prior of state 0; a 7-wide pose block gives 6 columns
        assert [b[0].shape for b in got["window"]["blocks"]] == [(15, 30)] * (K - 1) + [(6, 6), (9, 9)]
        _check_blocks_form_the_plan(got, _product_host())
