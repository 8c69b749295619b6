"""The reduction rule of k_lm_min_w (host/lm_min_rule.h) on the host: icgh_lm_min_twin walks the kernel's 64 lanes — the strided passes, the
xor butterfly, the last look at the first landmark, all through the inline functions the kernel itself calls — and returns the sequential
loop of MarginalizationBatch's first guard beside it.  The two are equal as values on the cases a device test must not provoke: a NaN in
the first landmark (stays), NaN elsewhere (ignored), ties, zeros of both signs (== 0.0, the sign is not pinned), infinities, and runs
that span several passes of a lane.  Also: the entry is declared, exported, listed and wrapped."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "icg_reproj_landmark_min_windows"
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def twin():
    import harness
    lib = C.CDLL(harness.HOST_LIB)
    lib.icgh_lm_min_twin.restype = None

    def run(h):
        h = np.ascontiguousarray(h, np.float64)
        out = np.full(2, -7.0)
        lib.icgh_lm_min_twin(h.ctypes.data_as(C.c_void_p), int(len(h)), out.ctypes.data_as(C.c_void_p))
        return float(out[0]), float(out[1])
    return run


def loop(h):
    if len(h) == 0:
        return 0.0
    mn = h[0]
    for x in h:
        mn = x if x < mn else mn
    return float(mn)


def same_value(a, b):
    return (a != a and b != b) or a == b


def _cases():
    rng = np.random.RandomState(3)
    down = np.arange(130, 0, -1).astype(float)  # a descending run of 130: the minimum is the last element, in a lane's third pass
    mid = rng.uniform(1, 2, 130)
    mid[[5, 64, 70, 129]] = NAN
    c = {
        "empty": [], "one": [3.5], "one_nan": [NAN], "nan_first": np.concatenate([[NAN], down]), "nan_first_then_smaller": [NAN, -1.0, 2.0],
        "nan_middle": mid, "nan_last": [2.0, 1.0, NAN], "all_nan_but_first": [4.0] + [NAN] * 99, "all_equal": np.full(130, 0.25), "descending_130": down,
        "ascending_130": down[::-1], "ties_at_min": [3.0, 1.0, 2.0, 1.0] * 40, "zero_min_pos_first": [0.0, 1.0, -0.0, 2.0] + [5.0] * 70,
        "zero_min_neg_first": [-0.0, 1.0, 0.0, 2.0] + [5.0] * 70, "neg_zero_late": [1.0] * 64 + [-0.0] + [0.0] * 3, "inf_only": [INF] * 70,
        "inf_first": [INF, 3.0], "neg_inf": [1.0] * 100 + [-INF], "nan_and_inf": [INF, NAN, INF], "negative": -rng.uniform(1, 2, 300),
    }
    for n in (63, 64, 65, 127, 128, 129, 300):  # the minimum at every position of runs around the wave boundary
        base = rng.uniform(1, 2, n)
        for at in sorted({0, 1, 62, 63, 64, 65, n - 1} & set(range(n))):
            h = base.copy()
            h[at] = 0.5
            c["min_at_%d_of_%d" % (at, n)] = h
    return c


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_of_the_kernel_rule_equals_the_sequential_loop(twin, name):
    h = np.asarray(CASES[name], np.float64)
    got, ref = twin(h)
    exp = loop(h)
    assert same_value(ref, exp), (name, ref, exp)  # the C loop beside the twin is the loop stated here
    assert same_value(got, exp), (name, got, exp)


def test_the_cases_say_what_they_claim(twin):
    assert np.isnan(twin(CASES["nan_first"])[0]) and np.isnan(twin(CASES["nan_first_then_smaller"])[0]) and np.isnan(twin(CASES["one_nan"])[0])
    assert twin(CASES["nan_middle"])[0] == np.nanmin(CASES["nan_middle"]) and twin(CASES["all_nan_but_first"])[0] == 4.0
    assert twin(CASES["descending_130"])[0] == 1.0 and twin(CASES["all_equal"])[0] == 0.25 and twin(CASES["empty"])[0] == 0.0
    for name in ("zero_min_pos_first", "zero_min_neg_first", "neg_zero_late"):
        assert twin(CASES[name])[0] == 0.0  # (== : either zero)
    assert twin(CASES["inf_only"])[0] == INF and twin(CASES["neg_inf"])[0] == -INF


def test_entry_is_declared_exported_listed_and_wrapped(hiplib):
    import icgvins
    txt = open(os.path.join(ROOT, "include", "icgvins_hip.h")).read()
    at = txt.index("int " + ENTRY + "(")
    comment = txt[txt.rindex("/*", 0, at):at]
    assert "factors/marginalization_info.h:170-192" in comment and "mn = (h_ll[l] < mn) ? h_ll[l] : mn" in comment
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", code)
    assert hasattr(hiplib, ENTRY) and ENTRY in icgvins.EXPORTS and hasattr(icgvins.Context, "reproj_landmark_min_windows")
    src = open(os.path.join(ROOT, "ic-gvins_amd", "csrc", "reproj_schur.hip")).read()
    assert "k_lm_min_w" in src and "icg_lm_min::take" in src and '#include "../host/lm_min_rule.h"' in src  # the kernel calls the twin's functions
