"""profiles/probe_common.py and ic-gvins_amd/ctypes_util.py without a GPU: the leg runner on a tiny script (a leg's result collected, the
first failing leg ends the run with its status, nothing is started after it, a leg past its limit counts as failed), the option parser,
the statistics and the verdict, the bit views, the two pointer helpers and the error buffer."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

from ctypes_util import ErrBuf, bits, ptr, ptr_or_null, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import probe_common as pc  # noqa: E402

SCRIPT = """import os, sys, time
sys.path.insert(0, {profiles!r})
import probe_common as pc

def run_leg(leg, opt):
    if leg == "a":
        print("a line that is not the result")
        return {{"leg": "a", "reps": opt["--reps"]}}
    if leg == "b":
        sys.exit(3)
    if leg == "c":
        open({marker!r}, "w").write("started")
        return {{"leg": "c"}}
    time.sleep(30)

if __name__ == "__main__":
    pc.main(__file__, {{"--cpus": 0, "--reps": 3}}, {legs!r}, {{"a": 20, "b": 20, "c": 20, "d": 1}}, run_leg, lambda opt, cpus, legs: {{"cpus": cpus, "legs": legs}})
"""


def run(tmp_path, legs, *args):
    script, marker, out = tmp_path / "probe.py", tmp_path / "marker", tmp_path / "out.json"
    script.write_text(SCRIPT.format(profiles=os.path.join(ROOT, "profiles"), marker=str(marker), legs=list(legs)))
    r = subprocess.run([sys.executable, str(script), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return r, marker, out


def test_a_leg_result_is_collected_printed_and_written(tmp_path):
    r, _, out = run(tmp_path, "a", "--reps", "7")
    assert r.returncode == 0, r.stderr
    result = json.loads(r.stdout.strip().splitlines()[-1])
    assert result["legs"] == {"a": {"leg": "a", "reps": 7}} and result["cpus"] == len(os.sched_getaffinity(0))
    assert json.loads(out.read_text()) == result


def test_first_failing_leg_ends_the_run_with_its_status(tmp_path):
    r, marker, out = run(tmp_path, "abc")
    assert r.returncode == 3
    assert r.stdout == "" and not out.exists()  # no result, printed or written
    assert not marker.exists()  # leg c was not started
    assert "leg a done" in r.stderr and "leg b ended with status 3; nothing further is started" in r.stderr


def test_leg_past_its_limit_ends_the_run(tmp_path):
    r, marker, out = run(tmp_path, "adc")
    assert r.returncode == 124
    assert r.stdout == "" and not out.exists() and not marker.exists()


def test_parse_options():
    defaults = {"--cpus": 0, "--reps": 3}
    assert pc.parse_options([], defaults) == ({"--cpus": 0, "--reps": 3}, None, [])
    assert pc.parse_options(["out.json", "--reps", "5", "--leg", "C2", "--cpus", "2"], defaults) == ({"--cpus": 2, "--reps": 5}, "C2", ["out.json"])
    assert defaults == {"--cpus": 0, "--reps": 3}


def test_stats_and_verdict():
    assert pc.stats([3.0, 1.0004, 2.5, 1.5]) == {"best": 1.0, "median": 2.0, "scatter": 2.0}
    labels = ("faster", "slower", "not a result")
    assert pc.verdict(0.5, 0.2, *labels) == "faster"
    assert pc.verdict(0.1, 0.2, *labels) == "not a result" and pc.verdict(-0.1, 0.2, *labels) == "not a result"
    assert pc.verdict(-0.5, 0.2, *labels) == "slower"


def test_bit_views_and_pointers():
    nan = np.array([0x7ff8000000000000, 0x7ff8000000000001], np.uint64).view(np.float64)
    assert not np.array_equal(bits([0.0]), bits([-0.0])) and not same_bits([0.0], [-0.0])
    assert not np.array_equal(bits(nan[:1]), bits(nan[1:]))
    assert same_bits(nan[:1], nan[1:]) and not same_bits(nan[:1], [1.0])  # NaN in the same places: the payload is no result of IEEE arithmetic
    assert not same_bits(nan[:1], nan[1:], nan_payload=True) and same_bits(nan, nan, nan_payload=True) and not same_bits([0.0], [-0.0], nan_payload=True)
    assert same_bits([[1.0, -0.0]], [1.0, -0.0]) and bits(np.zeros((2, 3))).shape == (6,)
    assert ptr_or_null(np.zeros(0)) is None and ptr_or_null(None) is None and ptr(None) is None
    assert ptr(np.zeros(0)) is not None and ptr_or_null(np.zeros(1)) is not None


def test_error_buffer():
    err = ErrBuf(8)
    assert err.args[1] == 8 and err.value == b"" and err.text() == ""
    C.memmove(err.args[0], b"no\0", 3)
    assert err.value == b"no" and err.text() == "no"
    C.memmove(err, b"yes\0", 4)  # the object alone passes as its buffer
    assert err.text() == "yes"
