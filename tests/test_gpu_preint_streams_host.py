"""GPU: Preintegration::integrateStreams / PreintegrationOdo::integrateStreams against integrateBatch on the same intervals, through
icgh_backend_preint_streams / icgh_backend_preint_odo_streams (mode 0 = integrateBatch, 1 = integrateStreams).

8 streams with 8 different stations (has_station: every interval derives its Earth rate from its own start position) x 5 intervals of 41,
41, 7, 2 and 1 samples, Earth and EarthOdo; and a Normal / Odo list with two distinct plain rows.  Mode 1 leaves every member as mode 0
does, bit for bit (NaN in the same places: the host forms the square-root information of mode 0, the device that of mode 1), with the same
ready(); the profiler counts one integration launch per distinct (variant, row) group in mode 0 (40 for the Earth lists) and one per variant
present in mode 1; a clean list launches nothing; after reintegration(state) of three intervals one call integrates exactly those."""
import ctypes as C

import numpy as np
import pytest

import preint_streams_data as sd
from ctypes_util import bits, same_bits

pytestmark = pytest.mark.gpu

LENS = (41, 41, 7, 2, 1)
N_STREAMS = 8
REDO = (0, 16, 37)  # 41, 41 and 7 samples: results with a regular covariance


@pytest.fixture(scope="module")
def hostlib():
    import harness
    return C.CDLL(harness.HOST_LIB)


def _earth_list(fam):
    items, rows, stations = [], [], []
    base = fam.rows(N_STREAMS)
    for s in range(N_STREAMS):
        for j, n in enumerate(LENS):
            items.append((fam.interval(n, 100 + 5 * s + j), fam.state(0.5 * s + j)))
            rows.append(base[s])
            stations.append([0.2 + 0.1 * s, 0.5 + 0.2 * s, 30.0 + 10.0 * s])
    abv = np.repeat(fam.abv(N_STREAMS), len(LENS), axis=0)
    return items, sd.host_rows(fam, np.stack(rows), abv=abv, stations=np.array(stations))


@pytest.fixture(scope="module")
def earth_runs(hostlib):
    out = {}
    for name, fam in sd.FAMILIES.items():
        items, hostrows = _earth_list(fam)
        redo_state = np.stack([fam.state(9.0 + k) for k in range(len(REDO))])
        out[name] = {mode: sd.streams(hostlib, fam, fam.earth, items, hostrows, mode, redo=REDO, redo_state=redo_state) for mode in (0, 1)}
        out[name]["items"] = items
    return out


def _same_members(fam, a, b, stage):
    for name, sl in sd.member_fields(fam).items():
        assert same_bits(a["members"][stage][:, sl], b["members"][stage][:, sl]), (stage, name)
    assert np.array_equal(a["ready"][stage], b["ready"][stage])
    assert np.array_equal(a["pn_doubles"][stage], b["pn_doubles"][stage])
    assert np.array_equal(bits(a["pn"][stage]), bits(b["pn"][stage]))


@pytest.mark.parametrize("family", ["imu", "odo"])
def test_streams_leave_what_integrate_batch_leaves(earth_runs, family):
    fam, r = sd.FAMILIES[family], earth_runs[family]
    a, b = r[0], r[1]
    assert a["rc"] == 0 and b["rc"] == 0, (a["msg"], b["msg"])
    f = sd.member_fields(fam)
    for stage in (0, 1):
        _same_members(fam, a, b, stage)
        assert not np.any(bits(b["members"][stage]) == bits(sd.SENTINEL))
    n = len(r["items"])
    lens = np.array([len(i) for i, _ in r["items"]])
    # ready() exactly where the covariance is regular and S is a number: the 41- and 7-sample intervals
    assert np.array_equal(b["ready"][0] == 1, lens >= 7) or np.array_equal(b["ready"][0] == 1, lens >= 2)
    assert np.all(b["ready"][0][lens == 1] == 0) and np.all(b["ready"][0][lens == 41] == 1)
    S = b["members"][0][:, f["sqrt_info"]]
    assert np.all(bits(S[lens == 1]) == 0) and np.all(np.isfinite(S[lens == 41])) and np.abs(S[lens == 41]).max() > 0
    assert np.array_equal(b["pn_doubles"][0], 4 * (lens - 1))
    # every interval was integrated with an Earth rate of its own
    assert len({row.tobytes() for row in b["members"][0][:, f["iewn"]]}) == n == 40


@pytest.mark.parametrize("family", ["imu", "odo"])
def test_launch_counts(earth_runs, family):
    fam, r = sd.FAMILIES[family], earth_runs[family]
    a, b = r[0], r[1]
    # after the first pass: one launch per (variant, row) group in mode 0, one per variant present in mode 1; S launches only in mode 1
    assert a["prof"][0][0] == 40 and a["prof"][0][2] == 0, a["prof"]
    assert b["prof"][0][0] == 1 and b["prof"][0][2] == 1, b["prof"]
    # a second call on the clean list launches nothing
    assert np.array_equal(a["prof"][1][[0, 2]], a["prof"][0][[0, 2]]) and np.array_equal(b["prof"][1][[0, 2]], b["prof"][0][[0, 2]])
    # after reintegration(state) of three intervals: exactly one call in mode 1 (three groups in mode 0)
    assert b["prof"][2][0] == 2 and b["prof"][2][2] == 2, b["prof"]
    assert a["prof"][2][0] == 43, a["prof"]


@pytest.mark.parametrize("family", ["imu", "odo"])
@pytest.mark.parametrize("mode", [0, 1])
def test_reintegration_changes_exactly_the_three(earth_runs, family, mode):
    fam, r = sd.FAMILIES[family], earth_runs[family][mode]
    f = sd.member_fields(fam)
    changed = [k for k in range(r["members"].shape[1]) if not same_bits(r["members"][0][k], r["members"][1][k])]
    assert changed == sorted(REDO)
    for k in REDO:
        for name in ("cur", "delta", "iewn", "jac", "cov", "sqrt_info"):
            assert not same_bits(r["members"][0][k, f[name]], r["members"][1][k, f[name]]), (k, name)
        assert r["ready"][1][k] == r["ready"][0][k]


@pytest.mark.parametrize("family", ["imu", "odo"])
def test_plain_list_with_two_distinct_rows(hostlib, family):
    fam = sd.FAMILIES[family]
    items = fam.items() + fam.items([7])
    two = fam.rows(2)
    pick = np.arange(len(items)) % 2
    hostrows = sd.host_rows(fam, two[pick], abv=fam.abv(2)[pick])
    a = sd.streams(hostlib, fam, fam.variants[0], items, hostrows, 0)
    b = sd.streams(hostlib, fam, fam.variants[0], items, hostrows, 1)
    assert a["rc"] == 0 and b["rc"] == 0, (a["msg"], b["msg"])
    _same_members(fam, a, b, 0)
    _same_members(fam, a, b, 1)
    assert a["prof"][0][0] == 2 and b["prof"][0][0] == 1 and b["prof"][0][2] == 1
    assert np.array_equal(a["prof"][2], a["prof"][0]) and np.array_equal(b["prof"][2][[0, 2]], b["prof"][0][[0, 2]])  # nothing was dirty again


@pytest.mark.parametrize("family", ["imu", "odo"])
def test_both_variants_in_one_list_make_one_call_each(hostlib, family):
    fam = sd.FAMILIES[family]
    items = fam.items() * 2
    variant = np.array([fam.variants[k % 2] for k in range(len(items))], np.int32)
    hostrows = sd.host_rows(fam, fam.rows(len(items)))
    a = sd.streams(hostlib, fam, variant, items, hostrows, 0)
    b = sd.streams(hostlib, fam, variant, items, hostrows, 1)
    assert a["rc"] == 0 and b["rc"] == 0, (a["msg"], b["msg"])
    _same_members(fam, a, b, 0)
    assert a["prof"][0][0] == len(items) and b["prof"][0][0] == 2 and b["prof"][0][2] == 2
