#!/usr/bin/env python3
"""Generates tests/golden/preint_edge_ref_golden.npz by running the REFERENCE's IMU preintegration (oracle/_ref/libref_preint.so, built by
oracle/ref_build from the reference's preintegration sources compiled unmodified) on the edge cases of tests/preint_edge_data.py.  Run in the
build container only (the library needs the reference's sources):
    make -C oracle/ref_build && python tests/golden/make_preint_edge_golden.py
Inputs are stored once per case (`in_<case>_imu / _s0 / _params`); a result entry k names its case, variant and station and holds the
reference's Earth rate `iewn` and its cur / delta / jac / cov / dt.
  * Normal variant (ref_preint_integrate): every case.
  * Earth variant (ref_preint_integrate_earth): the reference derives the Earth rate from the station, so a rate cannot be prescribed.  Every
    case runs with station (0, 0, 0) (the value the shipped system effectively uses), `plain` and `long` also with STATION of
    make_preint_golden.py (a tilted rate).  The consumer integrates with the stored `iewn`.
  * The `zero` and `amplified` Earth rates of preint_edge_data.EARTH_RATES, and with them the Earth variant of `zero_rotation` (which needs the
    zero rate), cannot be produced by the reference: they rest on preint_edge_data.integrate_ld alone."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import preint_edge_data as ed  # noqa: E402
from make_preint_golden import STATION  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "preint_edge_ref_golden.npz")


def run_case(lib, variant, imu, s0, params, station):
    p = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)
    cur, delta, jac, cov = np.zeros(16), np.zeros(16), np.zeros((15, 15)), np.zeros((15, 15))
    dt, iewn = C.c_double(), np.zeros(3)
    if variant == 0:
        assert lib.ref_preint_integrate(len(imu), p(imu), p(s0), p(params), p(cur), p(delta), p(jac), p(cov), C.byref(dt)) == 0
    else:
        assert lib.ref_preint_integrate_earth(len(imu), p(imu), p(s0), p(params), p(station), p(cur), p(delta), p(jac), p(cov),
                                              C.byref(dt), p(iewn)) == 0
    return dict(cur=cur, delta=delta, jac=jac, cov=cov, dt=dt.value, iewn=iewn)


def build(lib):
    base = ed.cases(0)  # the inputs of the base cases are the same in both variants; the Earth rate in params is not used by the reference
    out = {"case_names": np.array(list(base))}
    for name, (imu, s0, params) in base.items():
        out.update({f"in_{name}_imu": imu, f"in_{name}_s0": s0, f"in_{name}_params": params})
    k = 0
    for variant in (0, 1):
        for name, (imu, s0, params) in base.items():
            stations = [np.zeros(3)] if variant == 0 or name not in ("plain", "long") else [np.zeros(3), STATION]
            for station in stations:
                c = run_case(lib, variant, imu, s0, params, station)
                out.update({f"r{k}_case": np.array(name), f"r{k}_variant": variant, f"r{k}_station": station})
                out.update({f"r{k}_{key}": val for key, val in c.items()})
                k += 1
    out["n_results"] = k
    return out


def main():
    out = build(C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_preint.so")))
    np.savez_compressed(OUT, **out)
    print("wrote", int(out["n_results"]), "results,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
