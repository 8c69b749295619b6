#!/usr/bin/env python3
"""Generates tests/golden/preint_odo_ref_golden.npz by running the REFERENCE's odometer preintegration (PreintegrationOdo /
PreintegrationEarthOdo behind PreintegrationFactor) on the cases of tests/preint_odo_data.py.  No library of oracle/_ref exports these
classes, so this script compiles a harness of this project's own, tests/golden/ref_preint_odo.cc (it #includes the reference's sources
where they lie, as oracle/ref_build/ref_preint.cc does), against the interface shims of oracle/ref_build/shim with the flags of
oracle/ref_build/Makefile into a temporary directory, loads it and writes the data.  Run by hand in the build container only (it needs the
reference's sources); build() does not run it and no test needs it:
    python tests/golden/make_preint_odo_golden.py [--ref /path/to/ic_gvins/ic_gvins]
Inputs are stored once per case (`in_<case>_imu / _s0 / _par25 / _abv`; par25 as icg_preint_odo_batch takes it, with this project's cvb);
a result entry k names its case, variant (2 Odo, 3 EarthOdo) and station and holds the reference's Earth rate `iewn`, its cur 16 / delta 20
(p q v bg ba s sodo) / jac 19x19 / cov 19x19 / dt, the pn rows (EarthOdo; (n - 1) x 4), and PreintegrationFactor::Evaluate at one evaluation
point off the integrated state: `point` 34, `r` 19, `J` 646 = 19x7 | 19x10 | 19x7 | 19x10.
  * Odo: every case of GOLDEN_NAMES.  EarthOdo: every case with station (0, 0, 0) (the value the shipped system effectively uses), `plain`
    and `long` also with the tilted STATION of make_preint_golden.py.  The reference derives the Earth rate from the station; the consumer
    integrates with the stored `iewn`.
  * Noise: odo_std = (0.05, 0.04, 0.06) m/s and odo_srw = 1e-4 (preint_odo_data.ODO_STD / ODO_SRW).  With them the host P2, fed this file's own
    integration results, sits more than 10x inside the project's P2 bound 1e-6 * max(1, max|expected|) on every case
    (tests/test_preint_odo_host.py prints the measured maximum), so the noise parameters were left at their first, realistic values.
The file is written with fixed zip timestamps: regenerating it reproduces it byte for byte."""
import argparse
import ctypes as C
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import preint_odo_data as od  # noqa: E402
from make_preint_golden import STATION  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "preint_odo_ref_golden.npz")
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-Wno-unused-variable"]


def build_harness(ref, tmp):
    lib = os.path.join(tmp, "libref_preint_odo.so")
    cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + ["-I" + os.path.join(ROOT, "oracle", "ref_build", "shim"), "-I" + ref, "-shared", "-o", lib,
                                                      os.path.join(ROOT, "tests", "golden", "ref_preint_odo.cc")]
    subprocess.run(cmd, check=True)
    return C.CDLL(lib)


def run_case(lib, variant, imu, s0, par25, abv, station):
    p = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)
    par16 = np.concatenate([par25[:6], par25[9:13], abv, par25[22:25]])
    n = len(imu)
    cur, delta, jac, cov, iewn = np.zeros(16), np.zeros(20), np.zeros((19, 19)), np.zeros((19, 19)), np.zeros(3)
    pn = np.zeros((n - 1 if variant == od.EARTH_ODO else 0, 4))
    dt = C.c_double()
    scratch_r, scratch_J = np.zeros(19), np.zeros(646)
    # first pass: the integration result (the evaluation point is placed off ITS end state), second pass: the factor at that point
    assert lib.ref_preint_odo(variant, n, p(imu), p(s0), p(par16), p(station), p(cur), p(delta), p(jac), p(cov), C.byref(dt), p(iewn),
                              p(pn) if pn.size else None, None, p(scratch_r), p(scratch_J)) == 0
    point = od.eval_point(s0, cur)
    r, J = np.zeros(19), np.zeros(646)
    assert lib.ref_preint_odo(variant, n, p(imu), p(s0), p(par16), p(station), p(cur), p(delta), p(jac), p(cov), C.byref(dt), p(iewn),
                              None, p(point), p(r), p(J)) == 0
    return dict(cur=cur, delta=delta, jac=jac, cov=cov, dt=np.float64(dt.value), iewn=iewn, pn=pn, point=point, r=r, J=J)


def build(lib):
    cs = od.cases()
    out = {"case_names": np.array(od.GOLDEN_NAMES)}
    for name in od.GOLDEN_NAMES:
        imu, s0, par25, abv = cs[name]
        out.update({f"in_{name}_imu": imu, f"in_{name}_s0": s0, f"in_{name}_par25": par25, f"in_{name}_abv": abv})
    k = 0
    for variant in od.VARIANTS:
        for name in od.GOLDEN_NAMES:
            imu, s0, par25, abv = cs[name]
            stations = [np.zeros(3)] if variant == od.ODO or name not in ("plain", "long") else [np.zeros(3), STATION]
            for station in stations:
                c = run_case(lib, variant, imu, s0, par25, abv, station)
                out.update({f"r{k}_case": np.array(name), f"r{k}_variant": np.int64(variant), f"r{k}_station": station})
                out.update({f"r{k}_{key}": val for key, val in c.items()})
                k += 1
    out["n_results"] = np.int64(k)
    return out


def save_reproducibly(path, arrays):
    """np.savez_compressed's layout with a fixed timestamp per member, so that the same data gives the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference/ic_gvins/ic_gvins", help="the reference's source directory (the one holding preintegration/)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        out = build(build_harness(args.ref, tmp))
    save_reproducibly(OUT, out)
    print("wrote", int(out["n_results"]), "results,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
