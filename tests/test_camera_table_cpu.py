"""Per-stream camera calibration on the oracle-backed host library (no GPU): that build links on a C ABI without the camera-table entries
(icg_set_cameras, icg_lk_track_fb_cams, icg_tracker_create_cams, icg_reproj_error_batch_cams).  A table of bit-equal cameras must go the
single-camera way and need none of them; a heterogeneous table must be refused at construction, by name — never tracked with camera 0."""
import ctypes as C

import numpy as np
import pytest

import camera_table_utils as ct
import harness as H
from stream_utils import ensure_oracle_host


def test_oracle_backed_library_has_no_camera_table_entries():
    """the premise of the two tests below"""
    lib = C.CDLL(ensure_oracle_host())
    for s in ("icg_set_cameras", "icg_lk_track_fb_cams", "icg_tracker_create_cams", "icg_reproj_error_batch_cams"):
        assert not hasattr(lib, s), s
    assert hasattr(lib, "icgh_batch_create_cams")


def test_homogeneous_table_equals_the_existing_constructor():
    """cams= with four bit-equal cameras: digests, states, features and dumps of the existing constructor (table engine)"""
    names = ["base"] * 4
    fr, po, cams, refs = ct.batch_inputs(names)
    a = ct.drive(ensure_oracle_host(), "table", fr, po, cam10=ct.cameras()["base"])
    b = ct.drive(ensure_oracle_host(), "table", fr, po, cams=cams)
    for s in range(4):
        assert a[s]["stats"]["mappoints_created"] > 40, a[s]["stats"]
        ct.assert_stream_equal(b[s], a[s], f"stream {s}")
        ct.assert_stream_equal(b[s], refs[s], f"stream {s} vs its own run")


def test_heterogeneous_table_is_refused_by_name():
    cams = np.array([ct.cameras()[n] for n in ("base", "wide", "tele", "skew")], np.float64)
    lib = C.CDLL(ensure_oracle_host())
    lib.icgh_batch_create_cams.restype = C.c_void_p
    for engine in ("table", "object", "device"):
        with pytest.raises(RuntimeError) as e:
            H.StreamBatch(ensure_oracle_host(), 4, ct.W, ct.HGT, cams[0], max_features=ct.NFEAT, engine=engine, cams=cams)
        assert "icgh_batch_create_cams failed" in str(e.value) and "icg_set_cameras" in str(e.value), str(e.value)
    # the driver entry itself: no batch object comes back
    from ctypes_util import ErrBuf
    err = ErrBuf()
    h = lib.icgh_batch_create_cams(0, 4, cams.ctypes.data_as(C.c_void_p), ct.W, ct.HGT, ct.NFEAT, C.c_double(20.0), C.c_double(0.5), 0, C.c_double(1.5), 10, 1,
                                   1, *err.args)
    assert not h
    assert "icg_set_cameras" in err.text()
    # cameras that differ only between groups (each group's own are equal) need no table: accepted, every group on its own single camera
    two = np.array([ct.cameras()["base"], ct.cameras()["tele"]], np.float64)
    sb = H.StreamBatch(ensure_oracle_host(), 2, ct.W, ct.HGT, two[0], max_features=ct.NFEAT, engine="table", groups=2, cams=two)
    assert sb.n_groups() == 2
    sb.close()
