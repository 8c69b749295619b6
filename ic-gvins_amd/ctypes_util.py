"""The ctypes helpers of the bindings, the test data modules and the probes, each defined once: array -> pointer, array converters, the
bit views behind every bit-for-bit assertion, and the error buffer of the host layer's C entries."""
import ctypes as C

import numpy as np


def ptr(a):
    """array -> c_void_p; None -> NULL"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def ptr_or_null(a):
    """as ptr, an empty array -> NULL as well"""
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def ptrs(arrays):
    """a table of pointers, one per array (None -> NULL)"""
    return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def bits(a):
    """the bit patterns of a's doubles, flat"""
    return np.ascontiguousarray(a, np.float64).ravel().view(np.uint64)


def same_bits(a, b, nan_payload=False):
    """bit patterns equal on every non-NaN entry, NaN in the same places (sign and payload of a NaN are not results of IEEE arithmetic and
    differ between an x86 host and the device; on one machine the patterns are equal anyway).  nan_payload: every pattern equal, those of
    the NaNs too (two runs of the same instructions)"""
    a, b = np.ascontiguousarray(a, np.float64).ravel(), np.ascontiguousarray(b, np.float64).ravel()
    if nan_payload:
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


class ErrBuf:
    """the character buffer a C entry writes its message into: `*err.args` is the (buffer, length) pair where the entry takes it (the
    object alone passes as the buffer), err.value the message afterwards as bytes, err.text() as a string"""

    def __init__(self, size=512):
        self.buf, self.size = C.create_string_buffer(size), size
        self._as_parameter_ = self.buf

    @property
    def args(self):
        return self.buf, self.size

    @property
    def value(self):
        return self.buf.value

    def text(self):
        return self.value.decode()
