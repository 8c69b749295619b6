"""The identities the level prologue of k_lk_track / k_lk_track_fb (csrc/lk.hip) rests on since it left FP64 and 64-bit vector arithmetic:
the level scale 2^-level formed from its bit pattern, and one 32-bit byte offset row * pitch + col per lane (a 24-bit multiply) for the tile
loads that lie inside a level, valid for every layout icg_ctx_create (csrc/ctx.hip) admits.  numpy only, except for the bound itself, which is
asked of the library through the C ABI: the refusal comes before a device is touched, so it is checked without one."""
import ctypes as C

import numpy as np
import pytest

MAX_LEVELS = 4  # ICG_MAX_LEVELS (csrc/icg_internal.h)
LK_WIN = 21     # ICG_LK_WIN
ERR_INVALID = -1


def test_level_scale_is_its_bit_pattern():
    """(float) (1. / (1 << level)) == bits((127 - level) << 23) for every level a pyramid can have"""
    for level in range(MAX_LEVELS):
        want = np.float32(1.0 / (1 << level))
        assert want.view(np.uint32) == np.uint32((127 - level) << 23), level
        assert np.array([(127 - level) << 23], np.uint32).view(np.float32)[0] == want


def layout(w, h):
    """the pyramid layout of icg_ctx_create: [(w, h, pitch)] per level"""
    out = []
    for l in range(MAX_LEVELS):
        if l > 0:
            w, h = (w + 1) // 2, (h + 1) // 2
            if w <= LK_WIN or h <= LK_WIN:
                break
        out.append((w, h, (w + 127) // 128 * 128))
    return out


def admitted(w, h):
    """the bound of icg_ctx_create"""
    return w < 2 ** 24 and h < 2 ** 24 and (w + 127) // 128 * 128 * h < 2 ** 31


def largest_layouts():
    """for heights from the smallest image to the largest the bound can admit: the widest admitted image, and the tallest of that width"""
    out = []
    for h in (32, 33, 127, 128, 129, 1000, 4096, 32767, 32768, 46340, 46341, 65535, 65536, 1 << 20, (1 << 24) - 1):
        pitch = min((2 ** 31 - 1) // h // 128 * 128, (2 ** 24 - 1) // 128 * 128)
        assert pitch >= 128, h
        hh = min((2 ** 31 - 1) // pitch, 2 ** 24 - 1)
        assert not admitted(pitch, hh + 1) and not admitted(pitch + 128, hh)  # (maximal in both directions)
        out += [(pitch, h), (pitch - 127, hh), (pitch, hh)]
    return out


def test_offsets_of_the_largest_admitted_layouts_fit_32_bits():
    cases = largest_layouts()
    assert any(w * h > 2 ** 31 - 2 ** 24 for w, h in cases)  # (they do come close to the bound)
    for w, h in cases:
        assert admitted(w, h), (w, h)
        for wl, hl, pitch in layout(w, h):
            assert hl < 2 ** 24 and pitch < 2 ** 24, (w, h, wl, hl, pitch)
            row, col = hl - 1, wl - 4  # the last dword of the last row
            exact = row * pitch + col
            assert exact + 3 < 2 ** 31, (w, h, wl, hl, pitch)
            # what lk_offset computes: the low 32 bits of a 24-bit x 24-bit product, plus the column, in 32-bit unsigned arithmetic
            mul24 = ((row & 0xffffff) * (pitch & 0xffffff)) & 0xffffffff
            assert (mul24 + col) & 0xffffffff == exact, (w, h, wl, hl, pitch)


JUST_OVER = [(65536, 32768), (32768 - 127, 65536), (1 << 24, 32), (32, 1 << 24), (46341 + 127, 46341),
             ((1 << 24) - 128 + 1, 128)]


class _Cfg(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("device", "width", "height", "n_slots", "max_batch", "max_points", "max_factors")]


def _create(lib, w, h):
    cfg = _Cfg(0, w, h, 2, 1, 64, 0)
    ctx = C.c_void_p()
    rc = lib.icg_ctx_create(C.byref(cfg), C.byref(ctx))
    return rc, ctx, lib.icg_last_error(None).decode()


def test_a_context_over_the_bound_is_refused(hiplib):
    """every size just over the bound is ICG_ERR_INVALID with a message that names the bound — decided before a device is asked for and
    before any allocation (these sizes would be 2 GiB and more per slot)"""
    for w, h in JUST_OVER:
        assert not admitted(w, h), (w, h)
        rc, ctx, msg = _create(hiplib, w, h)
        assert rc == ERR_INVALID and not ctx.value, (w, h, rc)
        assert "2^31" in msg, (w, h, msg)


@pytest.mark.gpu
def test_a_normal_context_creates_after_a_refusal(hiplib):
    rc, ctx, msg = _create(hiplib, *JUST_OVER[0])
    assert rc == ERR_INVALID and not ctx.value
    rc, ctx, msg = _create(hiplib, 640, 480)
    assert rc == 0 and ctx.value, (rc, msg)
    assert hiplib.icg_pyramid_levels(ctx) == 4
    hiplib.icg_ctx_destroy(ctx)
