"""The algebra and the byte selection behind the vertical pixel pairs of csrc/lk.hip (round 13), restated in numpy int64 on the CPU.

1. A Q14 bilinear blend is four products and one 32-bit sum.  The kernel forms it with two v_dot2_i32_i16; whether the two taps of a dot2 are
   horizontal neighbours, dot2(JB, (w10, w11), dot2(JA, (w00, w01), c)), or vertical ones, dot2(VP[k+1], (w01, w11), dot2(VP[k], (w00, w10), c)),
   the result is the same integer, and so is every value derived from it — provided no intermediate accumulator leaves 32 bits.
2. lk_fetch_J and the interior set-up build the vertical pairs with v_alignbyte_b32 / v_perm_b32; their selectors are emulated here against
   direct indexing of the staged tiles."""
import itertools

import numpy as np
import pytest

F32 = np.float32
MAGIC = F32(12582912.0)  # 1.5 * 2^23


def _bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def _s16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def weights_pk(a, b):
    """lk_weights_pk: (w00, w01, w10, w11) as the signed 16-bit halves the dot2 reads"""
    a, b = F32(a), F32(b)
    A = F32(a * F32(16384.0))
    A1 = F32(F32(16384.0) - A)
    b1 = F32(F32(1.0) - b)
    r00, r01, r10 = _bits(F32(F32(A1 * b1) + MAGIC)), _bits(F32(F32(A * b1) + MAGIC)), _bits(F32(F32(A1 * b) + MAGIC))
    r11 = (0x4000 - (r00 + r01 + r10)) & 0xFFFFFFFF
    return _s16(r00), _s16(r01), _s16(r10), _s16(r11)


FRACS = (0.0, 2.0 ** -15, 0.25, 0.5, 1.0 - 2.0 ** -24)
STARTS = (256 - 512 * 0, 256 - 512 * 8160, 1 << 8)  # c0 = 256 - 512 I for I = 0 and 8160, and rnd8


def _patterns():
    yy, xx = np.mgrid[0:2, 0:9]
    pats = [np.zeros((2, 9), np.int64), np.full((2, 9), 255, np.int64), ((xx + yy) & 1) * 255, ((xx + yy + 1) & 1) * 255]
    rng = np.random.RandomState(1313)
    pats += [rng.randint(0, 256, (2, 9)).astype(np.int64) for _ in range(12)]
    return pats


def test_weights_at_the_integer_position():
    assert weights_pk(0.0, 0.0) == (16384, 0, 0, 0)
    for a, b in itertools.product(FRACS, FRACS):
        w = weights_pk(a, b)
        assert sum(w) == 16384 and min(w) >= 0, (a, b, w)


@pytest.mark.parametrize("c", STARTS)
def test_blend_chains_agree(c):
    """final value and every intermediate accumulator of the horizontal-pair and the vertical-pair chain, 8 positions of two rows"""
    lim = 1 << 31
    for (a, b), P in itertools.product(itertools.product(FRACS, FRACS), _patterns()):
        w00, w01, w10, w11 = (np.int64(v) for v in weights_pk(a, b))
        up, lo = P[0].astype(np.int64), P[1].astype(np.int64)
        # horizontal pairs: JA[k] = (up[k], up[k+1]) . (w00, w01), then JB[k] = (lo[k], lo[k+1]) . (w10, w11)
        h1 = c + up[:-1] * w00 + up[1:] * w01
        h2 = h1 + lo[:-1] * w10 + lo[1:] * w11
        # vertical pairs: VP[k] = (up[k], lo[k]) . (w00, w10), then VP[k+1] . (w01, w11)
        v1 = c + up[:-1] * w00 + lo[:-1] * w10
        v2 = v1 + up[1:] * w01 + lo[1:] * w11
        for acc in (h1, h2, v1, v2):
            assert (np.abs(acc) < lim).all(), (a, b, c)
        assert np.array_equal(h2, v2), (a, b, c)
        assert np.array_equal(h2 >> 9, v2 >> 9)                      # the iteration's residual
        assert np.array_equal(256 - (h2 & ~511), 256 - (v2 & ~511))  # the set-up's c0
        # a direct statement of the blend
        assert np.array_equal(v2, c + w00 * up[:-1] + w01 * up[1:] + w10 * lo[:-1] + w11 * lo[1:])


# ---- the byte selection ----
def alignbyte(hi, lo, sh):
    """v_alignbyte_b32: ({hi, lo} >> 8 sh) & 0xffffffff"""
    return (((hi << 32) | lo) >> (8 * sh)) & 0xFFFFFFFF


def perm(hi, lo, sel):
    """v_perm_b32 for the selector bytes the kernel uses: 0..3 a byte of lo, 4..7 a byte of hi, 0x0c the constant 0"""
    src = (hi << 32) | lo
    out = 0
    for i in range(4):
        s = (sel >> (8 * i)) & 0xFF
        assert s <= 7 or s == 0x0C
        out |= (0 if s == 0x0C else (src >> (8 * s)) & 0xFF) << (8 * i)
    return out


def vpair_sel(c):
    """lk_vpair_sel: (byte c & 3 of the upper row's dword, 0, byte c & 3 of the lower row's dword, 0)"""
    return 0x0C000C00 | (c & 3) | ((4 + (c & 3)) << 16)


def _dwords(tile):
    return np.ascontiguousarray(tile).view("<u4").astype(np.int64)


def test_fetch_pairs_every_phase():
    """lk_fetch_J on a 32 x 36-byte tile of the next image: three aligned dwords per row, v_alignbyte by the byte phase, one v_perm per column"""
    rng = np.random.RandomState(1314)
    tile = rng.randint(0, 256, (32, 36)).astype(np.uint8)
    dw = _dwords(tile)  # 9 dwords per row
    for row0 in (0, 13, 30):
        for idx, sh in itertools.product(range(7), range(4)):
            o = 4 * idx + sh
            d0, d1, d2 = (int(dw[row0, idx + q]) for q in range(3))
            e0, e1, e2 = (int(dw[row0 + 1, idx + q]) for q in range(3))
            a0, a1 = alignbyte(d1, d0, sh), alignbyte(d2, d1, sh)
            b0, b1 = alignbyte(e1, e0, sh), alignbyte(e2, e1, sh)
            for k in range(8):
                got = perm(b0 if k < 4 else b1, a0 if k < 4 else a1, vpair_sel(k))
                assert got == int(tile[row0, o + k]) | (int(tile[row0 + 1, o + k]) << 16), (row0, sh, k)


def test_setup_pairs_both_half_rows():
    """the interior set-up on the 24 x 28-byte tile of the previous image: lane (br, bs) reads four dwords of rows br, br + 1 at dword 3 bs
    and pairs columns 12 bs .. 12 bs + 12"""
    rng = np.random.RandomState(1315)
    tile = rng.randint(0, 256, (24, 28)).astype(np.uint8)
    dw = _dwords(tile)  # 7 dwords per row
    for br, bs in itertools.product(range(23), (0, 1)):
        d = [[int(dw[br + r, 3 * bs + q]) for q in range(4)] for r in range(2)]
        for c in range(13):
            got = perm(d[1][c >> 2], d[0][c >> 2], vpair_sel(c))
            assert got == int(tile[br, 12 * bs + c]) | (int(tile[br + 1, 12 * bs + c]) << 16), (br, bs, c)


def test_blend_through_the_emulated_registers():
    """both pieces together: the packed registers of the fetch, read as the signed 16-bit halves of v_dot2_i32_i16 with the column-packed
    weights, give the direct blend"""
    rng = np.random.RandomState(1316)
    tile = rng.randint(0, 256, (32, 36)).astype(np.uint8)
    tile[4:6, 8:20] = 255
    dw = _dwords(tile)

    def dot2(x, y, acc):
        return _s16(x) * _s16(y) + _s16(x >> 16) * _s16(y >> 16) + acc

    for (a, b), sh in itertools.product(itertools.product(FRACS, FRACS), range(4)):
        w00, w01, w10, w11 = weights_pk(a, b)
        Wl, Wr = (w00 & 0xFFFF) | ((w10 & 0xFFFF) << 16), (w01 & 0xFFFF) | ((w11 & 0xFFFF) << 16)
        row0, idx = 4, 2
        o = 4 * idx + sh
        d = [[int(dw[row0 + r, idx + q]) for q in range(3)] for r in range(2)]
        A = [alignbyte(d[0][1], d[0][0], sh), alignbyte(d[0][2], d[0][1], sh)]
        B = [alignbyte(d[1][1], d[1][0], sh), alignbyte(d[1][2], d[1][1], sh)]
        VP = [perm(B[k >> 2], A[k >> 2], vpair_sel(k)) for k in range(8)]
        for k, c in itertools.product(range(7), STARTS):
            t = tile.astype(np.int64)
            exp = c + w00 * t[row0, o + k] + w01 * t[row0, o + k + 1] + w10 * t[row0 + 1, o + k] + w11 * t[row0 + 1, o + k + 1]
            assert dot2(VP[k + 1], Wr, dot2(VP[k], Wl, c)) == int(exp)
