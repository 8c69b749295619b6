"""The algebra under the interior-window set-up of k_lk_track_fb (csrc/lk.hip): the Q14 bilinear blend and the Scharr stencil are integer linear
maps, so blending the Scharr derivatives of a tile equals differentiating the unrounded blend B of the tile,

    sum_ab w_ab Scharr(I)(x + a, y + b) == Scharr(B)(x, y),    B(x, y) = sum_ab w_ab I(x + a, y + b),

exactly, before the one descale.  Checked in int64 on 24x24 u8 tiles (the kernel's I tile) for random and adversarial contents and weight
sets, together with the bounds that let the kernel work in int32 / 24-bit products and the forms it actually evaluates (stencil x 4 with the
descaled value taken as a high half, the rounding constants carried inside the smooth terms, the patch sample from B + 256)."""
import numpy as np
import pytest

T = 24  # tile side: 22x22 derivative support + 1 halo


def _tiles():
    rng = np.random.RandomState(7)
    y, x = np.mgrid[0:T, 0:T]
    out = [(f"random{i}", rng.randint(0, 256, (T, T))) for i in range(4)]
    out += [(f"binary{i}", rng.randint(0, 2, (T, T)) * 255) for i in range(2)]
    out += [("checker1", ((x + y) % 2) * 255), ("checker1_inv", ((x + y + 1) % 2) * 255),
            ("checker2", ((x // 2 + y // 2) % 2) * 255), ("checker2_shift", (((x + 1) // 2 + (y + 1) // 2) % 2) * 255),
            ("stripes2_v", ((x // 2) % 2) * 255 + 0 * y), ("stripes2_v_shift", (((x + 1) // 2) % 2) * 255 + 0 * y),
            ("stripes2_h", ((y // 2) % 2) * 255 + 0 * x), ("stripes2_h_shift", (((y + 1) // 2) % 2) * 255 + 0 * x),
            ("const255", np.full((T, T), 255)), ("const0", np.zeros((T, T), int))]
    return [(n, np.asarray(t, np.int64)) for n, t in out]


def _weights(a, b):
    """the Q14 weights exactly as lk_weights forms them (float32 products, round to nearest even, w11 as the remainder)"""
    a, b = np.float32(a), np.float32(b)
    A = a * np.float32(1 << 14)
    A1 = np.float32(1 << 14) - A
    b1 = np.float32(1) - b
    w00, w01, w10 = int(np.rint(A1 * b1)), int(np.rint(A * b1)), int(np.rint(A1 * b))
    return w00, w01, w10, (1 << 14) - w00 - w01 - w10


def _fractions():
    rng = np.random.RandomState(11)
    edge = [0.0, 0.5, 1.0 - 2.0 ** -15, 2.0 ** -15]
    return [(a, b) for a in edge for b in edge] + [tuple(rng.uniform(0, 1, 2)) for _ in range(8)]


def _scharr(P):
    """unnormalised Scharr derivatives at the interior of P (int64): vertical smooth [3 10 3] x horizontal difference, and the transpose"""
    sm_v = 3 * (P[:-2, :] + P[2:, :]) + 10 * P[1:-1, :]
    df_v = P[2:, :] - P[:-2, :]
    dx = sm_v[:, 2:] - sm_v[:, :-2]
    dy = 3 * (df_v[:, :-2] + df_v[:, 2:]) + 10 * df_v[:, 1:-1]
    return dx, dy, sm_v, df_v


def _blend(P, w):
    w00, w01, w10, w11 = w
    return w00 * P[:-1, :-1] + w01 * P[:-1, 1:] + w10 * P[1:, :-1] + w11 * P[1:, 1:]


@pytest.mark.parametrize("name,tile", _tiles(), ids=[n for n, _ in _tiles()])
def test_blend_of_scharr_is_scharr_of_blend(name, tile):
    dxI, dyI, _, _ = _scharr(tile)  # 22x22 derivative support
    for a, b in _fractions():
        w = _weights(a, b)
        assert min(w) >= 0 and max(w) <= 1 << 14 and sum(w) == 1 << 14
        B = _blend(tile, w)  # 23x23
        assert B.min() >= 0 and B.max() <= 255 << 14
        dxB, dyB, sm_v, df_v = _scharr(B)  # 21x21: the window
        # the identity, before the descale
        assert np.array_equal(_blend(dxI, w), dxB), (name, a, b)
        assert np.array_equal(_blend(dyI, w), dyB), (name, a, b)
        # every intermediate of the 32-bit stencil stays below 2^27
        for v in (B, sm_v, df_v, dxB, dyB, 3 * (df_v[:, :-2] + df_v[:, 2:])):
            assert np.abs(v).max() < 1 << 27
        # the forms the kernel evaluates: B + 256 in LDS, 24-bit multiplicands, stencil x 4 with the rounding constant (j / 2) 2^15 inside the
        # smooth term of column j, the descaled value as the high half
        Bs = B + 256
        assert Bs.max() < 1 << 22 and (Bs[:-2] + Bs[2:]).max() < 1 << 23 and np.abs(df_v[:, :-2] + df_v[:, 2:]).max() < 1 << 23
        col = (np.arange(T - 1) >> 1) << 15
        sm4 = 12 * (Bs[:-2, :] + Bs[2:, :]) + 40 * Bs[1:-1, :] + col[None, :]
        assert sm4.max() < 1 << 31
        ix4 = sm4[:, 2:] - sm4[:, :-2]
        dv = Bs[2:, :] - Bs[:-2, :]
        iy4 = 12 * (dv[:, :-2] + dv[:, 2:]) + 40 * dv[:, 1:-1] + (1 << 15)
        assert np.abs(ix4).max() < 1 << 31 and np.abs(iy4).max() < 1 << 31
        assert np.array_equal(ix4 >> 16, (dxB + (1 << 13)) >> 14) and np.array_equal(iy4 >> 16, (dyB + (1 << 13)) >> 14)
        assert np.abs((dxB + (1 << 13)) >> 14).max() <= 4080 and np.abs((dyB + (1 << 13)) >> 14).max() <= 4080  # fit the packed i16 halves
        # the patch sample and the folded rounding constant c0 = 256 - 512 Ival from the same B
        ival = (B[1:-1, 1:-1] + 256) >> 9
        assert np.array_equal(256 - (Bs[1:-1, 1:-1] & ~511), 256 - 512 * ival)


def test_saturation_is_reached():
    """the adversarial tiles put the stencil at its bounds: |Scharr| = 16 * 255 per unit weight on width-2 stripes, B at 255 * 2^14"""
    tiles = dict(_tiles())
    w = _weights(0.0, 0.0)
    assert w == (1 << 14, 0, 0, 0)
    dx, dy, _, _ = _scharr(_blend(tiles["stripes2_v"], w))
    assert np.abs(dx).max() == 16 * 255 << 14 and np.abs(dy).max() == 0
    dx, dy, _, _ = _scharr(_blend(tiles["stripes2_h"], w))
    assert np.abs(dy).max() == 16 * 255 << 14 and np.abs(dx).max() == 0
    assert _blend(tiles["const255"], _weights(0.3, 0.7)).min() == 255 << 14
