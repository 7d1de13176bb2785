"""Tiled inference: the numpy definitions and the case grid that tests/test_tiled_cpu.py and tests/test_gpu_tiled.py share.

Geometry: S the tile side, G >= 1 tiles per side, 0 <= O <= S // 2 pixels of overlap, stride T = S - O, canvas side
C = S + (G - 1) * T.  Tile t = i * G + j covers canvas rows [i * T, i * T + S) and columns [j * T, j * T + S).
  gather   tiles[b * G^2 + t, c, y, x] = canvas[b, c, i * T + y, j * T + x]
  stitch   w1(u) = min(u + 1, S - u); a tile weighs w1(y) * w1(x) at its (y, x); a canvas pixel under exactly one tile is
           that tile's value, any other is (sum_t w_t * v_t) / (sum_t w_t) over the covering tiles in ascending t

BAR, the bar of the fp32 stitch against the fp64 one, is derived: a blended pixel takes at most 4 products, 3 sums and
1 division, each rounding by at most 2^-24 relative, on terms whose weights sum to 1 -- at most 8 * 2^-24 = 2^-21 of the
largest |value| (the weights and their sums are exact integers in fp32).  A prototype of the fp32 definition on this grid
stayed at 7.0e-8 relative."""
import functools

import numpy as np

# (S, G, O): no overlap, O = S // 2 for an odd and an even S, O = 1, G = 1, several blocks per row (70 at G = 2)
GRID = ((5, 1, 0), (5, 2, 0), (5, 2, 2), (5, 3, 1), (14, 3, 7), (37, 2, 18), (37, 3, 1), (70, 2, 14))
# beyond the grid, for the device code: S and T multiples of 4, the only sides at which it moves 16-byte vectors
VECTOR4 = (72, 2, 16)
FRAMES = (1, 3)
CHANNELS = (1, 3)
WORKING = (518, 2, 112)          # the model's size: C = 924
REL_BAR = 2.0 ** -21


def canvas_side(S, G, O):
    assert S >= 1 and G >= 1 and 0 <= O <= S // 2
    return S + (G - 1) * (S - O)


def origins(S, G, O):
    T = S - O
    return [(i * T, j * T) for i in range(G) for j in range(G)]


def w1(S):
    u = np.arange(S)
    return np.minimum(u + 1, S - u)


def cover_count(S, G, O):
    """int [C, C]: how many tiles cover every canvas pixel"""
    C = canvas_side(S, G, O)
    n = np.zeros((C, C), np.int64)
    for r, c in origins(S, G, O):
        n[r:r + S, c:c + S] += 1
    return n


def gather(canvas, S, G, O):
    """canvas [B, ch, C, C] -> tiles [B * G^2, ch, S, S], the same bits"""
    B = canvas.shape[0]
    assert canvas.shape[-2:] == (canvas_side(S, G, O),) * 2
    tiles = np.stack([canvas[:, :, r:r + S, c:c + S] for r, c in origins(S, G, O)], axis=1)
    return np.ascontiguousarray(tiles.reshape((B * G * G,) + canvas.shape[1:2] + (S, S)))


def stitch(tiles, G, O, dtype=np.float64):
    """tiles [B * G^2, ch, S, S] -> canvas [B, ch, C, C].  dtype float64: the definition.  dtype float32: the same steps
    with every product, sum and the division rounded to fp32, the sums in ascending t (the order the kernel keeps)."""
    S = tiles.shape[-1]
    C = canvas_side(S, G, O)
    B, ch = tiles.shape[0] // (G * G), tiles.shape[1]
    v = tiles.reshape(B, G * G, ch, S, S).astype(dtype)
    w = (w1(S).astype(dtype)[:, None] * w1(S).astype(dtype)[None, :]).astype(dtype)
    num, den = np.zeros((B, ch, C, C), dtype), np.zeros((C, C), dtype)
    single = np.zeros((B, ch, C, C), tiles.dtype)
    for t, (r, c) in enumerate(origins(S, G, O)):
        num[:, :, r:r + S, c:c + S] += (w * v[:, t]).astype(dtype)      # 0 + p = p: the first term is the product
        den[r:r + S, c:c + S] += w
        single[:, :, r:r + S, c:c + S] = tiles.reshape(B, G * G, ch, S, S)[:, t]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (num / den).astype(dtype)
    return np.where(cover_count(S, G, O) == 1, single.astype(dtype), out)


@functools.lru_cache(maxsize=None)
def case(S, G, O, frames, channels):
    """-> (tiles fp32 [frames * G^2, channels, S, S], values 3 * N(0, 1) + 1, seeded; its fp64 stitch), computed once and
    not to be written to"""
    rng = np.random.default_rng(1000003 * S + 1009 * G + 17 * O + 5 * frames + channels)
    tiles = (3.0 * rng.standard_normal((frames * G * G, channels, S, S)) + 1.0).astype(np.float32)
    want = stitch(tiles, G, O, np.float64)
    tiles.setflags(write=False)
    want.setflags(write=False)
    return tiles, want


@functools.lru_cache(maxsize=None)
def canvas_case(S, G, O, frames, channels):
    """a seeded fp32 canvas [frames, channels, C, C] for the gather"""
    C = canvas_side(S, G, O)
    rng = np.random.default_rng(7 + 1000003 * S + 1009 * G + 17 * O + 5 * frames + channels)
    canvas = (3.0 * rng.standard_normal((frames, channels, C, C)) + 1.0).astype(np.float32)
    canvas.setflags(write=False)
    return canvas


def bar(tiles):
    """BAR = 2^-21 * max |v|"""
    return REL_BAR * float(np.abs(tiles).max())


def grid():
    for S, G, O in GRID:
        for frames in FRAMES:
            for channels in CHANNELS:
                yield S, G, O, frames, channels
