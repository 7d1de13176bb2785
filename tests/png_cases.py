"""The case grid of the PNG encoder's tests (test_png_cpu.py, test_gpu_png.py) and its seeded generators; numpy only.

The size bar.  zlib is the reference: zRLE = len(zlib.compressobj(6, DEFLATED, 15, 8, Z_RLE) over the filtered bytes).
    size <= zRLE * 1.01 + 64 * segments + 16
The 1 % covers the 15-bit limit, the match-split rule and zlib's finer block adaption, the 64 bytes per segment this
format's own per-segment header and sync marker.  Measured on this grid (size - zRLE, per image):
    1x1x1, 1x1x3 (stored) +5 B; photo-like 7x5x3 +2 B (stored), 70x70x3 +5 B of 5.7 KB, three of 64x48x3 +5 .. +6 B of 3.8 KB
    all zeros 700x700x3: +947 B over 47 segments (20 B per segment; the bar allows 64)
    noise (stored): -8 .. -3 B per image; run lengths +6 B; two-valued 64x67x1 +6 B of 0.8 KB
    mask 518x518x1: +167 B over 9 segments (19 B per segment); 3x10000x3: -160 B of 9.6 KB; the 15-bit case: -16 B of 8.5 KB
The working sizes of test_gpu_png.py: photo-like panels 2 x 1554x518x3 +0.02 % and +0.18 %, 2772x924x3 +0.23 % of zRLE;
masks 518x518x1 +154 B, +154 B and +145 B over 9 segments (17 B per segment).
A first code builder that enforced the limit by halving the counts and rebuilding was replaced before these figures were
taken: the rule now repairs the Kraft sum of the clamped lengths (forward_utils.png_code_lengths_host)."""
import zlib

import numpy as np


def photo(images, H, W, C, seed):
    """photo-like data: a seeded random walk in both directions, blurred, stretched to 0 .. 255"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(images, H, W, C)).cumsum(axis=1).cumsum(axis=2)
    x = x + rng.normal(scale=2.0, size=x.shape)
    for axis in (1, 2):
        x = (x + np.roll(x, 1, axis=axis) + np.roll(x, -1, axis=axis)) / 3.0
    lo, hi = x.min(), x.max()
    return np.ascontiguousarray(((x - lo) / max(hi - lo, 1e-9) * 255.0).astype(np.uint8))


def noise(images, H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(images, H, W, C), dtype=np.uint8)


def run_lengths():
    """one row of runs of 2, 3, 4, 259, 260, 261, 262 and 517 equal bytes: both ends of the match rule"""
    row = []
    for k, n in enumerate((2, 3, 4, 259, 260, 261, 262, 517)):
        row += [16 * k + 9] * n
    return np.array(row, dtype=np.uint8).reshape(1, 1, len(row), 1)


def two_valued(seed):
    return (np.random.default_rng(seed).random((1, 64, 67, 1)) < 0.3).astype(np.uint8) * 255


def rectangle_mask():
    m = np.zeros((1, 518, 518, 1), dtype=np.uint8)
    m[0, 100:301, 57:400] = 255
    return m


def limit_case(seed=5):
    """A one-row grey image whose Sub-filtered bytes have counts 1, 1, 2, 3, 5, 8, 13, 21 and from there growing by 1.68 from
    symbol to symbol, over 20 symbols (27420 bytes): every merged node is lighter than the next leaf but one, so the unlimited Huffman tree is a
    chain, 19 deep, and still deeper than 15 with the few other symbols of the segment, and the code builder has to enforce its limit.  Two earlier attempts did NOT reach it.  Shuffled
    counts leave runs of the commonest symbol (two bytes in five); they become some 300 matches, whose length symbols
    stand between the chain's counts and make the tree bushy.  The same counts laid out by a rule are not stationary,
    and zlib's block splitting then wins 10 %.  So: the other symbols in a seeded order, and the commonest one dealt
    into the gaps between them, at most one per gap.  The bytes wanted are the row's DIFFERENCES, small in the filter's
    cost, so that Sub wins the row; the pixels are their running sum."""
    values = [10, 247, 9, 248, 8, 249, 7, 250, 6, 251, 5, 252, 4, 253, 3, 254, 2, 255, 1, 0]
    counts = [1, 1, 2, 3, 5, 8, 13, 21]
    while len(counts) < len(values):
        counts.append(int(counts[-1] * 1.68) + 1)
    rng = np.random.default_rng(seed)
    others = np.concatenate([np.full(c, v, dtype=np.int64) for c, v in zip(counts[:-1], values[:-1])])
    rng.shuffle(others)
    gaps = np.zeros(others.size + 1, dtype=bool)
    gaps[rng.choice(others.size + 1, size=counts[-1], replace=False)] = True
    diffs = []
    for k in range(others.size + 1):
        if gaps[k]:
            diffs.append(values[-1])
        if k < others.size:
            diffs.append(int(others[k]))
    return (np.cumsum(np.array(diffs, dtype=np.int64)) % 256).astype(np.uint8).reshape(1, 1, -1, 1)


def cases():
    """(name, pixels uint8 [images, H, W, C]) of the small grid"""
    return [
        ("1x1x1", np.array([201], dtype=np.uint8).reshape(1, 1, 1, 1)),
        ("1x1x3", np.array([3, 1, 4], dtype=np.uint8).reshape(1, 1, 1, 3)),
        ("photo-7x5x3", photo(1, 7, 5, 3, 11)),
        ("photo-70x70x3", photo(1, 70, 70, 3, 12)),
        ("zeros-700x700x3", np.zeros((1, 700, 700, 3), dtype=np.uint8)),
        ("noise-97x131x3", noise(1, 97, 131, 3, 13)),
        ("noise-150x131x3", noise(1, 150, 131, 3, 14)),
        ("noise-83x131x3", noise(1, 83, 131, 3, 15)),          # at W = 131, C = 3 a segment is 83 rows: exactly one,
        ("noise-84x131x3", noise(1, 84, 131, 3, 16)),          # a one-row tail,
        ("noise-166x131x3", noise(1, 166, 131, 3, 17)),        # exactly two
        ("run-lengths", run_lengths()),
        ("two-valued-64x67x1", two_valued(18)),
        ("mask-518x518x1", rectangle_mask()),
        ("wide-3x10000x3", photo(1, 3, 10000, 3, 19)),         # one row per segment
        ("limit-15", limit_case()),
        ("batch-3x64x48x3", photo(3, 64, 48, 3, 20)),          # three different images: the offsets
        ("no-images", np.zeros((0, 5, 4, 3), dtype=np.uint8)),
    ]


STORED = {"1x1x1", "1x1x3", "photo-7x5x3", "noise-97x131x3", "noise-150x131x3", "noise-83x131x3", "noise-84x131x3",
          "noise-166x131x3"}                                   # every segment of these takes the stored block
REFUSED_WIDTH = 10923                                          # at C = 3: 1 + 3 * 10923 = 32770 > 32768


def zrle_size(filtered):
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(co.compress(filtered.tobytes()) + co.flush())


def size_bar(filtered, segments):
    return zrle_size(filtered) * 1.01 + 64 * segments + 16
