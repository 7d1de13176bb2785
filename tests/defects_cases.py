"""Cases shared by tests/test_defects_cpu.py and tests/test_gpu_defects_device.py (the region table, csrc/region_table.hip):
every mask pattern of tests/pro_cases.py at small shapes that are no multiple of a wave or a workgroup, scores with many
exact ties, constant, all-negative and signed-zero scores, second masks that are a shifted copy, empty and full, and the
minimum areas 1, 2, 9, H * W and H * W + 1.  Everything is computed once per argument tuple and handed out read-only;
the host table of a case (forward_utils.region_table_host) is computed once and shared."""
import collections
import functools

import numpy as np

import pro_cases as PC

SHAPES = [(1, 1, 2), (5, 8, 8), (3, 37, 53), (2, 70, 130)]
BIG = (2, 518, 518)                        # the workload's own image size: one case
SCORE_KINDS = [4, 16, 64, 0, "constant", "negative", "zeros"]     # numbers: PC.LEVELS' quantisation, 0 = unquantised
OTHER_KINDS = ["shifted", "empty", "full", None]

Case = collections.namedtuple("Case", "shape pattern connectivity scores other min_area normalise")


def min_areas(shape):
    return [1, 2, 9, shape[1] * shape[2], shape[1] * shape[2] + 1]


@functools.lru_cache(maxsize=None)
def scores(shape, kind, pattern="blobs"):
    """fp32 scores [N, H, W], loosely correlated with the pattern's mask.  A number: quantised to that many levels (4: many
    exact ties, so the position rule decides) with min < 0 and max != 1; "constant"; "negative": four levels, all below
    zero; "zeros": -0.0 and +0.0 mixed, with -1.0 elsewhere, so every peak is a zero of either sign."""
    rng = np.random.default_rng(4242 + shape[1] * 7 + shape[2] + SCORE_KINDS.index(kind))
    m = PC.mask(pattern, shape)
    if kind == "constant":
        s = np.full(shape, 0.25, np.float32)
    elif kind == "zeros":
        s = np.where(rng.random(shape) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        s = np.where(rng.random(shape) < 0.3, np.float32(-1.0), s).astype(np.float32)
    else:
        levels = 4 if kind == "negative" else kind
        s = 0.4 * m + rng.random(shape)
        s = (s - s.min()) / max(s.max() - s.min(), 1e-30)
        if levels:
            s = np.round(s * (levels - 1)) / (levels - 1)
        s = (-1.0 - s if kind == "negative" else s * 3.0 - 0.5).astype(np.float32)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def other(shape, pattern, kind):
    m = PC.mask(pattern, shape)
    if kind is None:
        return None
    o = {"shifted": np.roll(m, (1, 2), axis=(1, 2)) * 3, "empty": np.zeros_like(m), "full": np.ones_like(m)}[kind]
    o = np.ascontiguousarray(o, dtype=np.uint8)
    o.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def cases(shape):
    """Every pattern at both connectivities; score kinds, second masks and two minimum areas (1 and one of the other four)
    rotate so that each appears with several patterns; "blobs" and "random50" take all five minimum areas."""
    out = []
    ma = min_areas(shape)
    for i, pattern in enumerate(PC.PATTERNS):
        for j, connectivity in enumerate((8, 4)):
            kind = SCORE_KINDS[(i + 3 * j) % len(SCORE_KINDS)]
            normalise = isinstance(kind, int) and (i + j) % 2 == 0 and shape != (1, 1, 2)
            areas = ma if pattern in ("blobs", "random50") and connectivity == 8 else [1, ma[1 + (i + j) % 4]]
            for min_area in areas:
                out.append(Case(shape, pattern, connectivity, kind, OTHER_KINDS[(i + j) % 4], min_area, normalise))
    return out


BIG_CASE = Case(BIG, "blobs", 8, 4, "shifted", 9, True)


def normalised(s):
    """numpy's float32 (x - min) / (max - min) where max != 1, as forward_utils.metrics_eval forms it"""
    return (s - s.min()) / (s.max() - s.min()) if s.max() != 1 else s


def inputs(case):
    """-> (mask, raw scores, the scores as they are compared, other)"""
    raw = scores(case.shape, case.scores, case.pattern)
    return (PC.mask(case.pattern, case.shape), raw, normalised(raw) if case.normalise else raw,
            other(case.shape, case.pattern, case.other))


@functools.lru_cache(maxsize=None)
def host_table(case):
    import forward_utils as FU
    mask, _, compared, second = inputs(case)
    table = FU.region_table_host(mask, compared, other=second, min_area=case.min_area, connectivity=case.connectivity)
    for a in (table.rows, table.image_offsets, table.kept_mask):
        a.setflags(write=False)
    return table


def range_record(raw):
    """the bytes of aaclip_metrics_range's record for finite scores: fp32 min, fp32 max, two 64-bit counts"""
    rec = np.zeros(3, np.int64)
    rec[:1].view(np.float32)[:] = [raw.min(), raw.max()]
    return rec
