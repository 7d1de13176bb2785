"""Heat-map overlays: the numpy definition, the seeded cases and the case grid that tests/test_overlay_cpu.py and
tests/test_gpu_overlay.py share.  The definition is written here a second time, independently of
forward_utils.render_overlays_host (the contour by a summed-area table instead of shifted copies, the panels pixel by
pixel in one array instead of panel by panel), so that the two check each other.

For B images of H x W pixels: frames fp32 [B, 3, H, W], maps fp32 [B, H, W], a range record or None, pred / truth
uint8 [B, H, W] or None, lut uint8 [256, 3], alpha256 in 0 .. 256, thickness T in 0 .. 8, two colours, mean / std.
  F[c]        = clamp(rint(((x[c] * std[c]) + mean[c]) * 255), 0, 255), every operation rounded to fp32, NaN -> 0
  q           = trunc(min(max(n, 0), 1) * 255), the fp32 product rounded toward zero, NaN -> 0; n = (x - min) / (max - min)
                in fp32 when the record's max != 1, else x; x without a record
  contour(M)  M != 0 and some pixel inside the image with |dy| <= T and |dx| <= T has M == 0
  blend(u, v) = (alpha256 * u + (256 - alpha256) * v + 128) >> 8
  frame = F; heat = blend(F, lut[q]), pred_colour on contour(pred); truth = blend(F, truth_colour) where truth != 0
  else F, then truth_colour on contour(truth), then pred_colour on contour(pred)
-> uint8 [B, n * H, W, 3], the selected panels in the order frame, heat, truth.

THE GRID.  What the device code does differently from case to case is decided by the size (the tile shape, whether a
tile spans the width, the alignment of every byte run), by T (the halo), by which masks exist (what is staged) and by
the panel subset (the number of runs and where each starts); alpha256 and B enter only the per-pixel blend and the outer
loop.  So every size meets every T, every mask combination and both B (8 * 4 * 4 * 2 = 256 cases), and within every size
alpha256 and the panel subsets permitted by the masks rotate so that each size meets every alpha256 and every subset.
The special cases follow, each at two sizes.  No tolerance anywhere: the outputs are compared with np.array_equal."""
import functools
import itertools

import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PANELS = ("frame", "heat", "truth")
# (H, W): one pixel, one row, odd sizes below a wave, 37 (rows of 111 bytes), 70 (the tiny model's side), (64, 72) whose
# rows are multiples of 4 bytes, 126 (the tiny model's 2 x 2 canvas)
SIZES = ((1, 1), (1, 7), (5, 3), (7, 5), (37, 37), (70, 70), (64, 72), (126, 126))
WORKING = ((2, 518, 518), (1, 924, 924))          # (B, H, W), once each
BATCHES = (1, 3)
THICKNESS = (0, 1, 2, 8)
ALPHAS = (0, 77, 128, 256)
MASKS = ((False, False), (True, False), (False, True), (True, True))          # (pred, truth)
SUBSETS = tuple(tuple(p for p, keep in zip(PANELS, bits) if keep)
                for bits in itertools.product((True, False), repeat=3) if any(bits))
PRED_COLOUR, TRUTH_COLOUR = (255, 255, 255), (0, 255, 0)
SPECIALS = ("zero masks", "full masks", "single pixel", "border region", "mask values 255", "nan and inf maps",
            "no range record", "record max is 1")


def jet():
    i = np.arange(256)[:, None]
    return np.clip(383 - np.abs(4 * i - 255 * np.array([3, 2, 1])[None, :]), 0, 255).astype(np.uint8)


def gray():
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def record(mn, mx, nonfinite=0, positives=0):
    """the int64 [3] record of engine.metrics_range: min | max as two fp32 in the first word, then two counts"""
    r = np.zeros(3, np.int64)
    r[:1].view(np.float32)[:] = (mn, mx)
    r[1], r[2] = nonfinite, positives
    return r


def record_of(maps):
    """the record of finite maps: their minimum and maximum (the cases with a NaN or an infinity name their record)"""
    return record(np.float32(maps.min()), np.float32(maps.max()))


def normalise_lut_value(b, c, mean=CLIP_MEAN, std=CLIP_STD):
    """what engine._normalise_lut stores for byte b of channel c: ToTensor's and Normalize's fp32 steps"""
    return (np.float32(b) / np.float32(255) - np.float32(mean[c])) / np.float32(std[c])


def contour(mask, T):
    """bool [B, H, W], by a summed-area table of the zero pixels: the window is cut to the image"""
    m = np.asarray(mask) != 0
    if T == 0:
        return np.zeros_like(m)
    B, H, W = m.shape
    table = np.zeros((B, H + 1, W + 1), np.int64)
    table[:, 1:, 1:] = np.cumsum(np.cumsum(~m, axis=1), axis=2)
    y0, y1 = np.clip(np.arange(H) - T, 0, H), np.clip(np.arange(H) + T + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - T, 0, W), np.clip(np.arange(W) + T + 1, 0, W)
    zeros = (table[:, y1][:, :, x1] - table[:, y0][:, :, x1] - table[:, y1][:, :, x0] + table[:, y0][:, :, x0])
    return m & (zeros > 0)


def frame_bytes(frames, mean=CLIP_MEAN, std=CLIP_STD):
    """int [B, H, W, 3]"""
    out = np.empty(frames.shape[:1] + frames.shape[2:] + (3,), np.int64)
    with np.errstate(all="ignore"):
        for c in range(3):
            v = frames[:, c] * np.float32(std[c])
            v = v + np.float32(mean[c])
            v = np.rint(v * np.float32(255))
            assert v.dtype == np.float32
            v = np.where(v != v, np.float32(0), v)
            out[..., c] = np.minimum(np.maximum(v, 0), 255).astype(np.int64)
    return out


def heat_bytes(maps, range_record):
    """int [B, H, W]"""
    n = maps
    with np.errstate(all="ignore"):
        if range_record is not None:
            mn, mx = np.asarray(range_record, np.int64)[:1].view(np.float32)
            if mx != np.float32(1):
                n = (maps - mn) / (mx - mn)
                assert n.dtype == np.float32
        c = np.minimum(np.maximum(n, np.float32(0)), np.float32(1))        # numpy's minimum / maximum pass a NaN on
        q = np.trunc(c.astype(np.float64) * 255.0)          # exact in fp64; truncating it = truncating the RZ fp32 product
    return np.where(np.isnan(n), 0, np.nan_to_num(q)).astype(np.int64)


def render(frames, maps, range_record=None, pred=None, truth=None, lut=None, alpha256=128, thickness=1,
           pred_colour=PRED_COLOUR, truth_colour=TRUTH_COLOUR, mean=CLIP_MEAN, std=CLIP_STD, panels=None):
    lut = jet() if lut is None else lut
    if panels is None:
        panels = PANELS if truth is not None else PANELS[:2]
    if not panels or any(p not in PANELS for p in panels) or ("truth" in panels and truth is None):
        raise ValueError(f"panels {panels}")
    B, _, H, W = frames.shape
    a = int(alpha256)
    F = frame_bytes(frames, mean, std)
    heat = (a * F + (256 - a) * lut[heat_bytes(maps, range_record)].astype(np.int64) + 128) >> 8
    out = np.empty((B, len([p for p in PANELS if p in panels]), H, W, 3), np.int64)
    slot = 0
    cp = None if pred is None else contour(pred, thickness)
    for name in PANELS:
        if name not in panels:
            continue
        if name == "frame":
            out[:, slot] = F
        elif name == "heat":
            out[:, slot] = heat
        else:
            filled = (a * F + (256 - a) * np.array(truth_colour, np.int64) + 128) >> 8
            out[:, slot] = np.where((truth != 0)[..., None], filled, F)
            out[:, slot][contour(truth, thickness)] = truth_colour
        if name != "frame" and cp is not None:
            out[:, slot][cp] = pred_colour
        slot += 1
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8).reshape(B, -1, W, 3)


def _frames(rng, B, H, W):
    """bytes through the normalisation, a tenth of them pushed off the byte grid, a few far outside, one NaN, one inf"""
    b = rng.integers(0, 256, (B, 3, H, W))
    x = np.stack([normalise_lut_value(b[:, c], c) for c in range(3)], axis=1).astype(np.float32)
    off = rng.random(x.shape) < 0.1
    x = np.where(off, x + rng.uniform(-0.02, 0.02, x.shape).astype(np.float32), x).astype(np.float32)
    far = rng.random(x.shape) < 0.02
    x = np.where(far, rng.uniform(-9, 9, x.shape).astype(np.float32), x).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size >= 8:
        flat[rng.integers(flat.size)] = np.nan
        flat[rng.integers(flat.size)] = np.inf
        flat[rng.integers(flat.size)] = -np.inf
    return np.ascontiguousarray(x)


def _mask(rng, B, H, W):
    """a few rectangles per image, one of them on the border, in the values 1, 7 and 255; one lone pixel; one hole"""
    m = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for k in range(3):
            h, w = rng.integers(1, max(2, H // 2 + 1)), rng.integers(1, max(2, W // 2 + 1))
            y, x = (0, W - w) if k == 0 else (rng.integers(0, H - h + 1), rng.integers(0, W - w + 1))
            m[b, y:y + h, x:x + w] = (1, 7, 255)[k]
        m[b, rng.integers(H), rng.integers(W)] = 1
        m[b, rng.integers(H), rng.integers(W)] = 0
    return m


@functools.lru_cache(maxsize=None)
def inputs(B, H, W):
    """-> dict of the seeded arrays of one (B, H, W), computed once and not to be written to: frames, maps (in
    [-0.2, 1.3], a range wider than [0, 1]), record (of the maps), pred, truth"""
    rng = np.random.default_rng(1000003 * H + 1009 * W + B)
    d = {"frames": _frames(rng, B, H, W), "maps": rng.uniform(-0.2, 1.3, (B, H, W)).astype(np.float32),
         "pred": _mask(rng, B, H, W), "truth": _mask(rng, B, H, W)}
    d["record"] = record_of(d["maps"])
    for v in d.values():
        v.setflags(write=False)
    return d


def _subsets_for(has_truth):
    return [s for s in SUBSETS if has_truth or "truth" not in s]


def grid(size):
    """the cases of one size: dicts of keyword arguments for `arguments`"""
    H, W = size
    k = SIZES.index(size)
    seen = {True: 0, False: 0}            # the 16 cases with a truth mask walk its 7 subsets, the 16 without walk their 3
    for n, (T, (has_pred, has_truth), B) in enumerate(itertools.product(THICKNESS, MASKS, BATCHES)):
        subsets = _subsets_for(has_truth)
        seen[has_truth] += 1
        yield {"B": B, "H": H, "W": W, "T": T, "pred": has_pred, "truth": has_truth, "alpha256": ALPHAS[(n // 2 + n + k) % 4],
               "panels": subsets[(seen[has_truth] + k) % len(subsets)], "lut": "gray" if n % 5 == 4 else "jet",
               "special": None}


def specials():
    for (H, W), name in itertools.product(((7, 5), (70, 70)), SPECIALS):
        yield {"B": 2, "H": H, "W": W, "T": 2 if name != "full masks" else 8, "pred": True, "truth": True, "alpha256": 77,
               "panels": PANELS, "lut": "jet", "special": name}


def arguments(case):
    """a case -> (frames, maps, keywords of render / render_overlays_host); the arrays are fresh copies where a special
    case changes them"""
    d = inputs(case["B"], case["H"], case["W"])
    B, H, W = case["B"], case["H"], case["W"]
    frames, maps = d["frames"], d["maps"]
    pred = d["pred"] if case["pred"] else None
    truth = d["truth"] if case["truth"] else None
    rec = d["record"]
    s = case["special"]
    if s == "zero masks":
        pred, truth = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8)
    elif s == "full masks":                       # nothing is zero anywhere: no contour, at any thickness
        pred, truth = np.full((B, H, W), 3, np.uint8), np.full((B, H, W), 255, np.uint8)
    elif s == "single pixel":
        pred, truth = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8)
        pred[:, H // 2, W // 2] = 1
        truth[:, 0, 0] = 1
    elif s == "border region":
        pred, truth = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8)
        pred[:, :3, :] = 1
        truth[:, H - 3:, W - 2:] = 1
        truth[:, :, 0] = 1
    elif s == "mask values 255":
        pred, truth = (d["pred"] != 0).astype(np.uint8) * 255, (d["truth"] != 0).astype(np.uint8) * 255
    elif s == "nan and inf maps":
        maps = np.array(maps)
        maps[0, 0, 0], maps[-1, H // 2, W // 2], maps[0, H - 1, W - 1] = np.nan, np.inf, -np.inf
        maps[-1, 0, W - 1] = np.nan
    elif s == "no range record":
        rec = None
    elif s == "record max is 1":                  # the decision of metrics_normalise: the maps stay as they are
        rec = record(np.float32(-0.2), np.float32(1.0))
    kw = {"range_record": rec, "pred": pred, "truth": truth, "lut": jet() if case["lut"] == "jet" else gray(),
          "alpha256": case["alpha256"], "thickness": case["T"], "panels": tuple(case["panels"])}
    return frames, maps, kw


def case_id(case):
    return (f"{case['H']}x{case['W']}-B{case['B']}-T{case['T']}-a{case['alpha256']}-{'p' if case['pred'] else ''}"
            f"{'t' if case['truth'] else ''}-{'+'.join(case['panels'])}" + (f"-{case['special']}" if case["special"] else ""))


@functools.lru_cache(maxsize=None)
def _expected(key):
    case = dict(key)
    frames, maps, kw = arguments(case)
    want = render(frames, maps, **kw)
    want.setflags(write=False)
    return want


def expected(case):
    """the definition's bytes of a case, computed once"""
    return _expected(tuple(sorted((k, v if not isinstance(v, list) else tuple(v)) for k, v in case.items())))
