"""Cases and host restatements shared by tests/test_pro_cpu.py and tests/test_gpu_pro_device.py (per-region overlap,
csrc/regions.hip): the adversarial masks, scipy's labelling in the canonical ids of aaclip_metrics_regions, a
sequential numpy model of the three union-find phases, a brute-force PRO sweep over every distinct threshold, and
the score sets of the curve tests.  Everything is computed once per argument tuple and handed out read-only."""
import functools

import numpy as np
from scipy import ndimage

SHAPES = [(5, 8, 8), (3, 37, 53), (2, 70, 130), (2, 518, 518)]
PATTERNS = ["empty", "full", "checkerboard", "diagonal", "spiral", "comb", "serpentine", "rings", "random30",
            "random50", "random60", "blobs", "image_edge", "row_wrap"]


def _spiral(H, W):
    """one 1-pixel chain winding inwards with a 1-pixel gap between its turns"""
    m = np.zeros((H, W), np.uint8)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    y, x = 0, 0
    m[0, 0] = 1
    while True:
        moved = False
        for dy, dx, lim in ((0, 1, "right"), (1, 0, "bottom"), (0, -1, "left"), (-1, 0, "top")):
            while True:
                ny, nx = y + dy, x + dx
                if not (top <= ny <= bottom and left <= nx <= right):
                    break
                y, x = ny, nx
                m[y, x] = 1
                moved = True
            if lim == "right":
                top += 2
            elif lim == "bottom":
                right -= 2
            elif lim == "left":
                bottom -= 2
            else:
                left += 2
            if top > bottom or left > right:
                return m
        if not moved:
            return m


@functools.lru_cache(maxsize=None)
def mask(pattern, shape):
    N, H, W = shape
    rng = np.random.default_rng(PATTERNS.index(pattern) * 7919 + N * 31 + H * 17 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros(shape, np.uint8)
    if pattern == "empty":
        pass
    elif pattern == "full":
        m[:] = 1
    elif pattern == "checkerboard":
        m[:] = ((yy + xx) % 2 == 0)
    elif pattern == "diagonal":                  # one component at 8, min(H, W) components at 4
        m[:] = (yy == xx)
        m[-1] = (yy == W - 1 - xx)
    elif pattern == "spiral":
        m[:] = _spiral(H, W)
        m[-1] = _spiral(H, W)[::-1, ::-1]
    elif pattern == "comb":                      # teeth in every other column, joined in the last row only: late merges
        m[:] = (xx % 2 == 0) | (yy == H - 1)
    elif pattern == "serpentine":                # rows joined alternately at the right and at the left end
        m[:] = (yy % 2 == 0) | ((yy % 4 == 1) & (xx == W - 1)) | ((yy % 4 == 3) & (xx == 0))
    elif pattern == "rings":
        d = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
        m[:] = (d % 2 == 0)
    elif pattern.startswith("random"):
        m[:] = rng.random(shape) < int(pattern[6:]) / 100.0
    elif pattern == "blobs":
        field = ndimage.gaussian_filter(rng.normal(size=shape), sigma=(0, max(H / 16.0, 1.0), max(W / 16.0, 1.0)))
        m[:] = field > np.quantile(field, 0.8)
    elif pattern == "image_edge":                # the last row of image k and the first row of image k + 1
        m[:, -1, :] = 1
        m[:, 0, :] = 1
        m[:, -1, ::3] = 0
    elif pattern == "row_wrap":                  # the last column of a row and the first column of the next
        m[:, :, -1] = 1
        m[:, :, 0] = 1
        m[:, ::2, -1] = 0
        m[:, 1::4, 0] = 0
    else:
        raise KeyError(pattern)
    m.setflags(write=False)
    return m


def structure(connectivity):
    return np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)


def canonical(m, connectivity):
    """scipy.ndimage.label of every image, in the ids of aaclip_metrics_regions: -> (region uint32, area uint32,
    (regions, anomalous, normal))"""
    N, H, W = m.shape
    region = np.zeros(m.shape, np.uint32)
    area = np.zeros(m.shape, np.uint32)
    regions = 0
    flat = np.arange(H * W, dtype=np.int64).reshape(H, W)
    for k in range(N):
        lab, count = ndimage.label(m[k] != 0, structure=structure(connectivity))
        if count == 0:
            continue
        first = ndimage.minimum(flat, lab, index=np.arange(1, count + 1)).astype(np.int64)
        sizes = np.bincount(lab.reshape(-1), minlength=count + 1)
        ids = np.concatenate([[0], first + k * H * W + 1])
        region[k] = ids[lab]
        area[k] = (sizes * (np.arange(count + 1) != 0))[lab]
        regions += count
    anomalous = int(np.count_nonzero(m))
    return region, area, (regions, anomalous, m.size - anomalous)


def union_find_model(m, connectivity, order=None):
    """The three phases of csrc/regions.hip, sequentially: init parent[i] = i; every anomalous pixel (in `order`) is
    joined with its W / N (and NW / NE where N is normal) neighbours by find + minimum; flatten, count at the root,
    gather.  -> (region, area) like canonical()."""
    N, H, W = m.shape
    flat = m.reshape(-1)
    n = flat.size
    parent = np.arange(n, dtype=np.int64)

    def find(i):
        while parent[i] < i:
            i = parent[i]
        return i

    def union(a, b):
        while True:
            a, b = find(a), find(b)
            if a == b:
                return
            if a < b:
                a, b = b, a
            old = parent[a]
            parent[a] = min(old, b)
            if old >= a:
                return
            a = old

    pixels = np.flatnonzero(flat) if order is None else order
    for i in pixels:
        i = int(i)
        x, y = i % W, (i // W) % H
        if x > 0 and flat[i - 1]:
            union(i, i - 1)
        if y == 0:
            continue
        if flat[i - W]:
            union(i, i - W)
        elif connectivity == 8:
            if x > 0 and flat[i - W - 1]:
                union(i, i - W - 1)
            if x + 1 < W and flat[i - W + 1]:
                union(i, i - W + 1)
    region = np.zeros(n, np.uint32)
    count = np.zeros(n, np.int64)
    for i in np.flatnonzero(flat):
        r = find(int(i))
        region[i] = r + 1
        count[r] += 1
    area = np.where(region != 0, count[region.astype(np.int64) - 1], 0).astype(np.uint32)
    return region.reshape(m.shape), area.reshape(m.shape)


def pro_brute_force(labels, scores, fpr_limit, connectivity=8):
    """The PRO curve by a sweep over every distinct threshold, the overlap of every region computed region by region;
    scores are taken as they are.  fp64 throughout."""
    labels = np.asarray(labels)
    region, _, (R, _, n_ok) = canonical((labels != 0).astype(np.uint8), connectivity)
    region, s = region.reshape(-1), np.asarray(scores).reshape(-1)
    ids = np.unique(region[region != 0])
    xs, ys = [0.0], [0.0]
    for t in np.unique(s)[::-1]:
        pred = s >= t
        xs.append(float(np.count_nonzero(pred & (region == 0))) / float(n_ok))
        overlap = [np.count_nonzero(pred & (region == r)) / float(np.count_nonzero(region == r)) for r in ids]
        ys.append(min(1.0, float(np.sum(overlap)) / float(R)))
    total = 0.0
    for g in range(1, len(xs)):
        if xs[g] <= fpr_limit:
            total += 0.5 * (xs[g] - xs[g - 1]) * (ys[g] + ys[g - 1])
        else:
            if xs[g - 1] < fpr_limit:
                yl = ys[g - 1] + (ys[g] - ys[g - 1]) * ((fpr_limit - xs[g - 1]) / (xs[g] - xs[g - 1]))
                total += 0.5 * (fpr_limit - xs[g - 1]) * (yl + ys[g - 1])
            break
    return total / fpr_limit


LEVELS = [4, 16, 64, 0]          # quantisation levels of the scores; 0 = unquantised


@functools.lru_cache(maxsize=None)
def curve_case(shape, levels):
    """-> (mask uint8 [N, H, W] of blobs, fp32 scores correlated with it): min < 0 and max != 1, so the normalisation
    acts"""
    m = mask("blobs", shape)
    rng = np.random.default_rng(1000 + shape[1] * 7 + levels)
    s = ndimage.gaussian_filter(m.astype(np.float64), sigma=(0, 1.5, 1.5)) + rng.normal(scale=0.35, size=shape)
    s = (s - s.min()) / (s.max() - s.min())
    if levels:
        s = np.round(s * (levels - 1)) / (levels - 1)
    s = (s * 3.0 - 0.5).astype(np.float32)
    s.setflags(write=False)
    return m, s


def harness_seed_is_safe(value, margin=1e-6):
    """value (an unrounded metric in [0, 1]) lies at least `margin` away from a rounding boundary of its fourth digit"""
    frac = (value * 1e4) % 1.0
    return abs(frac - 0.5) >= margin * 1e4
