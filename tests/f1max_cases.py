"""Shared inputs of the F1-max tests and a brute-force restatement of the definition (forward_utils.f1max_eval's
docstring): a sweep over every distinct threshold with exact rational comparison, nothing sorted.

  brute_force(labels, scores)     -> (tp, fp, fn, threshold, groups)
  f1max_inputs(n, kind)           -> (scores float32 [n] in [0, 1] unless kind is 'passthrough', labels uint8 [n])
  threshold_inputs(shape, mode)   -> (scores float32 [N, H, W], labels uint8 [N, H, W])
"""
import functools
from fractions import Fraction

import numpy as np

import metrics_device_cases as MD

CURVE_TILE = 4096
SIZES = lambda group: [2, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, group + 1, 2 ** 20 + 3]   # noqa: E731
CURVE_KINDS = ["plain", "coarse", "passthrough"]                       # the score sets of the curve tests
EXTRA_KINDS = ["ties_but_one", "top", "bottom", "tp0_top", "distinct"]
TIE_K = [1, 50, 700, 30000]                                            # n = 6 k; groups = 4 k + 1
THRESHOLD_SHAPES = [(5, 8, 8), (3, 37, 53), (2, 70, 130), (2, 518, 518)]


def brute_force(labels, scores):
    """Every distinct score as a threshold, predicted = score >= threshold; the largest F1 = 2 tp / (2 tp + fp + fn) as
    a Fraction, the highest threshold among equal ones."""
    scores = np.asarray(scores).reshape(-1)
    pos = np.asarray(labels).reshape(-1) != 0
    P = int(pos.sum())
    levels = np.unique(scores)                    # -0.0 and +0.0 are one level
    best = None
    for t in levels:
        flagged = scores >= t
        tp = int(np.count_nonzero(flagged & pos))
        fp = int(np.count_nonzero(flagged)) - tp
        cand = (Fraction(2 * tp, 2 * tp + fp + (P - tp)), float(t) + 0.0, tp, fp)
        if best is None or cand[:2] > best[:2]:
            best = cand
    return best[2], best[3], P - best[2], best[1], int(levels.size)


def exact_tie(k):
    """Descending labels 1,0,0,0,0,1 scaled by k: the top 2 k elements share one score (k positives, k negatives), 3 k
    negatives and then k positives follow with distinct scores.  F1 = 1/2 after the top group and again after all 6 k
    elements, less in between: the top group must win.  -> (scores float32 in [0, 1], labels uint8), shuffled."""
    n = 6 * k
    labels = np.concatenate([np.ones(k), np.zeros(k), np.zeros(3 * k), np.ones(k)]).astype(np.uint8)
    below = (np.arange(4 * k, 0, -1, dtype=np.float64) - 1) / (8 * k)          # distinct, descending, below 1/2
    scores = np.concatenate([np.full(2 * k, 1.0), below]).astype(np.float32)
    assert np.unique(scores).size == 4 * k + 1
    order = np.random.default_rng(k).permutation(n)
    return scores[order], labels[order]


@functools.lru_cache(maxsize=None)
def f1max_inputs(n, kind):
    if kind in CURVE_KINDS:
        scores, labels = MD.inputs(n, kind)
        return MD.normalise(scores), labels
    rng = np.random.default_rng(7000 + n)
    if kind == "distinct":                        # n groups: every thread of the argmax several, every workgroup a share
        scores = (rng.permutation(n).astype(np.float64) / n).astype(np.float32)
        assert np.unique(scores).size == n
        labels = (rng.random(n) < 0.25 + 0.5 * scores).astype(np.uint8)
        labels[np.argmax(scores)], labels[np.argmin(scores)] = 1, 0
        return scores, labels
    if kind == "ties_but_one":                    # two groups
        scores = np.full(n, 0.5, np.float32)
        labels = (rng.random(n) < 0.4).astype(np.uint8)
        labels[0], labels[n - 1] = 1, 0
        scores[0] = 1.0
        return scores, labels
    if kind == "top":                             # the only positive has the highest score: F1 = 1 at the top group
        scores = (rng.permutation(n).astype(np.float64) / n).astype(np.float32)
        labels = np.zeros(n, np.uint8)
        labels[np.argmax(scores)] = 1
        return scores, labels
    if kind == "bottom":                          # the only negative has the highest score: flag everything
        scores = (np.round(rng.random(n) * 64) / 128).astype(np.float32)
        labels = np.ones(n, np.uint8)
        k = int(rng.integers(n))
        labels[k], scores[k] = 0, 1.0
        return scores, labels
    assert kind == "tp0_top"                      # the highest scores are all negatives': groups with tp = 0 come first
    scores = (np.round(rng.random(n) * 255) / 512).astype(np.float32)
    labels = (rng.random(n) < 0.3).astype(np.uint8)
    labels[0], labels[n - 1] = 1, 0
    top = rng.random(n) < 0.2
    top[0], top[n - 1] = False, True
    scores[top] = (0.75 + np.round(rng.random(int(top.sum())) * 15) / 64).astype(np.float32)
    labels[top] = 0
    return scores, labels


@functools.lru_cache(maxsize=None)
def threshold_inputs(shape, mode):
    """mode 'raw': scores in about [-3, 5] on a grid of 1/8 (ties, max != 1: normalised on the fly), zeros of both signs;
    'unit': scores in [0, 1] with max == 1 on a grid of 1/32, taken as they are;
    'zero': every positive scores >= 0, some of them -0.0 and +0.0, every negative below 0: the threshold is 0 and a
    -0.0 has to be flagged."""
    rng = np.random.default_rng(sum(shape) + len(mode))
    n = int(np.prod(shape))
    labels = (rng.random(n) < 0.3).astype(np.uint8)
    labels[0], labels[n - 1] = 1, 0
    if mode == "raw":
        scores = (np.round((rng.normal(size=n) + 1.5 * labels) * 8) / 8).astype(np.float32)
        scores[[1, n // 2]] = -0.0, 0.0
    elif mode == "unit":
        scores = np.clip(np.round((rng.random(n) * 0.7 + 0.3 * labels) * 32) / 32, 0, 1).astype(np.float32)
        scores[0], scores[n - 1] = 1.0, 0.0
    else:
        assert mode == "zero"
        scores = np.where(labels != 0, np.round(rng.random(n) * 4) / 4, -0.25 - rng.random(n)).astype(np.float32)
        pos = np.flatnonzero(labels)
        scores[pos[0]] = -0.0
        scores[pos[-1]] = 0.0
    return scores.reshape(shape), labels.reshape(shape)
