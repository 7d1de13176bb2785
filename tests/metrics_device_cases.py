"""numpy restatement of csrc/metrics.hip, step by step -- the expected value of every test in
tests/test_gpu_metrics_device.py, and itself checked against sklearn and against the reference's own numbers
(tests/golden/metrics.npz) in tests/test_metrics_device_cpu.py.

  range / normalise   float32 min, max; (x - min) / (max - min) in float32 when max != 1
  keys                -0.0 -> +0.0; packed: bits << 1 | label (scores in [0, 1]); else bits ^ (sign ? ~0 : 1 << 31)
  sort                stable LSD radix sort, four passes of 8-bit digits, written out pass by pass
  curve               tie groups from the top: integer AUROC numerator, fp64 AP sum
"""
import functools

import numpy as np


def normalise(scores):
    """reference forward_utils.py:246-253 on a float32 array"""
    scores = np.asarray(scores, dtype=np.float32)
    mn, mx = scores.min(), scores.max()
    if mx != 1:
        return (scores - mn) / (mx - mn)
    return scores


def make_keys(scores, labels, packed):
    """-> uint32 keys (and the label beside them when it is not packed)"""
    bits = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1).view(np.uint32).copy()
    bits[bits == 0x80000000] = 0
    lab = (np.asarray(labels).reshape(-1) != 0)
    if packed:
        assert bits.max() <= 0x3F800000, "packed keys need scores in [0, 1]"
        return (bits << np.uint32(1)) | lab.astype(np.uint32)
    negative = (bits >> np.uint32(31)).astype(bool)
    return np.where(negative, ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def lsd_sort(keys, payload=None):
    """Stable LSD radix sort: per pass the digit counts, their exclusive prefix = the first output index of every
    digit, then every digit's keys, in input order, to consecutive places from there."""
    keys = np.asarray(keys, dtype=np.uint32)
    for shift in (0, 8, 16, 24):
        digit = ((keys >> np.uint32(shift)) & np.uint32(255)).astype(np.uint8)
        count = np.bincount(digit, minlength=256)
        first = np.concatenate([[0], np.cumsum(count)[:-1]])
        out = np.empty_like(keys)
        out_payload = None if payload is None else np.empty_like(payload)
        for v in np.nonzero(count)[0]:
            where = np.nonzero(digit == v)[0]            # ascending: input order is kept
            out[first[v]:first[v] + count[v]] = keys[where]
            if payload is not None:
                out_payload[first[v]:first[v] + count[v]] = payload[where]
        keys, payload = out, out_payload
    return keys, payload


def curve_sums(sorted_keys, sorted_labels, packed):
    """-> dict(num, P, N, groups, ap) from ascending keys"""
    k = np.asarray(sorted_keys, dtype=np.uint32)
    score = k >> np.uint32(1) if packed else k
    lab = (k & np.uint32(1)).astype(np.int64) if packed else (np.asarray(sorted_labels) != 0).astype(np.int64)
    n = k.size
    start = np.concatenate([[True], score[1:] != score[:-1]])
    i = np.nonzero(start)[0].astype(np.int64)                     # ascending group starts
    before = np.concatenate([[0], np.cumsum(lab)])                # positives before every index
    P = int(lab.sum())
    E = before[i]
    i2, E2 = np.concatenate([i[1:], [n]]), np.concatenate([E[1:], [P]])
    tp, tp0 = P - E, P - E2
    fp, fp0 = (n - i) - tp, (n - i2) - tp0
    num = int(np.sum(((fp - fp0) * (tp + tp0)).astype(np.uint64), dtype=np.uint64))
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = ((tp - tp0).astype(np.float64) / np.float64(P)) * (tp.astype(np.float64) / (tp + fp).astype(np.float64))
    return {"num": num, "P": P, "N": n - P, "groups": int(i.size), "ap": float(np.sum(terms[::-1]))}


def curve_metrics(scores, labels, per_image=0, normalise_scores=True):
    """What engine.curve_metrics computes: -> dict(auroc, ap, num, P, N, groups, image_max, normalised, keys,
    labels_sorted, packed)"""
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    labels = np.asarray(labels).reshape(-1)
    norm = normalise(scores) if normalise_scores else scores
    packed = bool(norm.min() >= 0 and norm.max() <= 1)
    keys = make_keys(norm, labels, packed)
    keys, lab = lsd_sort(keys, None if packed else (labels != 0).astype(np.uint8))
    out = curve_sums(keys, lab, packed)
    out["auroc"] = out["num"] / (2 * out["P"] * out["N"])
    out["image_max"] = norm.reshape(-1, per_image).max(axis=1) if per_image else None
    out.update(normalised=norm, keys=keys, labels_sorted=lab, packed=packed)
    return out


def metrics_eval_restated(pixel_label, image_label, pixel_preds, image_preds, class_names, domain):
    """forward_utils.metrics_eval with sklearn's two functions replaced by the restatement"""
    pixel_preds, image_preds = np.asarray(pixel_preds), np.asarray(image_preds)
    pixel_label, image_label = np.asarray(pixel_label), np.asarray(image_label)
    n = pixel_preds.shape[0]
    pixel = curve_metrics(pixel_preds, pixel_label, per_image=pixel_preds.size // n)
    image_preds = normalise(image_preds)
    if image_preds.ndim == 2 and image_preds.shape[1] == 2:
        image_preds = image_preds[:, 0]
    image_preds = image_preds.reshape(-1)
    score = pixel["image_max"] * 0.5 + image_preds * 0.5 if domain != "Medical" else pixel["image_max"]
    if image_label.max() != image_label.min():
        image = curve_metrics(score, image_label, normalise_scores=False)
        image_auc, image_ap = image["auroc"], image["ap"]
    else:
        image_auc = image_ap = 0
    return {"class name": class_names, "pixel AUC": round(pixel["auroc"], 4) * 100,
            "pixel AP": round(pixel["ap"], 4) * 100, "image AUC": round(image_auc, 4) * 100,
            "image AP": round(image_ap, 4) * 100}


# ------------------------------------------------------------------------------------------------- test inputs
def sort_sizes(group_items):
    """n of the sort tests: the wave width and the thread count +- 1, one workgroup's keys +- 1, two workgroups' + 1,
    the golden set's pixel count, and a size whose digit table has more rows than the scan has segments"""
    return [2, 63, 64, 65, 255, 256, 257, group_items - 1, group_items, group_items + 1, 2 * group_items + 1,
            27648, 2 ** 20 + 3]


@functools.lru_cache(maxsize=None)
def inputs(n, kind):
    """-> (scores float32 [n], labels uint8 [n]); both classes present, max != min.
    kind 'plain': normal scores (normalised by the code under test); 'coarse': the same on a grid of 1/4 (many ties);
    'passthrough': max == 1 exactly, negative scores, -0.0 and +0.0 (no normalisation: the label is a payload)"""
    rng = np.random.default_rng(1000 + n)
    labels = (rng.random(n) < 0.3).astype(np.uint8)
    labels[0], labels[1] = 1, 0
    scores = (rng.normal(size=n) + 1.2 * labels).astype(np.float32)
    if kind == "coarse":
        scores = (np.round(scores * 4) / 4).astype(np.float32)
        if scores.max() == scores.min():
            scores[0] += 1
    elif kind == "passthrough":
        scores = np.minimum(np.round(scores * 8) / 8, 1).astype(np.float32)
        scores[0] = 1.0
        scores[1] = -0.5
        if n > 4:
            scores[2], scores[3] = -0.0, 0.0
    else:
        assert kind == "plain"
        if n == 2:
            scores[:] = [0.7, 0.3]
    return scores, labels


@functools.lru_cache(maxsize=None)
def expected(n, kind):
    scores, labels = inputs(n, kind)
    return curve_metrics(scores, labels)
