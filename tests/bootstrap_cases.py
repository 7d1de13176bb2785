"""The bootstrap of AUROC / AP over images restated in numpy, one replicate at a time, and the inputs of
tests/test_bootstrap_cpu.py and tests/test_gpu_bootstrap.py.

  replicate_sums   one replicate's record from the ascending keys, the payload image << 1 | label and the image weights:
                   the weighted form of metrics_device_cases.curve_sums (which it is for weights of 1)
  records          every replicate of a count matrix -> dict(num, P, N, ap, valid)
  repeated         sklearn on the literally repeated images (np.repeat), what the weighted sums stand for

forward_utils.bootstrap_eval (vectorised over the replicates) and csrc/bootstrap.hip are both measured against this file.
"""
import functools

import numpy as np

import metrics_device_cases as MD

IMAGES, PER_IMAGE = 23, 535                # n = 12 305: three tiles of 4096 + 17, no multiple of 64
NORMAL = 12                                # images 0 .. 11 are normal, 12 .. 22 anomalous
KINDS = ["distinct", "coarse", "run"]
REPLICATES = [1, 64, 65, 200]              # a partial block, a whole one, a block + 1, four blocks with a partial last


def replicate_sums(sorted_keys, sorted_payload, weights):
    """-> dict(num, P, N, ap, valid): Python integers and a float; an invalid replicate (P == 0 or N == 0) has num = ap = 0"""
    k = np.asarray(sorted_keys, dtype=np.uint32)
    pay = np.asarray(sorted_payload).astype(np.int64)
    w = np.asarray(weights, dtype=np.int64)[pay >> 1]
    lab = pay & 1
    n = k.size
    start = np.concatenate([[True], k[1:] != k[:-1]])
    i = np.nonzero(start)[0]
    i2 = np.concatenate([i[1:], [n]])
    M = np.concatenate([[0], np.cumsum(w)])
    E = np.concatenate([[0], np.cumsum(w * lab)])
    P, Mtot = int(E[-1]), int(M[-1])
    if P == 0 or Mtot - P == 0:
        return {"num": 0, "P": P, "N": Mtot - P, "ap": 0.0, "valid": False}
    tp, tp0 = P - E[i], P - E[i2]
    fp, fp0 = (Mtot - M[i]) - tp, (Mtot - M[i2]) - tp0
    num = int(np.sum(((fp - fp0) * (tp + tp0)).astype(np.uint64), dtype=np.uint64))
    ap = 0.0
    for g in np.nonzero(tp != tp0)[0]:                       # a group without a weighted positive adds exactly 0
        ap += (float(tp[g] - tp0[g]) / float(P)) * (float(tp[g]) / float(tp[g] + fp[g]))
    return {"num": num, "P": P, "N": Mtot - P, "ap": ap, "valid": True}


def records(sorted_keys, sorted_payload, counts):
    rows = [replicate_sums(sorted_keys, sorted_payload, c) for c in np.asarray(counts)]
    return {"num": np.array([r["num"] for r in rows], np.int64), "P": np.array([r["P"] for r in rows], np.int64),
            "N": np.array([r["N"] for r in rows], np.int64), "ap": np.array([r["ap"] for r in rows], np.float64),
            "valid": np.array([r["valid"] for r in rows], bool)}


def sorted_pairs(scores, labels, per_image):
    """the stable pair sort that engine.metrics_sort_pairs performs: -> (ascending uint32 keys, payload in their order)"""
    scores = np.asarray(scores, np.float32).reshape(-1)
    payload = ((np.arange(scores.size) // per_image) << 1 | (np.asarray(labels).reshape(-1) != 0)).astype(np.int32)
    return MD.lsd_sort(MD.make_keys(scores, None if labels is None else labels, False), payload)


def repeated(labels, scores, counts_row):
    """sklearn's two numbers of the images repeated counts_row[i] times each; labels, scores [images, per_image]"""
    from sklearn.metrics import average_precision_score, roc_auc_score
    idx = np.repeat(np.arange(len(counts_row)), counts_row)
    l, s = np.asarray(labels)[idx].reshape(-1), np.asarray(scores)[idx].reshape(-1)
    return roc_auc_score(l, s), average_precision_score(l, s)


# ------------------------------------------------------------------------------------------------- test inputs
@functools.lru_cache(maxsize=None)
def small_class(kind):
    """12 images x 37 pixels for the sklearn comparison: 'ties' (steps of 1/2) or 'no ties'"""
    rng = np.random.default_rng(7)
    image_label = np.arange(12) % 2
    labels = ((rng.random((12, 37)) < 0.3) & (image_label[:, None] == 1)).astype(np.uint8)
    labels[1, 0] = 1
    scores = rng.normal(size=(12, 37)) + labels
    if kind == "ties":
        scores = np.round(scores * 2) / 2
    else:
        assert kind == "no ties"
    return labels, scores.astype(np.float32), image_label


@functools.lru_cache(maxsize=None)
def pixel_class(kind):
    """-> (scores float32 [23, 535], labels uint8 [23, 535], image_label [23]); scores in (0, 1), passed through as they are.
    'distinct': every score its own group; 'coarse': 40 levels; 'run': one constant run of 9 000 sorted elements, from
    sorted index 1 000 to 10 000, across the tile boundaries at 4 096 and 8 192 (tile 1 has no start)"""
    rng = np.random.default_rng(23)
    image_label = (np.arange(IMAGES) >= NORMAL).astype(np.uint8)
    labels = ((rng.random((IMAGES, PER_IMAGE)) < 0.25) & (image_label[:, None] == 1)).astype(np.uint8)
    labels[NORMAL:, 0] = 1                                   # every anomalous image holds a positive pixel
    n = IMAGES * PER_IMAGE
    rank = rng.permutation(n).reshape(IMAGES, PER_IMAGE)
    rank = np.where(labels == 1, np.minimum(rank + n // 3, n - 1), rank)      # positives lean upwards; ties appear, fine
    if kind == "distinct":
        rank = np.argsort(np.argsort(rank.reshape(-1) * 2 + labels.reshape(-1), kind="stable")).reshape(IMAGES, PER_IMAGE)
        scores = (rank + 1) / (n + 2)
    elif kind == "coarse":
        scores = (rank * 40 // n + 1) / 42
    else:
        assert kind == "run"
        order = np.argsort(np.argsort(rank.reshape(-1) * 2 + labels.reshape(-1), kind="stable")).reshape(IMAGES, PER_IMAGE)
        scores = np.where((order >= 1000) & (order < 10000), 1000, order) + 1
        scores = scores / (n + 2)
    return scores.astype(np.float32), labels, image_label


def hand_counts():
    """all ones; image 13 (anomalous) 23 times; every anomalous image 0 (invalid); every normal image 0 (invalid)"""
    rows = np.zeros((4, IMAGES), np.uint8)
    rows[0] = 1
    rows[1, 13] = IMAGES
    rows[2, :NORMAL] = [2] * (NORMAL - 1) + [1]
    rows[3, NORMAL:] = [2] * (IMAGES - NORMAL) + [0] * 0
    rows[3, NORMAL] += 1
    assert rows.sum(axis=1).tolist() == [IMAGES] * 4
    return rows


@functools.lru_cache(maxsize=None)
def expected(kind):
    """-> (keys, payload, {R: (counts, records)}) of pixel_class(kind): drawn rows with seed 0 followed by hand_counts"""
    import forward_utils as FU
    scores, labels, _ = pixel_class(kind)
    keys, payload = sorted_pairs(scores, labels, PER_IMAGE)
    out = {}
    drawn = FU.bootstrap_counts(IMAGES, max(REPLICATES), 0, 0)
    for R in REPLICATES:
        counts = np.concatenate([drawn[:R - 4], hand_counts()])[:R] if R >= 4 else hand_counts()[:R]
        out[R] = (counts, records(keys, payload, counts))
    return keys, payload, out
