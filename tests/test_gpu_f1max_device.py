"""The exact F1-max and the masks at a threshold on the device (csrc/metrics.hip: aaclip_metrics_f1max,
aaclip_metrics_threshold) against the host definition forward_utils.f1max_eval, which tests/test_f1max_cpu.py ties to a
brute-force sweep and to sklearn, and against numpy.

Everything here is integers, or an fp32 threshold that is one of the input scores: every comparison is for EQUALITY.
F1 itself is 2 tp / (2 tp + fp + fn), one division of Python integers on both sides: equal bits follow from equal counts.
Every output of the two entries lies between guard words, and their workspaces are filled with garbage first."""
import numpy as np
import pytest
import torch

import f1max_cases as FC
import metrics_device_cases as MD
from aaclip_hip import _lib, engine

pytestmark = pytest.mark.gpu

GROUP = _lib.load().aaclip_metrics_sort_group_items()
T = torch.from_numpy
GUARD = 8                       # int64 words in front of and behind a record
SENTINEL = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def f1_bits(x):
    return np.float32(x).view(np.uint32)


# ------------------------------------------------------------------------------------------ aaclip_metrics_f1max
def f1max_raw(dev, keys, labels_sorted, packed):
    """aaclip_metrics_f1max with guard words around the record and a workspace full of garbage -> the record's dict"""
    lib = _lib.load()
    n = keys.numel()
    buf = torch.full((engine.F1MAX_RECORD_WORDS + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    need = lib.aaclip_metrics_f1max_workspace_bytes(n)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    _lib.check(lib.aaclip_metrics_f1max(keys.data_ptr(), None if packed else labels_sorted.data_ptr(), n, int(packed),
                                        buf[GUARD:].data_ptr(), ws.data_ptr(), need, stream(dev)), "metrics_f1max")
    h = buf.cpu()
    assert h[:GUARD].tolist() == [SENTINEL] * GUARD and h[-GUARD:].tolist() == [SENTINEL] * GUARD, "guard words written"
    return engine.f1max_record_host(h[GUARD:-GUARD].contiguous())


def check_f1max(dev, scores, labels):
    """both key forms (the packed one where the scores lie in [0, 1]) against f1max_eval; the curve's record untouched"""
    import forward_utils as FU
    want = FU.f1max_eval(labels, scores)
    s, l = T(np.array(scores)).to(dev), T(np.array(labels)).to(dev)
    forms = [False] + ([True] if scores.min() >= 0 and scores.max() <= 1 else [])
    for packed in forms:
        keys, labels_sorted, _ = engine.metrics_sort(s, l, packed)
        before = engine.metrics_curve(keys, labels_sorted, packed).cpu()          # a call made without the new entry
        got = f1max_raw(dev, keys, labels_sorted, packed)
        assert (got["tp"], got["fp"], got["P"] - got["tp"], got["groups"]) == (want.tp, want.fp, want.fn, want.groups), \
            (packed, got, want)
        assert got["P"] + got["N"] == scores.size
        assert f1_bits(got["threshold"]) == f1_bits(want.threshold), (packed, got, want)
        first = int(np.count_nonzero(scores < np.float32(want.threshold)))        # ascending index of the group's start
        assert got["start"] == first == scores.size - want.tp - want.fp
        key = MD.make_keys(np.float32([want.threshold]), [0], packed)[0]
        assert got["key"] == (int(key) >> 1 if packed else int(key))
        assert f1max_raw(dev, keys, labels_sorted, packed) == got                 # two calls, equal records
        after = engine.metrics_curve(keys, labels_sorted, packed).cpu()
        assert torch.equal(before[:5], after[:5])                                 # the shared phases serve both entries
        rec = engine.metrics_f1max(keys, labels_sorted, packed)                   # the Python wrapper
        assert engine.f1max_record_host(rec) == got
    return want


@pytest.mark.parametrize("kind", FC.CURVE_KINDS + FC.EXTRA_KINDS)
@pytest.mark.parametrize("n", FC.SIZES(GROUP))
def test_f1max_record_is_f1max_evals(dev, n, kind):
    scores, labels = FC.f1max_inputs(n, kind)
    want = check_f1max(dev, scores, labels)
    if kind == "top":
        assert (want.f1, want.tp, want.fp) == (1.0, 1, 0)
    if kind == "bottom":
        assert want.tp + want.fp == n and want.fp == 1           # everything is flagged
    if kind == "distinct":
        assert want.groups == n
    if kind == "ties_but_one":
        assert want.groups == 2


@pytest.mark.parametrize("k", FC.TIE_K)
def test_exact_tie_goes_to_the_higher_score(dev, k):
    """the two groups of F1 = 1/2 are the first and the last of 4 k + 1: different threads at k = 1, and from k = 50 on
    (more than one workgroup) the first and the last workgroup's shares"""
    scores, labels = FC.exact_tie(k)
    want = check_f1max(dev, scores, labels)
    assert (want.f1, want.tp, want.fp, want.fn, want.threshold, want.groups) == (0.5, k, k, k, 1.0, 4 * k + 1)
    # the mirror image must not win either: with the LOW group alone at 1/2 (one positive less at the top) it does
    scores2, labels2 = scores.copy(), labels.copy()
    labels2[np.flatnonzero((scores == 1.0) & (labels == 1))[0]] = 0
    labels2[np.flatnonzero((scores < 0.5) & (labels == 0))[0]] = 1
    check_f1max(dev, scores2, labels2)


# -------------------------------------------------------------------------------------- aaclip_metrics_threshold
def threshold_raw(dev, scores, labels, per_image, range_record, f1_record, want_mask, offsets):
    """aaclip_metrics_threshold on base pointers offset by 1 .. 3 elements, guard bytes / words around every output and
    a workspace full of garbage -> (mask or None, image_counts or None, totals)"""
    lib = _lib.load()
    n = scores.size
    o_s, o_l, o_m, o_c = offsets
    s_buf = torch.zeros(n + 8, dtype=torch.float32, device=dev)
    s_buf[o_s:o_s + n] = T(scores.reshape(-1)).to(dev)
    l_buf = None
    if labels is not None:
        l_buf = torch.zeros(n + 8, dtype=torch.uint8, device=dev)
        l_buf[o_l:o_l + n] = T(labels.reshape(-1)).to(dev)
    G = 64
    m_buf = torch.full((n + 2 * G + 8,), 0x5A, dtype=torch.uint8, device=dev) if want_mask else None
    counts = labels is not None and per_image > 0
    images = n // per_image if per_image else 0
    c_buf = torch.full((4 * images + 2 * G + 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev) if counts else None
    t_buf = torch.full((4 + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    need = lib.aaclip_metrics_threshold_workspace_bytes(n, per_image)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    _lib.check(lib.aaclip_metrics_threshold(
        s_buf[o_s:].data_ptr(), None if l_buf is None else l_buf[o_l:].data_ptr(), n, per_image,
        None if range_record is None else range_record.data_ptr(), f1_record.data_ptr(),
        None if m_buf is None else m_buf[G + o_m:].data_ptr(), None if c_buf is None else c_buf[G + o_c:].data_ptr(),
        t_buf[GUARD:].data_ptr(), ws.data_ptr(), need, stream(dev)), "metrics_threshold")
    mask = image_counts = None
    if want_mask:
        h = m_buf.cpu().numpy()
        assert np.all(h[:G + o_m] == 0x5A) and np.all(h[G + o_m + n:] == 0x5A), "guard bytes of the mask were written"
        mask = h[G + o_m:G + o_m + n]
    if counts:
        h = c_buf.cpu().numpy()
        assert np.all(h[:G + o_c] == 0x5A5A5A5A) and np.all(h[G + o_c + 4 * images:] == 0x5A5A5A5A), "guard words written"
        image_counts = h[G + o_c:G + o_c + 4 * images].reshape(images, 4)
    h = t_buf.cpu()
    assert h[:GUARD].tolist() == [SENTINEL] * GUARD and h[-GUARD:].tolist() == [SENTINEL] * GUARD
    return mask, image_counts, [int(v) for v in h[GUARD:GUARD + 4]]


def numpy_counts(flag, pos, images):
    flag, pos = flag.reshape(images, -1), pos.reshape(images, -1)
    per = np.stack([(flag & pos).sum(1), (flag & ~pos).sum(1), (~flag & pos).sum(1), (~flag & ~pos).sum(1)], axis=1)
    return per, [int(v) for v in per.sum(0)]


@pytest.mark.parametrize("mode", ["raw", "unit", "zero"])
@pytest.mark.parametrize("shape", FC.THRESHOLD_SHAPES)
def test_threshold_masks_and_counts_are_numpys(dev, shape, mode):
    import forward_utils as FU
    scores, labels = FC.threshold_inputs(shape, mode)
    images, per_image, n = shape[0], shape[1] * shape[2], scores.size
    normalise = mode == "raw"
    records = {}
    _, f1 = engine.f1max_metrics(T(np.array(scores)).to(dev), T(np.array(labels)).to(dev), per_image=per_image,
                                 normalise=normalise, records=records)
    values = MD.normalise(scores) if normalise else scores                # what the sorted path sorted
    want = FU.f1max_eval(labels, values)
    assert f1 == want
    flag, pos = values >= np.float32(want.threshold), labels != 0
    assert np.count_nonzero(values == np.float32(want.threshold)) >= 1    # scores equal to the threshold are flagged
    if mode == "zero":
        assert want.threshold == 0.0 and flag.reshape(-1)[np.flatnonzero(np.signbit(scores.reshape(-1)) & (scores.reshape(-1) == 0))].all()
    per, tot = numpy_counts(flag, pos, images)
    rng = records["range"] if normalise else None
    for offsets in [(1, 1, 1, 1), (2, 3, 1, 2), (3, 2, 2, 3), (0, 0, 0, 0), (1, 0, 3, 0)]:
        mask, image_counts, totals = threshold_raw(dev, scores, labels, per_image, rng, records["f1max"], True, offsets)
        assert np.array_equal(mask, flag.reshape(-1).astype(np.uint8)), offsets
        assert np.array_equal(image_counts, per), offsets
        assert totals == tot and totals[:2] == [want.tp, want.fp] and totals[2] == want.fn, offsets
    # one segment (per_image = 0), no mask output, no labels
    mask, image_counts, totals = threshold_raw(dev, scores, labels, 0, rng, records["f1max"], False, (3, 1, 0, 0))
    assert mask is None and image_counts is None and totals == tot
    mask, image_counts, totals = threshold_raw(dev, scores, None, per_image, rng, records["f1max"], True, (2, 0, 3, 0))
    assert image_counts is None and np.array_equal(mask, flag.reshape(-1).astype(np.uint8))
    assert totals == [0, int(flag.sum()), 0, n - int(flag.sum())]
    # the Python wrapper: the record or a number, the mask in the scores' shape
    s, l = T(np.array(scores)).to(dev), T(np.array(labels)).to(dev)
    for threshold in (records["f1max"], want.threshold):
        m, c, t = engine.metrics_threshold(s, threshold, labels=l, per_image=per_image, range_record=rng)
        assert m.shape == s.shape and m.dtype == torch.uint8 and np.array_equal(m.cpu().numpy(), flag.astype(np.uint8))
        assert np.array_equal(c.cpu().numpy(), per) and t.cpu().tolist() == tot
    m, c, t = engine.metrics_threshold(s, want.threshold, range_record=rng, totals=False)
    assert c is None and t is None and np.array_equal(m.cpu().numpy(), flag.astype(np.uint8))


def test_threshold_wrapper_refusals(dev):
    s = torch.rand(4, 8, device=dev)
    with pytest.raises(ValueError, match="multiple of per_image"):
        engine.metrics_threshold(s, 0.5, per_image=5)
    with pytest.raises(ValueError, match="record of metrics_f1max"):
        engine.metrics_threshold(s, torch.zeros(3, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="record of metrics_range"):
        engine.metrics_threshold(s, 0.5, range_record=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="nothing to compute"):
        engine.metrics_threshold(s, 0.5, mask=False, totals=False)
    # NaN is never flagged, -0.0 >= +0.0 is
    x = torch.tensor([float("nan"), -0.0, 0.0, -1.0], device=dev)
    m, _, t = engine.metrics_threshold(x, 0.0)
    assert m.cpu().tolist() == [0, 1, 1, 0] and t.cpu().tolist() == [0, 2, 0, 2]


# -------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("kind", FC.CURVE_KINDS)
@pytest.mark.parametrize("n", [2, 4097, 27648, 2 ** 20 + 3])
def test_f1max_metrics_is_curve_metrics_plus_the_host_f1(dev, n, kind):
    import forward_utils as FU
    scores, labels = MD.inputs(n, kind)
    s, l = T(scores).to(dev), T(labels).to(dev)
    per_image = 2304 if n == 27648 else 0
    curve = engine.curve_metrics(s, l, per_image=per_image)
    both, f1 = engine.f1max_metrics(s, l, per_image=per_image)
    assert both[:4] == curve[:4] and both[5:] == curve[5:]                 # AUROC / AP bits, integers
    assert (both.image_max is None) == (per_image == 0)
    if per_image:
        assert torch.equal(both.image_max, curve.image_max)
    want = FU.f1max_eval(labels, MD.normalise(scores))
    assert f1 == want and f1_bits(f1.threshold) == f1_bits(want.threshold)
    assert np.float64(f1.f1).view(np.uint64) == np.float64(want.f1).view(np.uint64)
    assert FU.f1max_eval_device(l, T(MD.normalise(scores)).to(dev)) == want


def test_metrics_eval_device_rows_with_f1max_equal_the_host_rows(dev):
    import os
    import forward_utils as FU
    from conftest import GOLDEN
    from metrics_cases import derive_cases
    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    cases = derive_cases(*[g[f"base.{k}"] for k in ("masks", "labels", "preds", "scores")])
    for name, (pl, il, pp, ip, dom) in cases.items():
        hd, dd = {"masks": True}, {"masks": True}
        host = FU.metrics_eval(pl.copy(), il.copy(), pp.copy(), ip.copy(), name, dom, f1_max=True, details=hd)
        got = FU.metrics_eval_device(T(pl.astype(np.uint8)).to(dev), il.copy(), T(pp.copy()).to(dev), ip.copy(), name, dom,
                                     f1_max=True, details=dd)
        assert got == host and list(got)[-2:] == ["pixel F1-max", "image F1-max"], (name, got, host)
        assert dd["pixel threshold"] == hd["pixel threshold"] and dd["image threshold"] == hd["image threshold"]
        assert dd["masks"].is_cuda and np.array_equal(dd["masks"].cpu().numpy().reshape(-1), hd["masks"].reshape(-1))
        plain = FU.metrics_eval_device(T(pl.astype(np.uint8)).to(dev), il.copy(), T(pp.copy()).to(dev), ip.copy(), name, dom)
        assert plain == {k: v for k, v in host.items() if "F1" not in k}
    pl, il, pp, ip, dom = cases["industrial"]
    both = FU.metrics_eval_device(T(pl.astype(np.uint8)).to(dev), il.copy(), T(pp.copy()).to(dev), ip.copy(), "x", dom,
                                  fpr_limit=0.3, f1_max=True)
    assert both == FU.metrics_eval(pl.copy(), il.copy(), pp.copy(), ip.copy(), "x", dom, fpr_limit=0.3, f1_max=True)


def test_one_sort_serves_the_f1max_columns(dev, monkeypatch):
    """metrics_eval_device(f1_max=True) sorts as often as without the columns: once for the pixels, once for the images"""
    import os
    import forward_utils as FU
    from conftest import GOLDEN
    from metrics_cases import derive_cases
    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    pl, il, pp, ip, dom = derive_cases(*[g[f"base.{k}"] for k in ("masks", "labels", "preds", "scores")])["industrial"]
    calls = []
    real = engine.metrics_sort
    monkeypatch.setattr(engine, "metrics_sort", lambda *a, **k: calls.append(1) or real(*a, **k))
    for flag in (False, True):
        del calls[:]
        FU.metrics_eval_device(T(pl.astype(np.uint8)).to(dev), il.copy(), T(pp.copy()).to(dev), ip.copy(), "x", dom, f1_max=flag)
        assert len(calls) == 2, (flag, calls)


def test_eval_metrics_evaluate_gives_the_host_tables_and_the_masks(dev):
    import eval_last as EL
    import eval_metrics as EM
    import test_last as TL
    from test_gpu_metrics_device import StubModel, stub_class
    items, anchors = stub_class()
    model, anchors = StubModel(dev), anchors.to(dev)
    sets, emb = {"bottle": items, "grid": items[2:]}, {"bottle": anchors, "grid": anchors}
    args = (model, sets, emb, dev, 70, "MVTec")
    host, hd = EM.evaluate(*args, batch_size=4, use_iqm=True, f1_max=True, return_masks=True)
    got, dd = EM.evaluate(*args, batch_size=4, use_iqm=True, device_metrics=True, f1_max=True, return_masks=True)
    assert got == host and len(got) == 3 and all("pixel F1-max" in r and "image F1-max" in r for r in got)
    for col in ("pixel F1-max", "image F1-max"):
        assert got[-1][col] == float(np.mean([r[col] for r in got[:-1]])) and 0 < got[0][col] <= 100
    assert list(dd) == ["bottle", "grid"] == list(hd)
    for name in dd:
        assert dd[name]["pixel threshold"] == hd[name]["pixel threshold"]
        assert dd[name]["image threshold"] == hd[name]["image threshold"]
        m = dd[name]["masks"]
        assert m.is_cuda and m.dtype == torch.uint8 and m.shape == (len(sets[name]), 70, 70)
        assert np.array_equal(m.cpu().numpy(), hd[name]["masks"])
    # rows alone, both extra columns with AUPRO in front, and today's rows without the flag on either path
    assert EM.evaluate(*args, batch_size=4, use_iqm=True, device_metrics=True, f1_max=True) == got
    full = EM.evaluate(*args, batch_size=4, use_iqm=True, device_metrics=True, aupro_limit=0.3, f1_max=True)
    assert list(full[0])[-3:] == ["pixel AUPRO", "pixel F1-max", "image F1-max"]
    assert full == EM.evaluate(*args, batch_size=4, use_iqm=True, aupro_limit=0.3, f1_max=True)
    today = TL.evaluate(*args, batch_size=4, use_iqm=True)
    assert EM.evaluate(*args, batch_size=4, use_iqm=True, device_metrics=True) == today
    assert [{k: v for k, v in r.items() if "F1" not in k} for r in got] == today
    header = EL.format_table(got).split("\n")[0]
    assert header.endswith("pixel F1-max    image F1-max") and EL.format_table(today) == TL.format_table(today)


# ------------------------------------------------------------------------------------------------------ raises
def test_value_errors_come_before_the_sort(dev, monkeypatch):
    scores, labels = MD.inputs(27648, "plain")
    monkeypatch.setattr(engine, "metrics_sort", lambda *a, **k: pytest.fail("sorted before the checks"))
    cases = {"nan": (np.where(np.arange(scores.size) == 99, np.nan, scores).astype(np.float32), labels, "not finite"),
             "inf": (np.where(np.arange(scores.size) == 7, np.inf, scores).astype(np.float32), labels, "not finite"),
             "flat": (np.full_like(scores, 0.5), labels, "max == min"),
             "no positives": (scores, np.zeros_like(labels), "only one class"),
             "no negatives": (scores, np.ones_like(labels), "only one class")}
    for name, (s, l, msg) in cases.items():
        records = {}
        with pytest.raises(ValueError, match=msg):
            engine.f1max_metrics(T(s).to(dev), T(l).to(dev), records=records)
        assert records == {}, name
    import forward_utils as FU
    with pytest.raises(ValueError, match="only one class"):
        FU.f1max_eval_device(torch.zeros(64, dtype=torch.uint8, device=dev), torch.rand(64, device=dev))
    with pytest.raises(ValueError, match="not finite"):
        FU.f1max_eval_device(T(labels).to(dev), T(cases["nan"][0]).to(dev))
