"""Exact AUROC / AP on the GPU (csrc/metrics.hip) against the numpy restatement of tests/metrics_device_cases.py, which
tests/test_metrics_device_cpu.py ties to sklearn and to the reference's own numbers.

Bars: sorted keys (and, where the label is a payload, the labels in their order), normalised scores, the range record
and {num, P, N, groups} are EQUAL to the restatement's.  AUROC = num / (2 P N) is the same integer and the same one
division: bound 1e-12.  AP is an fp64 sum of the same terms in another association (per-thread strided sums, a tree,
then the workgroups in index order, against numpy's pairwise sum): at most ~n ulp-sized steps of a sum that is at most
1: bound 1e-10 (the measured differences are in the parity record named below).  Two calls give the same bits.

No size here is the largest class (170 x 518^2): the digit table's three-level scan (segment sums, one workgroup,
apply) has more rows than segments from 2^20 + 3 keys on (513 rows, 171 segments of 3), and the tile scan of the curve
sums walks more than one tile sum per thread there (257 tiles, 256 threads); larger sizes only lengthen those loops.
tools/bench_metrics.py compares the whole result at that size with the host's.

The harness loops of eval_last.py are compared with test_last.py's on a stub model with the IQM branch on, and its
torch.distributed branch with the collective stubbed out (no second GPU process is started).

Every measured difference goes to PARITY_ERRORS under metrics_device.* (profiles/metrics_device_parity_errors.json)."""
import os

import numpy as np
import pytest
import torch

import metrics_device_cases as MD
from aaclip_hip import _lib, engine, synth
from conftest import GOLDEN, PARITY_ERRORS
from metrics_cases import KEYS, derive_cases

pytestmark = pytest.mark.gpu

GROUP = _lib.load().aaclip_metrics_sort_group_items()
SIZES = MD.sort_sizes(GROUP)
KINDS = ["plain", "coarse", "passthrough"]
T = torch.from_numpy


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------- range, normalise
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n, per_image", [(2, 1), (257, 0), (27648, 2304), (GROUP + 1, 0), (2 ** 20 + 3, 0),
                                          (6 * 70000, 70000)])
def test_range_and_normalise_are_numpys(dev, n, per_image, kind):
    scores, labels = MD.inputs(n, kind)
    rec, image_max = engine.metrics_range(T(scores).to(dev), T(labels).to(dev), per_image)
    r = engine.metrics_range_host(rec)
    assert r == {"min": float(scores.min()), "max": float(scores.max()), "nonfinite": 0, "positives": int(labels.sum())}
    if per_image:
        assert np.array_equal(image_max.cpu().numpy(), scores.reshape(-1, per_image).max(axis=1))
    else:
        assert image_max is None
    want = MD.normalise(scores)
    got = engine.metrics_normalise(T(scores).to(dev), rec).cpu().numpy()
    differing = int((bits(got) != bits(want)).sum())
    PARITY_ERRORS[f"metrics_device.normalise.{kind}.n{n}"] = {"differing_words": differing}
    assert differing == 0
    if kind == "passthrough":
        assert scores.max() == 1 and scores.min() < 0 and np.array_equal(bits(got), bits(scores))
        if n > 4:
            assert bits(got)[2] == 0x80000000 and bits(got)[3] == 0          # both zeros pass through as they are
    if per_image:
        engine.metrics_normalise(image_max, rec, out=image_max)
        assert np.array_equal(bits(image_max.cpu().numpy()), bits(want.reshape(-1, per_image).max(axis=1)))


def test_normalise_with_a_zero_minimum(dev):
    """(x - min) for x = +-0 and min = +-0 depends on the SIGN of the minimum.  With zeros of one sign the minimum is
    that zero for numpy and for the kernels alike: equal bits.  With both signs numpy does not define which zero
    min() returns, and neither does the device's fminf: the values are equal, and only words that are a zero (of
    either sign) on both sides may differ.  The keys fold -0.0 into +0.0, so the metrics do not see it."""
    rng = np.random.default_rng(5)
    base = np.abs(rng.normal(size=9001)).astype(np.float32) + np.float32(0.125)
    labels = (rng.random(base.size) < 0.3).astype(np.uint8)
    labels[:2] = 1, 0
    for name, zeros in {"plus": [0.0, 0.0, 0.0], "minus": [-0.0, -0.0, -0.0], "both": [-0.0, 0.0, -0.0]}.items():
        scores = base.copy()
        scores[[17, 4000, 9000]] = np.array(zeros, np.float32)
        assert scores.min() == 0 and scores.max() != 1
        rec, _ = engine.metrics_range(T(scores).to(dev))
        got = engine.metrics_normalise(T(scores).to(dev), rec).cpu().numpy()
        want = MD.normalise(scores)
        differ = bits(got) != bits(want)
        PARITY_ERRORS[f"metrics_device.normalise.zero_min.{name}"] = {"differing_words": int(differ.sum())}
        assert np.array_equal(got, want)
        if name == "both":
            assert np.all((got[differ] == 0) & (want[differ] == 0)) and differ.sum() <= 3
        else:
            assert not differ.any()
        m = engine.curve_metrics(T(scores).to(dev), T(labels).to(dev))
        w = MD.curve_metrics(scores, labels)
        assert (m.num, m.P, m.N, m.groups) == (w["num"], w["P"], w["N"], w["groups"])


def test_range_counts_non_finite_scores(dev):
    scores, labels = MD.inputs(27648, "plain")
    scores = scores.copy()
    scores[[5, 9000, 27647]] = [np.nan, np.inf, -np.inf]
    rec, _ = engine.metrics_range(T(scores).to(dev))
    r = engine.metrics_range_host(rec)
    finite = scores[np.isfinite(scores)]
    assert r == {"min": float(finite.min()), "max": float(finite.max()), "nonfinite": 3, "positives": 0}


# ------------------------------------------------------------------------------------------------------- sort
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_sorted_keys_are_the_restatements(dev, n, kind):
    scores, labels = MD.inputs(n, kind)
    want = MD.expected(n, kind)
    packed = want["packed"]
    assert packed == (kind != "passthrough")
    keys, labels_sorted, outside = engine.metrics_sort(T(want["normalised"]).to(dev), T(labels).to(dev), packed)
    wrong = int((u32(keys) != want["keys"]).sum())
    PARITY_ERRORS[f"metrics_device.sort.{kind}.n{n}"] = {"differing_keys": wrong}
    assert wrong == 0 and int(outside.cpu()) == 0
    if packed:
        assert labels_sorted is None
    else:                                     # equal keys keep their input order: the sort is stable
        assert np.array_equal(labels_sorted.cpu().numpy(), want["labels_sorted"])
    rec = engine.metrics_curve(keys, labels_sorted, packed).cpu()
    assert [int(v) for v in rec[:4]] == [want["num"], want["P"], want["N"], want["groups"]]


def test_packed_sort_counts_scores_outside_the_unit_interval(dev):
    scores = torch.tensor([0.5, -0.25, 1.0, 1.5, 0.0, -0.0], device=dev)
    _, _, outside = engine.metrics_sort(scores, torch.zeros(6, dtype=torch.uint8, device=dev), True)
    assert int(outside.cpu()) == 2


# ------------------------------------------------------------------------------------------------ curve sums
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_curve_metrics_against_the_restatement(dev, n, kind):
    scores, labels = MD.inputs(n, kind)
    want = MD.expected(n, kind)
    s, l = T(scores).to(dev), T(labels).to(dev)
    record = torch.zeros(engine.CURVE_RECORD_WORDS, dtype=torch.int64, device=dev)
    got = engine.curve_metrics(s, l, record=record)
    assert (got.num, got.P, got.N, got.groups) == (want["num"], want["P"], want["N"], want["groups"])
    assert got.image_max is None
    d_auc, d_ap = abs(got.auroc - want["auroc"]), abs(got.ap - want["ap"])
    print(n, kind, "auroc diff", d_auc, "ap diff", d_ap)
    PARITY_ERRORS[f"metrics_device.curve.{kind}.n{n}"] = {"auroc_abs": d_auc, "ap_abs": d_ap, "groups": got.groups}
    assert d_auc <= 1e-12 and d_ap <= 1e-10
    again = torch.zeros_like(record)
    second = engine.curve_metrics(s, l, record=again)
    assert torch.equal(record, again) and second.ap == got.ap and second.auroc == got.auroc       # the same bits


def test_tie_structure(dev):
    n = 20011
    rng = np.random.default_rng(11)
    labels = (rng.random(n) < 0.2).astype(np.uint8)
    eight = rng.integers(0, 8, size=n).astype(np.float32) + labels * (rng.random(n) < 0.5)
    eight = np.minimum(eight, 7).astype(np.float32)
    want = MD.curve_metrics(eight, labels)
    got = engine.curve_metrics(T(eight).to(dev), T(labels).to(dev))
    assert got.groups == want["groups"] == 8 and (got.num, got.P, got.N) == (want["num"], want["P"], want["N"])
    assert abs(got.auroc - want["auroc"]) <= 1e-12 and abs(got.ap - want["ap"]) <= 1e-10
    PARITY_ERRORS["metrics_device.ties.eight_values"] = {"auroc_abs": abs(got.auroc - want["auroc"]),
                                                         "ap_abs": abs(got.ap - want["ap"])}
    # all positives above all negatives, and the mirror image
    split = np.zeros(n, np.uint8)
    split[n - 4000:] = 1
    ramp = (np.arange(n) * 0.37).astype(np.float32)
    up = engine.curve_metrics(T(ramp).to(dev), T(split).to(dev))
    down = engine.curve_metrics(T(-ramp).to(dev), T(split).to(dev))
    assert up.auroc == 1.0 and down.auroc == 0.0 and down.num == 0 and up.groups == down.groups == n
    assert abs(up.ap - 1.0) <= 1e-10                      # 4000 terms of 1 / 4000
    want_down = MD.curve_metrics(-ramp, split)
    assert abs(down.ap - want_down["ap"]) <= 1e-10
    # one positive among n
    one = np.zeros(n, np.uint8)
    one[777] = 1
    got = engine.curve_metrics(T(ramp).to(dev), T(one).to(dev))
    assert (got.P, got.N, got.num) == (1, n - 1, 2 * 777) and got.auroc == 777 / (n - 1)
    assert abs(got.ap - 1 / (n - 777)) <= 1e-10


def test_unnormalised_scores_and_image_maxima(dev):
    """normalise=False (the image-level call of metrics_eval_device) and the normalised per-image maxima"""
    scores, labels = MD.inputs(27648, "plain")
    want = MD.curve_metrics(scores, labels, per_image=2304)
    got = engine.curve_metrics(T(scores).to(dev).view(12, 48, 48), T(labels).to(dev).view(12, 48, 48), per_image=2304)
    assert np.array_equal(bits(got.image_max.cpu().numpy()), bits(want["image_max"])) and got.num == want["num"]
    for raw in (scores, np.full(300, 0.25, np.float32)):          # negative scores as they are; equal scores: one group
        lab = labels[: raw.size]
        want = MD.curve_metrics(raw, lab, normalise_scores=False)
        got = engine.curve_metrics(T(raw).to(dev), T(lab).to(dev), normalise=False)
        assert (got.num, got.P, got.N, got.groups) == (want["num"], want["P"], want["N"], want["groups"])
        assert abs(got.ap - want["ap"]) <= 1e-10
    assert got.groups == 1 and got.auroc == 0.5


# --------------------------------------------------------------------------------------------- ValueError cases
def test_value_errors_come_before_the_sort(dev):
    scores, labels = MD.inputs(27648, "plain")
    sentinel = -0x0123456789ABCDEF
    cases = {"nan": (np.where(np.arange(scores.size) == 99, np.nan, scores).astype(np.float32), labels, "not finite"),
             "inf": (np.where(np.arange(scores.size) == 7, np.inf, scores).astype(np.float32), labels, "not finite"),
             "flat": (np.full_like(scores, 0.5), labels, "max == min"),
             "no positives": (scores, np.zeros_like(labels), "only one class"),
             "no negatives": (scores, np.ones_like(labels), "only one class")}
    for name, (s, l, msg) in cases.items():
        record = torch.full((engine.CURVE_RECORD_WORDS,), sentinel, dtype=torch.int64, device=dev)
        with pytest.raises(ValueError, match=msg):
            engine.curve_metrics(T(s).to(dev), T(l).to(dev), record=record)
        torch.cuda.synchronize()
        assert record.cpu().tolist() == [sentinel] * engine.CURVE_RECORD_WORDS, name   # `groups` and the rest untouched
    with pytest.raises(ValueError):
        engine.curve_metrics(torch.rand(8, device=dev).double(), torch.zeros(8, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        engine.curve_metrics(torch.rand(1, device=dev), torch.zeros(1, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        engine.curve_metrics(torch.rand(8, device=dev), torch.zeros(9, dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------------------------------- metrics_eval_device
def test_metrics_eval_device_equals_reference_golden(dev):
    import forward_utils as FU
    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    cases = derive_cases(*[g[f"base.{k}"] for k in ("masks", "labels", "preds", "scores")])
    assert len(cases) == 8
    for name, (pl, il, pp, ip, dom) in cases.items():
        r = FU.metrics_eval_device(T(pl.astype(np.uint8)).to(dev), il.copy(), T(pp.copy()).to(dev), ip.copy(), name, dom)
        got = np.array([float(r[k]) for k in KEYS])
        assert r["class name"] == name
        assert np.array_equal(got, g[f"{name}.result"]), (name, got, g[f"{name}.result"])
        host = FU.metrics_eval(pl.copy(), il.copy(), pp.copy(), ip.copy(), name, dom)
        assert r == host, (name, r, host)
    # float masks and device-resident per-image arrays are taken as well
    pl, il, pp, ip, dom = cases["industrial"]
    r = FU.metrics_eval_device(T(pl).to(dev)[:, None], T(il).to(dev), T(pp).to(dev), T(ip).to(dev), "industrial", dom)
    assert np.array_equal(np.array([float(r[k]) for k in KEYS]), g["industrial.result"])


# ------------------------------------------------------------------------------------------------- the harness
def build_tiny(dev, precision):
    from model.adapter import AdaptedCLIP
    from model.model import CLIP
    cfg = synth.tiny_cfg()
    sd = synth.synth_clip_state_dict(cfg, seed=7)
    clip = CLIP(cfg.embed_dim,
                dict(image_size=cfg.image_size, layers=cfg.vision.layers, width=cfg.vision.width,
                     patch_size=cfg.patch_size),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=cfg.text.width, heads=cfg.text.heads,
                     layers=cfg.text.layers), precision=precision)
    clip.load_state_dict(sd, strict=True)
    ia = synth.synth_image_adapter_state_dict(cfg, until=2, levels=2, seed=7)
    ta = synth.synth_text_adapter_state_dict(cfg, until=1, seed=7)
    model = AdaptedCLIP(clip, text_adapt_until=1, image_adapt_until=2, levels=[2, 3], relu=False)
    model.image_adapter.load_state_dict(ia, strict=True)
    model.text_adapter.load_state_dict(ta, strict=True)
    return cfg, clip.to(dev).eval(), model.to(dev).eval()


def test_harness_with_device_metrics_returns_the_same_rows(dev, tmp_path):
    """The synthetic tree and reduced model of test_gpu_parity.test_harness_end_to_end_vs_oracle"""
    import dataset as D
    import forward_utils as FU
    import eval_last as EL
    import test_last as TL
    from synth_dataset import write_tree
    root = write_tree(str(tmp_path / "MVTec"))
    meta = str(tmp_path / "meta" / "MVTec" / "full-shot.jsonl")
    D.build_metadata(root, meta)
    cfg, clip, model = build_tiny(dev, "fp32")
    S = cfg.image_size
    classes = ["bottle", "grid"]
    with torch.no_grad():
        anchors = {c: FU.get_adapted_single_class_text_embedding(model, "MVTec", c, dev) for c in classes}
    host = {c: D.BaseSingleClassDataset(root, meta, S, c) for c in classes}
    rows_host = TL.evaluate(model, host, anchors, dev, S, "MVTec", batch_size=4, use_iqm=False)
    rows_dev = EL.evaluate(model, host, anchors, dev, S, "MVTec", batch_size=4, use_iqm=False, device_metrics=True)
    assert rows_dev == rows_host and len(rows_dev) == 3 and rows_dev[-1]["class name"] == "Average"
    with torch.no_grad():
        loader = torch.utils.data.DataLoader(host["bottle"], batch_size=4)
        on = EL.get_predictions(model, anchors["bottle"], loader, dev, S, "MVTec", use_iqm=False, on_device=True)
        off = TL.get_predictions(model, anchors["bottle"], loader, dev, S, "MVTec", use_iqm=False)
    assert on[0].is_cuda and on[0].dtype == torch.uint8 and on[2].is_cuda and on[3].is_cuda and not torch.is_tensor(on[1])
    assert np.array_equal(on[0].cpu().numpy(), off[0]) and np.array_equal(on[1], off[1]) and on[4] == off[4]
    assert np.array_equal(on[2].cpu().numpy(), off[2]) and np.array_equal(on[3].cpu().numpy(), off[3])


# ------------------------------------------------ the copied loops of eval_last against test_last's, IQM branch on
class StubModel:
    """What get_predictions needs of AdaptedCLIP: (two levels of unit patch rows [B, 25, 768], det row [B, 768], IQM
    output with last_hidden_state [B, 2, 768] when text_embeddings is given), a fixed function of the image"""

    def __init__(self, dev):
        g = torch.Generator().manual_seed(21)
        self.rows = [torch.randn(25, 768, generator=g).to(dev) for _ in range(2)]
        self.tilt = [torch.randn(25, 768, generator=g).to(dev) for _ in range(2)]
        self.det, self.hidden = torch.randn(768, generator=g).to(dev), torch.randn(2, 768, generator=g).to(dev)

    def __call__(self, image, text_embeddings=None):
        import types
        a = image.mean(dim=(1, 2, 3))[:, None, None]
        b = image[:, :, ::7, ::7].reshape(image.shape[0], -1)[:, :25, None]          # a little of every image's content
        seg = [torch.nn.functional.normalize(r[None] + a * t[None] + b, dim=-1).contiguous()
               for r, t in zip(self.rows, self.tilt)]
        det = torch.nn.functional.normalize(self.det[None] + a[:, 0], dim=-1)
        iqm = None
        if text_embeddings is not None:
            assert text_embeddings.shape == (image.shape[0], 768, 2)
            iqm = types.SimpleNamespace(last_hidden_state=(self.hidden[None] * (1 + a)).contiguous())
        return seg, det, iqm


def stub_class(n=10, S=70):
    g = torch.Generator().manual_seed(4)
    items = []
    for i in range(n):
        mask = torch.zeros(1, S, S)
        if i % 2:
            mask[0, 5 + i:20 + i, 10:30] = 1
        items.append({"image": torch.randn(3, S, S, generator=g) + mask, "mask": mask, "label": i % 2,
                      "file_name": f"f{i}.png", "class_name": "bottle"})
    anchors = torch.nn.functional.normalize(torch.randn(768, 2, generator=g), dim=0)
    return items, anchors


def test_eval_last_loops_equal_test_lasts_with_the_iqm_branch(dev):
    import eval_last as EL
    import test_last as TL
    items, anchors = stub_class()
    model, anchors = StubModel(dev), anchors.to(dev)
    loader = torch.utils.data.DataLoader(items, batch_size=4)
    with torch.no_grad():
        on = EL.get_predictions(model, anchors, loader, dev, 70, "MVTec", use_iqm=True, on_device=True)
        off = TL.get_predictions(model, anchors, loader, dev, 70, "MVTec", use_iqm=True)
        text_only = TL.get_predictions(model, anchors, loader, dev, 70, "MVTec", use_iqm=False)
    assert np.array_equal(on[0].cpu().numpy(), off[0]) and np.array_equal(on[1], off[1]) and on[4] == off[4]
    assert np.array_equal(on[2].cpu().numpy(), off[2]) and np.array_equal(on[3].cpu().numpy(), off[3])
    assert not np.array_equal(off[2], text_only[2])                      # the IQM term is in the maps
    sets, emb = {"bottle": items}, {"bottle": anchors}
    rows = EL.evaluate(model, sets, emb, dev, 70, "MVTec", batch_size=4, use_iqm=True, device_metrics=True)
    assert rows == TL.evaluate(model, sets, emb, dev, 70, "MVTec", batch_size=4, use_iqm=True)
    assert rows == EL.evaluate(model, sets, emb, dev, 70, "MVTec", batch_size=4, use_iqm=True)      # flag off: test_last's


def test_evaluate_device_metrics_under_a_process_group(dev, monkeypatch):
    """The torch.distributed branch of evaluate(device_metrics=True) with the collective stubbed out: rank 0 of 2
    holds a whole class (host arrays in, gathered host arrays uploaded once, image scores left on the host), then an
    empty shard whose rows come from the gather alone."""
    import torch.distributed as dist
    import eval_last as EL
    import test_last as TL
    items, anchors = stub_class()
    model, anchors = StubModel(dev), anchors.to(dev)
    sets, emb = {"bottle": items}, {"bottle": anchors}
    want = TL.evaluate(model, sets, emb, dev, 70, "MVTec", batch_size=4, use_iqm=True)
    for name, value in {"is_initialized": True, "get_world_size": 2, "get_rank": 0, "get_backend": "gloo"}.items():
        monkeypatch.setattr(dist, name, lambda *a, _v=value, **k: _v)
    seen = []

    def gather(arrays, total, device=None, group=None):
        assert device is None and total == len(items) and all(isinstance(a, np.ndarray) for a in arrays)
        assert [a.dtype for a in arrays] == [np.uint8, np.int64, np.float32, np.float32]
        if arrays[0].shape[0]:
            seen.append(tuple(a.copy() for a in arrays))
        else:
            assert [a.shape for a in arrays] == [(0, 1, 70, 70), (0,), (0, 70, 70), (0,)]
        return seen[0]

    monkeypatch.setattr(EL, "gather_predictions", gather)
    monkeypatch.setattr(EL, "shard_range", lambda total, rank, world: (0, total))
    assert EL.evaluate(model, sets, emb, dev, 70, "MVTec", batch_size=4, use_iqm=True, device_metrics=True) == want
    monkeypatch.setattr(EL, "shard_range", lambda total, rank, world: (0, 0))
    assert EL.evaluate(model, sets, emb, dev, 70, "MVTec", batch_size=4, use_iqm=True, device_metrics=True) == want
    assert len(seen) == 1
