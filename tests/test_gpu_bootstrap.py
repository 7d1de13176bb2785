"""Bootstrap of AUROC / AP over images on the GPU (csrc/bootstrap.hip) against the numpy restatement of
tests/bootstrap_cases.py, which tests/test_bootstrap_cpu.py ties to sklearn on the literally repeated images.

Bars: num, P, N and the valid mask are EQUAL to the restatement's; AP is an fp64 sum of the same terms in another
association (the groups inside a tile in index order, then the tiles in index order, against one loop over the groups):
bound 1e-10, the bar of tests/test_gpu_metrics_device.py for the same quantity.  Two calls give the same bytes.

Shapes: n = 23 x 535 = 12 305 = three tiles of 4096 + 17 (no multiple of 64), 12 normal and 11 anomalous images; scores
that are all distinct, on 40 levels, and with a constant run of 9 000 sorted elements across two tile boundaries (a tile
without a start); R = 1, 64, 65, 200 (a partial replicate block, a whole one, a block + 1, a partial last block); rows
drawn with seed 0 and hand-made rows (all ones, one image 23 times, every anomalous image 0, every normal image 0).
Larger classes only lengthen the loops over the tiles; tools/bench_bootstrap.py compares the largest class."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bootstrap_cases as BC
from aaclip_hip import _lib, engine

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def host(records):
    h = engine.bootstrap_records_host(records)
    return {"num": h.num, "P": h.P, "N": h.N, "ap": h.ap, "valid": h.valid}


def assert_records(got, want, what):
    for k in ("num", "P", "N", "valid"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    worst = float(np.abs(got["ap"] - want["ap"]).max())
    print(f"{what}: worst |d ap| {worst:.3g} over {want['ap'].size} replicates, {int((~want['valid']).sum())} invalid")
    assert worst <= 1e-10, (what, worst)


@pytest.fixture(scope="module")
def sorted_class(dev):
    """kind -> (keys, payload) on the device from ONE engine.metrics_sort_pairs, checked against the restatement's sort"""
    out = {}
    for kind in BC.KINDS:
        scores, labels, _ = BC.pixel_class(kind)
        n = scores.size
        payload = ((np.arange(n) // BC.PER_IMAGE) << 1 | labels.reshape(-1)).astype(np.int32)
        keys, carried = engine.metrics_sort_pairs(T(scores.reshape(-1)).to(dev), T(payload).to(dev))
        want_keys, want_payload, _ = BC.expected(kind)
        assert np.array_equal(keys.cpu().numpy().view(np.uint32), want_keys)
        assert np.array_equal(carried.cpu().numpy(), want_payload)
        out[kind] = (keys, carried)
    return out


@pytest.mark.parametrize("R", BC.REPLICATES)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_records_are_the_restatements(dev, sorted_class, kind, R):
    keys, payload = sorted_class[kind]
    counts, want = BC.expected(kind)[2][R]
    assert counts.shape == (R, BC.IMAGES)
    records = engine.bootstrap_curves(keys, payload, counts)
    assert records.shape == (R, engine.BOOTSTRAP_RECORD_WORDS) and records.dtype == torch.int64
    assert_records(host(records), want, f"{kind} R={R}")
    again = engine.bootstrap_curves(keys, payload, T(counts).to(dev))          # counts on the device are taken as well
    assert torch.equal(records, again)
    if R >= 4:                                                                  # the hand-made rows close the matrix
        assert want["valid"][:R - 4].all() and want["valid"][R - 4:].tolist() == [True, True, False, True]


@pytest.mark.parametrize("kind", BC.KINDS)
def test_counts_of_one_are_the_unweighted_curve(dev, kind):
    scores, labels, _ = BC.pixel_class(kind)
    s, l = T(scores).to(dev), T(labels).to(dev)
    curve = engine.curve_metrics(s, l, normalise=False)
    boot = engine.bootstrap_metrics(s, l, BC.PER_IMAGE, np.ones((1, BC.IMAGES), np.uint8), normalise=False)
    assert (int(boot.num[0]), int(boot.P[0]), int(boot.N[0])) == (curve.num, curve.P, curve.N)
    assert abs(boot.auroc[0] - curve.auroc) <= 1e-12 and abs(boot.ap[0] - curve.ap) <= 1e-10
    # normalised like curve_metrics: the range of the whole class, once
    curve = engine.curve_metrics(s * 3 - 1, l)
    boot = engine.bootstrap_metrics(s * 3 - 1, l, BC.PER_IMAGE, np.ones((1, BC.IMAGES), np.uint8))
    assert (int(boot.num[0]), int(boot.P[0]), int(boot.N[0])) == (curve.num, curve.P, curve.N)


def test_image_level_form(dev):
    """per_image = 1: n = images = 23; there both one-label hand rows are invalid.  Then n = 2 and n = 1."""
    import forward_utils as FU
    scores, _, image_label = BC.pixel_class("coarse")
    image_scores = scores.max(axis=1).astype(np.float32)
    image_scores[3] = image_scores[15]                                          # a tie across the labels
    counts = np.concatenate([FU.bootstrap_counts(BC.IMAGES, 61, 0, 0), BC.hand_counts()])
    keys, payload = BC.sorted_pairs(image_scores, image_label, 1)
    want = BC.records(keys, payload, counts)
    assert want["valid"][-4:].tolist() == [True, False, False, False] and want["valid"][:61].all()
    got = engine.bootstrap_metrics(T(image_scores).to(dev), T(image_label).to(dev), 1, counts, normalise=False)
    assert_records({"num": got.num, "P": got.P, "N": got.N, "ap": got.ap, "valid": got.valid}, want, "image level")
    assert np.array_equal(got.auroc[~got.valid], np.zeros(3))
    # n = 2
    two, lab = np.array([0.25, 0.75], np.float32), np.array([0, 1], np.uint8)
    counts2 = np.array([[1, 1], [2, 0], [0, 2], [3, 5]], np.uint8)
    want = BC.records(*BC.sorted_pairs(two, lab, 1), counts2)
    got = engine.bootstrap_metrics(T(two).to(dev), T(lab).to(dev), 1, counts2, normalise=False)
    assert_records({"num": got.num, "P": got.P, "N": got.N, "ap": got.ap, "valid": got.valid}, want, "n = 2")
    assert got.valid.tolist() == [True, False, False, True] and got.auroc[0] == 1.0 and got.auroc[3] == 1.0
    # n = 1: a single element is one label only
    rec = engine.bootstrap_curves(torch.tensor([5], dtype=torch.int32, device=dev),
                                  torch.tensor([1], dtype=torch.int32, device=dev), np.array([[1], [4]], np.uint8))
    h = host(rec)
    assert h["valid"].tolist() == [False, False] and h["P"].tolist() == [1, 4] and h["N"].tolist() == [0, 0]
    assert h["num"].tolist() == [0, 0] and h["ap"].tolist() == [0.0, 0.0]


def test_the_largest_image_count_and_beyond(dev):
    images = engine.bootstrap_max_images()
    assert images == _lib.load().aaclip_bootstrap_max_images() >= 1024
    rng = np.random.default_rng(5)
    image_label = (np.arange(images) % 3 == 0).astype(np.uint8)
    labels = np.repeat(image_label[:, None], 3, axis=1)
    labels[:, 2] = 0
    scores = (np.round(rng.normal(size=(images, 3)) * 8 + 3 * labels) / 64 + 0.5).astype(np.float32)
    counts = rng.integers(0, 4, size=(66, images)).astype(np.uint8)
    counts[1] = 0
    counts[1, images - 1], counts[1, images - 2], counts[1, 0] = 255, 7, 1     # the table's last rows, the largest count
    want = BC.records(*BC.sorted_pairs(scores, labels, 3), counts)
    got = engine.bootstrap_metrics(T(scores).to(dev), T(labels).to(dev), 3, counts, normalise=False)
    assert_records({"num": got.num, "P": got.P, "N": got.N, "ap": got.ap, "valid": got.valid}, want, f"{images} images")
    more = images + 1
    with pytest.raises(ValueError, match="images"):
        engine.bootstrap_metrics(torch.rand(more * 2, device=dev), (torch.arange(more * 2, device=dev) % 2).to(torch.uint8),
                                 2, np.ones((2, more), np.uint8), normalise=False)
    lib = _lib.load()
    assert lib.aaclip_bootstrap_workspace_bytes(more * 2, more, 2) == 0
    keys = torch.zeros(more * 2, dtype=torch.int32, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    rec = torch.zeros(2, 4, dtype=torch.int64, device=dev)
    cnt = torch.ones(2, more, dtype=torch.uint8, device=dev)
    plan = _lib.BootstrapPlan(n=more * 2, images=more, replicates=2, stream=None)
    assert lib.aaclip_bootstrap_curves(ctypes.byref(plan), keys.data_ptr(), keys.data_ptr(), cnt.data_ptr(), rec.data_ptr(),
                                       ws.data_ptr(), ws.numel()) == -1
    assert lib.aaclip_last_error().decode().startswith("bootstrap_curves: images must be")


def test_refusals_come_before_any_launch(dev):
    keys = torch.arange(8, dtype=torch.int32, device=dev)
    payload = (torch.arange(8, dtype=torch.int32, device=dev) // 2 << 1) | (torch.arange(8, device=dev) % 2).int()
    ones = np.ones((2, 4), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.bootstrap_curves(keys.cpu(), payload, ones)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.bootstrap_metrics(torch.rand(8), torch.zeros(8, dtype=torch.uint8), 2, ones)
    with pytest.raises(ValueError, match="0 .. 255"):
        engine.bootstrap_curves(keys, payload, np.full((2, 4), 256))
    with pytest.raises(ValueError, match="outside"):
        engine.bootstrap_curves(keys, payload, np.ones((2, 3), np.uint8))
    with pytest.raises(ValueError, match="unpacked"):
        engine.bootstrap_curves(keys, payload, ones, packed=True)
    big = torch.zeros(2 ** 23 + 2 ** 16, dtype=torch.int32, device=dev)            # 255 * (2^23 + 2^16) passes 2^31
    with pytest.raises(ValueError, match="2\\^31"):
        engine.bootstrap_curves(big, big, np.full((1, 1), 255, np.uint8))
    with pytest.raises(ValueError, match="only one class"):
        engine.bootstrap_metrics(torch.rand(8, device=dev), torch.zeros(8, dtype=torch.uint8, device=dev), 2, ones)


# ------------------------------------------------------------------------------------------- the stream contract
def test_entry_on_side_stream_capture_and_replay(dev):
    """The stream travels in the plan.  The case is built with tests/stream_cases.Case and run by the loop of
    tests/test_gpu_streams.py: the default stream with two value sets, a side stream, a capture that must execute nothing,
    and two replays with new data over poisoned scratch -- the same bytes every time.  70 replicates (a whole block of
    64 and a partial one) over 8 images; the keys are sorted draws from 300 values."""
    import stream_cases as SC
    from aaclip_hip import synth
    from test_gpu_streams import run_stream_case
    lib, c = _lib.load(), SC.Case(dev)
    n, images, R = 1000, 8, 70
    keys = c.inp(*[torch.sort(torch.randint(0, 300, (n,), generator=synth._gen("bc.keys", s)))[0].to(torch.uint32)
                   for s in SC.SEEDS])
    payload = c.ints("bc.payload", (n,), 0, 2 * images, torch.uint32)
    counts = c.ints("bc.counts", (R, images), 0, 4, torch.uint8)
    rec = c.out((R, 32), torch.uint8)
    ws = c.ws(lib.aaclip_bootstrap_workspace_bytes(n, images, R))

    def call(stream):
        plan = _lib.BootstrapPlan(n=n, images=images, replicates=R, stream=stream)
        return lib.aaclip_bootstrap_curves(ctypes.byref(plan), keys.data_ptr(), payload.data_ptr(), counts.data_ptr(),
                                           rec.data_ptr(), ws.data_ptr(), ws.numel())
    c.call = call
    run_stream_case(c, dev, "aaclip_bootstrap_curves[r70]")


# ------------------------------------------------------------------------------------------------- the harness
def test_metrics_eval_device_equals_metrics_eval(dev):
    import forward_utils as FU
    rng = np.random.default_rng(11)
    images, side = 14, 12
    il = (np.arange(images) % 2).astype(np.int64)
    pl = np.zeros((images, 1, side, side), np.float32)
    pl[il == 1, 0, 2:6, 3:9] = 1
    pp = (np.round((rng.normal(size=(images, side, side)) + 1.5 * pl[:, 0]) * 8) / 8).astype(np.float32)
    ip = (rng.normal(size=images) + il).astype(np.float32)
    for stratified, domain in ((False, "Industrial"), (True, "Medical")):
        boot = dict(R=150, seed=3, level=0.9, stratified=stratified, class_index=2)
        dh, dd = {}, {}
        want = FU.metrics_eval(pl.copy(), il.copy(), pp.copy(), ip.copy(), "stub", domain, details=dh, bootstrap=dict(boot))
        got = FU.metrics_eval_device(T(pl).to(dev), il.copy(), T(pp).to(dev), ip.copy(), "stub", domain, details=dd,
                                     bootstrap=dict(boot))
        assert got == want, (got, want)
        assert set(FU.bootstrap_interval_cols()) <= set(got)
        for col in FU.BOOTSTRAP_COLS:
            assert got[col + " lo"] <= got[col] <= got[col + " hi"], (col, got)
            assert np.abs(dd["bootstrap"][col] - dh["bootstrap"][col]).max() <= 1e-10
        assert np.array_equal(dd["bootstrap"]["valid"], dh["bootstrap"]["valid"])
        plain = FU.metrics_eval_device(T(pl).to(dev), il.copy(), T(pp).to(dev), ip.copy(), "stub", domain)
        assert plain == {k: v for k, v in got.items() if k in plain} and not set(FU.bootstrap_interval_cols()) & set(plain)
    # a one-label class: the image columns and their intervals are the fixed 0
    zero = np.zeros_like(il)
    one = FU.metrics_eval_device(T(pl).to(dev), zero, T(pp).to(dev), ip.copy(), "stub", "Industrial",
                                 bootstrap=dict(R=20, stratified=True))
    assert [one[c] for c in ("image AUC", "image AUC lo", "image AUC hi", "image AP lo", "image AP hi")] == [0] * 5
    assert one["pixel AUC lo"] <= one["pixel AUC"] <= one["pixel AUC hi"]


@pytest.fixture(scope="module")
def harness(dev, tmp_path_factory):
    """the tiny harness of test_gpu_png: the synthetic tree and the reduced fp32 model"""
    import dataset as D
    import forward_utils as FU
    from synth_dataset import write_tree
    from test_gpu_metrics_device import build_tiny
    tmp = tmp_path_factory.mktemp("bootstrap")
    root = write_tree(str(tmp / "MVTec"))
    meta = str(tmp / "meta" / "MVTec" / "full-shot.jsonl")
    D.build_metadata(root, meta)
    cfg, clip, model = build_tiny(dev, "fp32")
    classes = ["bottle", "grid"]
    with torch.no_grad():
        anchors = {c: FU.get_adapted_single_class_text_embedding(model, "MVTec", c, dev) for c in classes}
    sets = {c: D.BaseSingleClassDataset(root, meta, cfg.image_size, c) for c in classes}
    return dict(model=model, S=cfg.image_size, classes=classes, anchors=anchors, sets=sets, tmp=tmp)


def test_end_to_end(dev, harness):
    import eval_bootstrap as EB
    import eval_png as EP
    import forward_utils as FU
    h = harness
    where = (h["model"], h["sets"], h["anchors"], dev, h["S"], "MVTec")
    how = dict(batch_size=8, use_iqm=False, device_metrics=True)
    want = EP.evaluate(*where, **how)
    assert EB.evaluate(*where, **how, bootstrap=None) == want                    # without the keyword: eval_png's rows
    save, written = str(h["tmp"] / "run"), []
    boot = EB.bootstrap_settings(80, seed=1, level=0.9, stratified=True)
    rows = EB.evaluate(*where, **how, save_path=save, bootstrap=boot, bootstrap_written=written)
    for got, ref in zip(rows, want):
        assert {k: got[k] for k in ref} == ref                                  # the point estimates are untouched
        for col in FU.BOOTSTRAP_COLS:
            assert got[col + " lo"] <= got[col] + 1e-9 and got[col] <= got[col + " hi"] + 1e-9, (col, got)
    host_rows = EB.evaluate(*where, batch_size=8, use_iqm=False, device_metrics=False, bootstrap=boot)
    for got, ref in zip(rows, host_rows):
        for col in FU.bootstrap_interval_cols():
            assert abs(got[col] - ref[col]) <= 1e-6, (col, got, ref)
    assert [os.path.basename(p) for p in written] == ["bottle.npz", "grid.npz", "Average.npz"]
    average = np.load(written[-1])
    parts = [np.load(p) for p in written[:2]]
    assert int(average["R"]) == 80 and int(average["seed"]) == 1 and int(average["images"]) == 12
    assert np.array_equal(average["valid"], parts[0]["valid"] & parts[1]["valid"])
    assert np.allclose(average["pixel_auc"], (parts[0]["pixel_auc"] + parts[1]["pixel_auc"]) / 2, atol=1e-15)
    lo, hi = FU.bootstrap_interval(average["pixel_auc"], average["valid"], 0.9)
    assert rows[-1]["pixel AUC lo"] == lo * 100 and rows[-1]["pixel AUC hi"] == hi * 100
    assert "pixel AUC lo" in EB.ED.format_table(rows).split("\n")[0]
