"""The defect instances on the device (csrc/region_table.hip) against the host definition
(forward_utils.region_table_host / defects_eval; tests/defects_cases.py): the raw entry on guarded buffers and a workspace
full of garbage, twice; a capacity below the kept count; the peak bits against aaclip_metrics_normalise; the chain at the
F1-max threshold with the threshold read on the device; metrics_eval_device's rows and lists against metrics_eval's; the
.jsonl files of eval_defects.evaluate on either metrics path.

Every comparison is equality: the table holds integers and input floats only."""
import os

import numpy as np
import pytest
import torch

import defects_cases as DC
import pro_cases as PC
from aaclip_hip import _lib, engine

pytestmark = pytest.mark.gpu

T = torch.from_numpy
GUARD = 64                      # 32-bit words (bytes for the mask) in front of and behind every output buffer
SENTINEL = 0x5A5A5A5A
F = {k: c for c, k in enumerate(engine.REGION_ROW_FIELDS)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------- raw entry
def labelled(dev, mask, connectivity):
    region, area, record = engine.metrics_regions(T(np.array(mask)).to(dev), connectivity)
    return region, area, int(record.cpu()[0])


def table_raw(dev, region, area, case, capacity, want_kept_mask=True):
    """aaclip_region_table on buffers with guard words around rows, image_offsets and kept_mask, a record between two
    sentinels and a workspace full of garbage -> (rows [capacity, 12] uint32, offsets, record, kept_mask)"""
    lib = _lib.load()
    N, H, W = case.shape
    n = N * H * W
    _, raw, _, second = DC.inputs(case)
    scores = T(np.array(raw)).to(dev)
    other = None if second is None else T(np.array(second)).to(dev)
    rng = T(DC.range_record(raw)).to(dev) if case.normalise else None
    rows = torch.full((capacity * 12 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    offsets = torch.full((N + 1 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    kept = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    record = torch.full((4 + 2,), -1, dtype=torch.int64, device=dev)
    need = lib.aaclip_region_table_workspace_bytes(N, H, W)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    _lib.check(lib.aaclip_region_table(
        region.data_ptr(), area.data_ptr(), scores.data_ptr(), None if rng is None else rng.data_ptr(),
        None if other is None else other.data_ptr(), N, H, W, case.min_area, capacity,
        rows[GUARD:].data_ptr() if capacity else None, offsets[GUARD:].data_ptr(),
        kept[GUARD:].data_ptr() if want_kept_mask else None, record[1:].data_ptr(), ws.data_ptr(), need,
        torch.cuda.current_stream(dev).cuda_stream), "region_table")
    outs = []
    for b in (rows, offsets):
        h = u32(b)
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[-GUARD:] == SENTINEL), "guard words were written"
        outs.append(h[GUARD:-GUARD])
    k = kept.cpu().numpy()
    assert np.all(k[:GUARD] == 0x5A) and np.all(k[-GUARD:] == 0x5A), "guard bytes of the mask were written"
    if not want_kept_mask:
        assert np.all(k == 0x5A)
    rec = record.cpu().numpy()
    assert rec[0] == -1 and rec[5] == -1
    return outs[0].reshape(capacity, 12), outs[1].view(np.int32), tuple(int(v) for v in rec[1:5]), k[GUARD:-GUARD].reshape(case.shape)


def check_case(dev, case, labels):
    key = (case.shape, case.pattern, case.connectivity)
    if key not in labels:
        labels[key] = labelled(dev, PC.mask(case.pattern, case.shape), case.connectivity)
    region, area, regions = labels[key]
    want = DC.host_table(case)
    kept = want.record[0]
    assert regions == want.record[1], case
    rows, offsets, rec, mask = table_raw(dev, region, area, case, regions)
    assert rec == want.record, (case, rec, want.record)
    assert np.array_equal(rows[:kept], want.rows.view(np.uint32)), case
    assert np.all(rows[kept:] == SENTINEL), "rows behind the kept ones were written"
    assert np.array_equal(offsets, want.image_offsets) and np.array_equal(mask, want.kept_mask), case
    again = table_raw(dev, region, area, case, regions)
    assert np.array_equal(again[0], rows) and np.array_equal(again[1], offsets) and again[2] == rec
    assert np.array_equal(again[3], mask)
    if kept >= 2:             # a capacity below the kept count: the first rows, the true counts, nothing behind them
        cap = kept // 2
        rows, offsets, rec, _ = table_raw(dev, region, area, case, cap, want_kept_mask=False)
        assert rec == (kept, want.record[1], want.record[2], kept - cap), (case, rec)
        assert np.array_equal(rows, want.rows.view(np.uint32)[:cap]) and np.array_equal(offsets, want.image_offsets), case
    return kept


@pytest.mark.parametrize("shape", DC.SHAPES)
def test_raw_table_is_the_host_definition(dev, shape):
    labels, total = {}, 0
    for case in DC.cases(shape):
        total += check_case(dev, case, labels)
    assert total > 0
    case = DC.Case(shape, "full", 8, "constant", "full", 1, False)       # capacity 0 and no rows at all
    region, area, regions = labels[(shape, "full", 8)]
    rows, offsets, rec, _ = table_raw(dev, region, area, case, 0)
    assert rec == (shape[0], shape[0], shape[0], shape[0]) and list(offsets) == list(range(shape[0] + 1))


def test_raw_table_at_the_workload_size(dev):
    case = DC.BIG_CASE
    kept = check_case(dev, case, {})
    assert kept > 10
    full = DC.Case(DC.BIG, "full", 8, 4, "shifted", 1, True)              # one region per image: every pixel on one row
    assert check_case(dev, full, {}) == 2


# -------------------------------------------------------------------------------- normalisation and threshold
def test_peak_bits_are_metrics_normalises(dev):
    shape = (3, 37, 53)
    mask, raw = PC.mask("blobs", shape), DC.scores(shape, 0, "blobs")
    scores = T(np.array(raw)).to(dev)
    rng, _ = engine.metrics_range(scores)
    norm = u32(engine.metrics_normalise(scores, rng))
    region, area, record = engine.metrics_regions(T(np.array(mask)).to(dev))
    table = engine.region_table(region, area, scores, range_record=rng, regions=record)
    rows = u32(table.rows)
    assert rows.shape == (int(record.cpu()[0]), 12) and table.kept_mask is None
    for r in rows:
        assert r[F["peak"]] == norm[r[F["image"]], r[F["peak_y"]], r[F["peak_x"]]]
    plain = u32(engine.region_table(region, area, scores, regions=int(record.cpu()[0])).rows)
    assert np.array_equal(plain[:, F["peak"]], np.array([raw[r[0], r[F["peak_y"]], r[F["peak_x"]]] for r in plain]).view(np.uint32))
    lists = engine.region_table_host(table)
    assert [len(v) for v in lists] == list(np.diff(table.image_offsets.cpu().numpy()))
    assert lists[0][0]["peak"] == float(rows[0, F["peak"]].view(np.float32))
    with pytest.raises(RuntimeError, match="dropped"):
        engine.region_table(region, area, scores, regions=rows.shape[0] - 1)
    with pytest.raises(ValueError, match="min_area"):
        engine.region_table(region, area, scores, min_area=0)
    filtered = engine.region_table(region, area, scores, min_area=9, kept_mask=True, regions=record)
    want = rows[rows[:, F["area"]] >= 9]
    assert np.array_equal(u32(filtered.rows)[:, :8], want[:, :8]) and filtered.kept_mask.shape == region.shape


def host_chain(gt, raw, min_area):
    import forward_utils as FU
    norm = DC.normalised(raw)
    f1 = FU.f1max_eval(gt.reshape(-1), norm.reshape(-1))
    return f1, FU.defects_eval(gt, norm, f1.threshold, min_area)


@pytest.mark.parametrize("min_area", [1, 9])
@pytest.mark.parametrize("shape", DC.SHAPES[1:])
def test_defects_at_the_f1max_threshold_equal_the_host_chain(dev, shape, min_area, monkeypatch):
    """the threshold travels as the device record of metrics_f1max only: threshold_record, which uploads a number, is
    never called"""
    import forward_utils as FU
    gt, raw = PC.curve_case(shape, 16)
    f1, want = host_chain(gt, raw, min_area)
    records = {}
    scores, labels = T(np.array(raw)).to(dev), T(np.array(gt)).to(dev)
    got_f1 = engine.f1max_metrics(scores, labels, per_image=shape[1] * shape[2], records=records)[1]
    assert got_f1 == f1
    monkeypatch.setattr(engine, "threshold_record", lambda *a, **k: pytest.fail("the threshold was read on the host"))
    d = engine.defects_at_threshold(scores, records["f1max"], records["range"], gt_mask=labels, min_area=min_area)
    assert tuple(int(v) for v in d.record.cpu()) == want["record"]
    assert engine.region_table_host(d.predicted) == want["predicted"]
    assert engine.region_table_host(d.truth) == want["truth"]
    assert np.array_equal(d.mask.cpu().numpy(), want["kept mask"])
    got = FU.defects_eval_device(labels, scores, records["f1max"], min_area, range_record=records["range"])
    assert {k: got[k] for k in FU.DEFECT_COLS + ["record", "predicted", "truth"]} == \
           {k: want[k] for k in FU.DEFECT_COLS + ["record", "predicted", "truth"]}
    monkeypatch.undo()
    # a number as threshold, normalised scores, no ground truth
    norm = T(np.array(DC.normalised(raw))).to(dev)
    alone = engine.defects_at_threshold(norm, f1.threshold, None, min_area=min_area)
    assert alone.truth is None and engine.region_table_host(alone.predicted) == \
        [[dict(r, overlap=0) for r in v] for v in want["predicted"]]
    assert [int(v) for v in alone.record.cpu()] == [want["record"][0], 0, 0, 0, shape[0], want["record"][5]]


# ------------------------------------------------------------------------------------------- row-level equality
def assert_rows_and_lists_equal(dev, pl, il, pp, ip, name, dom, min_area):
    import forward_utils as FU
    hd, dd = {"masks": True}, {"masks": True}
    host = FU.metrics_eval(pl.copy(), il.copy(), pp.copy(), ip.copy(), name, dom, f1_max=True, details=hd, defects=min_area)
    got = FU.metrics_eval_device(T(pl.astype(np.uint8)).to(dev), il.copy(), T(pp.copy()).to(dev), ip.copy(), name, dom,
                                 f1_max=True, details=dd, defects=min_area)
    assert got == host and list(got)[-3:] == FU.DEFECT_COLS, (name, got, host)
    assert dd["defects"] == hd["defects"], name
    assert dd["kept masks"].is_cuda and np.array_equal(dd["kept masks"].cpu().numpy(), hd["kept masks"])
    assert np.array_equal(dd["masks"].cpu().numpy().reshape(-1), hd["masks"].reshape(-1))
    return got


def test_metrics_eval_device_rows_with_defects_equal_the_host_rows(dev):
    import forward_utils as FU
    from conftest import GOLDEN
    from metrics_cases import derive_cases
    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    cases = derive_cases(*[g[f"base.{k}"] for k in ("masks", "labels", "preds", "scores")])
    for name, (pl, il, pp, ip, dom) in cases.items():
        for min_area in (1, 4):
            got = assert_rows_and_lists_equal(dev, pl, il, pp, ip, name, dom, min_area)
        plain = FU.metrics_eval_device(T(pl.astype(np.uint8)).to(dev), il.copy(), T(pp.copy()).to(dev), ip.copy(), name, dom,
                                       f1_max=True)
        assert plain == {k: v for k, v in got.items() if k not in FU.DEFECT_COLS}


# ---------------------------------------------------------------------------------------------------- end to end
def test_eval_defects_end_to_end(dev, tmp_path):
    """The synthetic tree and reduced model of test_gpu_metrics_device.test_harness_with_device_metrics_returns_the_same_rows"""
    import dataset as D
    import eval_defects as ED
    import eval_last as EL
    import eval_metrics as EM
    import forward_utils as FU
    from synth_dataset import write_tree
    from test_gpu_metrics_device import build_tiny
    root = write_tree(str(tmp_path / "MVTec"))
    meta = str(tmp_path / "meta" / "MVTec" / "full-shot.jsonl")
    D.build_metadata(root, meta)
    cfg, clip, model = build_tiny(dev, "fp32")
    S = cfg.image_size
    classes = ["bottle", "grid"]
    with torch.no_grad():
        anchors = {c: FU.get_adapted_single_class_text_embedding(model, "MVTec", c, dev) for c in classes}
    sets = {c: D.BaseSingleClassDataset(root, meta, S, c) for c in classes}
    args = (model, sets, anchors, dev, S, "MVTec")
    how = dict(batch_size=4, use_iqm=False)
    out = {}
    for path in ("host", "device"):
        out[path] = ED.evaluate(*args, **how, device_metrics=path == "device", defects=2, return_masks=True,
                                save_path=str(tmp_path / path))
    (host, hd), (got, dd) = out["host"], out["device"]
    assert got == host and len(got) == 3 and list(got[0])[-3:] == FU.DEFECT_COLS
    for col in FU.DEFECT_COLS:
        assert got[-1][col] == float(np.mean([r[col] for r in got[:-1]]))
    files = {}
    for path in ("host", "device"):
        folder = tmp_path / path / "defects" / "MVTec"
        assert sorted(os.listdir(folder)) == ["bottle.jsonl", "grid.jsonl"]
        files[path] = {c: open(folder / f"{c}.jsonl", "rb").read() for c in classes}
    assert files["device"] == files["host"]
    import json
    for c in classes:
        lines = files["host"][c].decode().splitlines()
        assert len(lines) == len(sets[c]) and [json.loads(x)["file_name"] for x in lines] == hd[c]["file_names"]
        assert all(d["area"] >= 2 for x in lines for d in json.loads(x)["defects"])
        assert dd[c]["defects"] == hd[c]["defects"] and dd[c]["kept masks"].is_cuda
        assert np.array_equal(dd[c]["kept masks"].cpu().numpy(), hd[c]["kept masks"])
        assert np.array_equal(dd[c]["masks"].cpu().numpy(), hd[c]["masks"])                   # unfiltered, as before
        assert not np.any(hd[c]["kept masks"] & ~hd[c]["masks"])
    assert sum(len(json.loads(x)["defects"]) for c in classes for x in files["host"][c].decode().splitlines()) > 0
    # two synthetic classes, row by row: the maps of the harness through both metrics functions
    for c in classes:
        loader = torch.utils.data.DataLoader(sets[c], batch_size=4)
        with torch.no_grad():
            masks, labels, preds, preds_image, _ = EL.get_predictions(model, anchors[c], loader, dev, S, "MVTec", use_iqm=False)
        assert_rows_and_lists_equal(dev, (masks != 0).astype(np.uint8), labels, preds, preds_image, c, "Industrial", 3)
    # without defects: eval_metrics.evaluate's rows, on either path
    for device_metrics in (False, True):
        assert ED.evaluate(*args, **how, device_metrics=device_metrics, f1_max=True) == \
            EM.evaluate(*args, **how, device_metrics=device_metrics, f1_max=True)
    assert ED.evaluate(*args, **how, device_metrics=True) == EM.evaluate(*args, **how, device_metrics=True)
    assert [{k: v for k, v in r.items() if k not in FU.DEFECT_COLS} for r in got] == \
        EM.evaluate(*args, **how, device_metrics=True, f1_max=True)
