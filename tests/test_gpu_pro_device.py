"""The per-region overlap (AUPRO) on the device (csrc/regions.hip, the pair sort of csrc/metrics.hip) against the host
definition forward_utils.pro_eval and scipy's labelling (tests/pro_cases.py).

Regions, areas, records, sorted keys and carried values are compared for EQUALITY.  AUPRO: both sides form the same
fp64 terms (1 / area, each <= 1) in different orders, n * 2^-53 <= 1.2e-10 at n <= 2^20 terms; the bar is 8 x that,
1e-9 absolute.  regions / normal / groups are equal integers."""
import numpy as np
import pytest
import torch

import metrics_device_cases as MD
import pro_cases as PC
from aaclip_hip import _lib, engine

pytestmark = pytest.mark.gpu

GROUP = _lib.load().aaclip_metrics_sort_group_items()
T = torch.from_numpy
GUARD = 64                      # words in front of and behind every output buffer
SENTINEL = 0x5A5A5A5A
BOUND = 1e-9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------- regions
def regions_raw(dev, m, connectivity):
    """aaclip_metrics_regions on buffers with guard words around both outputs and a workspace full of garbage"""
    lib = _lib.load()
    N, H, W = m.shape
    n = m.size
    mask = T(np.array(m)).to(dev)
    bufs = [torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2)]
    record = torch.full((3 + 2,), -1, dtype=torch.int64, device=dev)
    need = lib.aaclip_metrics_regions_workspace_bytes(N, H, W)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    _lib.check(lib.aaclip_metrics_regions(mask.data_ptr(), N, H, W, connectivity, bufs[0][GUARD:].data_ptr(),
                                          bufs[1][GUARD:].data_ptr(), record[1:].data_ptr(), ws.data_ptr(), need,
                                          torch.cuda.current_stream(dev).cuda_stream), "metrics_regions")
    outs = []
    for b in bufs:
        h = u32(b)
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[-GUARD:] == SENTINEL), "guard words were written"
        outs.append(h[GUARD:-GUARD].reshape(m.shape))
    rec = record.cpu().numpy()
    assert rec[0] == -1 and rec[4] == -1
    return outs[0], outs[1], tuple(int(v) for v in rec[1:4])


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("shape", PC.SHAPES)
def test_regions_are_scipys(dev, shape, connectivity):
    for pattern in PC.PATTERNS:
        m = PC.mask(pattern, shape)
        want_region, want_area, want_rec = PC.canonical(m, connectivity)
        region, area, rec = regions_raw(dev, m, connectivity)
        assert rec == want_rec, (pattern, rec, want_rec)
        assert np.array_equal(region, want_region), pattern
        assert np.array_equal(area, want_area), pattern
        again = regions_raw(dev, m, connectivity)
        assert np.array_equal(again[0], region) and np.array_equal(again[1], area) and again[2] == rec
    # the Python wrapper: the same arrays in the mask's shape, [N, 1, H, W] included
    m = PC.mask("blobs", shape)
    want_region, want_area, want_rec = PC.canonical(m, connectivity)
    region, area, rec = engine.metrics_regions(T(np.array(m[:, None])).to(dev), connectivity)
    assert region.shape == (shape[0], 1) + shape[1:] and region.dtype == torch.int32
    assert np.array_equal(u32(region)[:, 0], want_region) and np.array_equal(u32(area)[:, 0], want_area)
    assert tuple(int(v) for v in rec.cpu()) == want_rec


def test_regions_refusals(dev):
    mask = torch.zeros(2, 8, 8, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="connectivity"):
        engine.metrics_regions(mask, connectivity=6)
    with pytest.raises(ValueError, match="uint8"):
        engine.metrics_regions(mask.float())
    with pytest.raises(ValueError, match="pixels"):
        engine.metrics_regions(mask[:1, :1, :1])


# -------------------------------------------------------------------------------------------------- pair sort
@pytest.mark.parametrize("n", [2, 63, 64, 65, 2047, 2048, 2049, GROUP + 1, 2 ** 20 + 3])
def test_pair_sort_is_numpys_stable_argsort(dev, n):
    rng = np.random.default_rng(n)
    scores = (np.round(rng.random(n) * 15) / 15 * 4 - 2).astype(np.float32)       # 16 levels in [-2, 2]
    if n > 8:
        scores[[1, 5]] = -0.0, 0.0                                                # one key for both zeros
    values = np.arange(n, dtype=np.int32)                                         # the index: stability is visible
    keys, carried = engine.metrics_sort_pairs(T(scores).to(dev), T(values).to(dev))
    want_keys = MD.make_keys(scores, np.zeros(n, np.uint8), packed=False)
    order = np.argsort(want_keys, kind="stable")
    assert np.array_equal(u32(keys), want_keys[order])
    assert np.array_equal(carried.cpu().numpy(), values[order])
    assert np.array_equal(scores[order], np.sort(scores))                         # the key order is the float order
    # a value that uses all 32 bits, and equal bits from a second call
    wide = (values.astype(np.int64) * 2654435761 % 2 ** 32).astype(np.uint32).view(np.int32)
    keys2, carried2 = engine.metrics_sort_pairs(T(scores).to(dev), T(wide).to(dev))
    assert torch.equal(keys2, keys) and np.array_equal(carried2.cpu().numpy(), wide[order])


# ---------------------------------------------------------------------------------------------- curve, pro_metrics
def check(dev, m, s, limit, connectivity=8, bound=BOUND):
    import forward_utils as FU
    want = FU.pro_eval_record(m, s, fpr_limit=limit, connectivity=connectivity)
    got = engine.pro_metrics(T(np.array(s)).to(dev), T(np.array(m)).to(dev), fpr_limit=limit,
                             connectivity=connectivity)
    print(m.shape, limit, connectivity, "aupro", got.aupro, "host", want[0], "diff", abs(got.aupro - want[0]))
    assert (got.regions, got.normal, got.groups) == want[1:]
    assert abs(got.aupro - want[0]) <= bound
    return got


@pytest.mark.parametrize("levels", PC.LEVELS)
@pytest.mark.parametrize("shape", PC.SHAPES)
def test_pro_metrics_against_pro_eval(dev, shape, levels):
    m, s = PC.curve_case(shape, levels)
    for limit in (0.05, 0.3, 1.0):
        got = check(dev, m, s, limit)
        again = engine.pro_metrics(T(s.copy()).to(dev), T(m.copy()).to(dev), fpr_limit=limit)
        assert np.float64(again.aupro).view(np.uint64) == np.float64(got.aupro).view(np.uint64) and again[1:] == got[1:]
    check(dev, m, s, 0.3, connectivity=4)


def test_pro_curve_record_and_a_group_exactly_on_the_limit(dev):
    """N_ok a multiple of 4 and exactly a quarter of the normal pixels above a score gap: x = 0.25 is a curve point"""
    import forward_utils as FU
    m = PC.mask("blobs", (3, 37, 53)).copy()
    normal = np.flatnonzero(m.reshape(-1) == 0)
    m.reshape(-1)[normal[:normal.size % 4]] = 1                 # N_ok becomes a multiple of 4
    normal = np.flatnonzero(m.reshape(-1) == 0)
    rng = np.random.default_rng(11)
    s = (rng.random(m.size) * 0.4).astype(np.float32)
    s[rng.permutation(normal)[:normal.size // 4]] += np.float32(0.55)
    anomalous = np.flatnonzero(m.reshape(-1))
    s[anomalous] = (0.5 + 0.5 * np.round(rng.random(anomalous.size) * 8) / 8).astype(np.float32)
    s = s.reshape(m.shape)
    assert np.count_nonzero((s >= 0.5) & (m == 0)) * 4 == normal.size and s.max() == 1
    got = check(dev, m, s, 0.25)
    # the stages one by one, and the y of the record at the limit: every anomalous pixel scores >= 0.5, so y(0.25) = 1
    mask, scores = T(m).to(dev), T(s).to(dev)
    _, area, regions_record = engine.metrics_regions(mask)
    keys, areas_sorted = engine.metrics_sort_pairs(scores, area)
    rec = engine.metrics_pro_curve(keys, areas_sorted, regions_record, 0.25).cpu()
    assert float(rec[0:1].view(torch.float64)) == got.aupro and [int(v) for v in rec[1:4]] == list(got[1:])
    assert abs(float(rec[4:5].view(torch.float64)) - 1.0) <= 1e-12
    want = FU.pro_eval_record(m, s, fpr_limit=0.25)
    assert want[1:] == tuple(got[1:])
    with pytest.raises(ValueError, match="fpr_limit"):
        engine.metrics_pro_curve(keys, areas_sorted, regions_record, 0.0)


def test_pro_metrics_edge_cases(dev):
    import forward_utils as FU
    rng = np.random.default_rng(5)
    shape = (2, 37, 53)
    base = rng.random(shape).astype(np.float32) * 3 - 1
    # the first tie group already beyond the limit: 60 % of the pixels share the top score
    m = PC.mask("blobs", shape)
    s = base.copy()
    s[rng.random(shape) < 0.6] = 2.5
    got = check(dev, m, s, 0.3)
    assert got.aupro < 1.0
    # a single one-pixel region
    one = np.zeros(shape, np.uint8)
    one[1, 20, 33] = 1
    assert check(dev, one, base, 0.3).regions == 1
    top = base.copy()
    top[1, 20, 33] = 5.0
    assert abs(check(dev, one, top, 0.05).aupro - 1.0) <= 1e-12
    # one region that is a whole image, beside a normal image
    whole = np.zeros(shape, np.uint8)
    whole[0] = 1
    r = check(dev, whole, base, 0.3)
    assert (r.regions, r.normal) == (1, 37 * 53)
    # perfect and inverted scores
    perfect = (rng.random(shape) * 0.5 + m).astype(np.float32)
    for limit in (0.05, 0.3, 1.0):
        assert abs(check(dev, m, perfect, limit).aupro - 1.0) <= 1e-12
    assert check(dev, m, -perfect, 0.3).aupro < 0.05
    # scores taken as they are
    want = FU._pro_curve_area(m, base, 0.3, 8)
    got = engine.pro_metrics(T(base).to(dev), T(m.copy()).to(dev), fpr_limit=0.3, normalise=False)
    assert tuple(got[1:]) == want[1:] and abs(got.aupro - want[0]) <= BOUND
    flat = np.full(shape, 0.25, np.float32)                      # equal scores are one group then, not an error
    got = engine.pro_metrics(T(flat).to(dev), T(m.copy()).to(dev), fpr_limit=0.3, normalise=False)
    assert got.groups == 1 and abs(got.aupro - FU._pro_curve_area(m, flat, 0.3, 8)[0]) <= BOUND


def test_pro_metrics_refusals(dev):
    m, s = PC.curve_case((5, 8, 8), 16)
    mask, scores = T(m.copy()).to(dev), T(s.copy()).to(dev)
    with pytest.raises(ValueError, match="0 regions"):
        engine.pro_metrics(scores, torch.zeros_like(mask))
    with pytest.raises(ValueError, match="0 normal pixels"):
        engine.pro_metrics(scores, torch.ones_like(mask))
    for bad in (float("nan"), float("inf")):
        broken = scores.clone()
        broken[2, 3, 4] = bad
        with pytest.raises(ValueError, match="not finite"):
            engine.pro_metrics(broken, mask)
    with pytest.raises(ValueError, match="equal"):
        engine.pro_metrics(torch.full_like(scores, 0.5), mask)
    for limit in (0.0, 1.5):
        with pytest.raises(ValueError, match="fpr_limit"):
            engine.pro_metrics(scores, mask, fpr_limit=limit)
    with pytest.raises(ValueError, match="one size"):
        engine.pro_metrics(scores[:4], mask)


# ------------------------------------------------------------------------------------------------- the harness
def test_metrics_eval_device_with_a_limit_equals_metrics_eval(dev):
    import forward_utils as FU
    found = 0
    for shape, levels in [((3, 37, 53), 16), ((2, 70, 130), 0), ((5, 8, 8), 4), ((3, 37, 53), 64)]:
        m, s = PC.curve_case(shape, levels)
        if not PC.harness_seed_is_safe(FU.pro_eval(m, s, fpr_limit=0.3)):      # too near a rounding boundary: next set
            continue
        found += 1
        image_label = (m.reshape(shape[0], -1).max(axis=1) > 0).astype(np.int64)
        image_label[0] = 1 - image_label[0] if image_label.min() == image_label.max() else image_label[0]
        image_preds = np.linspace(0.2, 0.7, shape[0]).astype(np.float32)
        mask4 = m[:, None].astype(np.float32)
        host = FU.metrics_eval(mask4, image_label, s, image_preds, "x", "Industrial", fpr_limit=0.3)
        got = FU.metrics_eval_device(T(mask4).to(dev), image_label, T(s.copy()).to(dev), image_preds, "x", "Industrial",
                                     fpr_limit=0.3)
        assert got == host and "pixel AUPRO" in got, (got, host)
        plain = FU.metrics_eval_device(T(mask4).to(dev), image_label, T(s.copy()).to(dev), image_preds, "x", "Industrial")
        assert plain == {k: v for k, v in host.items() if k != "pixel AUPRO"}
        assert abs(FU.pro_eval_device(T(m.copy()).to(dev), T(s.copy()).to(dev)) - FU.pro_eval(m, s)) <= BOUND
    assert found >= 2


def test_evaluate_with_aupro_returns_the_host_rows(dev):
    import eval_aupro as EA
    import eval_last as EL
    import test_last as TL
    from test_gpu_metrics_device import StubModel, stub_class
    items, anchors = stub_class()
    model, anchors = StubModel(dev), anchors.to(dev)
    sets, emb = {"bottle": items, "grid": items[2:]}, {"bottle": anchors, "grid": anchors}
    args = (model, sets, emb, dev, 70, "MVTec")
    host = EA.evaluate(*args, batch_size=4, use_iqm=True, aupro_limit=0.3)
    got = EA.evaluate(*args, batch_size=4, use_iqm=True, device_metrics=True, aupro_limit=0.3)
    assert got == host and len(got) == 3 and all("pixel AUPRO" in r for r in got)
    assert got[-1]["pixel AUPRO"] == float(np.mean([r["pixel AUPRO"] for r in got[:-1]]))
    # without a limit the rows are test_last's, on either path
    today = TL.evaluate(*args, batch_size=4, use_iqm=True)
    assert EA.evaluate(*args, batch_size=4, use_iqm=True, device_metrics=True) == today
    assert EL.evaluate(*args, batch_size=4, use_iqm=True, device_metrics=True) == today
    assert EL.evaluate(*args, batch_size=4, use_iqm=True) == today
    assert [{k: v for k, v in r.items() if k != "pixel AUPRO"} for r in got] == today
    assert EL.format_table(today) == TL.format_table(today) and "pixel AUPRO" in EL.format_table(got).split("\n")[0]
