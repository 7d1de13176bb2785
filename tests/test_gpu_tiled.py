"""Tiled inference on the device (csrc/tiles.hip) against the numpy definitions of tests/tiled_cases.py: the raw entries on
guarded buffers over the whole case grid, at the three vector widths and at the working size; refusals that write nothing;
the stream in the plan; engine's argument checks; and the evaluation harness with tiles on both metrics paths.

The bar of the stitch is tiled_cases.REL_BAR * max |v|, derived from the number formats, not measured.  The worst values
seen go to the parity record that conftest.PARITY_ERRORS writes at the end of the session."""
import ctypes

import numpy as np
import pytest
import torch

import tiled_cases as TC
from aaclip_hip import _lib, engine

pytestmark = pytest.mark.gpu

T = torch.from_numpy
GUARD = 64
SENTINEL = 0x5A5A5A5A
ENTRIES = ("aaclip_tile_gather", "aaclip_tile_stitch")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def record(name, **values):
    from conftest import PARITY_ERRORS
    PARITY_ERRORS[name] = values


def err():
    return _lib.load().aaclip_last_error().decode()


def make_plan(images, channels, S, G, O, stream=None, override=None):
    p = _lib.TilePlan()
    p.images, p.channels, p.tile, p.grid, p.overlap, p.stream = images, channels, S, G, O, stream
    for k, v in (override or {}).items():
        setattr(p, k, v)
    return p


def raw(dev, entry, plan, src, out_shape, shift=0, null=()):
    """One raw call of `entry` (gather: src = canvas; stitch: src = tiles) into a buffer of sentinel words with GUARD
    words on either side, the output `shift` words behind a 256-byte boundary -> (rc, output as fp32 of out_shape, or None
    where no word of it was written).  Asserts that no guard word changed."""
    lib = _lib.load()
    n = int(np.prod(out_shape))
    buf = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=torch.int32, device=dev)
    out = buf[GUARD + shift:GUARD + shift + n]
    s = src if torch.is_tensor(src) else T(np.array(src)).to(dev)
    src_ptr = None if "src" in null else s.data_ptr()
    out_ptr = None if "out" in null else out.data_ptr()
    rc = getattr(lib, entry)(None if "plan" in null else ctypes.byref(plan), src_ptr, out_ptr)
    torch.cuda.synchronize(dev)
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD + shift] == SENTINEL) and np.all(h[GUARD + shift + n:] == SENTINEL), "guard words were written"
    body = h[GUARD + shift:GUARD + shift + n]
    if np.all(body == SENTINEL):
        return rc, None
    return rc, body.view(np.float32).reshape(out_shape)


def check_gather(dev, S, G, O, frames, channels, shifts=(0, 1)):
    canvas = TC.canvas_case(S, G, O, frames, channels)
    want = TC.gather(canvas, S, G, O)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for shift in shifts:                    # 0: the widest vectors the sides allow; 1: a 4-byte aligned output, scalar stores
        plan = make_plan(frames, channels, S, G, O, stream)
        rc, got = raw(dev, "aaclip_tile_gather", plan, canvas, want.shape, shift)
        assert rc == 0, err()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "gather is not a copy of bits"
        rc, again = raw(dev, "aaclip_tile_gather", plan, canvas, want.shape, shift)
        assert rc == 0 and np.array_equal(again.view(np.uint32), got.view(np.uint32))


def check_stitch(dev, S, G, O, frames, channels, shifts=(0, 1)):
    """-> the worst |device - fp64 definition| over the shifts, relative to max |v|"""
    tiles, want = TC.case(S, G, O, frames, channels)
    one = TC.cover_count(S, G, O) == 1
    fp32 = TC.stitch(tiles, G, O, np.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    worst = 0.0
    for shift in shifts:
        plan = make_plan(frames, channels, S, G, O, stream)
        rc, got = raw(dev, "aaclip_tile_stitch", plan, tiles, want.shape, shift)
        assert rc == 0, err()
        e = float(np.abs(got.astype(np.float64) - want).max())
        differ = int((got.view(np.uint32) != fp32.view(np.uint32)).sum())
        print(f"stitch ({S}, {G}, {O}) x{frames} ch{channels} shift {shift}: max abs err {e:.3e}, bar {TC.bar(tiles):.3e}, "
              f"{differ} of {got.size} words differ from the fp32 definition")
        assert e <= TC.bar(tiles)
        assert np.array_equal(got[..., one].view(np.uint32), want[..., one].astype(np.float32).view(np.uint32)), \
            "a pixel under one tile does not carry that tile's bits"
        rc, again = raw(dev, "aaclip_tile_stitch", plan, tiles, want.shape, shift)
        assert rc == 0 and np.array_equal(again.view(np.uint32), got.view(np.uint32)), "a second call gives other bytes"
        worst = max(worst, e / float(np.abs(tiles).max()))
    return worst


# ---------------------------------------------------------------------------------------------------- the raw entries
@pytest.mark.parametrize("S,G,O", TC.GRID + (TC.VECTOR4,))
def test_gather_and_stitch_on_the_grid(dev, S, G, O):
    worst = 0.0
    for frames in TC.FRAMES:
        for channels in TC.CHANNELS:
            check_gather(dev, S, G, O, frames, channels)
            worst = max(worst, check_stitch(dev, S, G, O, frames, channels))
    print(f"stitch ({S}, {G}, {O}): worst error {worst:.3e} of max |v|, bar {TC.REL_BAR:.3e}")
    record(f"tiled_stitch.S{S}_G{G}_O{O}", max_rel_err=worst, bar=TC.REL_BAR)


def test_gather_and_stitch_at_the_working_size(dev):
    S, G, O = TC.WORKING
    assert TC.canvas_side(S, G, O) == 924
    check_gather(dev, S, G, O, 2, 1, shifts=(0,))
    worst = check_stitch(dev, S, G, O, 2, 1, shifts=(0,))
    print(f"stitch at the working size: worst error {worst:.3e} of max |v|, bar {TC.REL_BAR:.3e}")
    record("tiled_stitch.working_size", max_rel_err=worst, bar=TC.REL_BAR)


def test_bad_plans_are_refused_and_write_nothing(dev):
    S, G, O, frames, channels = 70, 2, 14, 1, 3
    canvas, (tiles, want) = TC.canvas_case(S, G, O, frames, channels), TC.case(S, G, O, frames, channels)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for entry, src, shape in (("aaclip_tile_gather", canvas, tiles.shape), ("aaclip_tile_stitch", tiles, want.shape)):
        for override, msg in ((dict(struct_bytes=32), "struct_bytes"), (dict(struct_bytes=48), "struct_bytes"),
                              (dict(grid=0), "grid"), (dict(tile=0), "tile"), (dict(channels=0), "channels"),
                              (dict(overlap=-1), "overlap"), (dict(overlap=S // 2 + 1), "overlap"), (dict(images=-1), "images")):
            rc, got = raw(dev, entry, make_plan(frames, channels, S, G, O, stream, override), src, shape)
            assert rc < 0 and got is None, (entry, override)
            assert err().startswith(entry) and msg in err(), (entry, override, err())
        for null in (("src",), ("out",), ("plan",)):
            rc, got = raw(dev, entry, make_plan(frames, channels, S, G, O, stream), src, shape, null=null)
            assert rc < 0 and got is None and err().startswith(entry) and "null" in err(), (entry, null, err())
        rc, got = raw(dev, entry, make_plan(0, channels, S, G, O, stream), src, shape)
        assert rc == 0 and got is None, entry                       # no images: no launch, nothing written
        rc, got = raw(dev, entry, make_plan(frames, channels, S, G, O, stream), src, shape)
        assert rc == 0 and got is not None, err()                   # and the good plan does write


def test_the_stream_in_the_plan_is_the_stream_of_the_launch(dev):
    """both entries on a side stream give the bytes of the default-stream call (no graph capture here)"""
    S, G, O, frames, channels = 70, 2, 14, 3, 3
    canvas = T(np.array(TC.canvas_case(S, G, O, frames, channels))).to(dev)
    tiles = T(np.array(TC.case(S, G, O, frames, channels)[0])).to(dev)
    want_tiles = engine.tile_gather(canvas, S, G, O)
    want_canvas = engine.tile_stitch(tiles, G, O, frames)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream != 0
        got_tiles = engine.tile_gather(canvas, S, G, O)                 # engine: torch's current stream
        got_canvas = engine.tile_stitch(tiles, G, O, frames)
    side.synchronize()
    assert torch.equal(got_tiles, want_tiles) and torch.equal(got_canvas, want_canvas)
    assert np.array_equal(want_tiles.cpu().numpy(), TC.gather(canvas.cpu().numpy(), S, G, O))
    # the raw entries: work queued on the side stream only -- the call is complete once THAT stream is
    lib = _lib.load()
    for entry, src, want in (("aaclip_tile_gather", canvas, want_tiles), ("aaclip_tile_stitch", tiles, want_canvas)):
        out = torch.zeros_like(want)
        torch.cuda.synchronize(dev)
        plan = make_plan(frames, channels, S, G, O, side.cuda_stream)
        assert getattr(lib, entry)(ctypes.byref(plan), src.data_ptr(), out.data_ptr()) == 0, err()
        side.synchronize()
        assert torch.equal(out, want), entry


def test_engine_refuses_what_does_not_match_the_plan(dev):
    S, G, O = 70, 2, 14
    canvas = torch.zeros(2, 3, 126, 126, device=dev)
    tiles = torch.zeros(8, 3, S, S, device=dev)
    assert engine.tile_gather(canvas, S, G, O).shape == (8, 3, S, S) and engine.tile_stitch(tiles, G, O, 2).shape == canvas.shape
    assert engine.tile_gather(canvas[:, 0].contiguous(), S, G, O).shape == (8, S, S)                      # maps: no channel axis
    assert engine.tile_stitch(tiles[:, 0].contiguous(), G, O, 2).shape == (2, 126, 126)
    for bad in (canvas.cpu(), canvas.half(), canvas.double(), canvas[:, :, :125], canvas[:, :, :, :125], canvas[..., ::2],
                canvas.transpose(2, 3), canvas[0, 0], torch.zeros(2, 3, 127, 127, device=dev)):
        with pytest.raises(ValueError):
            engine.tile_gather(bad, S, G, O)
    for bad, images in ((tiles.cpu(), 2), (tiles.half(), 2), (tiles, 3), (tiles[:7], 2), (tiles[:, :, :, :69], 2),
                        (tiles.transpose(2, 3), 2), (tiles[0, 0], 2), (tiles, -1)):
        with pytest.raises(ValueError):
            engine.tile_stitch(bad, G, O, images)
    for call in (lambda: engine.tile_gather(canvas, S, G, 36), lambda: engine.tile_gather(canvas, S, 0, O),
                 lambda: engine.tile_stitch(tiles, G, 36, 2), lambda: engine.tile_stitch(tiles, 0, O, 2)):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def harness(dev, tmp_path_factory):
    """The synthetic tree and reduced fp32 model of test_gpu_support.test_harness_with_a_support_bank (S = 70), with the
    datasets built at S and at the canvas side of tiles=(2, 14), C = 126"""
    import dataset as D
    import forward_utils as FU
    from synth_dataset import write_tree
    from test_gpu_metrics_device import build_tiny
    tmp = tmp_path_factory.mktemp("tiled")
    root = write_tree(str(tmp / "MVTec"))
    meta = str(tmp / "meta" / "MVTec" / "full-shot.jsonl")
    D.build_metadata(root, meta)
    cfg, clip, model = build_tiny(dev, "fp32")
    S = cfg.image_size
    assert S == 70 and engine.tile_canvas(S, 2, 14) == 126
    classes = ["bottle", "grid"]
    with torch.no_grad():
        anchors = {c: FU.get_adapted_single_class_text_embedding(model, "MVTec", c, dev) for c in classes}
    sets = {side: {c: D.BaseSingleClassDataset(root, meta, side, c) for c in classes} for side in (S, 126)}
    return dict(cfg=cfg, model=model, S=S, classes=classes, anchors=anchors, sets=sets)


def test_one_tile_is_the_untiled_harness(dev, harness):
    import eval_last as EL
    import eval_tiled as ET
    h = harness
    for c in h["classes"]:
        loader = torch.utils.data.DataLoader(h["sets"][h["S"]][c], batch_size=4)
        with torch.no_grad():
            want = EL.get_predictions(h["model"], h["anchors"][c], loader, dev, h["S"], "MVTec", use_iqm=False, on_device=True)
            got = ET.get_predictions_tiled(h["model"], h["anchors"][c], loader, dev, h["S"], "MVTec", use_iqm=False,
                                           on_device=True, tiles=(1, 0))
        assert torch.equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[4] == want[4]
        assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])                # maps and scores, bit for bit


def test_tiled_maps_are_the_stitched_tile_maps(dev, harness):
    import eval_tiled as ET
    import forward_utils as FU
    h = harness
    S, G, O, C = h["S"], 2, 14, 126
    model, c = h["model"], "bottle"
    anchors = h["anchors"][c]
    loader = torch.utils.data.DataLoader(h["sets"][C][c], batch_size=2)
    with torch.no_grad():
        masks, labels, maps, scores, names = ET.get_predictions_tiled(model, anchors, loader, dev, S, "MVTec", use_iqm=False,
                                                                      on_device=True, tiles=(G, O))
        # the untiled steps on explicitly sliced tiles, in the loader's batches (frame-major, then t)
        tile_maps, tile_scores = [], []
        for batch in loader:
            image = batch["image"].to(dev)
            sliced = torch.stack([image[:, :, r:r + S, x:x + S] for r, x in FU.tile_origins(S, G, O)], dim=1)
            sliced = sliced.reshape(-1, 3, S, S).contiguous()
            patch_features, det_feature, _ = model(sliced, text_embeddings=None)
            tile_scores.append(FU.image_score(det_feature, anchors).float())
            tile_maps.append(FU.calculate_anomaly_map(patch_features, anchors, S, domain="Industrial"))
        tile_maps, tile_scores = torch.cat(tile_maps), torch.cat(tile_scores)
    n = len(h["sets"][C][c])
    assert masks.shape == (n, 1, C, C) and masks.dtype == torch.uint8 and maps.shape == (n, C, C) and scores.shape == (n,)
    assert len(names) == n and labels.shape == (n,)
    want = FU.tile_stitch_host(tile_maps, G, O)
    bar = TC.REL_BAR * float(tile_maps.abs().max())
    e = float(np.abs(maps.cpu().numpy().astype(np.float64) - want).max())
    print(f"harness: |tiled map - host stitch of the tile maps| {e:.3e}, bar {bar:.3e}")
    assert e <= bar
    record("tiled_harness.fp32", max_abs_err=e, bar=bar)
    assert torch.equal(scores, tile_scores.reshape(n, G * G).max(dim=1).values)            # the maximum of the tile scores
    with pytest.raises(ValueError, match="126"):                                           # datasets built at S, not at C
        ET.get_predictions_tiled(model, anchors, torch.utils.data.DataLoader(h["sets"][S][c], batch_size=2), dev, S,
                                 "MVTec", use_iqm=False, on_device=True, tiles=(G, O))


def test_evaluate_with_tiles_on_both_metrics_paths(dev, harness):
    import eval_coreset as EC
    import eval_tiled as ET
    h = harness
    S, G, O, C = h["S"], 2, 14, 126
    where = (h["model"], h["sets"][C], h["anchors"], dev, S, "MVTec")
    how = dict(batch_size=8, use_iqm=False, tiles=G, tile_overlap=O)
    out, details = {}, {}
    for path in ("host", "device"):
        out[path], details[path] = ET.evaluate(*where, **how, device_metrics=path == "device", f1_max=True, defects=1,
                                               return_masks=True)
    assert out["device"] == out["host"] and len(out["host"]) == 3                          # row for row
    for c in h["classes"]:
        d = details["device"][c]
        assert tuple(d["masks"].shape) == (len(h["sets"][C][c]), C, C) and "support nearest" not in d
        assert d["file_names"] == details["host"][c]["file_names"] and d["pixel threshold"] == details["host"][c]["pixel threshold"]
    assert ET.evaluate(*where, **how, device_metrics=True) == ET.evaluate(*where, **how)    # and the plain rows
    # support: the bank of a class holds the tiles of its 2 support frames
    P = (S // h["cfg"].patch_size) ** 2
    banks, evaluated = ET.tiled_support_banks(h["model"], h["sets"][C], 2, dev, S, (G, O))
    for c in h["classes"]:
        assert banks[c].shots == 2 * G * G and banks[c].patches == P and len(banks[c].rows) == 2
        assert all(r.shape[0] == 2 * G * G * P for r in banks[c].rows) and len(evaluated[c]) == len(h["sets"][C][c]) - 2
    rows = {path: ET.evaluate(*where, **how, device_metrics=path == "device", f1_max=True, support=2) for path in out}
    assert rows["device"] == rows["host"] and len(rows["host"]) == 3
    # tiles=None: eval_coreset.evaluate
    plain = (h["model"], h["sets"][S], h["anchors"], dev, S, "MVTec")
    assert ET.evaluate(*plain, batch_size=4, use_iqm=False, device_metrics=True, f1_max=True, support=2) == \
        EC.evaluate(*plain, batch_size=4, use_iqm=False, device_metrics=True, f1_max=True, support=2)
    with pytest.raises(ValueError, match="126"):
        ET.evaluate(*plain, batch_size=4, use_iqm=False, tiles=G, tile_overlap=O)
