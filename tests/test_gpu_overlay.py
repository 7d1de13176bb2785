"""Heat-map overlays on the device (csrc/overlay.hip) against the numpy definition of tests/overlay_cases.py, byte for byte:
the raw entry on guarded byte buffers at three output alignments over the whole case grid and at the working sizes;
refusals that write nothing; the stream in the plan; engine's argument checks; and eval_overlay end to end on both
metrics paths, untiled and tiled.

There is no tolerance: every step of the definition is an integer operation or a separately rounded fp32 one."""
import ctypes
import os

import numpy as np
import pytest
import torch

import overlay_cases as OC
from aaclip_hip import _lib, engine

pytestmark = pytest.mark.gpu

T = torch.from_numpy
GUARD = 512                # bytes on either side of the output
SENTINEL = 0xA5
ENTRY = "aaclip_overlay_render"
BITS = {"frame": 1, "heat": 2, "truth": 4}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def err():
    return _lib.load().aaclip_last_error().decode()


def make_plan(B, H, W, kw, stream=None, override=None):
    p = _lib.OverlayPlan()
    p.images, p.height, p.width = B, H, W
    p.panels = sum(BITS[name] for name in kw["panels"])
    p.alpha256, p.thickness, p.stream = kw["alpha256"], kw["thickness"], stream
    for c in range(3):
        p.pred_colour[c], p.truth_colour[c] = OC.PRED_COLOUR[c], OC.TRUTH_COLOUR[c]
        p.mean[c], p.std[c] = OC.CLIP_MEAN[c], OC.CLIP_STD[c]
    for k, v in (override or {}).items():
        if k == "std0":
            p.std[0] = v
        else:
            setattr(p, k, v)
    return p


def upload(dev, frames, maps, kw):
    up = lambda a: None if a is None else T(np.array(a)).to(dev)
    return {"frames": up(frames), "maps": up(maps), "record": up(kw["range_record"]), "pred": up(kw["pred"]),
            "truth": up(kw["truth"]), "lut": up(kw["lut"])}


def raw(dev, plan, t, out_shape, shift=0, null=()):
    """One raw call into a buffer of sentinel bytes with GUARD bytes on either side, the output `shift` bytes behind a
    256-byte boundary -> (rc, the output as uint8 of out_shape, or None where no byte of it was written).  Asserts that
    no guard byte changed."""
    lib = _lib.load()
    n = int(np.prod(out_shape))
    buf = torch.full((n + 2 * GUARD + 256,), SENTINEL, dtype=torch.uint8, device=dev)
    start = GUARD + (shift - buf.data_ptr() - GUARD) % 256          # the first such position with a full guard in front
    out = buf[start:start + n]
    assert out.data_ptr() % 256 == shift
    ptr = lambda name: None if name in null or t[name] is None else t[name].data_ptr()
    rc = getattr(lib, ENTRY)(None if "plan" in null else ctypes.byref(plan), ptr("frames"), ptr("maps"), ptr("record"),
                             ptr("pred"), ptr("truth"), ptr("lut"), None if "out" in null else out.data_ptr())
    torch.cuda.synchronize(dev)
    h = buf.cpu().numpy()
    assert np.all(h[:start] == SENTINEL) and np.all(h[start + n:] == SENTINEL), "guard bytes were written"
    body = h[start:start + n]
    if np.all(body == SENTINEL):
        return rc, None
    return rc, body.reshape(out_shape)


def check_case(dev, case, shifts=(0, 1, 2)):
    frames, maps, kw = OC.arguments(case)
    want = OC.expected(case)
    t = upload(dev, frames, maps, kw)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for shift in shifts:
        plan = make_plan(case["B"], case["H"], case["W"], kw, stream)
        rc, got = raw(dev, plan, t, want.shape, shift)
        assert rc == 0, err()
        assert got is not None and np.array_equal(got, want), \
            f"{OC.case_id(case)} shift {shift}: {int((got != want).sum())} of {want.size} bytes differ"
    rc, again = raw(dev, plan, t, want.shape, shifts[-1])
    assert rc == 0 and np.array_equal(again, got), "a second call gives other bytes"


# ---------------------------------------------------------------------------------------------------- the raw entry
@pytest.mark.parametrize("size", OC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_raw_entry_gives_the_definitions_bytes_on_the_grid(dev, size):
    cases = list(OC.grid(size))
    assert len(cases) == 32
    for case in cases:
        check_case(dev, case)


@pytest.mark.parametrize("name", OC.SPECIALS)
def test_the_special_cases(dev, name):
    cases = [c for c in OC.specials() if c["special"] == name]
    assert len(cases) == 2
    for case in cases:
        check_case(dev, case)


@pytest.mark.parametrize("B,H,W", OC.WORKING)
def test_the_working_sizes(dev, B, H, W):
    case = {"B": B, "H": H, "W": W, "T": 1, "pred": True, "truth": True, "alpha256": 128, "panels": OC.PANELS, "lut": "jet",
            "special": None}
    check_case(dev, case, shifts=(2,))


def test_refusals_write_nothing(dev):
    case = {"B": 2, "H": 37, "W": 37, "T": 1, "pred": True, "truth": True, "alpha256": 128, "panels": OC.PANELS,
            "lut": "jet", "special": None}
    frames, maps, kw = OC.arguments(case)
    want = OC.expected(case)
    t = upload(dev, frames, maps, kw)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for override, msg in ((dict(struct_bytes=64), "struct_bytes"), (dict(struct_bytes=80), "struct_bytes"),
                          (dict(images=-1), "images"), (dict(height=0), "height"), (dict(width=0), "width"),
                          (dict(panels=0), "panels"), (dict(panels=8), "panels"), (dict(alpha256=-1), "alpha256"),
                          (dict(alpha256=257), "alpha256"), (dict(thickness=-1), "thickness"), (dict(thickness=9), "thickness"),
                          (dict(std0=0.0), "std"), (dict(std0=float("inf")), "std"), (dict(std0=float("nan")), "std")):
        rc, got = raw(dev, make_plan(2, 37, 37, kw, stream, override), t, want.shape)
        assert rc == -1 and got is None, override
        assert err().startswith(ENTRY) and msg in err(), (override, err())
    for null in ("plan", "frames", "maps", "lut", "out", "truth"):
        rc, got = raw(dev, make_plan(2, 37, 37, kw, stream), t, want.shape, null=(null,))
        assert rc == -1 and got is None and err().startswith(ENTRY), (null, err())
    rc, got = raw(dev, make_plan(0, 37, 37, kw, stream), t, want.shape)
    assert rc == 0 and got is None                              # no images: no launch, nothing written
    rc, got = raw(dev, make_plan(0, 37, 37, kw, stream, dict(thickness=9)), t, want.shape)
    assert rc == -1 and got is None                             # ... but the plan is still checked
    lib = _lib.load()                                           # out over an input
    plan = make_plan(2, 37, 37, kw, stream)
    assert getattr(lib, ENTRY)(ctypes.byref(plan), t["frames"].data_ptr(), t["maps"].data_ptr(), None, None,
                               t["truth"].data_ptr(), t["lut"].data_ptr(), t["frames"].data_ptr() + 64) == -1
    assert "overlap" in err()
    torch.cuda.synchronize(dev)
    assert np.array_equal(t["frames"].cpu().numpy().view(np.uint32), frames.view(np.uint32))
    rc, got = raw(dev, plan, t, want.shape)
    assert rc == 0 and np.array_equal(got, want), err()         # and the good plan does write


def test_a_side_stream_gives_the_default_streams_bytes(dev):
    case = {"B": 3, "H": 70, "W": 70, "T": 2, "pred": True, "truth": True, "alpha256": 77, "panels": OC.PANELS, "lut": "jet",
            "special": None}
    frames, maps, kw = OC.arguments(case)
    t = upload(dev, frames, maps, kw)
    call = lambda: engine.overlay_render(t["frames"], t["maps"], t["record"], t["pred"], t["truth"], alpha=77 / 256,
                                         lut=t["lut"], thickness=2)
    want = call()
    torch.cuda.synchronize(dev)
    assert np.array_equal(want.cpu().numpy(), OC.expected(case))
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream != 0
        got = call()                                            # engine: torch's current stream
    side.synchronize()
    assert torch.equal(got, want)
    out = torch.zeros_like(want)                                # the raw entry: queued on the side stream only
    torch.cuda.synchronize(dev)
    plan = make_plan(3, 70, 70, kw, side.cuda_stream)
    assert getattr(_lib.load(), ENTRY)(ctypes.byref(plan), t["frames"].data_ptr(), t["maps"].data_ptr(), t["record"].data_ptr(),
                                       t["pred"].data_ptr(), t["truth"].data_ptr(), t["lut"].data_ptr(), out.data_ptr()) == 0, err()
    side.synchronize()
    assert torch.equal(out, want)


def test_engine_checks_its_arguments_on_device_tensors(dev):
    import forward_utils as FU
    case = {"B": 2, "H": 7, "W": 5, "T": 1, "pred": True, "truth": True, "alpha256": 128, "panels": OC.PANELS, "lut": "jet",
            "special": None}
    frames, maps, kw = OC.arguments(case)
    t = upload(dev, frames, maps, kw)
    f, m, r, p, g = t["frames"], t["maps"], t["record"], t["pred"], t["truth"]
    out = engine.overlay_render(f, m, r, p, g)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 21, 5, 3) and np.array_equal(out.cpu().numpy(), OC.expected(case))
    assert tuple(engine.overlay_render(f, m, r, p).shape) == (2, 14, 5, 3)                 # no truth: its panel is dropped
    assert tuple(engine.overlay_render(f, m, panels=("heat",)).shape) == (2, 7, 5, 3)
    assert torch.equal(engine.overlay_render(f, m, r, p, g, panels=("truth", "frame")),
                       engine.overlay_render(f, m, r, p, g, panels=("frame", "truth")))         # always in the fixed order
    assert torch.equal(FU.render_overlays(f, m, r, p, g, alpha256=128), out)
    assert np.array_equal(FU.render_overlays_host(f, m, r, p, g), out.cpu().numpy())          # device tensors, host definition
    wide = torch.zeros(2, 3, 7, 10, device=dev)
    for bad in (dict(frames=f.cpu()), dict(maps=m.cpu()), dict(pred=p.cpu()), dict(truth=g.cpu()), dict(frames=f.half()),
                dict(frames=f.double()), dict(maps=m.half()), dict(pred=p.float()), dict(truth=g.bool()),
                dict(frames=f[:, :2]), dict(frames=f[0]), dict(maps=m[:1]), dict(maps=m[:, :6]), dict(pred=p[:, :, :4]),
                dict(frames=wide[..., ::2]), dict(maps=m.transpose(1, 2)), dict(truth=g[:, :, :4]),
                dict(range_record=r.cpu()), dict(range_record=r.int()), dict(range_record=r[:2]), dict(lut="hot"),
                dict(lut=t["lut"].cpu()), dict(lut=t["lut"][:255]), dict(lut=t["lut"].int()), dict(alpha=-0.1), dict(alpha=1.1),
                dict(thickness=-1), dict(thickness=9), dict(panels=()), dict(panels=("heat", "heat")), dict(panels=("edges",)),
                dict(truth=None, panels=("truth",)), dict(pred_colour=(0, 0, 256)), dict(truth_colour=(1, 2)),
                dict(std=(1.0, 0.0, 1.0)), dict(mean=(0.5, 0.5))):
        args = dict(frames=f, maps=m, range_record=r, pred=p, truth=g)
        args.update(bad)
        with pytest.raises(ValueError):
            engine.overlay_render(**args)


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def harness(dev, tmp_path_factory):
    """The synthetic tree and reduced fp32 model of test_gpu_tiled (S = 70), the datasets built at S and at the canvas side
    of tiles=(2, 14), C = 126"""
    import dataset as D
    import forward_utils as FU
    from synth_dataset import write_tree
    from test_gpu_metrics_device import build_tiny
    tmp = tmp_path_factory.mktemp("overlay")
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
    return dict(model=model, S=S, classes=classes, anchors=anchors, sets=sets, tmp=tmp)


def decode(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.array(im)


@pytest.mark.parametrize("tiles", [None, 2], ids=["untiled", "tiled"])
def test_end_to_end_on_both_metrics_paths(dev, harness, tiles):
    import eval_last as EL
    import eval_overlay as EO
    import eval_tiled as ET
    import forward_utils as FU
    h = harness
    S, O = h["S"], 14
    side = S if tiles is None else 126
    where = (h["model"], h["sets"][side], h["anchors"], dev, S, "MVTec")
    how = dict(batch_size=8, use_iqm=False, f1_max=True, defects=1, return_masks=True)
    if tiles is not None:
        how.update(tiles=tiles, tile_overlap=O)
    rows, details, written, pngs = {}, {}, {}, {}
    for path in ("host", "device"):
        save = str(h["tmp"] / f"{path}-{side}")
        written[path] = {}
        rows[path], details[path] = EO.evaluate(*where, **how, device_metrics=path == "device", save_path=save, overlay=0.3,
                                                overlay_thickness=2, overlay_written=written[path])
        assert rows[path] == ET.evaluate(*where, **how, device_metrics=path == "device")[0]          # the rows are eval_tiled's
        for c in h["classes"]:
            names = details[path][c]["file_names"]
            folder = os.path.join(save, "overlays", "MVTec", c)
            assert len(written[path][c]) == len(names) == len(h["sets"][side][c]) == len(os.listdir(folder))      # one each
            assert [os.path.basename(p) for p in written[path][c]] == [EO.overlay_name(n) for n in names]
            pngs[path, c] = [decode(p) for p in written[path][c]]
    assert rows["host"] == rows["device"]
    for c in h["classes"]:
        assert all(np.array_equal(a, b) for a, b in zip(pngs["host", c], pngs["device", c]))            # both paths, one picture
        # the definition on the dataset's frames, the maps of the predictions, the class range and the kept masks
        loader = torch.utils.data.DataLoader(h["sets"][side][c], batch_size=8, shuffle=False)
        frames = torch.cat([b["image"] for b in loader]).float().numpy()
        with torch.no_grad():
            if tiles is None:
                masks, _, maps, _, names = EL.get_predictions(h["model"], h["anchors"][c], loader, dev, S, "MVTec",
                                                              use_iqm=False, on_device=True)
            else:
                masks, _, maps, _, names = ET.get_predictions_tiled(h["model"], h["anchors"][c], loader, dev, S, "MVTec",
                                                                    use_iqm=False, on_device=True, tiles=(tiles, O))
        assert names == details["device"][c]["file_names"]
        maps = maps.cpu().numpy()
        kept = details["device"][c]["kept masks"]
        want = FU.render_overlays_host(frames, maps, {"min": maps.min(), "max": maps.max()}, kept,
                                       masks.reshape(maps.shape), alpha256=round(0.3 * 256), thickness=2)
        assert want.shape == (len(names), 3 * side, side, 3)
        for i, got in enumerate(pngs["device", c]):
            assert np.array_equal(got, want[i]), (c, names[i])
        assert any(k.any() for k in kept.cpu().numpy()) and float(maps.max()) != 1.0      # there is something to draw
    # --overlay_limit, and eval_tiled's rows without the masks when they were not asked for
    save = str(h["tmp"] / f"limit-{side}")
    how.pop("return_masks")
    limited = {}
    got = EO.evaluate(*where, **how, device_metrics=True, save_path=save, overlay=0.3, overlay_limit=2, overlay_written=limited)
    assert got == rows["device"]
    for c in h["classes"]:
        assert len(limited[c]) == 2 == len(os.listdir(os.path.join(save, "overlays", "MVTec", c)))
        assert all(np.array_equal(decode(p)[:side], q[:side]) for p, q in zip(limited[c], pngs["device", c]))      # the frame panel
    assert EO.evaluate(*where, **how, device_metrics=True, overlay=None) == ET.evaluate(*where, **how, device_metrics=True)
