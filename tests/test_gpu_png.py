"""PNG encoding on the device (csrc/png.hip) against the host definition forward_utils.png_encode_host, byte for byte: the
raw entry over the whole grid of tests/png_cases.py with the pixels at an even and at an odd address and a sentinel behind
the payload; a second call; a side stream; refusals that write nothing; the working sizes against zlib, the size bar and
Pillow; and eval_png end to end, untiled and tiled.

There is no tolerance: the format is defined in integers."""
import ctypes
import io
import os
import zlib

import numpy as np
import pytest
import torch

import png_cases as PC
from aaclip_hip import _lib, engine

pytestmark = pytest.mark.gpu

T = torch.from_numpy
SENTINEL = 0xA5
GUARD = 512
ENTRY = "aaclip_png_encode"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def definition():
    """the host definition's (payload, offsets) of every case of the grid, computed once"""
    import forward_utils as FU
    return {name: FU.png_encode_host(px) for name, px in PC.cases()}


def err():
    return _lib.load().aaclip_last_error().decode()


def make_plan(shape, stream=None, **override):
    p = _lib.PngPlan()
    p.images, p.height, p.width, p.channels = (int(v) for v in shape)
    p.stream = stream
    for k, v in override.items():
        setattr(p, k, v)
    return p


def raw(dev, pixels, shift=0, stream=None, plan=None, null=(), capacity=None, ws_short=0):
    """One raw call: the pixels `shift` bytes behind a 256-byte boundary, the payload a buffer of sentinel bytes with
    GUARD more behind its capacity -> (rc, payload up to offsets[-1] as numpy, offsets as a list), or (rc, None, None)
    where nothing was written.  Asserts that no byte behind offsets[-1] changed."""
    lib = _lib.load()
    shape = pixels.shape
    plan = plan or make_plan(shape, torch.cuda.current_stream(dev).cuda_stream if stream is None else stream)
    good = make_plan(shape)
    cap, ws_bytes = lib.aaclip_png_capacity_bytes(ctypes.byref(good)), lib.aaclip_png_workspace_bytes(ctypes.byref(good))
    src = torch.zeros(pixels.size + 512, dtype=torch.uint8, device=dev)
    start = (shift - src.data_ptr()) % 256
    src[start:start + pixels.size] = T(pixels.reshape(-1)).to(dev)
    assert (src.data_ptr() + start) % 256 == shift
    payload = torch.full((cap + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    offsets = torch.full((shape[0] + 1,), -7, dtype=torch.int64, device=dev)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    ptr = lambda name, t: None if name in null else t
    rc = getattr(lib, ENTRY)(None if "plan" in null else ctypes.byref(plan), ptr("pixels", src.data_ptr() + start),
                             ptr("workspace", ws.data_ptr()), ws_bytes - ws_short, ptr("payload", payload.data_ptr()),
                             cap if capacity is None else capacity, ptr("offsets", offsets.data_ptr()))
    torch.cuda.synchronize(dev)
    host, offs = payload.cpu().numpy(), offsets.cpu().tolist()
    if rc != 0 or shape[0] == 0:
        assert np.all(host == SENTINEL) and all(o == -7 for o in offs), "a refused or empty call wrote something"
        return rc, None, None
    assert offs[0] == 0 and offs[-1] <= cap and np.all(host[offs[-1]:] == SENTINEL), "bytes behind offsets[-1] were written"
    return rc, host[:offs[-1]], offs


CASES = PC.cases()


# ---------------------------------------------------------------------------------------------------- the raw entry
@pytest.mark.parametrize("name,pixels", CASES, ids=[c[0] for c in CASES])
def test_the_raw_entry_gives_the_definitions_bytes(dev, definition, name, pixels):
    want, want_offsets = definition[name]
    if pixels.shape[0] == 0:
        rc, got, _ = raw(dev, pixels)
        assert rc == 0 and got is None                           # no images: no launch, nothing written
        return
    for shift in (0, 1):
        rc, got, offsets = raw(dev, pixels, shift)
        assert rc == 0, err()
        assert offsets == want_offsets, (name, shift, offsets, want_offsets)
        assert np.array_equal(got, want), f"{name} shift {shift}: {int((got != want).sum())} of {want.size} bytes differ"
    rc, again, offsets = raw(dev, pixels, 1)
    assert rc == 0 and offsets == want_offsets and np.array_equal(again, got), "a second call gives other bytes"


def test_a_side_stream_gives_the_default_streams_bytes(dev, definition):
    name, pixels = next(c for c in CASES if c[0] == "batch-3x64x48x3")
    want, want_offsets = definition[name]
    on = T(pixels).to(dev)
    payload, offsets = engine.png_encode(on)
    torch.cuda.synchronize(dev)
    assert offsets.cpu().tolist() == want_offsets and np.array_equal(payload[:want_offsets[-1]].cpu().numpy(), want)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream != 0
        p2, o2 = engine.png_encode(on)                            # engine: torch's current stream
    side.synchronize()
    assert torch.equal(o2, offsets) and torch.equal(p2[:want_offsets[-1]], payload[:want_offsets[-1]])
    rc, got, offs = raw(dev, pixels, 3, stream=side.cuda_stream)   # the raw entry: queued on the side stream only
    assert rc == 0 and offs == want_offsets and np.array_equal(got, want), err()
    grey = T(pixels[..., 0].copy()).to(dev)                       # [images, H, W] is C = 1
    p3, o3 = engine.png_encode(grey)
    p4, o4 = engine.png_encode(grey[..., None])
    assert torch.equal(o3, o4) and torch.equal(p3[:int(o3[-1])], p4[:int(o4[-1])])
    none, zero = engine.png_encode(on[:0])
    assert none.numel() == 0 and zero.tolist() == [0] and none.is_cuda and zero.is_cuda
    for bad in (on.cpu(), on.float(), on[:, :, :, :2], on[:, :, ::2], on[0, 0], on.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError):
            engine.png_encode(bad)


def test_refusals_write_nothing(dev, definition):
    name, pixels = next(c for c in CASES if c[0] == "batch-3x64x48x3")
    shape = pixels.shape
    for override, msg in ((dict(struct_bytes=24), "struct_bytes"), (dict(struct_bytes=40), "struct_bytes"),
                          (dict(images=-1), "images"), (dict(height=-1), "height"), (dict(width=-2), "width"),
                          (dict(height=0), "height"), (dict(width=0), "width"), (dict(channels=2), "channels"),
                          (dict(channels=4), "channels"), (dict(channels=0), "channels"),
                          (dict(width=PC.REFUSED_WIDTH), "32768"), (dict(width=2 ** 31 - 1), "32768"),
                          (dict(images=2 ** 31 - 1, height=2 ** 31 - 1, width=10922), "too large")):
        rc, got, _ = raw(dev, pixels, plan=make_plan(shape, None, **override))
        assert rc == -1 and got is None, override
        assert err().startswith(ENTRY + ":") and msg in err(), (override, err())
    for null in ("plan", "pixels", "workspace", "payload", "offsets"):
        rc, got, _ = raw(dev, pixels, null=(null,))
        assert rc == -1 and got is None and err().startswith(ENTRY + ":"), (null, err())
    lib = _lib.load()
    cap = lib.aaclip_png_capacity_bytes(ctypes.byref(make_plan(shape)))
    assert cap == 3 * (8 + 64 * (1 + 48 * 3) + 5 * 1)
    rc, got, _ = raw(dev, pixels, capacity=cap - 1)
    assert rc == -1 and got is None and "capacity" in err()
    rc, got, _ = raw(dev, pixels, ws_short=1)
    assert rc == -1 and got is None and "workspace" in err()
    want, want_offsets = definition[name]
    rc, got, offs = raw(dev, pixels)
    assert rc == 0 and offs == want_offsets and np.array_equal(got, want), err()       # and the good call does write


# ---------------------------------------------------------------------------------------------------- the working sizes
WORKING = [("panels-2x1554x518x3", (2, 1554, 518, 3), 31), ("panel-1x2772x924x3", (1, 2772, 924, 3), 32),
           ("masks-3x518x518x1", (3, 518, 518, 1), 33)]


@pytest.mark.parametrize("name,shape,seed", WORKING, ids=[w[0] for w in WORKING])
def test_the_working_sizes(dev, name, shape, seed):
    """the pure definition is too slow to be the reference here: every stream inflates with zlib to the numpy filter
    definition's bytes, meets the size bar of png_cases.py, and its file decodes in Pillow to the input"""
    import forward_utils as FU
    from PIL import Image
    images, H, W, C = shape
    if C == 3:
        pixels = PC.photo(images, H, W, C, seed)
    else:
        pixels = np.zeros(shape, dtype=np.uint8)
        for i in range(images):
            pixels[i, 40 + 30 * i:300 + 60 * i, 100 - 20 * i:420] = 255
            pixels[i, 400:430, 10 + i:470:7] = 255
    payload, offsets = engine.png_encode(T(pixels).to(dev))
    torch.cuda.synchronize(dev)
    offsets = offsets.cpu().tolist()
    host = payload[:offsets[-1]].cpu().numpy()
    geom = engine.png_segments(H, W, C)
    assert offsets[0] == 0 and payload.numel() == images * geom["capacity"]
    files = FU.png_files(host, offsets, H, W, C)
    for i in range(images):
        filtered = FU.png_filter_host(pixels[i])
        stream = host[offsets[i]:offsets[i + 1]].tobytes()
        assert zlib.decompress(stream) == filtered.tobytes(), (name, i)
        size, reference = len(stream), PC.zrle_size(filtered)
        print(f"{name}[{i}]: {size} bytes, zRLE {reference} ({100.0 * (size - reference) / reference:+.3f} %), "
              f"{geom['segments']} segments")
        assert size <= PC.size_bar(filtered, geom["segments"]), (name, i, size, reference)
        with Image.open(io.BytesIO(files[i])) as im:
            assert im.mode == ("RGB" if C == 3 else "L")
            assert np.array_equal(np.array(im).reshape(H, W, C), pixels[i]), (name, i)


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def harness(dev, tmp_path_factory):
    """the tiny harness of test_gpu_overlay: the synthetic tree and reduced fp32 model (S = 70), the datasets built at S
    and at the canvas side of tiles=(2, 14), C = 126"""
    import dataset as D
    import forward_utils as FU
    from synth_dataset import write_tree
    from test_gpu_metrics_device import build_tiny
    tmp = tmp_path_factory.mktemp("png")
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


def decode(path, mode):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == mode, (path, im.mode)
        return np.array(im)


@pytest.mark.parametrize("tiles,defects", [(None, None), (2, 1)], ids=["untiled", "tiled-defects"])
def test_end_to_end(dev, harness, tiles, defects):
    import eval_overlay as EO
    import eval_png as EP
    h = harness
    S = h["S"]
    side = S if tiles is None else 126
    where = (h["model"], h["sets"][side], h["anchors"], dev, S, "MVTec")
    how = dict(batch_size=8, use_iqm=False, f1_max=True, device_metrics=True, return_masks=True)
    if tiles is not None:
        how.update(tiles=tiles, tile_overlap=14)
    if defects is not None:
        how.update(defects=defects)
    rows, details, overlays, masks = {}, {}, {}, {}
    for encoder in EP.ENCODERS:
        save = str(h["tmp"] / f"{encoder}-{side}")
        overlays[encoder], masks[encoder] = {}, {}
        rows[encoder], details[encoder] = EP.evaluate(*where, **how, save_path=save, overlay=0.5, overlay_encoder=encoder,
                                                      masks_png=True, overlay_written=overlays[encoder],
                                                      masks_written=masks[encoder])
    want_rows = EO.evaluate(*where, **how, save_path=str(h["tmp"] / f"plain-{side}"), overlay=None)[0]
    assert rows["device"] == rows["pillow"] == want_rows
    key = "kept masks" if defects is not None else "masks"
    for c in h["classes"]:
        names = details["device"][c]["file_names"]
        for kind, written in (("overlays", overlays), ("masks", masks)):
            for encoder in EP.ENCODERS:
                folder = os.path.join(str(h["tmp"] / f"{encoder}-{side}"), kind, "MVTec", c)
                assert len(written[encoder][c]) == len(names) == len(os.listdir(folder))
                assert [os.path.basename(p) for p in written[encoder][c]] == [EO.overlay_name(n) for n in names]
        for a, b in zip(overlays["device"][c], overlays["pillow"][c]):
            pa, pb = decode(a, "RGB"), decode(b, "RGB")
            assert pa.shape == (3 * side, side, 3) and np.array_equal(pa, pb), a
        kept = details["device"][c][key]
        kept = (kept.cpu().numpy() if torch.is_tensor(kept) else np.asarray(kept)).reshape(len(names), side, side)
        assert kept.any()
        for i, (a, b) in enumerate(zip(masks["device"][c], masks["pillow"][c])):
            want = (kept[i] != 0).astype(np.uint8) * 255
            assert np.array_equal(decode(a, "L"), want) and np.array_equal(decode(b, "L"), want), a
    # masks without overlays
    only = {}
    save = str(h["tmp"] / f"masks-only-{side}")
    how.pop("return_masks")
    got = EP.evaluate(*where, **how, save_path=save, overlay_encoder="device", masks_png=True, masks_written=only)
    assert got == want_rows and not os.path.exists(os.path.join(save, "overlays"))
    for c in h["classes"]:
        assert all(np.array_equal(decode(a, "L"), decode(b, "L")) for a, b in zip(only[c], masks["device"][c]))
