"""PNG encoding without a GPU: forward_utils.png_encode_host over the grid of tests/png_cases.py against zlib (the streams
inflate to the numpy filter definition's bytes, the sizes meet the bar against zlib's Z_RLE strategy) and Pillow (the files
decode to the input); what each case of the grid is there for; the library's symbols, struct and refusals; engine's
host-side checks; csrc/png_plan.h in a host program under ASan + UBSan, whose encoder also gives the definition's bytes;
eval_png's parser, its path without the new flags and the masks' names."""
import ctypes
import inspect
import io
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

import png_cases as PC
from aaclip_hip import _lib, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "aa-clip-iqm_amd", "csrc")
ENTRY = "aaclip_png_encode"
CASES = PC.cases()


@pytest.fixture(scope="module")
def encoded():
    """name -> (pixels, payload, offsets, info) of the host definition, computed once"""
    import forward_utils as FU
    out = {}
    for name, pixels in CASES:
        info = {}
        payload, offsets = FU.png_encode_host(pixels, info)
        out[name] = (pixels, payload, offsets, info)
    return out


def err():
    return _lib.load().aaclip_last_error().decode()


# ------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_the_definition_against_zlib_and_pillow(encoded, name):
    import forward_utils as FU
    from PIL import Image
    pixels, payload, offsets, info = encoded[name]
    images, H, W, C = pixels.shape
    geom = engine.png_segments(H, W, C)
    assert len(offsets) == images + 1 and offsets[0] == 0 and offsets[-1] == payload.size and payload.dtype == np.uint8
    files = FU.png_files(payload, offsets, H, W, C)
    assert len(files) == images
    for i in range(images):
        filtered = FU.png_filter_host(pixels[i])
        assert filtered.shape == (H, geom["row_bytes"]) and filtered[:, 0].max() <= 4
        stream = payload[offsets[i]:offsets[i + 1]].tobytes()
        assert stream[:2] == b"\x78\x01" and stream[-6:-4] == b"\x03\x00"
        assert zlib.decompress(stream) == filtered.tobytes(), (name, i)
        size, reference = len(stream), PC.zrle_size(filtered)
        print(f"{name}[{i}]: {size} bytes, zRLE {reference}, {geom['segments']} segments")
        assert size <= PC.size_bar(filtered, geom["segments"]), (name, i, size, reference)
        assert size <= geom["capacity"]
        with Image.open(io.BytesIO(files[i])) as im:
            assert im.mode == ("RGB" if C == 3 else "L") and im.size == (W, H)
            assert np.array_equal(np.array(im).reshape(H, W, C), pixels[i]), (name, i)
    if images:
        assert np.array_equal(FU.png_encode_host(torch.from_numpy(pixels))[0], payload)      # a host tensor is taken too
    if C == 1:
        assert np.array_equal(FU.png_encode_host(pixels[..., 0])[0], payload)                # [images, H, W] is C = 1


def test_the_grid_covers_what_it_promises(encoded):
    import forward_utils as FU
    segments = lambda name: engine.png_segments(*encoded[name][0].shape[1:])["segments"]
    for name, (pixels, payload, offsets, info) in encoded.items():
        if name in PC.STORED:
            assert info.get("huffman", 0) == 0 and info["stored"] == segments(name), name
            assert offsets[-1] == pixels.shape[0] * (8 + 5 * segments(name)) + sum(FU.png_filter_host(p).size for p in pixels)
        elif pixels.shape[0]:
            assert info.get("stored", 0) == 0 and info["huffman"] == pixels.shape[0] * segments(name), name
    assert engine.png_segments(83, 131, 3)["rows_per_segment"] == 83
    assert [segments(f"noise-{h}x131x3") for h in (83, 84, 166, 97, 150)] == [1, 2, 2, 2, 2]
    assert segments("zeros-700x700x3") == 47 and segments("wide-3x10000x3") == 3 and segments("mask-518x518x1") == 9
    # all zeros: a literal, matches of 258 and what is left of the segment, end-of-block
    zeros = encoded["zeros-700x700x3"]
    assert zeros[2][-1] < 47 * 64 and zeros[3]["limited"] == 0
    # the 15-bit limit is taken, and the stream still inflates (above)
    assert encoded["limit-15"][3]["limited"] > 0 and encoded["limit-15"][3]["huffman"] == 1
    assert all(info.get("limited", 0) == 0 for name, (_, _, _, info) in encoded.items() if name != "limit-15")
    # the run lengths: both ends of the match rule, token by token
    where, kind, length = FU.png_tokens_host(np.concatenate(([1], PC.run_lengths().reshape(-1))))
    tokens = [(int(k), int(n)) for k, n in zip(kind, length)][1:]
    lit, match = (1, 0), lambda n: (2, n)
    assert tokens == ([lit, lit] + [lit, lit, lit] + [lit, match(3)] + [lit, match(258)] + [lit, match(258), lit]
                      + [lit, match(258), lit, lit] + [lit, match(258), match(3)] + [lit, match(258), match(258)])
    # the batch: three different images, three different streams
    pixels, payload, offsets, _ = encoded["batch-3x64x48x3"]
    streams = [payload[a:b].tobytes() for a, b in zip(offsets[:-1], offsets[1:])]
    assert len(set(streams)) == 3
    for i in range(3):
        assert np.array_equal(FU.png_encode_host(pixels[i:i + 1])[0], np.frombuffer(streams[i], np.uint8))
    assert encoded["no-images"][1].size == 0 and encoded["no-images"][2] == [0]
    with pytest.raises(ValueError, match="32768"):
        FU.png_encode_host(np.zeros((1, 1, PC.REFUSED_WIDTH, 3), np.uint8))
    assert FU.png_encode_host(np.zeros((1, 1, PC.REFUSED_WIDTH - 1, 3), np.uint8))[1][-1] > 8
    for bad in (np.zeros((1, 4, 4, 2), np.uint8), np.zeros((1, 4, 4, 3), np.int32), np.zeros((4, 4), np.uint8)):
        with pytest.raises(ValueError):
            FU.png_encode_host(bad)


def test_the_code_builder():
    import forward_utils as FU
    rng = np.random.default_rng(3)
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for counts, limit in ([(list(rng.integers(0, 50, 286)), 15) for _ in range(5)] + [(fib + [0] * 256, 15), (fib[:12] + [0] * 7, 7),
                          ([0] * 19, 7), ([0, 0, 5] + [0] * 16, 7), ([1] * 286, 15), ([1] * 19, 7)]):
        lengths, limited = FU.png_code_lengths_host(counts, limit)
        used = [n for n in lengths if n]
        assert max(lengths) <= limit and sum(2 ** (limit - n) for n in used) == 2 ** limit, (counts, lengths)      # Kraft
        assert all(n > 0 for n, c in zip(lengths, counts) if c) and len(used) == max(2, sum(1 for c in counts if c))
        assert (limited > 0) == (counts[:30] == fib or counts[:12] == fib[:12] and limit == 7)
        order = sorted(range(len(counts)), key=lambda s: (counts[s], s))
        assert all(lengths[a] >= lengths[b] for a, b in zip(order, order[1:]) if counts[a] and counts[b])
    assert FU.png_code_lengths_host([0] * 19, 7)[0][:3] == [1, 1, 0]                  # filled up with the lowest symbols
    assert FU.png_code_lengths_host([0, 0, 5] + [0] * 16, 7)[0][:3] == [1, 0, 1]
    assert FU._png_length_tokens([3] + [0] * 150 + [2, 0, 0, 1] + [0] * 10 + [4] + [0] * 3) == \
        [(3, 0, 0), (18, 7, 127), (18, 7, 1), (2, 0, 0), (0, 0, 0), (0, 0, 0), (1, 0, 0), (17, 3, 7), (4, 0, 0), (17, 3, 0)]


# ------------------------------------------------------------------------------------------------- the library
def test_symbols_struct_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name in (ENTRY, "aaclip_png_workspace_bytes", "aaclip_png_capacity_bytes"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert lib.aaclip_version() == _lib.ABI_VERSION == 10                         # additions: the ABI number stays
    assert int(re.search(r"#define\s+AACLIP_ABI_VERSION\s+(\d+)", header).group(1)) == 10
    body = re.search(r"typedef struct aaclip_png_plan \{(.*?)\} aaclip_png_plan;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in _lib.PngPlan._fields_] == ["struct_bytes", "images", "height", "width", "channels", "stream"]
    assert _lib.PngPlan().struct_bytes == ctypes.sizeof(_lib.PngPlan) == 32
    assert [getattr(_lib.PngPlan, n).offset for n in ("images", "height", "width", "channels", "stream")] == [8, 12, 16, 20, 24]
    proto = re.search(ENTRY + r"\s*\(([^()]*)\)\s*;", header).group(1)
    assert "stream" not in proto and proto.count(",") + 1 == len(_lib.SIGNATURES[ENTRY][1]) == 7     # the stream is in the plan
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "png.hip" in make and "png_plan.h" in make
    assert list(inspect.signature(engine.png_encode).parameters) == ["pixels"]
    assert list(inspect.signature(engine.png_segments).parameters) == ["H", "W", "C"]


def test_the_derived_sizes():
    lib = _lib.load()

    def sizes(images, H, W, C, **kw):
        p = _lib.PngPlan()
        p.images, p.height, p.width, p.channels = images, H, W, C
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.aaclip_png_capacity_bytes(ctypes.byref(p)), lib.aaclip_png_workspace_bytes(ctypes.byref(p))

    for images, H, W, C in ((1, 1, 1, 1), (3, 64, 48, 3), (64, 1554, 518, 3), (16, 2772, 924, 3), (3, 518, 518, 1), (2, 3, 10000, 3),
                            (1, 1, 10922, 3), (5, 40000, 1, 1)):
        g = engine.png_segments(H, W, C)
        assert g["row_bytes"] == 1 + W * C and g["rows_per_segment"] == max(1, 32768 // g["row_bytes"])
        assert g["segments"] == -(-H // g["rows_per_segment"]) and g["capacity"] == 8 + H * g["row_bytes"] + 5 * g["segments"]
        cap, ws = sizes(images, H, W, C)
        assert cap == images * g["capacity"]
        slot = (min(H, g["rows_per_segment"]) * g["row_bytes"] + 5 + 15) // 16 * 16
        assert ws == images * g["segments"] * (slot + 16)
    assert engine.png_segments(1554, 518, 3) == {"row_bytes": 1555, "rows_per_segment": 21, "segments": 74,
                                                 "stream_bytes": 1554 * 1555, "capacity": 8 + 1554 * 1555 + 370}
    assert sizes(0, 5, 5, 3) == (0, 0) and sizes(0, 0, 0, 1) == (0, 0)
    for bad in ((1, 4, 4, 2), (-1, 4, 4, 3), (1, 0, 4, 3), (1, 4, 0, 1), (1, 1, PC.REFUSED_WIDTH, 3), (1, 1, 32768, 1),
                (2 ** 31 - 1, 2 ** 31 - 1, 10922, 3)):
        assert sizes(*bad) == (0, 0), bad                                              # a refused plan: 0 bytes of both
    assert sizes(1, 4, 4, 3, struct_bytes=24) == (0, 0)
    assert lib.aaclip_png_capacity_bytes(None) == 0 and lib.aaclip_png_workspace_bytes(None) == 0
    for bad in ((4, 4, 2), (-1, 4, 3), (4, -1, 1), (1, PC.REFUSED_WIDTH, 3)):
        with pytest.raises(ValueError):
            engine.png_segments(*bad)


def test_bad_calls_are_refused_before_any_launch():
    """no GPU here: every check precedes the launch, so a refusal needs none; plausible device addresses stand in"""
    lib = _lib.load()
    fn = getattr(lib, ENTRY)
    PIX, WS, PAY, OFF = (0x7f0000001000 + i * 0x40000000 for i in range(4))

    def plan(**kw):
        p = _lib.PngPlan()
        p.images, p.height, p.width, p.channels = 2, 70, 70, 3
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    cap, ws = lib.aaclip_png_capacity_bytes(ctypes.byref(plan())), lib.aaclip_png_workspace_bytes(ctypes.byref(plan()))
    assert cap == 2 * (8 + 70 * 211 + 5) and ws > 2 * 70 * 211

    def refused(p, args, msg):
        assert fn(None if p is None else ctypes.byref(p), *args) == -1, msg
        assert err().startswith(ENTRY + ":") and msg in err(), (msg, err())

    good = (PIX, WS, ws, PAY, cap, OFF)
    for kw, msg in ((dict(struct_bytes=24), "struct_bytes"), (dict(struct_bytes=0), "struct_bytes"),
                    (dict(struct_bytes=40), "struct_bytes"), (dict(images=-1), "images"), (dict(height=-3), "height"),
                    (dict(width=-1), "width"), (dict(height=0), "height"), (dict(width=0), "width"), (dict(channels=0), "channels"),
                    (dict(channels=2), "channels"), (dict(channels=4), "channels"),
                    (dict(width=PC.REFUSED_WIDTH), "32768"), (dict(width=32768, channels=1), "32768"),
                    (dict(width=2 ** 31 - 1), "32768"),
                    (dict(images=2 ** 31 - 1, height=2 ** 31 - 1, width=10922), "too large"),
                    (dict(images=1 << 30, height=1 << 30, width=1, channels=1), "too large")):
        refused(plan(**kw), good, msg)
    refused(None, good, "null plan")
    for i in (0, 1, 3, 5):                                                          # pixels, workspace, payload, offsets
        refused(plan(), tuple(None if j == i else a for j, a in enumerate(good)), "null pointer")
    refused(plan(), (PIX, WS, ws - 1, PAY, cap, OFF), "workspace too small")
    refused(plan(), (PIX, WS, 0, PAY, cap, OFF), "workspace too small")
    refused(plan(), (PIX, WS, ws, PAY, cap - 1, OFF), "capacity too small")
    refused(plan(), (PIX, WS + 8, ws, PAY, cap, OFF), "aligned")
    refused(plan(), (PIX, WS, ws, PAY, cap, OFF + 4), "aligned")
    pixel_bytes = 2 * 70 * 70 * 3
    refused(plan(), (PIX, WS, ws, PIX + pixel_bytes - 1, cap, OFF), "overlap")      # payload starts on the pixels' last byte
    refused(plan(), (PIX, WS, ws, PIX - cap + 1, cap, OFF), "overlap")              # ... ends on their first
    refused(plan(), (PIX, WS, ws, PAY, cap, PIX + 8), "overlap")                    # offsets inside the pixels
    refused(plan(), (PIX, WS, ws, PAY, cap, PIX - 16), "overlap")                   # their last word on the first pixel
    assert fn(ctypes.byref(plan(images=0)), *good) == 0                             # nothing to do: no launch, no error
    assert fn(ctypes.byref(plan(images=0, height=0, width=0)), PIX + 1, None, 0, None, 0, None) == 0
    refused(plan(images=0, channels=2), good, "channels")                           # ... but the plan is still checked


def test_engine_refuses_on_the_host():
    pixels = torch.zeros(2, 7, 5, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        engine.png_encode(pixels)
    with pytest.raises(ValueError, match="GPU"):
        engine.png_encode(pixels.numpy())


def test_png_plan_header_under_the_sanitizers(tmp_path, encoded):
    """csrc/png_plan.h as png.hip and the C ABI use it, in a host program of its own with ASan + UBSan: its encoder against
    a naive filter, a sequential token parse at run lengths 1 .. 600, the Kraft sum and the limits of the code builder, the
    Adler byte loop, a small inflate, the plan's refusals and 64-bit offsets; no report from either sanitizer.  The same
    program's encoder then gives the host definition's bytes on the grid."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "png_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(CSRC, "png_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime of the host compiler is not installed: " + build.stderr.strip()[-200:])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and not run.stderr, (run.returncode, run.stdout, run.stderr)
    for name, (pixels, payload, offsets, _) in encoded.items():
        if pixels.shape[0] == 0:
            continue
        raw, out = tmp_path / "pixels.raw", tmp_path / "streams.bin"
        raw.write_bytes(pixels.tobytes())
        run = subprocess.run([str(exe), "encode", *(str(v) for v in pixels.shape[1:]), str(raw), str(out)],
                             capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (name, run.stderr)
        data, streams, at = out.read_bytes(), [], 0
        while at < len(data):
            size = int.from_bytes(data[at:at + 8], "little")
            streams.append(data[at + 8:at + 8 + size])
            at += 8 + size
        assert [len(s) for s in streams] == list(np.diff(offsets)) and b"".join(streams) == payload.tobytes(), name


# ------------------------------------------------------------------------------------------------- the script
def test_eval_png_parser_and_the_path_without_the_new_flags(monkeypatch, capsys):
    import eval_last as EL
    import eval_overlay as EO
    import eval_png as EP
    parse = EP.build_parser().parse_args
    a = parse([])
    assert a.overlay_encoder == "pillow" and a.masks_png is False and a.overlay is None
    a = parse(["--overlay", "--overlay_encoder", "device", "--masks_png"])
    assert (a.overlay, a.overlay_encoder, a.masks_png) == (0.5, "device", True)
    with pytest.raises(SystemExit):
        parse(["--overlay_encoder", "zlib"])
    defaults = {k: v for k, v in vars(parse([])).items() if k not in ("overlay_encoder", "masks_png")}
    assert defaults == vars(EO.build_parser().parse_args([]))                          # eval_overlay.py's arguments stay
    rows = [{"class name": "a", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0}] * 2
    calls = []

    def fake_run(parser, argv=None, table=None, finish=None):
        calls.append((argv, table, finish is not None))
        print((table or EL.format_table)(rows))
        return rows

    monkeypatch.setattr(EL, "run", fake_run)
    for argv in ([], ["--f1max"], ["--support", "4", "--defects"], ["--overlay_limit", "3"], ["--overlay_encoder", "device"],
                 ["--overlay_encoder", "pillow", "--overlay_colormap", "gray"]):
        overlay_argv = [v for v in argv if v not in ("--overlay_encoder", "device", "pillow")]
        del calls[:]
        assert EO.main(list(overlay_argv)) == rows
        want_calls, want_out = list(calls), capsys.readouterr().out
        del calls[:]
        assert EP.main(list(argv)) == rows
        assert capsys.readouterr().out == want_out and want_out                          # byte for byte
        assert [c[1:] for c in calls] == [c[1:] for c in want_calls]
    # --overlay with the pillow encoder and no masks is eval_overlay's run
    seen = []
    monkeypatch.setattr(EO, "run", lambda parser, argv=None: seen.append(argv) or "overlay rows")
    assert EP.main(["--overlay", "0.25"]) == "overlay rows" and seen == [["--overlay", "0.25"]]
    monkeypatch.undo()
    monkeypatch.setattr(EL, "run", fake_run)
    del calls[:]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for bad in (["--masks_png", "--tiles", "0"], ["--masks_png", "--support", "0"], ["--masks_png", "--defects", "0"],
                ["--overlay", "1.5", "--overlay_encoder", "device"], ["--overlay", "--overlay_encoder", "device", "--overlay_thickness", "9"],
                ["--masks_png", "--overlay_limit", "-1"]):
        with pytest.raises(SystemExit):
            EP.main(bad)
    monkeypatch.setenv("WORLD_SIZE", "2")
    for refused in (["--masks_png"], ["--overlay", "--overlay_encoder", "device"]):
        with pytest.raises(SystemExit):
            EP.main(refused)
    assert not calls                                                        # none of the refused calls reached a run
    sig, lead = inspect.signature(EP.evaluate).parameters, inspect.signature(EO.evaluate).parameters
    assert list(sig)[:len(lead)] == list(lead) and all(sig[k].default == lead[k].default for k in lead)
    assert list(sig)[len(lead):] == ["overlay_encoder", "masks_png", "masks_written"]
    assert sig["overlay_encoder"].default == "pillow" and sig["masks_png"].default is False


def test_evaluate_without_the_new_flags_is_eval_overlay(monkeypatch):
    import eval_overlay as EO
    import eval_png as EP
    seen, keywords = [], list(inspect.signature(EO.evaluate).parameters)[6:]
    monkeypatch.setattr(EO, "evaluate", lambda *a, **k: seen.append((a, k)) or "rows")
    assert EP.evaluate("m", "sets", "text", "dev", 70, "MVTec", batch_size=4, f1_max=True, tiles=2, overlay=0.25,
                       save_path="x", overlay_limit=3) == "rows"
    assert EP.evaluate("m", "sets", "text", "dev", 70, "MVTec", overlay_encoder="device") == "rows"      # nothing to encode
    (a, k), (_, k2) = seen
    assert a == ("m", "sets", "text", "dev", 70, "MVTec") and set(k) == set(keywords)       # every keyword of it, no other
    assert k["batch_size"] == 4 and k["tiles"] == 2 and k["overlay"] == 0.25 and k["overlay_limit"] == 3 and k2["overlay"] is None
    with pytest.raises(ValueError, match="save_path"):
        EP.evaluate("m", "sets", "text", "dev", 70, "MVTec", masks_png=True)
    with pytest.raises(ValueError, match="save_path"):
        EP.evaluate("m", "sets", "text", "dev", 70, "MVTec", overlay=0.5, overlay_encoder="device")
    with pytest.raises(ValueError):
        EP.evaluate("m", "sets", "text", "dev", 70, "MVTec", overlay=1.5, overlay_encoder="device", save_path="x")
    with pytest.raises(ValueError, match="overlay_encoder"):
        EP.evaluate("m", "sets", "text", "dev", 70, "MVTec", overlay=0.5, overlay_encoder="zlib", save_path="x")


def test_mask_names_duplicates_and_the_pillow_masks(tmp_path):
    import eval_overlay as EO
    import eval_png as EP
    from PIL import Image
    names = ["bottle/test/broken_large/000.png", "bottle/test/good/000.png", "bottle/test/good/001.jpg"]
    masks = np.zeros((3, 9, 7), np.uint8)
    masks[0, 2:5, 1:4], masks[2, :, :] = 1, 3
    folder = tmp_path / "masks" / "MVTec" / "bottle"
    paths = EP.write_masks(str(folder), names, masks, "cpu", encoder="pillow", batch_size=2)
    assert paths == EO.overlay_paths(str(folder), names) == [str(folder / n) for n in ("broken_large_000.png", "good_000.png",
                                                                                        "good_001.png")]
    for path, mask in zip(paths, masks):
        with Image.open(path) as im:
            assert im.mode == "L" and np.array_equal(np.array(im), (mask != 0) * 255)
    assert EP.write_masks(str(folder), names, torch.from_numpy(masks), "cpu") == paths      # a host tensor is taken too
    other = tmp_path / "other"
    with pytest.raises(ValueError, match="both be written"):
        EP.write_masks(str(other), ["a/good/0.png", "b/good/0.png"], masks[:2], "cpu")
    with pytest.raises(ValueError, match="both be written"):
        EP.write_overlays(str(other), [0, 1], masks[:2], masks[:2].astype(np.float32), ["a/good/0.png", "b/good/0.png"], None,
                          "cpu", encoder="device")
    assert not other.exists()                                               # refused before anything is written
    with pytest.raises(ValueError, match="encoder"):
        EP.write_masks(str(other), names, masks, "cpu", encoder="zlib")
    with pytest.raises(ValueError, match="3 masks and 2"):
        EP.write_masks(str(other), names[:2], masks, "cpu")
    assert EP.write_masks(str(other), [], masks[:0], "cpu") == [] and not other.exists()
