"""Heat-map overlays without a GPU: forward_utils.render_overlays_host against the independent definition of
tests/overlay_cases.py over the grid, the colour tables, the byte round trip, the blend's ends, the library's symbols,
struct and refusals, engine's host-side checks, csrc/overlay_plan.h in a host program under ASan + UBSan, eval_overlay's
parser and its path without --overlay, and evaluate_rows' after_class keyword."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import overlay_cases as OC
from aaclip_hip import _lib, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "aa-clip-iqm_amd", "csrc")
ENTRY = "aaclip_overlay_render"


# ------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("size", OC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_host_definition_is_the_cases_definition_on_the_grid(size):
    import forward_utils as FU
    for case in OC.grid(size):
        frames, maps, kw = OC.arguments(case)
        want = OC.expected(case)
        got = FU.render_overlays_host(frames, maps, **kw)
        n = len(case["panels"])
        assert got.dtype == np.uint8 and got.shape == want.shape == (case["B"], n * case["H"], case["W"], 3)
        assert np.array_equal(got, want), OC.case_id(case)


@pytest.mark.parametrize("name", OC.SPECIALS)
def test_the_host_definition_on_the_special_cases(name):
    import forward_utils as FU
    for case in (c for c in OC.specials() if c["special"] == name):
        frames, maps, kw = OC.arguments(case)
        want = OC.expected(case)
        assert np.array_equal(FU.render_overlays_host(frames, maps, **kw), want), OC.case_id(case)
        H = case["H"]
        heat, truth = want[:, H:2 * H].reshape(-1, 3), want[:, 2 * H:].reshape(-1, 3)
        white, green = np.all(heat == OC.PRED_COLOUR, axis=1), np.all(truth == OC.TRUTH_COLOUR, axis=1)
        if name == "full masks":                                    # nothing is zero anywhere: no contour at T = 8
            assert not FU.overlay_contour_host(kw["pred"], 8).any() and not OC.contour(kw["truth"], 8).any()
        if name == "single pixel":                                  # a lone pixel is all contour
            assert FU.overlay_contour_host(kw["pred"], 1).sum() == case["B"] and white.sum() >= case["B"]
        if name == "border region":                                 # pixels outside the image count as nothing
            c = OC.contour(kw["pred"], 2)
            assert not c[:, 0].any() and c[:, 1:3].all() and green.any()
        if name == "no range record":
            assert np.array_equal(want, OC.render(frames, maps, **dict(kw, range_record=OC.record(0.0, 1.0))))


def test_the_grid_covers_what_it_promises():
    cases = [c for size in OC.SIZES for c in OC.grid(size)]
    assert len(cases) == 256 and len({OC.case_id(c) for c in cases}) == 256
    for size in OC.SIZES:
        mine = [c for c in cases if (c["H"], c["W"]) == size]
        assert {(c["T"], c["pred"], c["truth"], c["B"]) for c in mine} == \
            {(t, p, g, b) for t in OC.THICKNESS for p, g in OC.MASKS for b in OC.BATCHES}
        assert {c["alpha256"] for c in mine} == set(OC.ALPHAS) and {c["panels"] for c in mine} == set(OC.SUBSETS)
    assert len(OC.SUBSETS) == 7 and len(list(OC.specials())) == 2 * len(OC.SPECIALS)
    d = OC.inputs(3, 37, 37)
    assert OC.inputs(3, 37, 37) is d and not d["frames"].flags.writeable            # computed once, left unchanged
    assert np.isnan(d["frames"]).any() and np.isinf(d["frames"]).any() and set(np.unique(d["pred"])) >= {0, 1, 255}
    assert float(d["maps"].min()) < 0.0 and float(d["maps"].max()) > 1.0


def test_the_colour_tables_are_their_integer_formulas():
    jet, gray = engine.overlay_lut("jet").numpy(), engine.overlay_lut("gray").numpy()
    assert jet.dtype == gray.dtype == np.uint8 and jet.shape == gray.shape == (256, 3)
    for i in range(256):
        assert tuple(gray[i]) == (i, i, i)
        assert tuple(jet[i]) == tuple(min(max(383 - abs(4 * i - 255 * c), 0), 255) for c in (3, 2, 1))
    assert tuple(jet[0]) == (0, 0, 128) and tuple(jet[128]) == (130, 255, 126) and tuple(jet[255]) == (128, 0, 0)
    assert len({tuple(r) for r in jet}) == 256
    assert np.array_equal(jet, OC.jet()) and np.array_equal(gray, OC.gray())
    # the classic clamp(1.5 - |4 v - c|) ramp at v = i / 255, times 255, is (765 - 2 |4 i - 255 c|) / 2: an odd numerator,
    # so EVERY ramp value is a .5 tie, floating point lands on either side of it, and the integer form (half up) defines it
    twice = 765 - 2 * np.abs(4 * np.arange(256)[:, None] - 255 * np.array([3, 2, 1])[None, :])
    assert np.all(twice % 2 == 1) and np.array_equal(np.clip((twice + 1) // 2, 0, 255), jet)
    ramp = 255 * (1.5 - np.abs(4 * np.arange(256)[:, None] / 255 - np.array([3, 2, 1])[None, :]))
    assert np.allclose(ramp, twice / 2) and np.abs(np.clip(np.rint(ramp), 0, 255) - jet).max() == 1       # ties, some lost
    with pytest.raises(ValueError, match="hot"):
        engine.overlay_lut("hot")


def test_every_byte_comes_back_through_the_frame_byte():
    lut = engine._normalise_lut(engine.CLIP_MEAN, engine.CLIP_STD).numpy()                # [3, 256]
    assert np.array_equal(lut.view(np.uint32), np.stack([OC.normalise_lut_value(np.arange(256), c) for c in range(3)]).view(np.uint32))
    frames = np.ascontiguousarray(lut.reshape(1, 3, 16, 16))
    want = np.arange(256).reshape(16, 16)
    assert all(np.array_equal(OC.frame_bytes(frames)[0, ..., c], want) for c in range(3))
    worst = 0.0
    for c in range(3):
        v = ((lut[c] * np.float32(OC.CLIP_STD[c])) + np.float32(OC.CLIP_MEAN[c])) * np.float32(255)
        worst = max(worst, float(np.abs(v.astype(np.float64) - np.arange(256)).max()))
    print(f"worst distance of a restored byte from its integer: {worst:.2e}")
    assert worst < 1e-4


def test_the_ends_of_the_blend():
    import forward_utils as FU
    d = OC.inputs(3, 37, 37)
    F = OC.frame_bytes(d["frames"]).astype(np.uint8)
    q = OC.heat_bytes(d["maps"], d["record"])
    assert q.min() == 0 and q.max() == 255
    heat = lambda a: FU.render_overlays_host(d["frames"], d["maps"], d["record"], alpha256=a, panels=("heat",))
    assert np.array_equal(heat(0), OC.jet()[q]) and np.array_equal(heat(256), F)
    truth = lambda a: FU.render_overlays_host(d["frames"], d["maps"], d["record"], truth=d["truth"], alpha256=a, thickness=0,
                                              panels=("truth",))
    assert np.array_equal(truth(256), F)
    assert np.array_equal(truth(0), np.where((d["truth"] != 0)[..., None], np.array(OC.TRUTH_COLOUR, np.uint8), F))
    with pytest.raises(ValueError):
        FU.render_overlays_host(d["frames"], d["maps"], panels=("truth",))              # truth selected, no truth given
    with pytest.raises(ValueError):
        FU.render_overlays_host(d["frames"], d["maps"], panels=())
    assert FU.render_overlays_host(d["frames"], d["maps"]).shape == (3, 74, 37, 3)        # the default drops the truth panel
    assert np.array_equal(FU.render_overlays_host(d["frames"], d["maps"], {"min": d["maps"].min(), "max": d["maps"].max()}),
                          FU.render_overlays_host(torch.from_numpy(np.array(d["frames"])), d["maps"], torch.from_numpy(d["record"].copy())))


# ------------------------------------------------------------------------------------------------- the library
def err():
    return _lib.load().aaclip_last_error().decode()


def test_symbol_struct_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    assert ENTRY in _lib.SIGNATURES and getattr(lib, ENTRY) is not None and ENTRY + "(" in header
    assert lib.aaclip_version() == _lib.ABI_VERSION == 10                         # an addition: the ABI number stays
    assert int(re.search(r"#define\s+AACLIP_ABI_VERSION\s+(\d+)", header).group(1)) == 10
    body = re.search(r"typedef struct aaclip_overlay_plan \{(.*?)\} aaclip_overlay_plan;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*(?:\[3\])?\s*;", body)
    assert fields == [n for n, _ in _lib.OverlayPlan._fields_] == ["struct_bytes", "images", "height", "width", "panels",
                                                                  "alpha256", "thickness", "pred_colour", "truth_colour",
                                                                  "mean", "std", "stream"]
    assert _lib.OverlayPlan().struct_bytes == ctypes.sizeof(_lib.OverlayPlan) == 72
    assert [getattr(_lib.OverlayPlan, n).offset for n in ("images", "pred_colour", "truth_colour", "mean", "std", "stream")] == \
        [8, 32, 35, 40, 52, 64]
    proto = re.search(ENTRY + r"\s*\(([^()]*)\)\s*;", header).group(1)
    assert "stream" not in proto and proto.count(",") + 1 == len(_lib.SIGNATURES[ENTRY][1]) == 8     # the stream is in the plan
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "overlay.hip" in make and "overlay_plan.h" in make and "-ffp-contract=off" in make
    assert list(inspect.signature(engine.overlay_render).parameters) == [
        "frames", "maps", "range_record", "pred", "truth", "alpha", "lut", "thickness", "panels", "pred_colour", "truth_colour",
        "mean", "std"]
    sig = inspect.signature(engine.overlay_render).parameters
    assert sig["alpha"].default == 0.5 and sig["lut"].default == "jet" and sig["thickness"].default == 1
    assert sig["pred_colour"].default == (255, 255, 255) and sig["truth_colour"].default == (0, 255, 0)
    assert sig["mean"].default == engine.CLIP_MEAN and sig["std"].default == engine.CLIP_STD


def test_bad_calls_are_refused_before_any_launch():
    """no GPU here: every check precedes the launch, so a refusal needs none; plausible device addresses stand in"""
    lib = _lib.load()
    fn = getattr(lib, ENTRY)
    F, M, R, P, G, L, OUT = (0x7f0000001000 + i * 0x40000000 for i in range(7))

    def plan(**kw):
        p = _lib.OverlayPlan()
        p.images, p.height, p.width, p.panels, p.alpha256, p.thickness = 2, 70, 70, 7, 128, 1
        for c in range(3):
            p.mean[c], p.std[c] = engine.CLIP_MEAN[c], engine.CLIP_STD[c]
        for k, v in kw.items():
            if k.startswith("std"):
                p.std[int(k[3])] = v
            else:
                setattr(p, k, v)
        return p

    def refused(p, args, msg):
        assert fn(None if p is None else ctypes.byref(p), *args) == -1, msg
        assert err().startswith(ENTRY + ":") and msg in err(), (msg, err())

    good = (F, M, R, P, G, L, OUT)
    for kw, msg in ((dict(struct_bytes=64), "struct_bytes"), (dict(struct_bytes=0), "struct_bytes"),
                    (dict(struct_bytes=80), "struct_bytes"), (dict(images=-1), "images"), (dict(height=0), "height"),
                    (dict(height=-3), "height"), (dict(width=0), "width"), (dict(panels=0), "panels"), (dict(panels=8), "panels"),
                    (dict(alpha256=-1), "alpha256"), (dict(alpha256=257), "alpha256"), (dict(thickness=-1), "thickness"),
                    (dict(thickness=9), "thickness"), (dict(std0=0.0), "std"), (dict(std1=-0.5), "std"),
                    (dict(std2=float("inf")), "std"), (dict(std0=float("nan")), "std"),
                    (dict(images=2 ** 31 - 1, height=2 ** 31 - 1, width=2 ** 31 - 1), "too large"),
                    (dict(images=1 << 21, height=1 << 18, width=1 << 18), "too large")):
        refused(plan(**kw), good, msg)
    refused(None, good, "null plan")
    for i in (0, 1, 5, 6):                                                          # frames, maps, lut, out
        refused(plan(), tuple(None if j == i else a for j, a in enumerate(good)), "null pointer")
    refused(plan(), (F, M, R, P, None, L, OUT), "truth")                           # the truth panel without a truth mask
    assert fn(ctypes.byref(plan(images=0, panels=3)), F, M, None, None, None, L, OUT) == 0       # ... none needed without it
    refused(plan(), (F + 2, M, R, P, G, L, OUT), "aligned")
    refused(plan(), (F, M + 1, R, P, G, L, OUT), "aligned")
    refused(plan(), (F, M, R + 4, P, G, L, OUT), "aligned")
    for other, size in ((F, 2 * 3 * 70 * 70 * 4), (M, 2 * 70 * 70 * 4), (R, 24), (P, 2 * 70 * 70), (G, 2 * 70 * 70), (L, 768)):
        refused(plan(), (F, M, R, P, G, L, other + size - 1), "overlap")           # out starts on the input's last byte
        refused(plan(), (F, M, R, P, G, L, other - 2 * 3 * 70 * 70 * 3 + 1), "overlap")      # out ends on its first
    assert fn(ctypes.byref(plan(images=0)), *good) == 0                             # nothing to do: no launch, no error
    assert fn(ctypes.byref(plan(images=0)), F, M, None, None, G, L, OUT + 1) == 0  # any output alignment, masks optional
    refused(plan(images=0, thickness=9), good, "thickness")                         # ... but the plan is still checked
    refused(plan(images=0), (F, M, R, P, G, L, None), "null pointer")


def test_engine_refuses_on_the_host():
    f, m = torch.zeros(2, 3, 7, 5), torch.zeros(2, 7, 5)
    with pytest.raises(ValueError, match="GPU"):
        engine.overlay_render(f, m)
    with pytest.raises(ValueError, match="hot"):
        engine.overlay_lut("hot")
    assert engine.overlay_panels(None, True) == ("frame", "heat", "truth") and engine.overlay_panels(None, False) == ("frame", "heat")
    assert engine.overlay_panels(("truth", "frame"), True) == ("frame", "truth") and engine.overlay_panels("heat", False) == ("heat",)
    for bad, has_truth in (((), True), (("heat", "heat"), True), (("edges",), True), (("truth",), False)):
        with pytest.raises(ValueError):
            engine.overlay_panels(bad, has_truth)


def test_overlay_plan_header_under_the_sanitizers(tmp_path):
    """csrc/overlay_plan.h as overlay.hip and the C ABI use it, in a host program of its own with ASan + UBSan: refusals,
    tile geometry and LDS layout, the store phase's chunks, 64-bit offsets, blend, clamp and window against brute force;
    no report from either sanitizer"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "overlay_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(CSRC, "overlay_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime of the host compiler is not installed: " + build.stderr.strip()[-200:])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and not run.stderr, (run.returncode, run.stdout, run.stderr)


# ------------------------------------------------------------------------------------------------- the script
def test_eval_overlay_parser_and_the_path_without_overlay(monkeypatch, capsys):
    import eval_last as EL
    import eval_overlay as EO
    import eval_tiled as ET
    parse = EO.build_parser().parse_args
    a = parse([])
    assert a.overlay is None and a.overlay_limit is None and a.overlay_thickness == 1 and a.overlay_colormap == "jet"
    assert parse(["--overlay"]).overlay == 0.5 and parse(["--overlay", "0.25"]).overlay == 0.25
    a = parse(["--overlay", "--overlay_limit", "5", "--overlay_thickness", "3", "--overlay_colormap", "gray"])
    assert (a.overlay_limit, a.overlay_thickness, a.overlay_colormap) == (5, 3, "gray")
    defaults = {k: v for k, v in vars(parse([])).items() if not k.startswith("overlay")}
    assert defaults == vars(ET.build_parser().parse_args([]))                          # eval_tiled.py's arguments stay
    rows = [{"class name": "a", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0}] * 2
    calls = []

    def fake_run(parser, argv=None, table=None, finish=None):
        calls.append((argv, table, finish is not None))
        print((table or EL.format_table)(rows))
        return rows

    monkeypatch.setattr(EL, "run", fake_run)
    for argv in ([], ["--f1max"], ["--support", "4", "--defects"], ["--overlay_limit", "3"], ["--overlay_colormap", "gray"]):
        tiled_argv = [v for v in argv if not v.startswith("--overlay_") and v not in ("3", "gray")]
        del calls[:]
        assert ET.main(list(tiled_argv)) == rows
        want_calls, want_out = list(calls), capsys.readouterr().out
        del calls[:]
        assert EO.main(list(argv)) == rows
        assert capsys.readouterr().out == want_out and want_out                          # byte for byte
        assert [c[1:] for c in calls] == [c[1:] for c in want_calls]
    del calls[:]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for bad in (["--overlay", "1.5"], ["--overlay", "-0.1"], ["--overlay", "--overlay_thickness", "9"],
                ["--overlay", "--overlay_thickness", "-1"], ["--overlay", "--overlay_limit", "-1"],
                ["--overlay", "--overlay_colormap", "hot"], ["--overlay", "--tiles", "0"], ["--overlay", "--support", "0"]):
        with pytest.raises(SystemExit):
            EO.main(bad)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        EO.main(["--overlay"])
    assert not calls                                                        # none of the refused calls reached a run
    sig, lead = inspect.signature(EO.evaluate).parameters, inspect.signature(ET.evaluate).parameters
    assert list(sig)[:len(lead)] == list(lead) and all(sig[k].default == lead[k].default for k in lead)
    assert list(sig)[len(lead):] == ["overlay", "overlay_limit", "overlay_thickness", "overlay_colormap", "overlay_written"]
    assert sig["overlay"].default is None and callable(EO.write_overlays)


def test_evaluate_without_overlay_is_eval_tiled(monkeypatch):
    import eval_overlay as EO
    import eval_tiled as ET
    seen, keywords = [], list(inspect.signature(ET.evaluate).parameters)[6:]
    monkeypatch.setattr(ET, "evaluate", lambda *a, **k: seen.append((a, k)) or "rows")
    assert EO.evaluate("m", "sets", "text", "dev", 70, "MVTec", batch_size=4, f1_max=True, tiles=2, tile_overlap=14) == "rows"
    (a, k), = seen
    assert a == ("m", "sets", "text", "dev", 70, "MVTec") and set(k) == set(keywords)       # every keyword of it, no other
    assert k["batch_size"] == 4 and k["f1_max"] is True and k["tiles"] == 2 and k["tile_overlap"] == 14
    with pytest.raises(ValueError, match="save_path"):
        EO.evaluate("m", "sets", "text", "dev", 70, "MVTec", overlay=0.5)
    with pytest.raises(ValueError):
        EO.evaluate("m", "sets", "text", "dev", 70, "MVTec", overlay=1.5, save_path="x")


def test_overlay_names_and_duplicates(tmp_path):
    import eval_overlay as EO
    assert EO.overlay_name("bottle/test/broken_large/000.png") == "broken_large_000.png"
    assert EO.overlay_name("a\\b\\good\\7.jpeg") == "good_7.png" and EO.overlay_name("x.bmp") == "x.png"
    paths = EO.overlay_paths("dir", ["c/test/good/000.png", "c/test/bad/000.png"])
    assert paths == [os.path.join("dir", "good_000.png"), os.path.join("dir", "bad_000.png")]
    with pytest.raises(ValueError, match="good_000.png"):
        EO.overlay_paths("dir", ["c/test/good/000.png", "d/other/good/000.jpg"])
    # two images of a class with one name: refused before anything is written
    folder = tmp_path / "overlays"
    maps = np.zeros((2, 5, 5), np.float32)
    with pytest.raises(ValueError, match="both be written"):
        EO.write_overlays(str(folder), [0, 1], maps, maps, ["a/good/0.png", "b/good/0.png"], None, "cpu")
    assert not folder.exists()


def test_after_class_none_leaves_evaluate_rows_as_it_was(monkeypatch):
    import eval_last as EL
    import eval_tiled as ET
    assert inspect.signature(EL.evaluate_rows).parameters["after_class"].default is None
    assert inspect.signature(ET.evaluate_tiled).parameters["after_class"].default is None
    assert list(inspect.signature(EL.evaluate_rows).parameters)[-1] == "after_class"

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 3

        def __getitem__(self, i):
            return {"image": torch.zeros(3, 4, 4), "mask": torch.zeros(1, 4, 4), "label": i % 2, "file_name": f"c/test/x/{i}.png",
                    "class_name": "c"}

    def fake_predictions(model, class_text_embeddings, test_loader, device, img_size, dataset, use_iqm, on_device):
        n = len(test_loader.dataset)
        maps = np.arange(n * 16, dtype=np.float32).reshape(n, 4, 4) / (n * 16)
        masks = (maps > 0.5).astype(np.float32)[:, None]
        return masks, np.array([0, 1, 1][:n]), maps, maps.reshape(n, -1).max(axis=1), [f"c/test/x/{i}.png" for i in range(n)]

    monkeypatch.setattr(EL, "get_predictions", fake_predictions)
    where = (None, {"c": DS()}, {"c": None}, "cpu", 4, "MVTec")
    plain = EL.evaluate_rows(*where, batch_size=2)
    assert EL.evaluate_rows(*where, batch_size=2, after_class=None) == plain
    seen = []
    got = EL.evaluate_rows(*where, batch_size=2, after_class=lambda *a: seen.append(a))
    assert got == plain and len(seen) == 1
    name, ds, masks, labels, preds, scores, names, details = seen[0]
    assert name == "c" and len(ds) == 3 and masks.shape == (3, 1, 4, 4) and preds.shape == (3, 4, 4) and details is None
    assert names == [f"c/test/x/{i}.png" for i in range(3)] and len(labels) == len(scores) == 3
    details_out, seen = {}, []
    rows = EL.evaluate_rows(*where, batch_size=2, f1_max=True, details=details_out, return_masks=True,
                            after_class=lambda *a: seen.append(a))
    assert rows == EL.evaluate_rows(*where, batch_size=2, f1_max=True, details={}, return_masks=True)
    assert seen[0][-1] is details_out["c"] and seen[0][-1]["masks"].shape == (3, 4, 4)      # the row is computed by then
