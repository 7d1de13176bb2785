"""Tiled inference without a GPU: the definition's own properties (tests/tiled_cases.py), the fp32 definition against the
fp64 one, forward_utils.tile_stitch_host against both, the library's symbols, struct and host entry, csrc/tile_plan.h in
a host program under ASan + UBSan, and eval_tiled's parser and its path without --tiles."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import tiled_cases as TC
from aaclip_hip import _lib, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "aa-clip-iqm_amd", "csrc")
NEW_SYMBOLS = ("aaclip_tile_canvas", "aaclip_tile_gather", "aaclip_tile_stitch")


# ------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("S,G,O,frames,channels", list(TC.grid()))
def test_the_fp32_definition_is_within_the_bar_of_the_fp64_one(S, G, O, frames, channels):
    tiles, want = TC.case(S, G, O, frames, channels)
    got = TC.stitch(tiles, G, O, np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape == (frames, channels) + (TC.canvas_side(S, G, O),) * 2
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"fp32 definition ({S}, {G}, {O}) x{frames} ch{channels}: {err:.3e}, bar {TC.bar(tiles):.3e}")
    assert err <= TC.bar(tiles)
    one = TC.cover_count(S, G, O) == 1
    assert np.array_equal(got[..., one], want[..., one].astype(np.float32))      # a single tile's bits


def test_the_grid_covers_what_it_promises():
    cases = list(TC.grid())
    assert len(cases) == len(set(cases)) == len(TC.GRID) * 4
    assert any(O == 0 and G > 1 for _, G, O in TC.GRID) and any(G == 1 for _, G, _ in TC.GRID)
    assert any(O == S // 2 and S % 2 for S, _, O in TC.GRID) and any(O == S // 2 and S % 2 == 0 for S, _, O in TC.GRID)
    assert any(O == 1 for _, _, O in TC.GRID)
    tiles, _ = TC.case(5, 2, 2, 3, 3)
    assert tiles.dtype == np.float32 and abs(float(tiles.mean()) - 1.0) < 0.3 and abs(float(tiles.std()) - 3.0) < 0.3
    assert TC.case(5, 2, 2, 3, 3)[0] is tiles and not tiles.flags.writeable            # computed once, left unchanged


@pytest.mark.parametrize("S,G,O", TC.GRID + (TC.WORKING, (518, 3, 112)))
def test_properties_of_the_geometry(S, G, O):
    C = TC.canvas_side(S, G, O)
    T = S - O
    assert C == S + (G - 1) * T and C == TC.origins(S, G, O)[-1][0] + S
    count = TC.cover_count(S, G, O)
    assert count.min() == 1 and count.max() <= 4 and count.max() == (4 if G > 1 and O > 0 else 1)
    # across an overlap the two 1-D weights add up to O + 1: a linear cross-fade
    w = TC.w1(S)
    assert w.min() == 1 and w.max() == (S + 1) // 2 and np.array_equal(w, w[::-1])
    for u in range(O):
        assert w[T + u] + w[u] == O + 1
    assert 4 * int(w.max()) ** 2 < 2 ** 24                                         # every weight sum is exact in fp32


@pytest.mark.parametrize("S,G,O", [c for c in TC.GRID if c[1] == 1 or c[2] == 0])
def test_one_tile_and_no_overlap_are_pure_copies(S, G, O):
    tiles, want = TC.case(S, G, O, 3, 3)
    for dtype in (np.float32, np.float64):
        got = TC.stitch(tiles, G, O, dtype)
        assert np.array_equal(got, want.astype(dtype))
        assert np.array_equal(TC.gather(got.astype(np.float32), S, G, O), tiles)      # and the gather undoes it
    if G == 1:
        assert np.array_equal(want.astype(np.float32), tiles)


@pytest.mark.parametrize("S,G,O", TC.GRID)
def test_gather_then_stitch_returns_the_canvas(S, G, O):
    """tiles cut from one canvas agree wherever they overlap, so their weighted mean is the canvas again"""
    canvas = TC.canvas_case(S, G, O, 3, 1)
    tiles = TC.gather(canvas, S, G, O)
    assert tiles.shape == (3 * G * G, 1, S, S) and tiles.flags.c_contiguous
    for t, (r, c) in enumerate(TC.origins(S, G, O)):
        assert np.array_equal(tiles[2 * G * G + t, 0], canvas[2, 0, r:r + S, c:c + S])
    back = TC.stitch(tiles, G, O, np.float64)
    assert float(np.abs(back - canvas).max()) <= TC.bar(tiles)


@pytest.mark.parametrize("S,G,O", TC.GRID)
def test_forward_utils_host_definition_is_the_definition(S, G, O):
    import forward_utils as FU
    tiles, want = TC.case(S, G, O, 3, 3)
    assert FU.tile_origins(S, G, O) == TC.origins(S, G, O)
    got = FU.tile_stitch_host(tiles, G, O)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(FU.tile_stitch_host(torch.from_numpy(np.array(tiles[:, 0])), G, O), want[:, 0])    # maps [N, S, S]
    for bad in ((0, 1, 0), (5, 0, 0), (5, 2, -1), (5, 2, 3)):
        with pytest.raises(ValueError):
            FU.tile_origins(*bad)
    with pytest.raises(ValueError):
        FU.tile_stitch_host(np.zeros((G * G, S + 1, S), np.float32), G, O)
    if G > 1:
        with pytest.raises(ValueError):
            FU.tile_stitch_host(np.zeros((G * G + 1, S, S), np.float32), G, O)
    assert FU.TILE_OVERLAP == 112


# ------------------------------------------------------------------------------------------------- the library
def err():
    return _lib.load().aaclip_last_error().decode()


def test_symbols_struct_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert lib.aaclip_version() == _lib.ABI_VERSION == 10                         # additions: the ABI number stays
    assert int(re.search(r"#define\s+AACLIP_ABI_VERSION\s+(\d+)", header).group(1)) == 10
    body = re.search(r"typedef struct aaclip_tile_plan \{(.*?)\} aaclip_tile_plan;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert fields == [n for n, _ in _lib.TilePlan._fields_] == ["struct_bytes", "images", "channels", "tile", "grid",
                                                               "overlap", "stream"]
    assert _lib.TilePlan().struct_bytes == ctypes.sizeof(_lib.TilePlan) == 40
    # the stream travels in the plan: no entry takes a `void* stream` parameter
    for name in NEW_SYMBOLS[1:]:
        proto = re.search(name + r"\s*\(([^()]*)\)\s*;", header).group(1)
        assert "stream" not in proto and proto.count(",") + 1 == len(_lib.SIGNATURES[name][1]) == 3
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "tiles.hip" in make and "tile_plan.h" in make and "-ffp-contract=off" in make
    for name in ("tile_canvas", "tile_gather", "tile_stitch"):
        assert callable(getattr(engine, name))
    assert list(inspect.signature(engine.tile_gather).parameters) == ["canvas", "S", "G", "O"]
    assert list(inspect.signature(engine.tile_stitch).parameters) == ["tiles", "G", "O", "images"]


def test_tile_canvas_on_the_host():
    lib = _lib.load()
    for S, G, O in TC.GRID + (TC.WORKING, (518, 3, 112), (1, 1, 0), (2 ** 31 - 1, 1, 0), (2, 2 ** 31 - 2, 1)):
        assert lib.aaclip_tile_canvas(S, G, O) == S + (G - 1) * (S - O) == engine.tile_canvas(S, G, O), (S, G, O)
    assert engine.tile_canvas(*TC.WORKING) == 924 and engine.tile_canvas(70, 2, 14) == 126
    for bad in ((0, 1, 0), (-5, 1, 0), (5, 0, 0), (5, -1, 0), (5, 2, -1), (5, 2, 3), (6, 2, 4), (2 ** 31 - 1, 2, 0),
                (2, 2 ** 31 - 1, 1), (1 << 20, 1 << 11, 0)):
        assert lib.aaclip_tile_canvas(*bad) < 0 and err().startswith("aaclip_tile_canvas"), bad
        with pytest.raises(ValueError, match="tile_canvas"):
            engine.tile_canvas(*bad)


def test_bad_plans_are_refused_before_any_launch():
    """no GPU here: every check precedes the launch, so a refusal needs none; plausible device addresses stand in"""
    lib = _lib.load()
    A, B = 0x7f0000001000, 0x7f4000001000

    def plan(**kw):
        p = _lib.TilePlan()
        p.images, p.channels, p.tile, p.grid, p.overlap = 2, 3, 70, 2, 14
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    for name in ("aaclip_tile_gather", "aaclip_tile_stitch"):
        fn = getattr(lib, name)
        for kw, msg in ((dict(struct_bytes=32), "struct_bytes"), (dict(struct_bytes=0), "struct_bytes"),
                        (dict(struct_bytes=48), "struct_bytes"), (dict(grid=0), "grid"), (dict(tile=0), "tile"),
                        (dict(channels=0), "channels"), (dict(overlap=-1), "overlap"), (dict(overlap=36), "overlap"),
                        (dict(images=-1), "images"), (dict(tile=2 ** 31 - 1, overlap=0), "overflows int"),
                        (dict(images=2 ** 31 - 1), "2^31"), (dict(tile=1 << 20, grid=1, overlap=0, images=1 << 27), "too large")):
            assert fn(ctypes.byref(plan(**kw)), A, B) == -1, (name, kw)
            assert err().startswith(name + ":") and msg in err(), (name, kw, err())
        for a, b in ((None, B), (A, None), (None, None)):
            assert fn(ctypes.byref(plan()), a, b) == -1 and err().startswith(name + ":") and "null pointer" in err()
        assert fn(None, A, B) == -1 and err().startswith(name + ":") and "null plan" in err()
        assert fn(ctypes.byref(plan()), A + 2, B) == -1 and "aligned" in err()
        assert fn(ctypes.byref(plan()), A, A + 64) == -1 and "must not overlap" in err()
        assert fn(ctypes.byref(plan(images=0)), A, B) == 0                          # nothing to do: no launch, no error
        assert fn(ctypes.byref(plan(images=0, grid=0)), A, B) == -1                 # ... but the plan is still checked


def test_engine_refuses_cpu_tensors_dtypes_and_shapes_on_the_host():
    canvas = torch.zeros(1, 3, 126, 126)
    with pytest.raises(ValueError, match="GPU"):
        engine.tile_gather(canvas, 70, 2, 14)
    with pytest.raises(ValueError, match="GPU"):
        engine.tile_stitch(torch.zeros(4, 70, 70), 2, 14, 1)
    with pytest.raises(ValueError, match="tile_canvas"):
        engine.tile_gather(canvas, 70, 2, 36)


def test_tile_plan_header_under_the_sanitizers(tmp_path):
    """csrc/tile_plan.h as tiles.hip and the C ABI use it, in a host program of its own with ASan + UBSan: canvas side,
    covers, weights, 64-bit offsets, vector width and refusals against brute force; no report from either sanitizer"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "tile_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(CSRC, "tile_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime of the host compiler is not installed: " + build.stderr.strip()[-200:])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and not run.stderr, (run.returncode, run.stdout, run.stderr)


# ------------------------------------------------------------------------------------------------- the script
def test_eval_tiled_parser_and_the_path_without_tiles(monkeypatch, capsys):
    import eval_coreset as EC
    import eval_last as EL
    import eval_tiled as ET
    parse = ET.build_parser().parse_args
    a = parse([])
    assert a.tiles is None and a.tile_overlap == 112
    a = parse(["--tiles", "3", "--tile_overlap", "56"])
    assert (a.tiles, a.tile_overlap) == (3, 56)
    for name in ("tiles", "tile_overlap"):
        assert not hasattr(EC.build_parser().parse_args([]), name)              # eval_coreset.py's arguments stay what they were
    defaults = {k: v for k, v in vars(parse([])).items() if not k.startswith("tile")}
    assert defaults == vars(EC.build_parser().parse_args([]))

    rows = [{"class name": "a", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0}] * 2
    calls = []

    def fake_run(parser, argv=None, table=None, finish=None):
        args = parser.parse_args(argv)
        calls.append((argv, table, finish is not None, getattr(args, "support", None), getattr(args, "tiles", None)))
        print((table or EL.format_table)(rows))
        return rows

    monkeypatch.setattr(EL, "run", fake_run)
    for argv in ([], ["--f1max"], ["--support", "4", "--defects"], ["--aupro", "--device_metrics"],
                 ["--support", "4", "--support_coreset", "0.25"], ["--tile_overlap", "56"]):
        coreset_argv = [v for v in argv if v not in ("--tile_overlap", "56")]
        del calls[:]
        assert EC.main(list(coreset_argv)) == rows
        want_calls, want_out = list(calls), capsys.readouterr().out
        del calls[:]
        assert ET.main(list(argv)) == rows
        assert capsys.readouterr().out == want_out and want_out                           # byte for byte
        assert [c[1:4] for c in calls] == [c[1:4] for c in want_calls] and calls[0][4] is None
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for bad in (["--tiles", "0"], ["--tiles", "-2"], ["--tiles", "2", "--tile_overlap", "-1"],
                ["--tiles", "2", "--tile_overlap", "260"], ["--tiles", "2", "--img_size", "70", "--tile_overlap", "36"],
                ["--tiles", "2", "--support_coreset", "0.1"], ["--tiles", "2", "--support", "0"]):
        with pytest.raises(SystemExit):
            ET.main(bad)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        ET.main(["--tiles", "2"])
    assert len(calls) == 1                                              # none of the refused calls reached a run
    sig = inspect.signature(ET.evaluate).parameters
    lead = inspect.signature(EC.evaluate).parameters
    assert list(sig)[:len(lead)] == list(lead) and list(sig)[len(lead):] == ["tiles", "tile_overlap"]
    assert all(sig[k].default == lead[k].default for k in lead)
    assert sig["tiles"].default is None and sig["tile_overlap"].default == 112
    p = inspect.signature(ET.get_predictions_tiled).parameters
    assert list(p)[:8] == ["model", "class_text_embeddings", "test_loader", "device", "img_size", "dataset", "use_iqm",
                           "on_device"] and list(p)[8:] == ["tiles", "support", "support_weight"]


def test_evaluate_without_tiles_is_eval_coreset(monkeypatch):
    import eval_coreset as EC
    import eval_tiled as ET
    seen, keywords = [], list(inspect.signature(EC.evaluate).parameters)[6:]
    monkeypatch.setattr(EC, "evaluate", lambda *a, **k: seen.append((a, k)) or "rows")
    assert ET.evaluate("m", "sets", "text", "dev", 70, "MVTec", batch_size=4, f1_max=True, support=2, coreset=0.5) == "rows"
    (a, k), = seen
    assert a == ("m", "sets", "text", "dev", 70, "MVTec") and "tiles" not in k and "tile_overlap" not in k
    assert k["batch_size"] == 4 and k["f1_max"] is True and k["support"] == 2 and k["coreset"] == 0.5 and k["coreset_dim"] == 128
    assert set(k) == set(keywords)                                     # every keyword of eval_coreset.evaluate, no other


def test_evaluate_with_tiles_checks_the_mask_size():
    import eval_tiled as ET

    class DS(torch.utils.data.Dataset):
        img_size = 70

        def __len__(self):
            return 1

        def __getitem__(self, i):
            return {"image": torch.zeros(3, 70, 70), "mask": torch.zeros(1, 70, 70), "label": 0, "file_name": "a",
                    "class_name": "c"}

    model = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="126"):
        ET.evaluate(model, {"c": DS()}, {"c": torch.zeros(8, 2)}, "cpu", 70, "MVTec", tiles=2, tile_overlap=14)
    with pytest.raises(ValueError, match="tile"):
        ET.evaluate(model, {"c": DS()}, {"c": torch.zeros(8, 2)}, "cpu", 70, "MVTec", tiles=2, tile_overlap=36)
