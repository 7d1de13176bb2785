"""CPU side of the per-region overlap (AUPRO; csrc/regions.hip): forward_utils.pro_eval against hand-worked curves and
against a brute-force sweep over every distinct threshold (tests/pro_cases.py); a sequential numpy model of the three
union-find phases against scipy.ndimage.label on every adversarial mask; the find / union code itself, built as a
stand-alone host program under AddressSanitizer + UBSan, against a flood fill in shuffled pixel orders; the new C ABI
symbols, workspace queries and every argument rejection that needs no device; metrics_eval's, eval_last's and eval_aupro's surface.

Bound of pro_eval against the sweep: both form the same fp64 points, pro_eval by running sums and the sweep region by
region; at most a few hundred terms of size <= 1 per point on these sets: 1e-12."""
import inspect
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import pro_cases as PC
from aaclip_hip import _lib, engine

CSRC = os.path.join(os.path.dirname(__file__), "..", "aa-clip-iqm_amd", "csrc")
NEW_SYMBOLS = ["aaclip_metrics_regions_workspace_bytes", "aaclip_metrics_regions",
               "aaclip_metrics_sort_pairs_workspace_bytes", "aaclip_metrics_sort_pairs",
               "aaclip_metrics_pro_curve_workspace_bytes", "aaclip_metrics_pro_curve"]


# ---------------------------------------------------------------------------------------------------- pro_eval
def strip(scores_of):
    """one image 1 x 13: region A = pixels 0, 1, region B = pixel 4, ten normal pixels; scores by pixel, 0 elsewhere"""
    label = np.zeros((1, 1, 13), np.uint8)
    label[0, 0, [0, 1, 4]] = 1
    scores = np.zeros((1, 1, 13), np.float32)
    for value, pixels in scores_of.items():
        scores[0, 0, pixels] = value
    return label, scores


def test_pro_eval_perfect_scores():
    import forward_utils as FU
    for shape in PC.SHAPES[:3]:
        m, _ = PC.curve_case(shape, 0)
        rng = np.random.default_rng(2)
        s = (rng.random(shape) * 0.5 + m).astype(np.float32)          # every anomalous pixel above every normal one
        for limit in (0.05, 0.3, 1.0):
            assert abs(FU.pro_eval(m, s, fpr_limit=limit) - 1.0) <= 1e-12
        assert FU.pro_eval(m, -s, fpr_limit=0.3) < 0.05               # inverted: the regions come last


def test_pro_eval_tie_group_straddling_the_limit():
    """points (0, .25), (.1, .75), (.5, 1), (1, 1); up to 0.3: 0 + 0.05 + 0.5 * 0.2 * (0.875 + 0.75) = 0.2125"""
    import forward_utils as FU
    label, scores = strip({1.0: [0], 0.75: [4, 5], 0.5: [1, 6, 7, 8, 9]})
    aupro, regions, normal, groups = FU.pro_eval_record(label, scores, fpr_limit=0.3)
    assert (regions, normal, groups) == (2, 10, 4)
    assert abs(aupro - 0.2125 / 0.3) <= 1e-15
    assert abs(FU.pro_eval(label, scores, fpr_limit=0.5) - (0.05 + 0.5 * 0.4 * 1.75) / 0.5) <= 1e-15    # a point ON the limit
    assert abs(FU.pro_eval(label, scores, fpr_limit=1.0) - (0.05 + 0.35 + 0.5)) <= 1e-15
    # the same curve from scores that the normalisation has to map first (max != 1)
    assert abs(FU.pro_eval(label, scores * 3 - 1, fpr_limit=0.3) - 0.2125 / 0.3) <= 1e-15
    # the labels in metrics_eval's mask layout [N, 1, H, W]
    assert FU.pro_eval(label[:, None], scores, fpr_limit=0.3) == aupro
    # 4-connectivity does not change a strip; a diagonal pair is one region at 8 and two at 4
    assert FU.pro_eval(label, scores, fpr_limit=0.3, connectivity=4) == aupro
    lab2 = np.zeros((1, 3, 3), np.uint8)
    lab2[0, 0, 0] = lab2[0, 1, 1] = 1
    sc2 = np.arange(9, dtype=np.float32).reshape(1, 3, 3)
    assert FU.pro_eval_record(lab2, sc2)[1] == 1 and FU.pro_eval_record(lab2, sc2, connectivity=4)[1] == 2


def test_pro_eval_first_group_beyond_the_limit():
    """first point (0.5, 0.25): interpolated from the origin, y(0.3) = 0.15, area 0.5 * 0.3 * 0.15"""
    import forward_utils as FU
    label, scores = strip({1.0: [0, 5, 6, 7, 8, 9], 0.5: [1, 4]})
    assert abs(FU.pro_eval(label, scores, fpr_limit=0.3) - 0.0225 / 0.3) <= 1e-15


def test_pro_eval_refusals():
    import forward_utils as FU
    label, scores = strip({1.0: [0], 0.5: [1]})
    for bad_label in (np.zeros_like(label), np.ones_like(label)):
        with pytest.raises(ValueError, match="regions and"):
            FU.pro_eval(bad_label, scores)
    with pytest.raises(ValueError, match="equal"):
        FU.pro_eval(label, np.full_like(scores, 0.25))
    for bad in (np.nan, np.inf):
        s = scores.copy()
        s[0, 0, 3] = bad
        with pytest.raises(ValueError, match="finite"):
            FU.pro_eval(label, s)
    for limit in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="fpr_limit"):
            FU.pro_eval(label, scores, fpr_limit=limit)
    with pytest.raises(ValueError, match="connectivity"):
        FU.pro_eval(label, scores, connectivity=6)


@pytest.mark.parametrize("levels", [4, 16, 0])
@pytest.mark.parametrize("shape", [(5, 8, 8), (3, 37, 53)])
def test_pro_eval_equals_the_threshold_sweep(shape, levels):
    import forward_utils as FU
    m, s = PC.curve_case(shape, levels)
    if levels == 0:
        s = np.round(s * 64) / 64            # a few hundred thresholds keep the sweep quick
    norm = (s - s.min()) / (s.max() - s.min())
    for connectivity in (8, 4):
        for limit in (0.05, 0.3, 1.0):
            got = FU.pro_eval(m, s, fpr_limit=limit, connectivity=connectivity)
            want = PC.pro_brute_force(m, norm, limit, connectivity)
            print(shape, levels, connectivity, limit, "diff", abs(got - want))
            assert abs(got - want) <= 1e-12


# ------------------------------------------------------------------------------------------------- union-find
@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("pattern", PC.PATTERNS)
def test_union_find_model_is_scipys_labelling(pattern, connectivity):
    for shape in [(5, 8, 8), (2, 13, 21)]:
        m = PC.mask(pattern, shape)
        region, area, (regions, anomalous, normal) = PC.canonical(m, connectivity)
        assert anomalous + normal == m.size and regions == np.unique(region[region != 0]).size
        for order in (None, np.random.default_rng(7).permutation(np.flatnonzero(m.reshape(-1)))):
            got_region, got_area = PC.union_find_model(m, connectivity, order)
            assert np.array_equal(got_region, region) and np.array_equal(got_area, area), (pattern, shape)
    if pattern == "diagonal":
        m = PC.mask(pattern, (5, 8, 8))
        assert PC.canonical(m, 8)[2][0] == 5 and PC.canonical(m, 4)[2][0] == 5 * 8
    if pattern in ("image_edge", "row_wrap"):      # nothing joins across images or across the row wrap
        m = PC.mask(pattern, (5, 8, 8))
        region = PC.canonical(m, 8)[0]
        for k in range(1, 5):
            assert not set(region[k][region[k] != 0]) & set(region[k - 1][region[k - 1] != 0])


def test_union_find_under_the_sanitizers(tmp_path):
    """csrc/regions_uf.h as regions.hip uses it, in a host program of its own with ASan + UBSan: every pattern at both
    connectivities, five pixel orders each, equal to a flood fill, and no report from either sanitizer"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "regions_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(CSRC, "regions_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime of the host compiler is not installed: " + build.stderr.strip()[-200:])
    assert build.returncode == 0, build.stderr
    cases = [(PC.mask(p, shape), c) for p in PC.PATTERNS for shape in [(5, 8, 8), (3, 37, 53)] for c in (8, 4)]
    with open(tmp_path / "masks.bin", "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for m, c in cases:
            f.write(struct.pack("<4i", *m.shape, c))
            f.write(np.ascontiguousarray(m).tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "masks.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith(f"ok {len(cases)} cases") and not run.stderr, \
        (run.returncode, run.stdout, run.stderr)


# ------------------------------------------------------------------------------------------------- the library
def err():
    return _lib.load().aaclip_last_error().decode()


def test_symbols_and_abi():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aaclip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    for name in ("aaclip_metrics_regions_record", "aaclip_metrics_pro_record"):
        assert name in header
    assert lib.aaclip_version() == 10 == _lib.ABI_VERSION
    assert engine.ProMetrics._fields == ("aupro", "regions", "normal", "groups")


def test_workspace_sizes():
    lib = _lib.load()
    sizes = [2, 3, 64, 65, 8191, 8192, 8193, 27648, 2 ** 20 + 3, 170 * 518 * 518, 2 ** 31 - 1]
    for fn in (lib.aaclip_metrics_sort_pairs_workspace_bytes, lib.aaclip_metrics_pro_curve_workspace_bytes,
               lambda n: lib.aaclip_metrics_regions_workspace_bytes(1, 1, n)):
        got = [fn(n) for n in sizes]
        assert got[0] > 0 and all(b >= a for a, b in zip(got, got[1:])), got
        assert fn(0) == fn(1) == fn(2 ** 31) == fn(-5) == 0
    n = 170 * 518 * 518
    assert 8 * n <= lib.aaclip_metrics_sort_pairs_workspace_bytes(n) <= 9 * n      # a second copy of keys and values
    assert 12 * n <= lib.aaclip_metrics_pro_curve_workspace_bytes(n) <= 12.1 * n   # 4 + 8 bytes per possible tie group
    assert lib.aaclip_metrics_regions_workspace_bytes(170, 518, 518) == lib.aaclip_metrics_regions_workspace_bytes(1, 1, n)
    assert 8 * n <= lib.aaclip_metrics_regions_workspace_bytes(170, 518, 518) <= 8.1 * n   # parents and counters
    per = [lib.aaclip_metrics_regions_workspace_bytes(k, 518, 518) for k in (1, 2, 12, 170)]
    assert per[0] > 0 and all(b >= a for a, b in zip(per, per[1:]))
    for bad in ((0, 8, 8), (2, 0, 8), (2, 8, -1), (1, 1, 1), (2 ** 20, 2 ** 20, 2 ** 20), (1, 2 ** 31, 1),
                (2 ** 40, 2 ** 40, 2 ** 40)):
        assert lib.aaclip_metrics_regions_workspace_bytes(*bad) == 0, bad
    # aaclip_metrics_sort's layout is what it was: a second copy of the keys (4 n) and of the label bytes (n)
    assert 5 * n <= lib.aaclip_metrics_sort_workspace_bytes(n) <= 6 * n


P = 1 << 20          # a non-null, 16-byte aligned address: every call below is refused before anything reads it
A, B, C, D = P + (1 << 24), P + (2 << 24), P + (3 << 24), P + (4 << 24)
WS = P + (1 << 28)
BIG = 1 << 40


def test_regions_rejections():
    lib = _lib.load()
    N, H, W = 2, 70, 130
    n = N * H * W
    need = lib.aaclip_metrics_regions_workspace_bytes(N, H, W)
    for args, msg in [((None, N, H, W, 8, A, B, C, WS, need, None), "null pointer"),
                      ((P, N, H, W, 8, None, B, C, WS, need, None), "null pointer"),
                      ((P, N, H, W, 8, A, None, C, WS, need, None), "null pointer"),
                      ((P, N, H, W, 8, A, B, None, WS, need, None), "null pointer"),
                      ((P, N, H, W, 8, A, B, C, None, need, None), "null pointer"),
                      ((P, N, H, W, 6, A, B, C, WS, need, None), "connectivity must be 4 or 8"),
                      ((P, N, H, W, 0, A, B, C, WS, need, None), "connectivity must be 4 or 8"),
                      ((P, 0, H, W, 8, A, B, C, WS, BIG, None), "must be positive"),
                      ((P, N, -3, W, 8, A, B, C, WS, BIG, None), "must be positive"),
                      ((P, 1, 1, 1, 8, A, B, C, WS, BIG, None), "must be positive"),
                      ((P, 2 ** 20, 2 ** 20, 2 ** 20, 8, A, B, C, WS, BIG, None), "must be positive"),
                      ((P, N, H, W, 8, A + 2, B, C, WS, need, None), "aligned"),
                      ((P, N, H, W, 8, A, B, C + 4, WS, need, None), "aligned"),
                      ((P, N, H, W, 8, A, B, C, WS + 4, need, None), "aligned"),
                      ((P, N, H, W, 8, A, A + 4 * n - 4, C, WS, need, None), "must not overlap"),
                      ((P, N, H, W, 8, P + n - 4, B, C, WS, need, None), "must not overlap"),
                      ((P, N, H, W, 8, A, B, B + 8, WS, need, None), "must not overlap"),
                      ((P, N, H, W, 8, A, B, WS + need - 8, WS, need, None), "must not overlap"),
                      ((WS + 5, N, H, W, 8, A, B, C, WS, need, None), "must not overlap"),
                      ((P, N, H, W, 8, A, B, C, WS, need - 1, None), "workspace too small")]:
        assert lib.aaclip_metrics_regions(*args) == -1
        assert err().startswith("metrics_regions:") and msg in err(), (err(), msg)


def test_sort_pairs_and_pro_curve_rejections():
    lib = _lib.load()
    n = 27648
    need = lib.aaclip_metrics_sort_pairs_workspace_bytes(n)
    for args, msg in [((None, A, n, B, C, WS, need, None), "null pointer"),
                      ((P, None, n, B, C, WS, need, None), "null pointer"),
                      ((P, A, n, None, C, WS, need, None), "null pointer"),
                      ((P, A, n, B, None, WS, need, None), "null pointer"),
                      ((P, A, n, B, C, None, need, None), "null pointer"),
                      ((P, A, 1, B, C, WS, BIG, None), "n must be"),
                      ((P, A, 2 ** 31, B, C, WS, BIG, None), "n must be"),
                      ((P, A + 2, n, B, C, WS, need, None), "aligned"),
                      ((P, A, n, B, C, WS + 4, need, None), "aligned"),
                      ((P, A, n, P + 8, C, WS, need, None), "overlap"),
                      ((P, A, n, B, A + 4, WS, need, None), "overlap"),
                      ((P, A, n, B, B + 4 * n - 4, WS, need, None), "must not overlap one another"),
                      ((P, A, n, WS + 256, C, WS, need, None), "must not overlap one another"),
                      ((P, WS + need - 4, n, B, C, WS, need, None), "must not overlap one another"),
                      ((P, A, n, B, C, WS, need - 1, None), "workspace too small")]:
        assert lib.aaclip_metrics_sort_pairs(*args) == -1
        assert err().startswith("metrics_sort_pairs:") and msg in err(), (err(), msg)
    need = lib.aaclip_metrics_pro_curve_workspace_bytes(n)
    for args, msg in [((None, A, n, B, 0.3, C, WS, need, None), "null pointer"),
                      ((P, None, n, B, 0.3, C, WS, need, None), "null pointer"),
                      ((P, A, n, None, 0.3, C, WS, need, None), "null pointer"),
                      ((P, A, n, B, 0.3, None, WS, need, None), "null pointer"),
                      ((P, A, n, B, 0.3, C, None, need, None), "null pointer"),
                      ((P, A, 1, B, 0.3, C, WS, BIG, None), "n must be"),
                      ((P, A, 2 ** 31, B, 0.3, C, WS, BIG, None), "n must be"),
                      ((P, A, n, B, 0.0, C, WS, need, None), "fpr_limit must lie in (0, 1]"),
                      ((P, A, n, B, 1.0000001, C, WS, need, None), "fpr_limit must lie in (0, 1]"),
                      ((P, A, n, B, float("nan"), C, WS, need, None), "fpr_limit must lie in (0, 1]"),
                      ((P + 2, A, n, B, 0.3, C, WS, need, None), "aligned"),
                      ((P, A, n, B + 4, 0.3, C, WS, need, None), "aligned"),
                      ((P, A, n, B, 0.3, C + 4, WS, need, None), "aligned"),
                      ((P, A, n, B, 0.3, P + 16, WS, need, None), "must not overlap one another"),
                      ((P, A, n, B, 0.3, B + 8, WS, need, None), "must not overlap one another"),
                      ((P, A, n, B, 0.3, WS + need - 8, WS, need, None), "must not overlap one another"),
                      ((P, WS + 64, n, B, 0.3, C, WS, need, None), "must not overlap one another"),
                      ((P, A, n, WS + 8, 0.3, C, WS, need, None), "must not overlap one another"),
                      ((P, A, n, B, 0.3, C, WS, need - 1, None), "workspace too small")]:
        assert lib.aaclip_metrics_pro_curve(*args) == -1
        assert err().startswith("metrics_pro_curve:") and msg in err(), (err(), msg)


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import forward_utils as FU
    scores, mask = torch.rand(2, 4, 4), torch.zeros(2, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.metrics_regions(mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.metrics_sort_pairs(scores, torch.zeros(32, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.pro_metrics(scores, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FU.pro_eval_device(mask, scores)
    sig = inspect.signature(engine.pro_metrics).parameters
    assert [(k, v.default) for k, v in sig.items()][2:] == [("fpr_limit", 0.3), ("connectivity", 8), ("normalise", True)]
    for fn in (FU.pro_eval, FU.pro_eval_device):
        sig = inspect.signature(fn).parameters
        assert [(k, v.default) for k, v in sig.items()][2:] == [("fpr_limit", 0.3), ("connectivity", 8)]


# ------------------------------------------------------------------------------------------------- the harness
def test_metrics_eval_without_a_limit_returns_the_old_dict():
    import forward_utils as FU
    m, s = PC.curve_case((5, 8, 8), 16)
    image_label = np.array([0, 1, 1, 0, 1])
    image_preds = np.linspace(0.1, 0.9, 5).astype(np.float32)
    mask4 = m[:, None].astype(np.float32)
    old = FU.metrics_eval(mask4, image_label, s, image_preds, "x", "Industrial")
    assert list(old) == ["class name", "pixel AUC", "pixel AP", "image AUC", "image AP"]
    assert FU.metrics_eval(mask4, image_label, s, image_preds, "x", "Industrial", fpr_limit=None) == old
    new = FU.metrics_eval(mask4, image_label, s, image_preds, "x", "Industrial", fpr_limit=0.3)
    assert list(new) == list(old) + ["pixel AUPRO"] and {k: new[k] for k in old} == old
    assert new["pixel AUPRO"] == round(FU.pro_eval(m, s, fpr_limit=0.3), 4) * 100
    for fn in (FU.metrics_eval, FU.metrics_eval_device):
        assert inspect.signature(fn).parameters["fpr_limit"].default is None


def test_eval_aupro_flag_and_table():
    import eval_aupro as EA
    import eval_last as EL
    import test_last as TL
    parse = EA.build_parser().parse_args
    assert not hasattr(EL.build_parser().parse_args([]), "aupro")      # eval_last.py's arguments stay what they were
    assert parse([]).aupro is None and parse(["--aupro"]).aupro == 0.3 and parse(["--aupro", "0.05"]).aupro == 0.05
    assert parse(["--aupro", "--device_metrics"]).device_metrics
    assert inspect.signature(EA.evaluate).parameters["aupro_limit"].default is None
    assert list(inspect.signature(EA.evaluate).parameters)[:-1] == list(inspect.signature(EL.evaluate).parameters)
    assert inspect.signature(EL.evaluate_rows).parameters["fpr_limit"].default is None
    rows = [{"class name": "a", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0},
            {"class name": "Average", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0}]
    assert EL.format_table(rows) == TL.format_table(rows)              # no column: exactly what it printed before
    with_col = [dict(r, **{"pixel AUPRO": 12.34}) for r in rows]
    lines = EL.format_table(with_col).split("\n")
    assert lines[0].endswith("pixel AUPRO") and all(line.endswith("12.34") for line in lines[1:])
    assert [line[:len(old)] for line, old in zip(lines, TL.format_table(rows).split("\n"))] == TL.format_table(rows).split("\n")
