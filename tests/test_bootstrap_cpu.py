"""CPU side of the bootstrap intervals (csrc/bootstrap.hip, forward_utils.bootstrap_*): the definition against sklearn on
the literally repeated images; the draw; the 0 / 0 rule, the invalid rule and the 5 % cap; the interval and the Average
row's rule; tools/bootstrap_diff.py; the new C ABI symbols and every refusal that needs no device; and bootstrap_plan.h
-- the tile decomposition that the kernels run -- as a stand-alone host program under AddressSanitizer + UBSan.

Bars against sklearn: AUROC 1e-12 (one integer numerator, one division), AP 1e-10 (the same fp64 terms in another
order): the bars of tests/test_gpu_metrics_device.py for the same two quantities."""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import bootstrap_cases as BC
import metrics_device_cases as MD
from aaclip_hip import _lib, engine

REPO = os.path.join(os.path.dirname(__file__), "..")
CSRC = os.path.join(REPO, "aa-clip-iqm_amd", "csrc")
NEW_SYMBOLS = ["aaclip_bootstrap_max_images", "aaclip_bootstrap_workspace_bytes", "aaclip_bootstrap_curves"]


def FU():
    import forward_utils
    return forward_utils


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("kind", ["ties", "no ties"])
def test_definition_is_sklearn_on_repeated_images(kind):
    labels, scores, _ = BC.small_class(kind)
    counts = FU().bootstrap_counts(12, 200, 0, 0)
    image_of = np.repeat(np.arange(12), 37)
    got = FU().bootstrap_eval(labels, scores, image_of, counts)
    keys, payload = BC.sorted_pairs(scores, labels, 37)
    restated = BC.records(keys, payload, counts)
    for k in ("num", "P", "N", "valid"):
        assert np.array_equal(getattr(got, k), restated[k]), k
    assert np.abs(got.ap - restated["ap"]).max() <= 1e-10
    worst_auc = worst_ap = 0.0
    for r in np.nonzero(got.valid)[0]:
        auc, ap = BC.repeated(labels, scores, counts[r])
        worst_auc, worst_ap = max(worst_auc, abs(auc - got.auroc[r])), max(worst_ap, abs(ap - got.ap[r]))
        assert abs(ap - restated["ap"][r]) <= 1e-10
    print(f"{kind}: worst |d AUROC| {worst_auc:.3g}, |d AP| {worst_ap:.3g}, {int((~got.valid).sum())} invalid of 200")
    assert got.valid.sum() >= 190 and worst_auc <= 1e-12 and worst_ap <= 1e-10


@pytest.mark.parametrize("kind", BC.KINDS)
def test_counts_of_one_are_curve_sums(kind):
    scores, labels, _ = BC.pixel_class(kind)
    keys, payload, _ = BC.expected(kind)
    want = MD.curve_sums(keys, payload & 1, False)
    ones = np.ones((1, BC.IMAGES), np.uint8)
    got = BC.records(keys, payload, ones)
    assert (int(got["num"][0]), int(got["P"][0]), int(got["N"][0])) == (want["num"], want["P"], want["N"])
    assert abs(got["ap"][0] - want["ap"]) <= 1e-10
    host = FU().bootstrap_eval(labels, scores, np.repeat(np.arange(BC.IMAGES), BC.PER_IMAGE), ones)
    assert (int(host.num[0]), int(host.P[0]), int(host.N[0])) == (want["num"], want["P"], want["N"])
    assert abs(host.auroc[0] - want["num"] / (2 * want["P"] * want["N"])) <= 1e-12
    if kind == "run":        # the run of 9 000 covers tile 1 entirely and crosses both of its boundaries
        start = np.nonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))[0]
        assert not ((start >= 4096) & (start < 8192)).any() and want["groups"] == BC.IMAGES * BC.PER_IMAGE - 8999


def test_gpu_case_matrix_holds_no_drawn_invalid_replicate():
    """what tests/test_gpu_bootstrap.py relies on: only the hand-made rows may be invalid"""
    for kind in BC.KINDS:
        for R, (counts, want) in BC.expected(kind)[2].items():
            assert counts.shape == (R, BC.IMAGES) and (counts.sum(axis=1) == BC.IMAGES).all()
            if R >= 4:
                assert want["valid"][:R - 4].all() and want["valid"][R - 4:].tolist() == [True, True, False, True]
            else:
                assert want["valid"].all()
            host = FU().bootstrap_eval(BC.pixel_class(kind)[1], BC.pixel_class(kind)[0],
                                       np.repeat(np.arange(BC.IMAGES), BC.PER_IMAGE), counts)
            assert np.array_equal(host.num, want["num"]) and np.array_equal(host.valid, want["valid"])
            assert np.abs(host.ap - want["ap"]).max() <= 1e-10


# ------------------------------------------------------------------------------------------------------ the draw
def test_bootstrap_counts():
    f = FU().bootstrap_counts
    a = f(23, 300, 0, 4)
    assert a.dtype == np.uint8 and a.shape == (300, 23) and (a.sum(axis=1) == 23).all()
    assert np.array_equal(a, f(23, 300, 0, 4))                                   # reproducible
    assert not np.array_equal(a, f(23, 300, 0, 5)) and not np.array_equal(a, f(23, 300, 1, 4))
    draw = np.random.default_rng([0, 4]).integers(0, 23, size=(300, 23))          # the stated draw
    assert np.array_equal(a, np.stack([np.bincount(row, minlength=23) for row in draw]))
    label = np.array([0, 1, 1, 0, 0, 1, 0, 0, 0, 1])
    s = f(10, 200, 7, 1, label)
    assert (s[:, label == 0].sum(axis=1) == 6).all() and (s[:, label == 1].sum(axis=1) == 4).all()
    assert np.array_equal(s, f(10, 200, 7, 1, label)) and not np.array_equal(s, f(10, 200, 7, 1))
    rng = np.random.default_rng([7, 1])                                          # label 0 first, then label 1
    d0, d1 = rng.integers(0, 6, size=(200, 6)), rng.integers(0, 4, size=(200, 4))
    assert np.array_equal(s[:, label == 0], np.stack([np.bincount(r, minlength=6) for r in d0]))
    assert np.array_equal(s[:, label == 1], np.stack([np.bincount(r, minlength=4) for r in d1]))
    assert (f(1, 3, 0, 0) == 1).all()
    with pytest.raises(ValueError):
        f(0, 5, 0, 0)
    with pytest.raises(ValueError, match="image labels"):
        f(5, 5, 0, 0, [0, 1])


def test_a_count_above_255_is_refused(monkeypatch):
    """300 draws that all name image 0: a count of 300 does not fit the uint8 storage"""
    class AlwaysZero:
        def integers(self, lo, hi, size):
            return np.zeros(size, np.int64)
    monkeypatch.setattr(np.random, "default_rng", lambda seed: AlwaysZero())
    with pytest.raises(ValueError, match="uint8"):
        FU().bootstrap_counts(300, 1, 0, 0)


# ------------------------------------------------------------------------------------------------- the two rules
def test_zero_over_zero_rule_and_invalid_rule():
    """four images of three pixels; image 3 holds the top scores.  With image 3 at weight 0 the top groups weigh nothing:
    they add exactly 0 to AP (no 0 / 0) and nothing to num, and the result is that of the other three images."""
    labels = np.array([[0, 0, 1], [0, 1, 0], [0, 0, 0], [1, 0, 1]])
    scores = np.array([[.1, .2, .6], [.15, .5, .3], [.05, .25, .35], [.9, .8, .95]], np.float32)
    image_of = np.repeat(np.arange(4), 3)
    counts = np.array([[1, 1, 1, 0], [2, 1, 1, 0], [1, 1, 1, 1], [0, 0, 4, 0], [0, 0, 0, 4], [0, 0, 3, 1]], np.uint8)
    got = FU().bootstrap_eval(labels, scores, image_of, counts)
    assert np.isfinite(got.ap).all() and np.isfinite(got.auroc).all()
    auc, ap = BC.repeated(labels[:3], scores[:3], [1, 1, 1])
    assert abs(got.auroc[0] - auc) <= 1e-12 and abs(got.ap[0] - ap) <= 1e-10
    auc, ap = BC.repeated(labels[:3], scores[:3], [2, 1, 1])
    assert abs(got.auroc[1] - auc) <= 1e-12 and abs(got.ap[1] - ap) <= 1e-10
    # the invalid rule: image 2 alone has no positive, image 3 alone has both labels, (2, 2, 2, 3) has both
    assert got.valid.tolist() == [True, True, True, False, True, True]
    assert (got.P[3], got.N[3], got.num[3], got.ap[3], got.auroc[3]) == (0, 12, 0, 0.0, 0.0)
    only_pos = FU().bootstrap_eval([1, 1, 0], [.3, .2, .1], [0, 0, 1], np.array([[2, 0], [0, 2], [1, 1]], np.uint8))
    assert only_pos.valid.tolist() == [False, False, True] and only_pos.N.tolist() == [0, 2, 1]
    assert only_pos.num[:2].tolist() == [0, 0] and only_pos.ap[:2].tolist() == [0.0, 0.0]
    restated = BC.records(*BC.sorted_pairs(scores, labels, 3), counts)
    assert np.array_equal(restated["num"], got.num) and np.abs(restated["ap"] - got.ap).max() <= 1e-12
    with pytest.raises(ValueError, match="0 .. 255"):
        FU().bootstrap_eval(labels, scores, image_of, np.full((1, 4), 256))
    with pytest.raises(ValueError, match="2\\^31"):
        FU().bootstrap_eval(np.zeros(2 ** 23 + 2 ** 16), np.zeros(2 ** 23 + 2 ** 16), np.zeros(2 ** 23 + 2 ** 16, np.int8),
                            np.full((1, 1), 255))


def stub_class(n_normal, n_bad, side=6, seed=3):
    rng = np.random.default_rng(seed)
    il = np.array([0] * n_normal + [1] * n_bad)
    pl = np.zeros((il.size, 1, side, side), np.float32)
    pl[il == 1, 0, 1:3, 2:5] = 1
    pp = (rng.normal(size=(il.size, side, side)) + 1.5 * pl[:, 0]).astype(np.float32)
    ip = (rng.normal(size=il.size) + il).astype(np.float32)
    return pl, il, pp, ip


def test_five_percent_cap():
    pl, il, pp, ip = stub_class(2, 2)
    with pytest.raises(ValueError, match="'tiny'.*--bootstrap_stratified"):
        FU().metrics_eval(pl, il, pp, ip, "tiny", "Industrial", bootstrap=dict(R=400, seed=0))
    details = {}
    row = FU().metrics_eval(pl, il, pp, ip, "tiny", "Industrial", details=details, bootstrap=dict(R=400, seed=0, stratified=True))
    assert details["bootstrap"]["valid"].all() and row["image AUC lo"] <= row["image AUC"] <= row["image AUC hi"]
    with pytest.raises(ValueError, match="bootstrap must be a dict"):
        FU().metrics_eval(pl, il, pp, ip, "tiny", "Industrial", bootstrap=dict(seed=0))
    with pytest.raises(ValueError, match="bootstrap must be a dict"):
        FU().metrics_eval(pl, il, pp, ip, "tiny", "Industrial", bootstrap=dict(R=5, replicates=3))


# ------------------------------------------------------------------------------------- the interval, the columns
def test_interval_is_numpys_default_quantile():
    values = np.array([0.9, 0.5, 0.1, 0.7, 0.3, 123.0])
    valid = np.array([True, True, True, True, True, False])
    # sorted valid values 0.1 0.3 0.5 0.7 0.9; position q (n - 1): 0.025 * 4 = 0.1 -> 0.1 + 0.1 * 0.2; 0.975 * 4 = 3.9
    lo, hi = FU().bootstrap_interval(values, valid, 0.95)
    assert abs(lo - 0.12) <= 1e-15 and abs(hi - 0.88) <= 1e-15
    lo, hi = FU().bootstrap_interval(values, valid, 0.5)
    assert abs(lo - 0.3) <= 1e-15 and abs(hi - 0.7) <= 1e-15
    with pytest.raises(ValueError):
        FU().bootstrap_interval(values, np.zeros(6, bool))
    with pytest.raises(ValueError):
        FU().bootstrap_interval(values, valid, 1.0)


def test_metrics_eval_columns_and_details():
    pl, il, pp, ip = stub_class(6, 7)
    plain = FU().metrics_eval(pl, il, pp, ip, "stub", "Industrial")
    details = {}
    boot = dict(R=120, seed=5, level=0.9, class_index=3)
    row = FU().metrics_eval(pl, il, pp, ip, "stub", "Industrial", details=details, bootstrap=boot)
    assert {k: row[k] for k in plain} == plain and list(row)[len(plain):] == FU().bootstrap_interval_cols()
    b = details["bootstrap"]
    assert (b["R"], b["seed"], b["level"], b["images"], b["class_index"], b["stratified"]) == (120, 5, 0.9, 13, 3, False)
    counts = FU().bootstrap_counts(13, 120, 5, 3)
    norm = MD.normalise(pp)
    pixel = FU().bootstrap_eval(pl, norm, np.repeat(np.arange(13), 36), counts)
    combined = norm.max(axis=(1, 2)) * 0.5 + MD.normalise(ip) * 0.5
    image = FU().bootstrap_eval(il, combined, np.arange(13), counts)
    valid = pixel.valid & image.valid
    assert np.array_equal(b["valid"], valid) and valid.sum() >= 114
    assert np.array_equal(b["pixel AUC"][valid], pixel.auroc[valid]) and np.array_equal(b["image AP"][valid], image.ap[valid])
    for col, values in (("pixel AUC", pixel.auroc), ("pixel AP", pixel.ap), ("image AUC", image.auroc), ("image AP", image.ap)):
        lo, hi = np.quantile(values[valid], [(1 - 0.9) / 2, (1 + 0.9) / 2])
        assert row[col + " lo"] == round(lo, 4) * 100 and row[col + " hi"] == round(hi, 4) * 100
        assert b["point"][col] == row[col]
    # a one-label class: the fixed 0 and its interval
    one = FU().metrics_eval(pl, np.zeros_like(il), pp, ip, "stub", "Industrial", bootstrap=dict(R=30))
    assert [one[c] for c in ("image AUC", "image AUC lo", "image AUC hi", "image AP lo", "image AP hi")] == [0] * 5


def test_average_rule():
    import eval_last as EL
    rng = np.random.default_rng(0)
    R = 50
    blocks = []
    for c in range(3):
        valid = np.ones(R, bool)
        valid[[c, 10 + c]] = False
        blocks.append(dict({col: rng.random(R) for col in FU().BOOTSTRAP_COLS}, valid=valid, level=0.8))
    avg = {}
    out = EL.bootstrap_average(avg, blocks)
    valid = np.ones(R, bool)
    valid[[0, 1, 2, 10, 11, 12]] = False                                         # invalid where any class is
    assert np.array_equal(out["valid"], valid)
    for col in FU().BOOTSTRAP_COLS:
        means = (blocks[0][col] + blocks[1][col] + blocks[2][col]) / 3
        assert np.allclose(out[col], means, rtol=0, atol=1e-15)
        lo, hi = np.quantile(out[col][valid], [(1 - 0.8) / 2, (1 + 0.8) / 2])
        assert avg[col + " lo"] == lo * 100 and avg[col + " hi"] == hi * 100
    assert set(avg) == set(FU().bootstrap_interval_cols())
    table = EL.format_table([dict({"class name": "a", "pixel AUC": 1.0, "pixel AP": 2.0, "image AUC": 3.0, "image AP": 4.0},
                                  **avg)])
    assert "pixel AUC lo" in table.split("\n")[0] and "image AP hi" in table.split("\n")[0]


# ------------------------------------------------------------------------------------------- tools/bootstrap_diff
def load_diff_tool():
    spec = importlib.util.spec_from_file_location("bootstrap_diff", os.path.join(REPO, "tools", "bootstrap_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_tree(folder, shift, seed=0, R=40, images=9, drop=()):
    rng = np.random.default_rng(1)
    os.makedirs(folder, exist_ok=True)
    for name in ("bottle", "grid", "Average"):
        base = {k: rng.random(R) * 0.1 + 0.8 for k in ("pixel_auc", "pixel_ap", "image_auc", "image_ap")}
        valid = np.ones(R, bool)
        valid[list(drop)] = False
        np.savez(os.path.join(folder, name + ".npz"), valid=valid, seed=np.int64(seed), images=np.int64(images),
                 R=np.int64(R), level=np.float64(0.95), stratified=np.bool_(False),
                 point=np.array([85.0 + 100 * shift] * 4), **{k: v + shift for k, v in base.items()})


def test_bootstrap_diff(tmp_path, capsys):
    tool = load_diff_tool()
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    write_tree(a, 0.0, drop=(3,))
    write_tree(b, 0.02, drop=(5,))
    rows = tool.diff_rows(tool.load_tree(a), tool.load_tree(b), 0.9)
    assert [r["class name"] for r in rows] == ["bottle", "grid", "Average"]
    for r in rows:
        assert r["replicates"] == 38                                             # valid in both
        for col, _ in tool.COLUMNS:
            assert abs(r[col + " diff"] - 2.0) <= 1e-9
            assert abs(r[col + " lo"] - 2.0) <= 1e-9 and abs(r[col + " hi"] - 2.0) <= 1e-9   # the same noise in both: it cancels
    assert tool.main([a, b]) == 0
    out = capsys.readouterr().out
    assert "Average" in out and "+2.00" in out
    for kwargs, word in ((dict(seed=1), "seed"), (dict(R=41), "R"), (dict(images=10), "images")):
        c = str(tmp_path / ("c_" + word))
        write_tree(c, 0.0, **kwargs)
        with pytest.raises(ValueError, match=word + " differs"):
            tool.diff_rows(tool.load_tree(a), tool.load_tree(c))
        assert tool.main([a, c]) == 2
    capsys.readouterr()
    os.remove(os.path.join(b, "grid.npz"))
    with pytest.raises(ValueError, match="different classes"):
        tool.diff_rows(tool.load_tree(a), tool.load_tree(b))
    with pytest.raises(ValueError, match="no such folder"):
        tool.load_tree(str(tmp_path / "missing"))


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_and_abi():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.aaclip_version() == 10 == _lib.ABI_VERSION
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name in NEW_SYMBOLS + ["aaclip_bootstrap_record", "aaclip_bootstrap_plan"]:
        assert name in header, name
    assert lib.aaclip_bootstrap_max_images() == engine.bootstrap_max_images() >= 1024


def test_workspace_query():
    lib = _lib.load()
    size = lib.aaclip_bootstrap_workspace_bytes
    n = 170 * 518 * 518
    assert size(n, 170, 1000) == size(n, 170, 512) == size(n, 170, 10 ** 6) < 2 ** 30   # no growth with R beyond a chunk
    assert size(n, 170, 1000) == 228134656                                              # DESIGN.md states this number
    assert size(n, 170, 64) < size(n, 170, 65) and size(n, 1, 1000) == size(n, 170, 1000)
    assert size(1, 1, 1) > 0 and size(4096, 1, 1) < size(4097, 1, 1)
    for bad in ((0, 1, 1), (2 ** 31, 1, 1), (10, 0, 1), (10, lib.aaclip_bootstrap_max_images() + 1, 1), (10, 1, 0),
                (10, 1, 2 ** 20 + 1)):
        assert size(*bad) == 0, bad


def test_refusals_that_need_no_device():
    lib = _lib.load()
    n, images, R = 100, 4, 3
    need = lib.aaclip_bootstrap_workspace_bytes(n, images, R)
    base = 1 << 20                                                               # addresses are only compared
    good = dict(keys=base, payload=base + 4096, n=n, counts=base + 8192, images=images, R=R, records=base + 12288,
                ws=base + 16384, ws_bytes=need, struct_bytes=None)
    err = lambda: lib.aaclip_last_error().decode()
    cases = [(dict(keys=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(n=0), "n must be"),
             (dict(images=0), "images must be"), (dict(images=1025), "images must be"), (dict(R=0), "R must be"),
             (dict(keys=base + 2), "aligned"), (dict(records=base + 12292), "aligned"),
             (dict(records=base + 8), "overlap"), (dict(ws=base + 12288 + 64), "overlap"),
             (dict(ws_bytes=need - 1), "workspace too small"), (dict(struct_bytes=8), "struct_bytes")]
    for change, msg in cases:
        a = dict(good, **change)
        plan = _lib.BootstrapPlan(n=a["n"], images=a["images"], replicates=a["R"], stream=None)
        assert plan.struct_bytes == 40
        if a["struct_bytes"] is not None:
            plan.struct_bytes = a["struct_bytes"]
        rc = lib.aaclip_bootstrap_curves(ctypes.byref(plan), a["keys"], a["payload"], a["counts"], a["records"], a["ws"],
                                         a["ws_bytes"])
        assert rc == -1, change
        assert err().startswith("bootstrap_curves:") and msg in err(), (change, err())
    assert lib.aaclip_bootstrap_curves(None, base, base + 4096, base + 8192, base + 12288, base + 16384, need) == -1
    assert "null pointer" in err()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.bootstrap_curves(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), np.ones((1, 1), np.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.bootstrap_metrics(torch.rand(8), torch.zeros(8, dtype=torch.uint8), 2, np.ones((2, 4), np.uint8))


def test_scripts_surface(monkeypatch):
    import eval_bootstrap as EB
    import eval_png as EP
    args = EB.build_parser().parse_args([])
    assert (args.bootstrap, args.bootstrap_seed, args.bootstrap_level, args.bootstrap_stratified) == (None, 0, 0.95, False)
    assert {a.dest for a in EP.build_parser()._actions} < {a.dest for a in EB.build_parser()._actions}
    assert EB.bootstrap_settings(None) is None
    assert EB.bootstrap_settings(10, 2, 0.9, True) == {"R": 10, "seed": 2, "level": 0.9, "stratified": True}
    with pytest.raises(ValueError):
        EB.bootstrap_settings(0)
    called = {}
    monkeypatch.setattr(EP, "evaluate", lambda *a, **k: called.update(args=a, kwargs=k) or "rows of eval_png")
    assert EB.evaluate("m", "d", "t", "dev", 70, "MVTec", f1_max=True, bootstrap=None) == "rows of eval_png"
    assert called["args"] == ("m", "d", "t", "dev", 70, "MVTec") and called["kwargs"]["f1_max"] is True
    assert "bootstrap" not in called["kwargs"]
    monkeypatch.setattr(EP, "run", lambda parser, argv: ("eval_png.run", argv))
    assert EB.main(["--save_path", "x"]) == ("eval_png.run", ["--save_path", "x"])     # without --bootstrap: eval_png.py
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        EB.main(["--bootstrap", "10"])
    monkeypatch.setenv("WORLD_SIZE", "1")
    for bad in (["--bootstrap", "0"], ["--bootstrap", "5", "--bootstrap_level", "1.0"]):
        with pytest.raises(SystemExit):
            EB.main(bad)


# --------------------------------------------------------------------------------------------- bootstrap_plan.h
def test_plan_header_under_the_sanitizers(tmp_path):
    """csrc/bootstrap_plan.h as bootstrap.hip uses it, in a host program of its own with ASan + UBSan: tile sums -> prefixes
    -> per-tile records -> the fold across tiles against a brute-force loop over the tie groups, around 1, 2 and 3 tiles
    +- 1, with a tie group longer than two tiles, groups across every boundary and images of weight 0; num, P, N equal, AP
    within 1e-10; no report from either sanitizer."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "bootstrap_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(CSRC, "bootstrap_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime of the host compiler is not installed: " + build.stderr.strip()[-200:])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and not run.stderr, (run.returncode, run.stdout, run.stderr)
    assert run.stdout.strip().endswith("228134656 bytes")
