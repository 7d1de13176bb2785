"""The few-shot support bank without a GPU: the case generator's promises, the host definition of the support map
against the brute force, BaseSingleClassDataset.support_split, eval_support's parser and its --support-less path, the
library's argument checks, and csrc/support_pack.h in a host program under ASan + UBSan."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import support_cases as SC
from aaclip_hip import _lib, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "aa-clip-iqm_amd", "csrc")
NEW_SYMBOLS = ("aaclip_support_nearest_workspace_bytes", "aaclip_support_nearest", "aaclip_support_bank_rows",
               "aaclip_support_map")


# ------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("E", SC.ES)
def test_the_cases_are_what_they_promise(E):
    M, N = SC.M_MAX, SC.N_MAX
    q, bank = SC.case("planted", M, N, E)
    assert np.allclose(np.linalg.norm(q, axis=1), 1, atol=1e-6) and np.allclose(np.linalg.norm(bank, axis=1), 1, atol=1e-6)
    gap = SC.top2_gap(q, bank)
    print(f"planted E={E}: smallest top-2 gap {gap.min():.4f}")
    assert gap.min() >= SC.PLANTED_GAP
    assert np.array_equal(SC.reference("planted", M, N, E)[1], SC.targets(M, N))
    small = SC.top2_gap(*SC.case("random", M, N, E)) < 2.2e-3
    assert 0.05 <= small.mean() <= 0.25                       # why the random kind compares values only
    best = SC.reference("antipodal", M, N, E)[0]
    assert best.max() < -0.8                                  # a padding column's 0 would win by a wide margin
    q, bank = SC.case("duplicates", M, N, E)
    assert np.array_equal(bank[0], bank[7]) and np.array_equal(bank[0], bank[N - 1]) and np.array_equal(bank[20], bank[27])
    want, idx = SC.reference("duplicates", M, N, E)
    t = SC.targets(M, N)
    assert np.all(idx <= t) and idx[1] == 0 and idx[2] == 0 and int((idx != t).sum()) > 10
    assert np.array_equal(bank[idx], bank[t])                 # the lower copy of the row the query aims at
    # a smaller case is a prefix
    assert np.array_equal(SC.case("random", 17, 127, E)[1], SC.case("random", M, N, E)[1][:127])


def test_rounding_alone_stays_far_below_the_fp16_bar():
    """the fp16 form's rounding, simulated: both operands times 2^4 to fp16, exact products and sums"""
    for E, seen in ((768, 1e-4), (64, 4e-4)):
        q, bank = SC.case("random", 257, 2738, E)
        h = lambda a: (a * 16.0).astype(np.float16).astype(np.float64) / 16.0
        got = (h(q) @ h(bank).T).max(axis=1)
        err = np.abs(got - SC.brute_force(q, bank)[0]).max()
        print(f"simulated fp16 rounding E={E}: {err:.3e}")
        assert err < seen < SC.BAR["fp16"]


# ------------------------------------------------------------------------------------------------- the host map
def _reference_map(segs, banks, S, domain, base, weight):
    """torch's own blur-free pieces: brute-force cosines, then conv2d with reflect padding and interpolate"""
    import torch.nn.functional as F
    sigma, ksize = (1.0, 7) if domain == "Industrial" else (1.5, 9)
    x = torch.arange(ksize, dtype=torch.float64) - ksize // 2
    taps = torch.exp(-x * x / (2 * sigma * sigma))
    taps = taps / taps.sum()
    total = 0
    for f, b in zip(segs, banks):
        B, P, E = f.shape
        g = int(round(P ** 0.5))
        best = SC.brute_force(f.reshape(B * P, E), b.reshape(-1, E))[0]
        d = torch.from_numpy(1.0 - best).reshape(B, 1, g, g)
        r = ksize // 2
        d = F.conv2d(F.pad(d, (r, r, 0, 0), mode="reflect"), taps.view(1, 1, 1, -1))
        d = F.conv2d(F.pad(d, (0, 0, r, r), mode="reflect"), taps.view(1, 1, -1, 1))
        total = total + F.interpolate(d, size=(S, S), mode="bilinear", align_corners=True)[:, 0]
    out = weight * total
    return (out if base is None else torch.from_numpy(base).double() + out).numpy()


@pytest.mark.parametrize("B,g,levels,S,domain", [(2, 5, 1, 70, "Industrial"), (2, 11, 4, 37, "Industrial"),
                                                 (1, 12, 2, 64, "Medical")])
def test_host_map_is_the_brute_force_through_torchs_blur_and_upsample(B, g, levels, S, domain):
    import forward_utils as FU
    segs, banks = SC.map_case(B, g, levels)
    base = np.random.default_rng(1).standard_normal((B, S, S)).astype(np.float32)
    for bs, w in ((None, 50.0), (base, 50.0), (base, 1.0)):
        nearest = []
        got = FU.support_anomaly_map_host(segs, banks, S, domain, base=bs, weight=w, nearest=nearest)
        want = _reference_map(segs, banks, S, domain, bs, w)
        assert got.shape == (B, S, S) and got.dtype == np.float64
        assert np.abs(got - want).max() <= 1e-10 * max(1.0, w)
        for l in range(levels):
            idx = SC.brute_force(segs[l].reshape(B * g * g, -1), banks[l].reshape(-1, segs[l].shape[-1]))[1]
            assert np.array_equal(nearest[l].reshape(-1), idx)
    # the device's own cosines instead of the brute force
    cos = [SC.brute_force(f.reshape(B * g * g, -1), b.reshape(-1, f.shape[-1]))[0] for f, b in zip(segs, banks)]
    assert np.abs(FU.support_anomaly_map_host(segs, None, S, domain, best_cos=cos) -
                  FU.support_anomaly_map_host(segs, banks, S, domain)).max() <= 1e-10      # fp64 sums in another order
    assert FU.SUPPORT_WEIGHT == 50.0
    assert inspect.signature(FU.support_anomaly_map).parameters["weight"].default == 50.0
    assert inspect.signature(engine.support_map).parameters["weight"].default == 50.0


# ------------------------------------------------------------------------------------------------- the dataset
def test_support_split(tmp_path):
    import dataset as D
    from synth_dataset import write_tree
    root = write_tree(str(tmp_path / "MVTec"), n_good=4, n_bad=3, size=(32, 32))
    meta = str(tmp_path / "meta" / "MVTec" / "full-shot.jsonl")
    D.build_metadata(root, meta)
    ds = D.BaseSingleClassDataset(root, meta, 28, "bottle")
    normals = [m["image_path"] for m in ds.normal_meta]
    everything = [m["image_path"] for m in ds.meta]
    assert len(normals) == 4 and len(everything) == 7
    for k in (1, 2, 4):
        support, rest = ds.support_split(k)
        assert [m["image_path"] for m in support.meta] == normals[:k]                       # the first k, in file order
        assert [m["image_path"] for m in rest.meta] == [p for p in everything if p not in normals[:k]]   # removed, order kept
        assert len(support) == k and len(rest) == 7 - k and all(m["label"] == 0 for m in support.meta)
        assert [m["image_path"] for m in rest.normal_meta] == normals[k:]
        assert support[0]["image"].shape == (3, 28, 28) and support[0]["file_name"] == normals[0]
        assert rest.img_size == 28 and rest.data_path == ds.data_path
    assert len(ds) == 7 and len(ds.normal_meta) == 4                                        # the dataset itself is untouched
    for bad in (5, 0, -1):
        with pytest.raises(ValueError, match="normal images"):
            ds.support_split(bad)


# ------------------------------------------------------------------------------------------------- the script
def test_eval_support_parser_and_the_path_without_support(monkeypatch, capsys):
    import eval_defects as ED
    import eval_last as EL
    import eval_support as ES
    parse = ES.build_parser().parse_args
    a = parse([])
    assert a.support is None and a.support_weight == 50.0 and a.support_form is None and a.support_meta is None
    a = parse(["--support", "4", "--support_weight", "20", "--support_form", "fp32", "--support_meta", "m.jsonl", "--defects"])
    assert (a.support, a.support_weight, a.support_form, a.support_meta, a.defects) == (4, 20.0, "fp32", "m.jsonl", 1)
    with pytest.raises(SystemExit):
        parse(["--support_form", "bf16"])
    for name in ("support", "support_weight", "support_form", "support_meta"):
        assert not hasattr(ED.build_parser().parse_args([]), name)          # eval_defects.py's arguments stay what they were
    defaults = {k: v for k, v in vars(parse([])).items() if not k.startswith("support")}
    assert defaults == vars(ED.build_parser().parse_args([]))

    rows = [{"class name": "a", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0}] * 2
    calls = []

    def fake_run(parser, argv=None, table=None, finish=None):
        args = parser.parse_args(argv)
        calls.append((argv, table, finish is not None, getattr(args, "support", None)))
        print((table or EL.format_table)(rows))
        return rows

    monkeypatch.setattr(EL, "run", fake_run)
    printed = {}
    for argv in ([], ["--f1max"], ["--defects", "4"], ["--aupro", "--device_metrics"]):
        del calls[:]
        assert ED.main(list(argv)) == rows
        want_calls, printed["defects"] = list(calls), capsys.readouterr().out
        del calls[:]
        assert ES.main(list(argv)) == rows
        printed["support"] = capsys.readouterr().out
        assert printed["support"] == printed["defects"] and printed["support"]       # byte for byte
        assert [c[:3] for c in calls] == [c[:3] for c in want_calls] and calls[0][3] is None
    del calls[:]
    ES.main(["--support", "4", "--defects"])
    assert calls[0][3] == 4 and calls[0][1] is ED.format_table
    for bad in (["--support", "0"], ["--support_meta", "m.jsonl"]):
        with pytest.raises(SystemExit):
            ES.main(bad)
    sig = inspect.signature(ES.evaluate).parameters
    assert list(sig)[:len(inspect.signature(ED.evaluate).parameters)] == list(inspect.signature(ED.evaluate).parameters)
    assert sig["support"].default is None and sig["support_weight"].default == 50.0
    assert "support" not in inspect.signature(EL.get_predictions).parameters     # its signature stays test_last's plus on_device
    for fn in (EL.get_predictions_support, EL.evaluate_rows):
        p = inspect.signature(fn).parameters
        assert p["support"].default is None and p["support_weight"].default == 50.0


# ------------------------------------------------------------------------------------------------- the library
def err():
    return _lib.load().aaclip_last_error().decode()


def test_symbols_and_python_surface():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "#define AACLIP_SUPPORT_FP16 1" in header and "#define AACLIP_SUPPORT_FP32 0" in header
    assert (engine.SUPPORT_FP16, engine.SUPPORT_FP32) == (1, 0) and lib.aaclip_version() == _lib.ABI_VERSION
    assert engine.SupportBank._fields == ("rows", "form", "patches", "shots")
    assert engine.support_form("fp16") == 1 and engine.support_form("FP32") == 0 and engine.support_form(1) == 1
    with pytest.raises(ValueError):
        engine.support_form("bf16")
    pack = open(os.path.join(CSRC, "support_pack.h")).read()
    assert f"SUPPORT_OPERAND_EXP = {engine.SUPPORT_OPERAND_EXP};" in pack
    assert "support.hip" in open(os.path.join(CSRC, "Makefile")).read()
    cpu = torch.zeros(2, 4, 64)
    for call in (lambda: engine.support_bank([[cpu]], "fp16"), lambda: engine.support_bank_rows(cpu[0], "fp32"),
                 lambda: engine.support_nearest(cpu, cpu[0]), lambda: engine.support_map_from_cos([cpu[0, :, 0]], 1, 8, 1, 1.0),
                 lambda: engine.support_map([cpu], engine.SupportBank([cpu[0]], 0, 4, 1), 8, 1, 1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_workspace_sizes_and_rejections():
    lib = _lib.load()
    fn = lib.aaclip_support_nearest_workspace_bytes
    got = [fn(M, 5476, 768, 1) for M in (1, 17, 129, 1369, 87616, 2 ** 31 - 1)]
    assert got[0] >= 8 and all(b >= a for a, b in zip(got, got[1:])) and 8 * 87616 <= got[4] <= 8 * 87616 + 256
    assert fn(1369, 1, 64, 0) == fn(1369, 175232, 1024, 1)                   # one word per query row, whatever the bank
    for bad in ((0, 1, 64, 1), (1, 0, 64, 1), (-1, 5, 64, 0), (2 ** 31, 5, 64, 1), (5, 2 ** 31, 64, 1), (5, 5, 32, 1),
                (5, 5, 1056, 0), (5, 5, 80, 1), (5, 5, 64, 2), (5, 5, 64, -1)):
        assert fn(*bad) == 0, bad
    P = 1 << 20
    Q, BANK, COS, IDX, WS = (P + (k << 26) for k in range(1, 6))
    M, N, E = 129, 130, 64
    need = fn(M, N, E, 1)

    def call(**kw):
        a = dict(q=Q, M=M, bank=BANK, N=N, E=E, form=1, best_cos=COS, best_idx=IDX, ws=WS, ws_bytes=need, stream=None)
        a.update(kw)
        return lib.aaclip_support_nearest(*a.values())

    for kw, msg in [(dict(q=None), "null pointer"), (dict(bank=None), "null pointer"), (dict(best_cos=None), "null pointer"),
                    (dict(ws=None), "null pointer"), (dict(M=0), "M and N"), (dict(N=0), "M and N"), (dict(N=2 ** 31), "M and N"),
                    (dict(E=48), "E must be"), (dict(E=2048), "E must be"), (dict(E=72), "E must be"), (dict(form=3), "form must be"),
                    (dict(q=Q + 8), "aligned"), (dict(bank=BANK + 2), "aligned"), (dict(best_cos=COS + 2), "aligned"),
                    (dict(best_idx=IDX + 1), "aligned"), (dict(ws=WS + 4), "aligned"),
                    (dict(best_idx=COS), "must not overlap"), (dict(best_cos=Q + 4 * M * E - 4), "must not overlap"),
                    (dict(best_idx=BANK + 2 * N * E - 4), "must not overlap"), (dict(ws=COS + 8), "must not overlap"),
                    (dict(ws=Q + 256), "must not overlap"), (dict(ws_bytes=need - 1), "workspace too small"),
                    (dict(ws_bytes=0), "workspace too small")]:
        assert call(**kw) == -1, kw
        assert err().startswith("support_nearest:") and msg in err(), (kw, err(), msg)
    assert lib.aaclip_support_bank_rows(None, N, E, 1, BANK, None) == -1 and "null pointer" in err()
    assert lib.aaclip_support_bank_rows(Q, N, 40, 1, BANK, None) == -1 and "E must be" in err()
    assert lib.aaclip_support_bank_rows(Q, N, E, 1, Q + 64, None) == -1 and "must not overlap" in err()
    arr = (_lib.C.c_void_p * 1)(COS)
    for kw, msg in [(dict(NL=0), "1..4 levels"), (dict(NL=5), "1..4 levels"), (dict(g=41), "bad shape"), (dict(B=0), "bad shape"),
                    (dict(ksize=16), "kernel size"), (dict(sigma=0.0), "sigma"), (dict(ws_bytes=2 * 25 * 4 - 1), "workspace"),
                    (dict(base=IDX + 4), "must not overlap"), (dict(out=None), "null pointer")]:
        a = dict(best_cos=arr, NL=1, base=None, weight=50.0, out=IDX, B=2, g=5, S=70, ksize=7, sigma=1.0, ws=WS,
                 ws_bytes=2 * 25 * 4, stream=None)
        a.update(kw)
        assert lib.aaclip_support_map(*a.values()) == -1 and "support_map:" in err() and msg in err(), (kw, err())


# ------------------------------------------------------------------------------------- the shared header on the host
def test_support_pack_header_under_the_sanitizers(tmp_path):
    """csrc/support_pack.h as support.hip uses it, in a host program of its own with ASan + UBSan: candidates packed,
    merged in several chunk orders and decoded, equal to a sequential scan; no report from either sanitizer"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "support_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(CSRC, "support_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime of the host compiler is not installed: " + build.stderr.strip()[-200:])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and not run.stderr, (run.returncode, run.stdout, run.stderr)
