"""The coreset of the support bank without a GPU: the definition's own properties (tests/coreset_cases.py), the
library's symbols, workspace sizes and argument checks, csrc/coreset_pack.h in a host program under ASan + UBSan,
eval_coreset's parser and its path without --support_coreset, the (shot, patch) pairs of a bank with an index, and the
coreset=None paths of support_banks and build_support_bank."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import coreset_cases as CC
from aaclip_hip import _lib, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "aa-clip-iqm_amd", "csrc")
NEW_SYMBOLS = ("aaclip_coreset_rows", "aaclip_coreset_select_workspace_bytes", "aaclip_coreset_select",
               "aaclip_coreset_unit_rows")


# ------------------------------------------------------------------------------------------------- the definition
def test_the_quantiser_rounds_half_to_even_and_clamps():
    k = np.arange(-6, 7, dtype=np.float32)
    q, _ = CC.quantise(((k + 0.5) / 16384.0)[None, :])
    assert np.array_equal(q[0], [-6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6, 6])          # both parities
    vals = np.array([[1.0, -1.0, 2.0, -2.0, -0.0, 0.0, 1e-45, -1e-39, 1.99993896484375, 3.4e38, -np.inf, np.nan]], np.float32)
    q, norm2 = CC.quantise(vals)
    assert np.array_equal(q[0], [16384, -16384, 32767, -32767, 0, 0, 0, 0, 32767, 32767, -32767, 0])
    assert norm2[0] == 0x7FFFFFFF                                                       # saturated, not wrapped
    q, norm2 = CC.quantise(np.array([[1.0] + [0.0] * 31], np.float32))
    assert norm2[0] == 1 << 28 and norm2.dtype == np.int32 and q.dtype == np.int16


@pytest.mark.parametrize("E", CC.ES)
def test_the_cases_are_what_they_promise(E):
    for kind in CC.KINDS:
        for N in CC.sizes(kind, E):
            rows = CC.case(kind, N, E)
            assert rows.shape == (N, E) and rows.dtype == np.float32
            assert np.allclose(np.linalg.norm(rows.astype(np.float64), axis=1), 1, atol=1e-6)
            q, norm2 = CC.quantised(kind, N, E)
            # unit rows: each component is off by at most 2^-15, so |norm - 2^14| <= sqrt(E) / 2 and norm2 is far below 2^29
            assert np.abs(np.sqrt(norm2.astype(np.float64)) - 2 ** 14).max() <= 0.5 * np.sqrt(E) + 1
            assert norm2.max() < CC.NORM2_LIMIT
    assert np.array_equal(CC.case("random", 65, E), CC.case("random", 2738, E)[:65])     # a smaller case is a prefix
    a = CC.case("antipodal", 66, E)
    assert np.array_equal(a[0::2], -a[1::2])
    d = CC.case("duplicates", 20, E)
    assert np.array_equal(d[:5], d[5:10]) and np.array_equal(d[:5], d[15:]) and len({r.tobytes() for r in d}) == 5
    t = CC.case("ties", 2 * E, E)
    assert np.array_equal(t[0::2], np.eye(E, dtype=np.float32)) and np.array_equal(t[1::2], -np.eye(E, dtype=np.float32))


@pytest.mark.parametrize("E", CC.ES)
def test_prefix_property_and_the_radius_never_increases(E):
    for kind in CC.KINDS:
        N = [n for n in CC.sizes(kind, E) if n <= 257][-1]
        q, _ = CC.quantised(kind, N, E)
        for start in CC.starts(N):
            picks, radius2, min_d2 = CC.definition(q, N, start)
            assert picks[0] == start and radius2[0] == CC.D2_INIT and picks.dtype == np.int32 and radius2.dtype == np.uint32
            assert np.all(np.diff(radius2.astype(np.int64)) <= 0)
            assert radius2[N] == 0 and np.all(min_d2 == 0)                   # every row picked or a duplicate of a pick
            for n in CC.counts(N):
                p, r, m = CC.definition(q, n, start)
                assert np.array_equal(p, picks[:n]) and np.array_equal(r, radius2[:n + 1])
                assert m.max() == radius2[n] and np.all(m[p] == 0)
            # the reference of the GPU tests is this definition
            rp, rr, kept = CC.reference(kind, N, E, start)
            assert np.array_equal(rp, picks) and np.array_equal(rr, radius2) and np.array_equal(kept[N], min_d2)
            n = CC.counts(N)[-2] if len(CC.counts(N)) > 1 else N
            assert np.array_equal(kept[n], CC.definition(q, n, start)[2])


def test_the_gram_form_is_the_definition_at_the_largest_shape():
    """N = 2738, E = 768, n = 274: one int64 matrix-vector product per pick against the float64 Gram matrix"""
    q, _ = CC.quantised("random", 2738, 768)
    want = CC.definition(q, 274, 1825)
    picks, radius2, kept = CC.reference("random", 2738, 768, 1825)
    assert np.array_equal(picks[:274], want[0]) and np.array_equal(radius2[:275], want[1]) and np.array_equal(kept[274], want[2])
    assert len(set(picks.tolist())) == 2738                                    # distinct rows: a permutation


@pytest.mark.parametrize("E", CC.ES)
def test_clusters_duplicates_antipodal_and_ties(E):
    rows = CC.case("clusters", 257, E)
    for start in CC.starts(257):
        picks, radius2, _ = CC.definition(CC.quantised("clusters", 257, E)[0], CC.CLUSTERS + 1, start)
        assert sorted(int(p) % CC.CLUSTERS for p in picks[:CC.CLUSTERS]) == list(range(CC.CLUSTERS))    # 10 picks, 10 clusters
        # with all clusters covered the radius falls from the separation of the centres to the size of the noise
        assert radius2[CC.CLUSTERS] < radius2[CC.CLUSTERS - 1] / 20
    assert rows.shape == (257, E)
    for start in CC.starts(20):
        picks, radius2, min_d2 = CC.definition(CC.quantised("duplicates", 20, E)[0], 20, start)
        assert sorted(int(p) % 5 for p in picks[:5]) == [0, 1, 2, 3, 4]
        assert radius2[4] > 0 and np.all(radius2[5:] == 0) and np.all(picks[5:] == 0)     # nothing left: row 0 again and again
    picks, radius2, _ = CC.definition(CC.quantised("antipodal", 66, E)[0], 2, 0)
    # d2(v, -v) = 4 norm2, and the quantised norm is 2^14 +- sqrt(E) / 2
    tol = 4 * (2 ** 14 * np.sqrt(E) + E)
    assert picks[1] == 1 and (1 << 30) - tol <= radius2[1] <= (1 << 30) + tol
    # ties: from e_0 the antipode -e_0 is farthest (d2 = 2^30); after that every row left is at 2^29 from the picks, so
    # the lowest index decides: rows in order
    N = 2 * E
    q = CC.quantised("ties", N, E)[0]
    picks, radius2, _ = CC.definition(q, N, 0)
    assert np.array_equal(picks, np.arange(N))
    assert radius2[1] == 1 << 30 and np.all(radius2[2:N] == 1 << 29) and radius2[N] == 0
    s = CC.starts(N)[1]
    picks, _, _ = CC.definition(q, N, s)
    assert picks[0] == s and picks[1] == (s ^ 1) and np.array_equal(picks[2:], [i for i in range(N) if i not in (s, s ^ 1)])


def test_the_grid():
    cases = list(CC.grid())
    assert len(cases) == len(set(cases)) and {c[0] for c in cases} == set(CC.KINDS)
    for kind, N, E, n, start in cases:
        assert 1 <= n <= N and 0 <= start < N and E in CC.ES
    for N in CC.NS:
        assert CC.counts(N) == tuple(sorted({1, 2, -(-N // 10), N} & set(range(1, N + 1))))
    assert {(2738, 274), (2738, 2738), (1, 1), (65, 7), (257, 26)} <= {(c[1], c[3]) for c in cases if c[0] == "random"}
    assert any(c[4] > 0 for c in cases)


# ------------------------------------------------------------------------------------------------- the library
def err():
    return _lib.load().aaclip_last_error().decode()


def test_symbols_and_python_surface():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert lib.aaclip_version() == _lib.ABI_VERSION                         # additions: the ABI number stays
    assert engine.CoresetBank._fields == ("rows", "form", "patches", "shots", "index", "radius2", "dim")
    assert engine.CoresetBank._fields[:4] == engine.SupportBank._fields
    pack = open(os.path.join(CSRC, "coreset_pack.h")).read()
    assert f"CORESET_SCALE_EXP = {engine.CORESET_SCALE_EXP};" in pack and engine.CORESET_NORM2_LIMIT == 1 << 29
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "coreset.hip" in make and "coreset_pack.h" in make
    assert inspect.signature(engine.coreset_select).parameters["start"].default == 0
    p = inspect.signature(engine.support_bank_coreset).parameters
    assert list(p) == ["seg_tokens_per_image_batch", "form", "ratio", "dim", "seed"] and p["dim"].default == 128 and p["seed"].default == 0
    cpu = torch.zeros(2, 4, 64)
    for call in (lambda: engine.coreset_rows(cpu[0]), lambda: engine.coreset_unit_rows(cpu[0]),
                 lambda: engine.coreset_select(cpu[0].to(torch.int16), torch.zeros(4, dtype=torch.int32), 2),
                 lambda: engine.support_bank_coreset([[cpu]], "fp32", 0.5, dim=0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for ratio in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ratio"):
            engine.support_bank_coreset([[cpu]], "fp32", ratio)
    w = engine.coreset_projection(64, 128, seed=0)
    assert w.shape == (128, 64) and torch.equal(w, engine.coreset_projection(64, 128, seed=0))
    assert not torch.equal(w, engine.coreset_projection(64, 128, seed=1)) and abs(float(w.std()) - 128 ** -0.5) < 0.01


def test_workspace_sizes_and_rejections():
    lib = _lib.load()
    fn = lib.aaclip_coreset_select_workspace_bytes
    for vary in ("N", "E", "n"):
        base = dict(N=300000, E=128, n=100)
        got = []
        for v in {"N": (100, 2738, 286121, 2 ** 31 - 1), "E": (32, 128, 768, 1024), "n": (1, 2, 31, 32, 100)}[vary]:
            got.append(fn(*dict(base, **{vary: v}).values()))
        assert got[0] > 0 and all(b >= a for a, b in zip(got, got[1:])), (vary, got)          # monotonic in each argument
    assert 8 * 28614 <= fn(286121, 128, 28613) <= 8 * 28614 + 256                            # one word per pick, and word 0
    for bad in ((0, 64, 1), (-1, 64, 1), (2 ** 31, 64, 1), (5, 0, 1), (5, 16, 1), (5, 48, 1), (5, 1056, 1), (5, 64, 0),
                (5, 64, 6), (5, 64, -1)):
        assert fn(*bad) == 0, bad
    P = 1 << 20
    Q, NORM, PICKS, RAD, MIN, WS, ROWS = (P + (k << 26) for k in range(1, 8))
    N, E, n = 257, 64, 26
    need = fn(N, E, n)

    def call(**kw):
        a = dict(q=Q, norm2=NORM, N=N, E=E, n=n, start=0, picks=PICKS, radius2=RAD, min_d2=MIN, ws=WS, ws_bytes=need, stream=None)
        a.update(kw)
        return lib.aaclip_coreset_select(*a.values())

    for kw, msg in [(dict(q=None), "null pointer"), (dict(norm2=None), "null pointer"), (dict(picks=None), "null pointer"),
                    (dict(radius2=None), "null pointer"), (dict(min_d2=None), "null pointer"), (dict(ws=None), "null pointer"),
                    (dict(N=0), "N must be"), (dict(N=2 ** 31), "N must be"), (dict(E=16), "E must be"), (dict(E=72), "E must be"),
                    (dict(E=2048), "E must be"), (dict(n=0), "n must be"), (dict(n=N + 1), "n must be"),
                    (dict(start=-1), "start must be"), (dict(start=N), "start must be"), (dict(q=Q + 8), "aligned"),
                    (dict(norm2=NORM + 2), "aligned"), (dict(picks=PICKS + 1), "aligned"), (dict(radius2=RAD + 2), "aligned"),
                    (dict(min_d2=MIN + 3), "aligned"), (dict(ws=WS + 4), "aligned"), (dict(ws_bytes=need - 1), "workspace too small"),
                    (dict(ws_bytes=0), "workspace too small"), (dict(picks=RAD + 4 * n), "must not overlap"),
                    (dict(radius2=MIN + 4 * N - 4), "must not overlap"), (dict(min_d2=NORM), "must not overlap"),
                    (dict(ws=Q + 2 * N * E - 8), "must not overlap"), (dict(picks=WS + 8), "must not overlap")]:
        assert call(**kw) == -1, kw
        assert err().startswith("coreset_select:") and msg in err(), (kw, err(), msg)
    for args, msg in [((None, N, E, Q, NORM, None), "null pointer"), ((ROWS, 0, E, Q, NORM, None), "N must be"),
                      ((ROWS, N, 40, Q, NORM, None), "E must be"), ((ROWS + 4, N, E, Q, NORM, None), "aligned"),
                      ((ROWS, N, E, Q + 2, NORM, None), "aligned"), ((ROWS, N, E, ROWS + 64, NORM, None), "must not overlap")]:
        assert lib.aaclip_coreset_rows(*args) == -1 and err().startswith("coreset_rows:") and msg in err(), (args, err())
    assert lib.aaclip_coreset_unit_rows(ROWS, N, E, ROWS + 64, None) == -1 and "must not overlap" in err()
    assert lib.aaclip_coreset_unit_rows(ROWS, N, 40, Q, None) == -1 and "E must be" in err()


def test_coreset_pack_header_under_the_sanitizers(tmp_path):
    """csrc/coreset_pack.h as coreset.hip uses it, in a host program of its own with ASan + UBSan: the quantiser, the
    candidate merge in shuffled orders and the whole selection, equal to plain loops; no report from either sanitizer"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "coreset_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(CSRC, "coreset_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime of the host compiler is not installed: " + build.stderr.strip()[-200:])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and not run.stderr, (run.returncode, run.stdout, run.stderr)


# ------------------------------------------------------------------------------------------------- the script
def test_eval_coreset_parser_and_the_path_without_coreset(monkeypatch, capsys):
    import eval_coreset as EC
    import eval_last as EL
    import eval_support as ES
    parse = EC.build_parser().parse_args
    a = parse([])
    assert a.support_coreset is None and a.support_coreset_dim == 128 and a.support is None
    a = parse(["--support", "8", "--support_coreset", "0.1", "--support_coreset_dim", "0", "--support_meta", "m.jsonl"])
    assert (a.support, a.support_coreset, a.support_coreset_dim, a.support_meta) == (8, 0.1, 0, "m.jsonl")
    for name in ("support_coreset", "support_coreset_dim"):
        assert not hasattr(ES.build_parser().parse_args([]), name)          # eval_support.py's arguments stay what they were
    defaults = {k: v for k, v in vars(parse([])).items() if not k.startswith("support_coreset")}
    assert defaults == vars(ES.build_parser().parse_args([]))

    rows = [{"class name": "a", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0}] * 2
    calls = []

    def fake_run(parser, argv=None, table=None, finish=None):
        args = parser.parse_args(argv)
        calls.append((argv, table, finish is not None, getattr(args, "support", None), getattr(args, "support_coreset", None),
                      getattr(args, "support_coreset_dim", None)))
        print((table or EL.format_table)(rows))
        return rows

    monkeypatch.setattr(EL, "run", fake_run)
    for argv in ([], ["--f1max"], ["--support", "4", "--defects"], ["--aupro", "--device_metrics"]):
        del calls[:]
        assert ES.main(list(argv)) == rows
        want_calls, want_out = list(calls), capsys.readouterr().out
        del calls[:]
        assert EC.main(list(argv)) == rows
        assert capsys.readouterr().out == want_out and want_out                           # byte for byte
        assert [c[:4] for c in calls] == [c[:4] for c in want_calls] and calls[0][4] is None
    del calls[:]
    EC.main(["--support", "4", "--support_coreset", "0.25"])
    assert calls[0][3:] == (4, 0.25, 128)
    for bad in (["--support_coreset", "0.1"], ["--support", "4", "--support_coreset", "0"],
                ["--support", "4", "--support_coreset", "1.5"], ["--support", "4", "--support_coreset", "-0.1"],
                ["--support", "4", "--support_coreset", "0.1", "--support_coreset_dim", "100"],
                ["--support", "0", "--support_coreset", "0.1"]):
        with pytest.raises(SystemExit):
            EC.main(bad)
    sig = inspect.signature(EC.evaluate).parameters
    assert list(sig)[:len(inspect.signature(ES.evaluate).parameters)] == list(inspect.signature(ES.evaluate).parameters)
    assert sig["coreset"].default is None and sig["coreset_dim"].default == 128


def test_support_nearest_pairs_through_an_index():
    import eval_last as EL
    P = 6
    full = engine.SupportBank([torch.zeros(4 * P, 8)] * 2, 0, P, 4)
    nearest = [[torch.tensor([[0, 5, 23, 7, 6, 12]], dtype=torch.int32), torch.tensor([[1, 1, 2, 3, 4, 5]], dtype=torch.int32)],
               [torch.tensor([[11, 0, 0, 0, 0, 18]], dtype=torch.int32), torch.tensor([[0, 0, 0, 0, 0, 0]], dtype=torch.int32)]]
    plain = EL._support_nearest_pairs(nearest, full, 1)
    assert [p.shape for p in plain] == [(2, P, 2)] * 2 and plain[0].dtype == np.int32
    assert plain[0][0].tolist() == [[0, 0], [0, 5], [3, 5], [1, 1], [1, 0], [2, 0]]
    # a coreset of 5 rows per level: the nearest row counts kept rows, the pairs name rows of the full bank
    index = [torch.tensor([0, 23, 7, 13, 18], dtype=torch.int32), torch.tensor([5, 6, 12, 1, 20], dtype=torch.int32)]
    core = engine.CoresetBank([torch.zeros(5, 8)] * 2, 0, P, 4, index, [np.zeros(6, np.uint32)] * 2, 0)
    near = [[torch.tensor([[0, 1, 2, 3, 4, 4]], dtype=torch.int32), torch.tensor([[4, 3, 2, 1, 0, 0]], dtype=torch.int32)]]
    got = EL._support_nearest_pairs(near, core, 1)
    assert got[0][0].tolist() == [[0, 0], [3, 5], [1, 1], [2, 1], [3, 0], [3, 0]] and got[0].dtype == np.int32
    assert got[1][0].tolist() == [[3, 2], [0, 1], [2, 0], [1, 0], [0, 5], [0, 5]]
    assert [g.shape for g in EL._support_nearest_pairs(None, core, 1)] == [(0, P, 2)] * 2


def test_coreset_none_leaves_the_bank_builders_as_they_were(monkeypatch):
    import eval_last as EL
    import forward_utils as FU
    for fn in (EL.support_banks, FU.build_support_bank):
        p = inspect.signature(fn).parameters
        assert p["coreset"].default is None and p["coreset_dim"].default == 128 and list(p)[-2:] == ["coreset", "coreset_dim"]
    assert list(inspect.signature(FU.build_support_bank).parameters)[:3] == ["model", "images", "form"]
    assert list(inspect.signature(EL.support_banks).parameters)[:8] == ["model", "image_datasets", "k", "device", "img_size", "form",
                                                                        "support_datasets", "batch_size"]

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, image, text_embeddings=None):
            return [image[:, :, :4, 0].reshape(image.shape[0], 6, 2)], None, None

    calls = []
    monkeypatch.setattr(engine, "support_bank", lambda tokens, form: calls.append(("full", len(tokens), form)) or "full bank")
    monkeypatch.setattr(engine, "support_bank_coreset",
                        lambda tokens, form, ratio, dim=128, seed=0: calls.append(("coreset", len(tokens), form, ratio, dim, seed)) or "coreset bank")
    images = [torch.zeros(2, 3, 4, 4), torch.ones(1, 3, 4, 4)]
    assert FU.build_support_bank(Model(), images) == "full bank"
    assert FU.build_support_bank(Model(), images, "fp16", coreset=None, coreset_dim=0) == "full bank"
    assert calls == [("full", 2, "fp32"), ("full", 2, "fp16")]
    del calls[:]
    assert FU.build_support_bank(Model(), images, "fp16", coreset=0.25) == "coreset bank"
    assert FU.build_support_bank(Model(), images, None, coreset=1.0, coreset_dim=0) == "coreset bank"
    assert calls == [("coreset", 2, "fp16", 0.25, 128, 0), ("coreset", 2, "fp32", 1.0, 0, 0)]

    # support_banks hands build_support_bank exactly today's arguments without a coreset
    seen = []
    monkeypatch.setattr(FU, "build_support_bank", lambda *a, **k: seen.append((len(a), a[2], k)) or "bank")

    class Shots(torch.utils.data.Dataset):
        def __len__(self):
            return 3

        def __getitem__(self, i):
            return {"image": torch.zeros(3, 4, 4)}

    class DS:
        def support_split(self, k):
            return Shots(), "rest"

    banks, evaluated = EL.support_banks(Model(), {"a": DS()}, 3, "cpu", 4, form="fp32")
    assert banks == {"a": "bank"} and evaluated == {"a": "rest"} and seen == [(3, "fp32", {})]
    del seen[:]
    EL.support_banks(Model(), {"a": DS()}, 3, "cpu", 4, coreset=0.1, coreset_dim=0)
    assert seen == [(3, None, {"coreset": 0.1, "coreset_dim": 0})]
