"""CPU side of the exact F1-max (aaclip_metrics_f1max, aaclip_metrics_threshold): forward_utils.f1max_eval against a
brute-force sweep over every distinct threshold (tests/f1max_cases.py) and against sklearn's precision_recall_curve; the
exact-tie rule; the new C ABI symbols, workspace queries and every argument rejection that needs no device;
metrics_eval's, eval_last's and eval_metrics' surface.

Bar against sklearn: its value nanmax(2 p r / (p + r)) passes through about six fp64 roundings (two divisions for p and
r, a product, a doubling that is exact, a sum, a division: <= 7e-16 relative on a value <= 1); the bar is 1e-12 absolute.
Counts and thresholds are compared with the brute force for EQUALITY."""
import inspect
import os

import numpy as np
import pytest
import torch

import f1max_cases as FC
from aaclip_hip import _lib, engine
from conftest import GOLDEN
from metrics_cases import KEYS, derive_cases

NEW_SYMBOLS = ["aaclip_metrics_f1max_workspace_bytes", "aaclip_metrics_f1max",
               "aaclip_metrics_threshold_workspace_bytes", "aaclip_metrics_threshold"]


# ---------------------------------------------------------------------------------------------------- f1max_eval
def random_sets():
    """40 score sets of 2 .. 5000 elements: untied, tied on grids of several widths, few and many positives"""
    rng = np.random.default_rng(2024)
    for k in range(40):
        n = int(rng.choice([2, 3, 7, 64, 257, 1000, 5000]))
        labels = (rng.random(n) < rng.choice([0.05, 0.3, 0.7])).astype(np.uint8)
        labels[0], labels[1] = 1, 0
        scores = rng.normal(size=n) + rng.choice([0.0, 0.8, 2.0]) * labels
        levels = int(rng.choice([0, 4, 16, 256]))
        if levels:
            scores = np.round(scores * levels) / levels
        yield labels, scores.astype(np.float32 if k % 2 else np.float64)


def test_f1max_eval_equals_the_brute_force_sweep_and_sklearn():
    import forward_utils as FU
    from sklearn.metrics import precision_recall_curve
    worst = 0.0
    for labels, scores in random_sets():
        got = FU.f1max_eval(labels, scores)
        tp, fp, fn, threshold, groups = FC.brute_force(labels, scores)
        assert (got.tp, got.fp, got.fn, got.groups) == (tp, fp, fn, groups)
        assert got.threshold == threshold and got.f1 == 2 * tp / (2 * tp + fp + fn)
        assert got.precision == tp / (tp + fp) and got.recall == tp / (tp + fn)
        flagged = scores >= scores.dtype.type(got.threshold)
        assert int(np.count_nonzero(flagged & (labels != 0))) == tp and int(np.count_nonzero(flagged)) == tp + fp
        p, r, _ = precision_recall_curve(labels, scores)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = float(np.nanmax(2 * p * r / (p + r)))
        worst = max(worst, abs(got.f1 - want))
        assert abs(got.f1 - want) <= 1e-12
    print("worst difference to sklearn", worst)


def test_exact_tie_goes_to_the_higher_score():
    """descending labels 1,0,0,0,0,1 with the first two tied: F1 = 2 / 4 after 2 elements, 4 / 8 after all 6"""
    import forward_utils as FU
    scores = np.array([0.9, 0.9, 0.7, 0.6, 0.5, 0.1], np.float32)
    labels = np.array([1, 0, 0, 0, 0, 1])
    got = FU.f1max_eval(labels, scores)
    assert (got.f1, got.tp, got.fp, got.fn, got.groups) == (0.5, 1, 1, 1, 5)
    assert got.threshold == float(np.float32(0.9)) and (got.precision, got.recall) == (0.5, 0.5)
    assert FC.brute_force(labels, scores)[:4] == (1, 1, 1, float(np.float32(0.9)))
    for k in FC.TIE_K[:3]:
        s, l = FC.exact_tie(k)
        got = FU.f1max_eval(l, s)
        assert (got.f1, got.tp, got.fp, got.fn, got.threshold, got.groups) == (0.5, k, k, k, 1.0, 4 * k + 1)


def test_f1max_eval_zero_signs_and_refusals():
    import forward_utils as FU
    scores = np.array([-0.0, 0.0, -1.0, -2.0, 3.0], np.float32)
    labels = np.array([1, 1, 0, 0, 1])
    got = FU.f1max_eval(labels, scores)
    assert (got.f1, got.tp, got.fp) == (1.0, 3, 0) and got.threshold == 0.0 and not np.signbit(got.threshold)
    assert got.groups == 4
    for bad in (np.zeros(5), np.ones(5)):
        with pytest.raises(ValueError, match="one class"):
            FU.f1max_eval(bad, scores)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            FU.f1max_eval(labels, np.where(np.arange(5) == 2, bad, scores))
    with pytest.raises(ValueError, match="labels for"):
        FU.f1max_eval(labels[:4], scores)
    assert engine.F1Max._fields == ("f1", "threshold", "tp", "fp", "fn", "precision", "recall", "groups")


# ------------------------------------------------------------------------------------------------- the library
def err():
    return _lib.load().aaclip_last_error().decode()


def test_symbols_and_abi():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aaclip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    for name in ("aaclip_metrics_f1max_record", "aaclip_metrics_threshold_record"):
        assert name in header
    assert lib.aaclip_version() == 10 == _lib.ABI_VERSION
    assert engine.F1MAX_RECORD_WORDS * 8 == 56 and engine.THRESHOLD_RECORD_WORDS * 8 == 32
    assert engine.CurveMetrics._fields == ("auroc", "ap", "P", "N", "image_max", "num", "groups")
    assert list(inspect.signature(engine.curve_metrics).parameters) == ["scores", "labels", "per_image", "record", "normalise"]


def test_workspace_sizes():
    lib = _lib.load()
    sizes = [2, 3, 64, 65, 4095, 4096, 4097, 27648, 2 ** 20 + 3, 170 * 518 * 518, 2 ** 31 - 1]
    for fn in (lib.aaclip_metrics_f1max_workspace_bytes, lambda n: lib.aaclip_metrics_threshold_workspace_bytes(n, 0)):
        got = [fn(n) for n in sizes]
        assert got[0] > 0 and all(b >= a for a, b in zip(got, got[1:])), got
        assert fn(0) == fn(1) == fn(2 ** 31) == fn(-5) == 0
    n = 170 * 518 * 518
    assert 8 * n <= lib.aaclip_metrics_f1max_workspace_bytes(n) <= 8.1 * n         # 8 bytes per possible tie group
    per = [lib.aaclip_metrics_threshold_workspace_bytes(k * 518 * 518, 518 * 518) for k in (1, 2, 12, 170)]
    assert per[0] > 0 and all(b >= a for a, b in zip(per, per[1:])) and per[-1] <= 1 << 20
    assert lib.aaclip_metrics_threshold_workspace_bytes(100, 7) == 0
    assert lib.aaclip_metrics_threshold_workspace_bytes(100, -1) == 0
    # the curve's own workspace is what it was
    assert 8 * n <= lib.aaclip_metrics_curve_workspace_bytes(n) <= 8.1 * n


P = 1 << 20          # a non-null, 16-byte aligned address: every call below is refused before anything reads it
FAR = P + (1 << 26)
WS = P + (1 << 27)
BIG = 1 << 40        # a workspace size that is never the reason


def test_f1max_rejections():
    lib = _lib.load()
    n = 27648
    need = lib.aaclip_metrics_f1max_workspace_bytes(n)
    for args, msg in [((None, None, n, 1, FAR, WS, need, None), "null pointer"),
                      ((P, None, n, 1, None, WS, need, None), "null pointer"),
                      ((P, None, n, 1, FAR, None, need, None), "null pointer"),
                      ((P, None, n, 3, FAR, WS, need, None), "packed must be"),
                      ((P, None, n, 0, FAR, WS, need, None), "labels_sorted is required"),
                      ((P, None, 1, 1, FAR, WS, BIG, None), "n must be"),
                      ((P, None, 2 ** 31, 1, FAR, WS, BIG, None), "n must be"),
                      ((P + 1, None, n, 1, FAR, WS, need, None), "aligned"),
                      ((P, None, n, 1, FAR + 4, WS, need, None), "aligned"),
                      ((P, None, n, 1, FAR, WS + 4, need, None), "aligned"),
                      ((WS + 64, None, n, 1, FAR, WS, need, None), "must not overlap one another"),
                      ((P, None, n, 1, WS + need - 8, WS, need, None), "must not overlap one another"),
                      ((P, None, n, 1, P + 4 * n - 8, WS, need, None), "must not overlap one another"),
                      ((P, WS + 3, n, 0, FAR, WS, need, None), "must not overlap one another"),
                      ((P, FAR - 1, n, 0, FAR, WS, need, None), "must not overlap one another"),
                      ((P, None, n, 1, FAR, WS, need - 1, None), "workspace too small")]:
        assert lib.aaclip_metrics_f1max(*args) == -1
        assert err().startswith("metrics_f1max:") and msg in err(), (err(), msg)


def test_threshold_rejections():
    lib = _lib.load()
    per = 2304
    n = 12 * per
    need = lib.aaclip_metrics_threshold_workspace_bytes(n, per)
    lab, rng, f1 = FAR, FAR + (1 << 20), FAR + (2 << 20)
    mask, cnt, tot = FAR + (3 << 20), FAR + (4 << 20), FAR + (5 << 20)
    ok = (P, lab, n, per, rng, f1, mask, cnt, tot, WS, need, None)

    def call(**change):
        names = ["scores", "labels", "n", "per_image", "range", "f1", "mask", "counts", "totals", "ws", "ws_bytes", "stream"]
        args = list(ok)
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.aaclip_metrics_threshold(*args)

    for change, msg in [(dict(scores=None), "null pointer"), (dict(f1=None), "null pointer"), (dict(ws=None), "null pointer"),
                        (dict(mask=None, counts=None, totals=None), "no output"),
                        (dict(n=1, per_image=0, counts=None, ws_bytes=BIG), "n must be"),
                        (dict(n=2 ** 31, per_image=0, counts=None, ws_bytes=BIG), "n must be"),
                        (dict(per_image=7, ws_bytes=BIG), "multiple of per_image"),
                        (dict(per_image=-1, ws_bytes=BIG), "multiple of per_image"),
                        (dict(labels=None), "per-image counts need labels"),
                        (dict(per_image=0, ws_bytes=BIG), "per-image counts need labels"),
                        (dict(scores=P + 2), "aligned"), (dict(counts=cnt + 2), "aligned"), (dict(range=rng + 4), "aligned"),
                        (dict(f1=f1 + 4), "aligned"), (dict(totals=tot + 4), "aligned"), (dict(ws=WS + 4), "aligned"),
                        (dict(mask=P + 4 * n - 1), "must not overlap"), (dict(mask=lab + n - 1), "must not overlap"),
                        (dict(mask=cnt - 1), "must not overlap"), (dict(mask=tot + 31), "must not overlap"),
                        (dict(mask=f1 + 55), "must not overlap"), (dict(mask=rng + 23), "must not overlap"),
                        (dict(mask=WS + need - 1), "must not overlap"), (dict(counts=tot - 16 * 12 + 4), "must not overlap"),
                        (dict(counts=P), "must not overlap"), (dict(totals=f1 + 48), "must not overlap"),
                        (dict(totals=WS + 8), "must not overlap"), (dict(range=WS + need - 8), "must not overlap"),
                        (dict(scores=WS + 4), "must not overlap"), (dict(labels=WS + 1), "must not overlap"),
                        (dict(ws_bytes=need - 1), "workspace too small")]:
        assert call(**change) == -1, change
        assert err().startswith("metrics_threshold:") and msg in err(), (change, err(), msg)
    # a one-byte-short workspace is the LAST check: with an overlap as well, the overlap is named
    assert call(ws_bytes=need - 1, totals=WS + 8) == -1 and "must not overlap" in err()


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import forward_utils as FU
    scores, labels = torch.rand(16), torch.zeros(16, dtype=torch.uint8)
    for call in (lambda: engine.f1max_metrics(scores, labels),
                 lambda: engine.metrics_f1max(torch.zeros(16, dtype=torch.int32), None, True),
                 lambda: engine.metrics_threshold(scores, 0.5),
                 lambda: FU.f1max_eval_device(labels, scores)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    sig = inspect.signature(engine.f1max_metrics).parameters
    assert [(k, v.default) for k, v in sig.items()][2:4] == [("per_image", 0), ("normalise", True)]
    assert list(inspect.signature(engine.metrics_f1max).parameters) == ["keys", "labels_sorted", "packed", "record"]


# ------------------------------------------------------------------------------------------------- the harness
def test_metrics_eval_flag_off_is_todays_row_and_on_adds_two_keys():
    import forward_utils as FU
    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    cases = derive_cases(*[g[f"base.{k}"] for k in ("masks", "labels", "preds", "scores")])
    for name, (pl, il, pp, ip, dom) in cases.items():
        old = FU.metrics_eval(pl.copy(), il.copy(), pp.copy(), ip.copy(), name, dom)
        assert list(old) == ["class name"] + list(KEYS)
        assert np.array_equal(np.array([float(old[k]) for k in KEYS]), g[f"{name}.result"])
        assert FU.metrics_eval(pl.copy(), il.copy(), pp.copy(), ip.copy(), name, dom, f1_max=False) == old
        details = {"masks": True}
        new = FU.metrics_eval(pl.copy(), il.copy(), pp.copy(), ip.copy(), name, dom, f1_max=True, details=details)
        assert list(new) == list(old) + ["pixel F1-max", "image F1-max"] and {k: new[k] for k in old} == old
        norm = np.asarray(pp, np.float32)
        if norm.max() != 1:
            norm = (norm - norm.min()) / (norm.max() - norm.min())
        want = FU.f1max_eval(pl, norm)
        assert new["pixel F1-max"] == round(want.f1, 4) * 100 and details["pixel threshold"] == want.threshold
        assert details["masks"].dtype == np.uint8 and int(details["masks"].sum()) == want.tp + want.fp
        assert np.array_equal(details["masks"].reshape(-1), (norm.reshape(-1) >= np.float32(want.threshold)))
        if name == "one_image_class":
            assert new["image F1-max"] == 0 and details["image threshold"] is None
        else:
            assert 0 < new["image F1-max"] <= 100 and 0.0 <= details["image threshold"] <= 1.0
        with_limit = FU.metrics_eval(pl.copy(), il.copy(), pp.copy(), ip.copy(), name, dom, fpr_limit=0.3, f1_max=True)
        assert list(with_limit) == list(old) + ["pixel AUPRO", "pixel F1-max", "image F1-max"]
    for fn in (FU.metrics_eval, FU.metrics_eval_device):
        assert inspect.signature(fn).parameters["f1_max"].default is False


def test_eval_metrics_parser_and_table():
    import eval_aupro as EA
    import eval_last as EL
    import eval_metrics as EM
    import test_last as TL
    parse = EM.build_parser().parse_args
    assert not hasattr(EL.build_parser().parse_args([]), "f1max") and not hasattr(EA.build_parser().parse_args([]), "f1max")
    assert parse([]).f1max is False and parse(["--f1max"]).f1max is True and parse([]).aupro is None
    both = parse(["--f1max", "--aupro", "--device_metrics"])
    assert both.f1max and both.aupro == 0.3 and both.device_metrics
    assert vars(parse([])).keys() == vars(EA.build_parser().parse_args([])).keys() | {"f1max"}
    params = inspect.signature(EM.evaluate).parameters
    assert list(params)[:-2] == list(inspect.signature(EA.evaluate).parameters)
    assert params["f1_max"].default is False and params["return_masks"].default is False
    assert inspect.signature(EL.evaluate_rows).parameters["f1_max"].default is False
    with pytest.raises(ValueError, match="return_masks needs f1_max"):
        EM.evaluate(None, {}, {}, None, 8, "MVTec", return_masks=True)
    rows = [{"class name": "a", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0},
            {"class name": "Average", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0}]
    plain = TL.format_table(rows).split("\n")
    assert EL.format_table(rows) == TL.format_table(rows)              # no column: exactly what it printed before
    f1 = [dict(r, **{"pixel F1-max": 56.78, "image F1-max": 90.12}) for r in rows]
    lines = EL.format_table(f1).split("\n")
    assert lines[0].endswith("pixel F1-max    image F1-max") and all(line.endswith("56.78           90.12") for line in lines[1:])
    assert [line[:len(old)] for line, old in zip(lines, plain)] == plain
    aupro = [dict(r, **{"pixel AUPRO": 12.34}) for r in f1]
    lines = EL.format_table(aupro).split("\n")
    assert lines[0].endswith("pixel AUPRO    pixel F1-max    image F1-max")
    assert all(line.endswith("12.34           56.78           90.12") for line in lines[1:])
    only = EL.format_table([dict(r, **{"pixel AUPRO": 12.34}) for r in rows]).split("\n")
    assert [line[:len(o)] for line, o in zip(lines, only)] == only     # the AUPRO table is a prefix, as it was
