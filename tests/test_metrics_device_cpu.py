"""CPU side of the on-device AUROC / AP (csrc/metrics.hip): the numpy restatement of tests/metrics_device_cases.py
against sklearn (unrounded) and against the reference's own numbers (tests/golden/metrics.npz); the new C ABI symbols,
their workspace queries and every argument rejection that needs no device; the Python surface on CPU tensors; and
eval_last.load_adapters on a checkpoint in train.train_image_adapter's format.

Bounds against sklearn: the AUROC numerator is an exact integer followed by one division, sklearn's is an fp64
trapezoid sum over up to n points of a sum that is at most 1: 1e-12.  AP is an fp64 sum over the tie groups in another
association than sklearn's, n ulp-sized steps at the most: 1e-10.  test_restatement_equals_sklearn prints both."""
import copy
import os

import numpy as np
import pytest
import torch

import metrics_device_cases as MD
from aaclip_hip import _lib, engine, synth
from conftest import GOLDEN
from metrics_cases import KEYS, derive_cases

NEW_SYMBOLS = ["aaclip_metrics_range_workspace_bytes", "aaclip_metrics_range", "aaclip_metrics_normalise",
               "aaclip_metrics_sort_workspace_bytes", "aaclip_metrics_sort_group_items", "aaclip_metrics_sort",
               "aaclip_metrics_curve_workspace_bytes", "aaclip_metrics_curve"]


# ------------------------------------------------------------------------------------------------ the restatement
def test_lsd_sort_is_np_sort_and_stable():
    rng = np.random.default_rng(3)
    for n in (2, 257, 5000):
        keys = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        keys[: n // 3] = keys[n // 3: 2 * (n // 3)]                     # duplicates
        payload = np.arange(n, dtype=np.int64)
        got, order = MD.lsd_sort(keys, payload)
        assert np.array_equal(got, np.sort(keys))
        assert np.array_equal(order, np.argsort(keys, kind="stable"))


def test_keys_preserve_the_order_of_floats():
    v = np.array([-np.float32(3e38), -2.5, -1e-40, -0.0, 0.0, 1e-40, 0.25, 1.0, 7.0, 3e38], dtype=np.float32)
    keys = MD.make_keys(v, np.zeros(v.size), packed=False).astype(np.int64)
    assert keys[3] == keys[4] and np.all(np.diff(keys) >= 0) and np.count_nonzero(np.diff(keys) == 0) == 1
    unit = np.array([-0.0, 0.0, 1e-40, 0.25, 0.5, 1.0], dtype=np.float32)
    packed = MD.make_keys(unit, np.array([1, 0, 1, 0, 1, 1]), packed=True).astype(np.int64)
    assert np.all(np.diff(packed >> 1) >= 0) and (packed >> 1)[0] == (packed >> 1)[1] == 0
    assert np.array_equal(packed & 1, [1, 0, 1, 0, 1, 1]) and packed.max() < 2 ** 31


@pytest.mark.parametrize("kind", ["plain", "coarse", "passthrough"])
@pytest.mark.parametrize("n", [2, 65, 4097, 27648])
def test_restatement_equals_sklearn(n, kind):
    from sklearn.metrics import average_precision_score, roc_auc_score
    scores, labels = MD.inputs(n, kind)
    got = MD.expected(n, kind)
    norm = MD.normalise(scores)
    assert got["packed"] == (kind != "passthrough")
    assert np.array_equal(got["keys"], np.sort(got["keys"]))
    assert got["P"] == int(labels.sum()) and got["P"] + got["N"] == n
    assert got["groups"] == np.unique(norm + np.float32(0)).size
    d_auc = abs(got["auroc"] - roc_auc_score(labels, norm))
    d_ap = abs(got["ap"] - average_precision_score(labels, norm))
    print(n, kind, "auroc diff", d_auc, "ap diff", d_ap)
    assert d_auc <= 1e-12 and d_ap <= 1e-10


def test_restatement_tie_structure():
    n = 1000
    labels = np.zeros(n, np.uint8)
    labels[600:] = 1
    up = np.linspace(0, 1, n).astype(np.float32)
    assert MD.curve_metrics(up, labels)["auroc"] == 1.0 and MD.curve_metrics(up[::-1].copy(), labels)["auroc"] == 0.0
    assert MD.curve_metrics(up, labels)["ap"] == 1.0
    one = np.zeros(n, np.uint8)
    one[123] = 1
    r = MD.curve_metrics(up, one)
    assert r["P"] == 1 and r["num"] == 2 * 123 and r["groups"] == n


def test_restatement_equals_reference_golden():
    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    cases = derive_cases(*[g[f"base.{k}"] for k in ("masks", "labels", "preds", "scores")])
    assert len(cases) == 8
    for name, (pl, il, pp, ip, dom) in cases.items():
        r = MD.metrics_eval_restated(pl.copy(), il.copy(), pp.copy(), ip.copy(), name, dom)
        got = np.array([float(r[k]) for k in KEYS])
        assert np.array_equal(got, g[f"{name}.result"]), (name, got, g[f"{name}.result"])


# ------------------------------------------------------------------------------------------------- the library
def err():
    return _lib.load().aaclip_last_error().decode()


def test_symbols_and_abi():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aaclip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert lib.aaclip_version() == 10 == _lib.ABI_VERSION
    assert lib.aaclip_metrics_sort_group_items() % 64 == 0 and lib.aaclip_metrics_sort_group_items() > 0


def test_workspace_sizes():
    lib = _lib.load()
    sizes = [2, 3, 64, 65, 8191, 8192, 8193, 27648, 2 ** 20 + 3, 170 * 518 * 518, 2 ** 31 - 1]
    for fn in (lib.aaclip_metrics_sort_workspace_bytes, lib.aaclip_metrics_curve_workspace_bytes,
               lambda n: lib.aaclip_metrics_range_workspace_bytes(n, 0)):
        got = [fn(n) for n in sizes]
        assert got[0] > 0 and all(b >= a for a, b in zip(got, got[1:])), got
        assert fn(0) == fn(1) == fn(2 ** 31) == fn(-5) == 0
    # the sort holds a second copy of the keys and of the labels; the curve holds 8 bytes per possible tie group
    n = 170 * 518 * 518
    assert 5 * n <= lib.aaclip_metrics_sort_workspace_bytes(n) <= 6 * n
    assert 8 * n <= lib.aaclip_metrics_curve_workspace_bytes(n) <= 8.1 * n
    per = [lib.aaclip_metrics_range_workspace_bytes(k * 2304, 2304) for k in (1, 2, 12, 170)]
    assert per[0] > 0 and all(b >= a for a, b in zip(per, per[1:]))
    assert lib.aaclip_metrics_range_workspace_bytes(100, 7) == 0 and lib.aaclip_metrics_range_workspace_bytes(100, -1) == 0


P = 1 << 20          # a non-null, 16-byte aligned address: every call below is refused before anything reads it
FAR = P + (1 << 26)
WS = P + (1 << 27)
BIG = 1 << 40        # a workspace size that is never the reason


def test_range_and_normalise_rejections():
    lib = _lib.load()
    n = 4608
    need = lib.aaclip_metrics_range_workspace_bytes(n, 2304)
    lab, imax, rec = FAR, FAR + (1 << 22), FAR + (1 << 23)
    for args, msg in [((None, lab, n, 2304, imax, rec, WS, need, None), "null pointer"),
                      ((P, lab, n, 2304, imax, None, WS, need, None), "null pointer"),
                      ((P, lab, n, 2304, imax, rec, None, need, None), "null pointer"),
                      ((P, lab, 1, 0, None, rec, WS, BIG, None), "n must be"),
                      ((P, lab, 2 ** 31, 0, None, rec, WS, BIG, None), "n must be"),
                      ((P, lab, n, 7, imax, rec, WS, BIG, None), "multiple of per_image"),
                      ((P, lab, n, -1, None, rec, WS, BIG, None), "multiple of per_image"),
                      ((P, lab, n, 0, imax, rec, WS, BIG, None), "image maxima need per_image"),
                      ((P + 2, lab, n, 2304, imax, rec, WS, need, None), "aligned"),
                      ((P, lab, n, 2304, imax, rec + 4, WS, need, None), "aligned"),
                      ((P, lab, n, 2304, imax, rec, P + 64, need, None), "must not overlap"),
                      ((P, lab, n, 2304, imax, WS + 8, WS, need, None), "must not overlap"),
                      ((P, lab, n, 2304, P + 128, rec, WS, need, None), "must not overlap"),
                      ((P, lab, n, 2304, rec, rec, WS, need, None), "must not overlap"),
                      ((P, WS + 1, n, 2304, imax, rec, WS, need, None), "must not overlap"),
                      ((P, lab, n, 2304, imax, rec, WS, need - 1, None), "workspace too small")]:
        assert lib.aaclip_metrics_range(*args) == -1
        assert err().startswith("metrics_range:") and msg in err(), (err(), msg)
    for args, msg in [((None, FAR, n, WS, None), "null pointer"), ((P, FAR, n, None, None), "null pointer"),
                      ((P, FAR, 0, WS, None), "n must be"), ((P, FAR, 2 ** 31, WS, None), "n must be"),
                      ((P, FAR + 1, n, WS, None), "aligned"), ((P, P + 4, n, WS, None), "overlap")]:
        assert lib.aaclip_metrics_normalise(*args) == -1
        assert err().startswith("metrics_normalise:") and msg in err(), (err(), msg)


def test_sort_and_curve_rejections():
    lib = _lib.load()
    n = 27648
    need = lib.aaclip_metrics_sort_workspace_bytes(n)
    keys, labs, bad, lab_in = FAR, FAR + (1 << 22), FAR + (1 << 23), FAR + (1 << 24)
    for args, msg in [((None, lab_in, n, 1, keys, None, bad, WS, need, None), "null pointer"),
                      ((P, None, n, 1, keys, None, bad, WS, need, None), "null pointer"),
                      ((P, lab_in, n, 1, keys, None, None, WS, need, None), "null pointer"),
                      ((P, lab_in, n, 2, keys, labs, bad, WS, need, None), "packed must be"),
                      ((P, lab_in, n, 0, keys, None, bad, WS, need, None), "labels_sorted is required"),
                      ((P, lab_in, 1, 1, keys, None, bad, WS, BIG, None), "n must be"),
                      ((P, lab_in, 2 ** 31, 1, keys, None, bad, WS, BIG, None), "n must be"),
                      ((P, lab_in, n, 1, keys + 2, None, bad, WS, need, None), "aligned"),
                      ((P, lab_in, n, 1, keys, None, bad + 4, WS, need, None), "aligned"),
                      ((P, lab_in, n, 1, P, None, bad, WS, need, None), "overlap"),
                      ((P, lab_in, n, 0, keys, lab_in + 5, bad, WS, need, None), "overlap"),
                      ((P, lab_in, n, 1, WS + 256, None, bad, WS, need, None), "must not overlap one another"),
                      ((P, lab_in, n, 0, keys, WS + need - 1, bad, WS, need, None), "must not overlap one another"),
                      ((P, lab_in, n, 1, keys, None, WS + 8, WS, need, None), "must not overlap one another"),
                      ((WS + 4, lab_in, n, 1, keys, None, bad, WS, need, None), "must not overlap one another"),
                      ((P, lab_in, n, 1, keys, None, keys + 8, WS, need, None), "must not overlap one another"),
                      ((P, lab_in, n, 0, keys, keys + 4, bad, WS, need, None), "must not overlap one another"),
                      ((P, lab_in, n, 1, keys, None, bad, WS, need - 1, None), "workspace too small")]:
        assert lib.aaclip_metrics_sort(*args) == -1
        assert err().startswith("metrics_sort:") and msg in err(), (err(), msg)
    need = lib.aaclip_metrics_curve_workspace_bytes(n)
    for args, msg in [((None, None, n, 1, FAR, WS, need, None), "null pointer"),
                      ((P, None, n, 1, None, WS, need, None), "null pointer"),
                      ((P, None, n, 3, FAR, WS, need, None), "packed must be"),
                      ((P, None, n, 0, FAR, WS, need, None), "labels_sorted is required"),
                      ((P, None, 1, 1, FAR, WS, BIG, None), "n must be"),
                      ((P, None, 2 ** 31, 1, FAR, WS, BIG, None), "n must be"),
                      ((P + 1, None, n, 1, FAR, WS, need, None), "aligned"),
                      ((P, None, n, 1, FAR, WS + 4, need, None), "aligned"),
                      ((WS + 64, None, n, 1, FAR, WS, need, None), "must not overlap one another"),
                      ((P, None, n, 1, WS + need - 8, WS, need, None), "must not overlap one another"),
                      ((P, None, n, 1, P + 16, WS, need, None), "must not overlap one another"),
                      ((P, WS + 3, n, 0, FAR, WS, need, None), "must not overlap one another"),
                      ((P, None, n, 1, FAR, WS, need - 1, None), "workspace too small")]:
        assert lib.aaclip_metrics_curve(*args) == -1
        assert err().startswith("metrics_curve:") and msg in err(), (err(), msg)


def test_python_surface_refuses_cpu_tensors():
    import forward_utils as FU
    scores, labels = torch.rand(16), torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.curve_metrics(scores, labels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.metrics_range(scores)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.metrics_sort(scores, labels, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FU.metrics_eval_device(torch.zeros(2, 4, 4), np.array([0, 1]), torch.rand(2, 4, 4), np.array([0.1, 0.9]), "x",
                               "Industrial")
    assert engine.CurveMetrics._fields[:5] == ("auroc", "ap", "P", "N", "image_max")


# ------------------------------------------------------------------------------------------------ load_adapters
def tiny_adapted(seed):
    from model.adapter import AdaptedCLIP
    from model.model import CLIP
    cfg = synth.tiny_cfg()
    clip = CLIP(cfg.embed_dim,
                dict(image_size=cfg.image_size, layers=cfg.vision.layers, width=cfg.vision.width,
                     patch_size=cfg.patch_size),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=cfg.text.width, heads=cfg.text.heads,
                     layers=cfg.text.layers), precision="fp32")
    model = AdaptedCLIP(clip, text_adapt_until=1, image_adapt_until=2, levels=[2, 3], relu=False)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():                                 # a branch no seeded initialisation gives
        for name in __import__("train").IQM_BRANCH_MODULES:
            for p in getattr(model, name).parameters():
                p.add_(torch.randn(p.shape, generator=gen) * 0.25)
    return cfg, model


def branch_equal(a, b):
    import train
    sa, sb = train.iqm_branch_state(a), train.iqm_branch_state(b)
    return all(set(sa[m]) == set(sb[m]) and all(torch.equal(sa[m][k], sb[m][k]) for k in sa[m]) for m in sa)


def test_load_adapters_restores_the_trained_iqm_branch(tmp_path, caplog):
    import logging
    import eval_last as EL
    import train
    cfg, trained = tiny_adapted(seed=1)
    state = {"epoch": 3, "image_adapter": trained.image_adapter.state_dict(), "image_optimizer": {"stub": 1},
             "iqm_branch": copy.deepcopy(train.iqm_branch_state(trained))}      # train_image_adapter's checkpoint
    torch.save(state, tmp_path / "image_adapter_3.pth")
    torch.save(dict(state, epoch=2, iqm_branch=train.iqm_branch_state(tiny_adapted(seed=5)[1])),
               tmp_path / "image_adapter_2.pth")
    _, fresh = tiny_adapted(seed=2)
    assert not branch_equal(fresh, trained)
    with caplog.at_level(logging.INFO):
        assert EL.load_adapters(fresh, str(tmp_path), logging.getLogger("t")) is False
    assert branch_equal(fresh, trained), "the newest checkpoint's iqm_branch entry, bit for bit"
    assert "iqm_branch" in caplog.text and "image_adapter_3.pth" in caplog.text
    # a separate iqm_branch.pth (flat keys) keeps precedence
    _, other = tiny_adapted(seed=3)
    prefixes = tuple(m + "." for m in train.IQM_BRANCH_MODULES)
    torch.save({k: v for k, v in other.state_dict().items() if k.startswith(prefixes)}, tmp_path / "iqm_branch.pth")
    _, fresh = tiny_adapted(seed=2)
    caplog.clear()
    with caplog.at_level(logging.INFO):
        EL.load_adapters(fresh, str(tmp_path), logging.getLogger("t"))
    assert branch_equal(fresh, other) and not branch_equal(fresh, trained)
    assert "iqm_branch.pth" in caplog.text


def test_eval_last_parser_is_test_lasts_plus_one_flag():
    """eval_last.py takes test_last.py's arguments with its defaults; the only addition is --device_metrics"""
    import inspect
    import re
    import eval_last as EL
    import test_last as TL
    pattern = re.compile(r'add_argument\("--(\w+)"(?:, type=(\w+))?(?:, default=([^,)]+))?(?:, action="(\w+)")?')
    mine = {m[0]: m[1:] for m in pattern.findall(inspect.getsource(EL.build_parser))}
    theirs = {m[0]: m[1:] for m in pattern.findall(inspect.getsource(TL.main))}
    assert len(theirs) == 20 and mine.pop("device_metrics") == ("", "", "store_true")
    assert mine == theirs
    args = EL.build_parser().parse_args(["--device_metrics", "--iqm", "off"])
    assert args.device_metrics and args.iqm == "off" and not EL.build_parser().parse_args([]).device_metrics
    for name in ("get_predictions", "evaluate", "load_adapters"):      # the same leading arguments, one more at the end
        a, b = list(inspect.signature(getattr(EL, name)).parameters), list(inspect.signature(getattr(TL, name)).parameters)
        assert a[:len(b)] == b and a[len(b):] == {"get_predictions": ["on_device"], "evaluate": ["device_metrics"],
                                                 "load_adapters": []}[name]
