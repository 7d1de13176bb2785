"""The few-shot support bank on the device (csrc/support.hip) against the fp64 brute-force definition
(tests/support_cases.py) and the host map (forward_utils.support_anomaly_map_host): the raw entry on guarded buffers and a
workspace full of garbage, both forms over every (M, N, E) of the grid and the four kinds of case; bit-identical repeats; the
workspace size; the map stage; the evaluation harness with a bank on both metrics paths.

The value bars are support_cases.BAR, derived from the number formats, not measured.  The worst values seen go to
the parity record that conftest.PARITY_ERRORS writes at the end of the session (committed as
profiles/support_parity_errors.json)."""
import itertools

import numpy as np
import pytest
import torch

import support_cases as SC
from aaclip_hip import _lib, engine

pytestmark = pytest.mark.gpu

T = torch.from_numpy
GUARD = 64
SENTINEL = 0x5A5A5A5A
FORMS = {"fp16": engine.SUPPORT_FP16, "fp32": engine.SUPPORT_FP32}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def record(name, **values):
    from conftest import PARITY_ERRORS
    PARITY_ERRORS[name] = values


def nearest_raw(dev, q, bank_rows, form, want_idx=True, ws_short=0):
    """aaclip_support_nearest on outputs with guard words round them and a workspace full of garbage ->
    (rc, cos fp32 [M], idx int32 [M] or None)"""
    lib = _lib.load()
    M, E = q.shape
    N = bank_rows.shape[0]
    qd = T(np.array(q)).to(dev)
    bank = engine.support_bank_rows(T(np.array(bank_rows)).to(dev), form)
    cos = torch.full((M + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    idx = torch.full((M + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    need = lib.aaclip_support_nearest_workspace_bytes(M, N, E, form)
    assert need >= M * 8
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev)
    rc = lib.aaclip_support_nearest(qd.data_ptr(), M, bank.data_ptr(), N, E, form, cos[GUARD:].data_ptr(),
                                    idx[GUARD:].data_ptr() if want_idx else None, ws.data_ptr(), need - ws_short,
                                    torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    outs = []
    for b in (cos, idx):
        h = b.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[-GUARD:] == SENTINEL), "guard words were written"
        outs.append(h[GUARD:-GUARD])
    assert np.all(ws[need:].cpu().numpy() == 0xA5), "the workspace was written behind its size"
    if not want_idx:
        assert np.all(outs[1] == SENTINEL)
    return rc, outs[0].view(np.float32), outs[1] if want_idx else None


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("E", SC.ES)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_nearest_is_the_brute_force(dev, kind, E, form):
    worst, rows_checked = 0.0, 0
    for M, N in itertools.product(SC.MS, SC.NS):
        q, bank = SC.case(kind, M, N, E)
        want, want_idx = SC.reference(kind, M, N, E)
        rc, cos, idx = nearest_raw(dev, q, bank, FORMS[form])
        assert rc == 0, _lib.load().aaclip_last_error()
        err = float(np.abs(cos.astype(np.float64) - want).max())
        print(f"support {form} {kind} M={M} N={N} E={E}: max |cos - fp64| {err:.3e}")
        worst = max(worst, err)
        assert err <= SC.BAR[form], (kind, M, N, E, err)
        assert idx.min() >= 0 and idx.max() < N, "an index outside the bank (a padding row won)"
        # whatever index came back, its own fp64 cosine must be the maximum up to the bar (never a padding column)
        own = np.einsum("me,me->m", q.astype(np.float64), bank[idx].astype(np.float64))
        assert np.abs(own - want).max() <= 2 * SC.BAR[form], (kind, M, N, E)
        if SC.index_is_checked(kind, N):
            assert np.array_equal(idx, want_idx), (kind, M, N, E, np.flatnonzero(idx != want_idx)[:8])
            rows_checked += M
    assert kind in ("random", "antipodal") or rows_checked >= sum(SC.MS) * 3
    record(f"support_nearest.{form}.{kind}.E{E}", max_abs_err=worst, bar=SC.BAR[form])


@pytest.mark.parametrize("form", list(FORMS))
def test_no_index_output_and_repeats_are_bit_identical(dev, form):
    M, N, E = 1369, 2738, 768
    q, bank = SC.case("duplicates", M, N, E)
    rc, cos, idx = nearest_raw(dev, q, bank, FORMS[form])
    assert rc == 0
    rc2, cos2, idx2 = nearest_raw(dev, q, bank, FORMS[form])
    assert rc2 == 0 and np.array_equal(cos.view(np.uint32), cos2.view(np.uint32)) and np.array_equal(idx, idx2)
    rc3, cos3, none = nearest_raw(dev, q, bank, FORMS[form], want_idx=False)
    assert rc3 == 0 and none is None and np.array_equal(cos.view(np.uint32), cos3.view(np.uint32))
    # the engine's call gives the same bytes
    b = engine.support_bank_rows(T(np.array(bank)).to(dev), form)
    c, i = engine.support_nearest(T(np.array(q)).to(dev), b)
    assert np.array_equal(c.cpu().numpy().view(np.uint32), cos.view(np.uint32)) and np.array_equal(i.cpu().numpy(), idx)


def test_signed_zeros_tie_and_the_lower_index_wins(dev):
    """a query orthogonal to the whole bank: every cosine is a zero, and row 0 must come back with +0.0"""
    E, N = 64, 130
    bank = np.zeros((N, E), np.float32)
    bank[:, 1] = np.where(np.arange(N) % 2 == 0, -1.0, 1.0)
    q = np.zeros((5, E), np.float32)
    q[:, 0] = 1.0
    q[:, 1] = [0.0, -0.0, 0.0, -0.0, 0.0]
    for form in FORMS.values():
        rc, cos, idx = nearest_raw(dev, q, bank, form)
        assert rc == 0 and np.all(idx == 0) and np.all(cos.view(np.uint32) == 0)


@pytest.mark.parametrize("form", list(FORMS))
def test_bad_arguments_are_refused_before_any_launch(dev, form):
    lib = _lib.load()
    q, bank = SC.case("random", 17, 127, 64)
    rc, cos, idx = nearest_raw(dev, q, bank, FORMS[form], ws_short=1)
    assert rc != 0 and b"workspace" in lib.aaclip_last_error()
    assert np.all(cos.view(np.int32) == SENTINEL) and np.all(idx == SENTINEL), "a refused call wrote its outputs"
    f = FORMS[form]
    assert lib.aaclip_support_nearest_workspace_bytes(17, 127, 48, f) == 0      # E < 64
    assert lib.aaclip_support_nearest_workspace_bytes(17, 127, 80, f) == 0      # not a multiple of 32
    assert lib.aaclip_support_nearest_workspace_bytes(17, 127, 1056, f) == 0    # E > 1024
    assert lib.aaclip_support_nearest_workspace_bytes(0, 127, 64, f) == 0
    assert lib.aaclip_support_nearest_workspace_bytes(17, 0, 64, f) == 0
    assert lib.aaclip_support_nearest_workspace_bytes(17, 127, 64, 7) == 0      # no such form
    assert lib.aaclip_support_nearest_workspace_bytes(17, 127, 96, f) >= 17 * 8
    qd = T(np.array(q)).to(dev)
    with pytest.raises(ValueError):
        engine.support_nearest(qd, torch.zeros(4, 32, dtype=torch.float32, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.support_nearest(T(np.array(q)), torch.zeros(4, 64))
    with pytest.raises(RuntimeError, match="E must be"):
        engine.support_bank_rows(torch.zeros(4, 48, device=dev), form)


def test_a_width_with_a_half_k_step(dev):
    """E = 96: the fp16 form's last K step of 64 is half padding"""
    rng = np.random.default_rng(3)
    bank = SC.unit(rng.standard_normal((130, 96))).astype(np.float32)
    q = SC.unit(bank[(np.arange(40) * 13) % 130] + 0.5 * SC.unit(rng.standard_normal((40, 96)))).astype(np.float32)
    want, want_idx = SC.brute_force(q, bank)
    for form, code in FORMS.items():
        rc, cos, idx = nearest_raw(dev, q, bank, code)
        assert rc == 0 and np.abs(cos - want).max() <= SC.BAR[form] and np.array_equal(idx, want_idx)


# ---------------------------------------------------------------------------------------------------- the map stage
MAP_BAR = 1e-4        # the map stage alone: fp32 on O(30) operations of magnitude <= 8 (weight 1, |base| of a few units)


@pytest.mark.parametrize("S", [70, 518])
@pytest.mark.parametrize("levels", [1, 4])
@pytest.mark.parametrize("g", [5, 37])
def test_support_map_is_the_host_map(dev, g, levels, S):
    import forward_utils as FU
    B = 2
    segs, banks = SC.map_case(B, g, levels)
    dsegs = [T(s).to(dev) for s in segs]
    base = np.random.default_rng(2).standard_normal((B, S, S)).astype(np.float32)
    dbase = T(base).to(dev)
    worst = {}
    for form in FORMS:
        bank = engine.support_bank([[T(b).to(dev) for b in banks]], form)
        assert bank.form == FORMS[form] and bank.patches == g * g and bank.shots == banks[0].shape[0] and len(bank.rows) == levels
        assert all(r.shape == (bank.shots * g * g, 64) for r in bank.rows)
        cos = [engine.support_nearest(s, r)[0] for s, r in zip(dsegs, bank.rows)]
        host_cos = [c.cpu().numpy() for c in cos]
        for bs, dbs in ((None, None), (base, dbase)):
            # (1) the map stage alone, on the device's own cosines, at weight 1: magnitude <= 2 per level, <= 8 in all
            got = engine.support_map_from_cos(cos, B, S, 7, 1.0, base=dbs, weight=1.0).cpu().numpy()
            want = FU.support_anomaly_map_host(segs, None, S, "Industrial", base=bs, weight=1.0, best_cos=host_cos)
            e1 = float(np.abs(got - want).max())
            assert got.shape == (B, S, S) and e1 <= MAP_BAR, (form, e1)
            # (2) end to end against the brute force: the form's bar per level
            nearest = []
            got = engine.support_map(dsegs, bank, S, 7, 1.0, base=dbs, weight=1.0, nearest=nearest).cpu().numpy()
            want = FU.support_anomaly_map_host(segs, banks, S, "Industrial", base=bs, weight=1.0)
            e2 = float(np.abs(got - want).max())
            assert e2 <= SC.BAR[form] * levels, (form, e2)
            assert len(nearest) == levels and all(n.shape == (B, g * g) and n.dtype == torch.int32 for n in nearest)
            # (3) the default weight through forward_utils: the weight scales the sum and its error alike
            got = FU.support_anomaly_map(dsegs, bank, S, "Industrial", base=dbs).cpu().numpy()
            want = FU.support_anomaly_map_host(segs, banks, S, "Industrial", base=bs)
            e3 = float(np.abs(got - want).max())
            assert e3 <= 50.0 * SC.BAR[form] * levels, (form, e3)
            worst[form] = [max(a, b) for a, b in zip(worst.get(form, [0, 0, 0]), [e1, e2, e3])]
        print(f"support map {form} g={g} levels={levels} S={S}: stage {worst[form][0]:.3e}, end to end {worst[form][1]:.3e}, "
              f"at weight 50 {worst[form][2]:.3e}")
    record(f"support_map.g{g}.levels{levels}.S{S}", **{f: dict(stage=v[0], end_to_end=v[1], weight50=v[2]) for f, v in worst.items()},
           bars=dict(stage=MAP_BAR, fp16=SC.BAR["fp16"] * levels, fp32=SC.BAR["fp32"] * levels))
    with pytest.raises(ValueError, match="levels"):
        engine.support_map(dsegs + dsegs, bank, S, 7, 1.0)
    with pytest.raises(ValueError, match="base map"):
        engine.support_map(dsegs, bank, S, 7, 1.0, base=dbase[:, :-1])


# ---------------------------------------------------------------------------------------------------- end to end
def test_harness_with_a_support_bank(dev, tmp_path):
    """The synthetic tree and reduced model of test_gpu_metrics_device.test_harness_with_device_metrics_returns_the_same_rows,
    two shots per class"""
    import dataset as D
    import eval_last as EL
    import eval_support as ES
    import forward_utils as FU
    import test_last as TL
    from synth_dataset import write_tree
    from test_gpu_metrics_device import build_tiny
    root = write_tree(str(tmp_path / "MVTec"))
    meta = str(tmp_path / "meta" / "MVTec" / "full-shot.jsonl")
    D.build_metadata(root, meta)
    cfg, clip, model = build_tiny(dev, "fp32")
    S = cfg.image_size
    classes = ["bottle", "grid"]
    with torch.no_grad():
        anchors = {c: FU.get_adapted_single_class_text_embedding(model, "MVTec", c, dev) for c in classes}
    sets = {c: D.BaseSingleClassDataset(root, meta, S, c) for c in classes}
    how = dict(batch_size=4, use_iqm=False)
    # support=None: today's rows, on either metrics path
    plain = (model, sets, anchors, dev, S, "MVTec")
    assert EL.evaluate_rows(*plain, **how, support=None) == TL.evaluate(*plain, **how)
    assert EL.evaluate_rows(*plain, **how, device_metrics=True, support=None) == EL.evaluate(*plain, **how, device_metrics=True)
    banks, evaluated = EL.support_banks(model, sets, 2, dev, S)
    P = (S // cfg.patch_size) ** 2
    for c in classes:
        assert banks[c].form == engine.SUPPORT_FP32 and banks[c].shots == 2 and banks[c].patches == P and len(banks[c].rows) == 2
        assert len(evaluated[c]) == len(sets[c]) - 2
        assert [m["image_path"] for m in evaluated[c].meta] == [m["image_path"] for m in sets[c].meta if m not in sets[c].normal_meta[:2]]
    where = (model, evaluated, anchors, dev, S, "MVTec")
    out, details = {}, {}
    for path in ("host", "device"):
        details[path] = {}
        out[path] = EL.evaluate_rows(*where, **how, device_metrics=path == "device", f1_max=True, details=details[path],
                                     return_masks=True, support=banks)
    assert out["device"] == out["host"] and len(out["host"]) == 3                      # row for row
    for c in classes:
        near = details["device"][c]["support nearest"]
        assert len(near) == 2 and all(n.shape == (len(evaluated[c]), P, 2) and n.dtype == np.int32 for n in near)
        assert all(n[..., 0].min() >= 0 and n[..., 0].max() < 2 and n[..., 1].min() >= 0 and n[..., 1].max() < P for n in near)
        assert all(np.array_equal(a, b) for a, b in zip(near, details["host"][c]["support nearest"]))
    # the function form of the script builds the same banks and returns the same rows
    assert ES.evaluate(*plain, **how, device_metrics=True, f1_max=True, support=2) == out["device"]
    assert ES.evaluate(*plain, **how, device_metrics=True) == EL.evaluate(*plain, **how, device_metrics=True)
    # the maps: with the bank = without it + 50 * the host support map of the same tokens (fp32 form: 1e-4 per level)
    c = "bottle"
    loader = torch.utils.data.DataLoader(evaluated[c], batch_size=4)
    with torch.no_grad():
        _, _, without, _, _ = EL.get_predictions(model, anchors[c], loader, dev, S, "MVTec", use_iqm=False, on_device=True)
        nearest = []
        _, _, with_bank, _, _ = EL.get_predictions_support(model, anchors[c], loader, dev, S, "MVTec", use_iqm=False, on_device=True,
                                                   support=banks[c], nearest=nearest)
        images = torch.stack([evaluated[c][i]["image"] for i in range(len(evaluated[c]))]).to(dev)
        shots = torch.stack([sets[c].support_split(2)[0][i]["image"] for i in range(2)]).to(dev)
        tokens = [t.float().cpu().numpy() for t in model(images)[0]]
        bank_tokens = [t.float().cpu().numpy() for t in model(shots)[0]]
    host_nearest = []
    want = FU.support_anomaly_map_host(tokens, bank_tokens, S, "Industrial", nearest=host_nearest)
    err = float(np.abs((with_bank - without).cpu().numpy() - want).max())
    print(f"harness: |(map with bank - map without) - 50 * host support map| {err:.3e}")
    assert err <= 50.0 * SC.BAR["fp32"] * 2
    assert want.min() > 0 and float((with_bank - without).min()) > 0               # no test image is in its own bank
    record("support_harness.fp32", max_abs_err=err, bar=50.0 * SC.BAR["fp32"] * 2)
    # an image that IS in the bank has distance 0 to itself: the reason support_split removes the shots
    with torch.no_grad():
        self_map = FU.support_anomaly_map(model(shots)[0], banks[c], S, "Industrial", weight=1.0)
    assert float(self_map.abs().max()) <= 2 * SC.BAR["fp32"]                  # two levels, the fp32 form's bar each
