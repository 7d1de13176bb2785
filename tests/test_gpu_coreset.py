"""The coreset of the support bank on the device (csrc/coreset.hip) against the numpy definition (tests/coreset_cases.py):
the raw entries on guarded buffers and a workspace full of garbage, the quantiser byte for byte, the selection EQUAL to the
definition over the whole grid and every kind, bit-identical repeats, refusals that leave the outputs alone, the bank
of kept rows under support_nearest, the projected selection, and the evaluation harness on both metrics paths.

The selection has no tolerance: integers.  The value bars of the searches over a coreset bank are support_cases.BAR
(derived from the number formats) plus a covering term derived below.  The worst values seen go to the parity record that
conftest.PARITY_ERRORS writes at the end of the session (committed as profiles/coreset_parity_errors.json)."""
import functools

import numpy as np
import pytest
import torch

import coreset_cases as CC
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


def guarded(n, dev):
    return torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)


def unguard(b):
    h = b.cpu().numpy()
    assert np.all(h[:GUARD] == SENTINEL) and np.all(h[-GUARD:] == SENTINEL), "guard words were written"
    return h[GUARD:-GUARD]


def rows_raw(dev, rows):
    """aaclip_coreset_rows on guarded outputs -> (rc, q int16 [N, E], norm2 int32 [N])"""
    lib = _lib.load()
    N, E = rows.shape
    r = T(np.array(rows, np.float32)).to(dev)
    q = guarded(N * E // 2, dev)
    norm2 = guarded(N, dev)
    rc = lib.aaclip_coreset_rows(r.data_ptr(), N, E, q[GUARD:].data_ptr(), norm2[GUARD:].data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, unguard(q).view(np.int16).reshape(N, E), unguard(norm2)


def select_raw(dev, q, norm2, n, start, ws_short=0, N=None, E=None, q_offset=0):
    """aaclip_coreset_select on outputs with guard words round them and a workspace full of garbage ->
    (rc, picks int32 [n], radius2 uint32 [n + 1], min_d2 uint32 [N]); the outputs start as SENTINEL words"""
    lib = _lib.load()
    rows, width = q.shape
    N = rows if N is None else N
    E = width if E is None else E
    qd = torch.zeros(rows * width + 8, dtype=torch.int16, device=dev)
    qd[q_offset:q_offset + rows * width] = T(np.array(q)).to(dev).reshape(-1)
    nd = T(np.array(norm2)).to(dev)
    size = max(n, 1)
    picks, radius2, min_d2 = guarded(size, dev), guarded(size + 1, dev), guarded(rows, dev)
    ws_n = size if size <= rows else 1              # a refused n: any workspace will do
    need = lib.aaclip_coreset_select_workspace_bytes(rows, width, ws_n)
    assert need >= (ws_n + 1) * 8
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev)
    rc = lib.aaclip_coreset_select(qd[q_offset:].data_ptr(), nd.data_ptr(), N, E, n, start, picks[GUARD:].data_ptr(),
                                   radius2[GUARD:].data_ptr(), min_d2[GUARD:].data_ptr(), ws.data_ptr(), need - ws_short,
                                   torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.all(ws[need:].cpu().numpy() == 0xA5), "the workspace was written behind its size"
    return rc, unguard(picks), unguard(radius2).view(np.uint32), unguard(min_d2).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- the quantiser
def test_the_quantiser_is_numpy_byte_for_byte(dev):
    E = 64
    k = np.arange(-32, 32, dtype=np.float32)
    special = np.zeros((6, E), np.float32)
    special[0] = (k + 0.5) / 16384.0                           # half-way values, both parities, both signs
    special[1] = (k * 517 + 0.5) / 16384.0
    special[2, :12] = [1.0, -1.0, 2.0, -2.0, -0.0, 0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.99993896484375, 1.999969482421875]
    special[3] = np.float32(32766.5 / 16384.0) + k * np.float32(2.0 ** -14)     # across the clamp
    special[4] = -special[3]
    special[5, :4] = [3.4e38, -3.4e38, np.inf, -np.inf]
    rc, q, norm2 = rows_raw(dev, special)
    want_q, want_n = CC.quantise(special)
    assert rc == 0 and np.array_equal(q, want_q) and np.array_equal(norm2, want_n)
    assert q[2, :6].tolist() == [16384, -16384, 32767, -32767, 0, 0] and not q[2, 6:10].any()
    assert q[0, 32:36].tolist() == [0, 2, 2, 4] and q[0, 28:32].tolist() == [-4, -2, -2, 0]
    assert norm2[3] == want_n[3] and norm2.max() <= 0x7FFFFFFF
    big = np.full((3, 1024), 2.0, np.float32)                   # 1024 * 32767^2 > 2^31: saturated, not wrapped
    rc, q, norm2 = rows_raw(dev, big)
    assert rc == 0 and np.all(q == 32767) and np.all(norm2 == 0x7FFFFFFF)
    for kind in ("random", "ties", "antipodal"):
        for E in CC.ES:
            for N in CC.sizes(kind, E):
                rows = CC.case(kind, N, E)
                rc, q, norm2 = rows_raw(dev, rows)
                want_q, want_n = CC.quantised(kind, N, E)
                assert rc == 0 and np.array_equal(q, want_q) and np.array_equal(norm2, want_n), (kind, N, E)
    for E in (96, 480, 992, 1024):                              # widths whose second chunk covers a part of the lanes
        rows = np.random.default_rng(E).standard_normal((67, E)).astype(np.float32) * 0.05
        rc, q, norm2 = rows_raw(dev, rows)
        want_q, want_n = CC.quantise(rows)
        assert rc == 0 and np.array_equal(q, want_q) and np.array_equal(norm2, want_n), E
    # the engine's call gives the same bytes
    eq, en = engine.coreset_rows(T(np.array(CC.case("random", 257, 128))).to(dev))
    want_q, want_n = CC.quantised("random", 257, 128)
    assert eq.dtype == torch.int16 and en.dtype == torch.int32
    assert np.array_equal(eq.cpu().numpy(), want_q) and np.array_equal(en.cpu().numpy(), want_n)


# ---------------------------------------------------------------------------------------------------- the selection
@pytest.mark.parametrize("E", CC.ES)
@pytest.mark.parametrize("kind", CC.KINDS)
def test_the_selection_equals_the_definition(dev, kind, E):
    cases = 0
    for N in CC.sizes(kind, E):
        q, norm2 = CC.quantised(kind, N, E)
        for start in CC.starts(N):
            picks, radius2, kept = CC.reference(kind, N, E, start)
            for n in CC.counts(N):
                rc, got_p, got_r, got_m = select_raw(dev, q, norm2, n, start)
                assert rc == 0, _lib.load().aaclip_last_error()
                where = (kind, N, E, n, start)
                assert np.array_equal(got_p, picks[:n]), (where, np.flatnonzero(got_p != picks[:n])[:8])
                assert np.array_equal(got_r, radius2[:n + 1]), (where, np.flatnonzero(got_r != radius2[:n + 1])[:8])
                assert np.array_equal(got_m, kept[n]), (where, np.flatnonzero(got_m != kept[n])[:8])
                cases += 1
    print(f"coreset {kind} E={E}: {cases} selections equal to the definition")
    record(f"coreset_select.{kind}.E{E}", cases=cases, mismatches=0)


def test_other_widths_equal_the_definition(dev):
    """E = 96 (12 chunks on 8 lanes), 480 (60 on 32), 992 (124 on 64), 1024 (128 on 64), 64 and 512 (no second chunk)"""
    for E in (64, 96, 480, 512, 992, 1024):
        rows = SC.unit(np.random.default_rng([7, E]).standard_normal((131, E))).astype(np.float32)
        q, norm2 = CC.quantise(rows)
        for n, start in ((131, 0), (14, 87)):
            want = CC.definition(q, n, start)
            rc, got_p, got_r, got_m = select_raw(dev, q, norm2, n, start)
            assert rc == 0 and np.array_equal(got_p, want[0]) and np.array_equal(got_r, want[1]) and np.array_equal(got_m, want[2]), (E, n)


def test_a_second_call_returns_the_same_bytes(dev):
    q, norm2 = CC.quantised("random", 2738, 128)
    first = select_raw(dev, q, norm2, 274, 5)
    second = select_raw(dev, q, norm2, 274, 5)
    assert first[0] == 0 and all(np.array_equal(a, b) for a, b in zip(first, second))
    # the engine's call gives the same bytes
    p, r, m = engine.coreset_select(T(np.array(q)).to(dev), T(np.array(norm2)).to(dev), 274, start=5)
    assert (p.dtype, r.dtype, m.dtype) == (torch.int32,) * 3 and p.shape == (274,) and r.shape == (275,) and m.shape == (2738,)
    assert np.array_equal(p.cpu().numpy(), first[1]) and np.array_equal(r.cpu().numpy().view(np.uint32), first[2])
    assert np.array_equal(m.cpu().numpy().view(np.uint32), first[3])


def test_refusals_leave_the_outputs_untouched(dev):
    lib = _lib.load()
    q, norm2 = CC.quantised("random", 65, 128)

    def refused(msg, **kw):
        rc, p, r, m = select_raw(dev, q, norm2, **{"n": 7, "start": 0, **kw})
        text = lib.aaclip_last_error().decode()
        assert rc != 0 and text.startswith("coreset_select:") and msg in text, (kw, rc, text)
        assert np.all(p == SENTINEL) and np.all(r.view(np.int32) == SENTINEL) and np.all(m.view(np.int32) == SENTINEL), kw

    refused("n must be", n=66)                      # n > N
    refused("n must be", n=0)
    refused("N must be", N=0)
    refused("E must be", E=48)                      # not a multiple of 32
    refused("E must be", E=2048)
    refused("E must be", E=16)
    refused("start must be", start=65)
    refused("start must be", start=-1)
    refused("workspace too small", ws_short=1)
    refused("aligned", q_offset=4)                  # q 8 bytes off a 16-byte boundary
    big = T(np.array(norm2)).to(dev).clone()
    big[3] = 1 << 29
    with pytest.raises(ValueError, match="2\\^29"):
        engine.coreset_select(T(np.array(q)).to(dev), big, 7)
    with pytest.raises(ValueError):
        engine.coreset_select(T(np.array(q)).to(dev).float(), big, 7)
    with pytest.raises(RuntimeError, match="n must be"):
        engine.coreset_select(T(np.array(q)).to(dev), T(np.array(norm2)).to(dev), 66)


# ---------------------------------------------------------------------------------------------------- the bank
@functools.lru_cache(maxsize=None)
def planted_selection(N, E):
    """the definition on support_cases' planted bank, all N picks from row 0"""
    return CC.definition_gram(CC.quantise(SC.case("planted", 1, N, E)[1])[0], N, 0)


def tokens_of(rows, P, dev):
    """rows [N, E] as one level of seg tokens [N / P, P, E]"""
    return [T(np.array(rows)).to(dev).reshape(-1, P, rows.shape[1])]


@pytest.mark.parametrize("form", list(FORMS))
def test_the_whole_bank_as_a_coreset(dev, form):
    """ratio = 1, dim = 0 on distinct rows: every row is kept, in pick order"""
    N, E, P = 2738, 768, 1369
    qs, bank_rows = SC.case("planted", 257, N, E)
    full = engine.support_bank([tokens_of(bank_rows, P, dev)], form)
    core = engine.support_bank_coreset([tokens_of(bank_rows, P, dev)], form, 1.0, dim=0)
    assert isinstance(core, engine.CoresetBank) and (core.form, core.patches, core.shots, core.dim) == (FORMS[form], P, 2, 0)
    index = core.index[0].cpu().numpy()
    assert core.index[0].dtype == torch.int32 and np.array_equal(np.sort(index), np.arange(N))        # a permutation
    assert core.rows[0].shape == (N, E) and core.rows[0].dtype == full.rows[0].dtype
    assert torch.equal(core.rows[0], full.rows[0][core.index[0].long()])                               # the original rows
    r2 = core.radius2[0]
    assert r2.dtype == np.uint32 and r2.shape == (N + 1,) and r2[0] == CC.D2_INIT and np.all(np.diff(r2.astype(np.int64)) <= 0)
    want = planted_selection(N, E)
    assert np.array_equal(index, want[0]) and np.array_equal(r2[:N], want[1][:N])
    qd = T(np.array(qs)).to(dev)
    cos_f, idx_f = engine.support_nearest(qd, full.rows[0])
    cos_c, idx_c = engine.support_nearest(qd, core.rows[0])
    err = float((cos_c - cos_f).abs().max())
    print(f"coreset bank {form}, ratio 1: max |cos over the coreset - cos over the full bank| {err:.3e}")
    assert err <= SC.BAR[form]
    assert SC.index_is_checked("planted", N) and SC.top2_gap(qs, bank_rows).min() >= SC.PLANTED_GAP
    assert np.array_equal(index[idx_c.cpu().numpy()], idx_f.cpu().numpy())                             # the same bank rows
    assert np.array_equal(idx_f.cpu().numpy(), SC.reference("planted", 257, N, E)[1])
    record(f"coreset_bank.ratio1.{form}", max_abs_err=err, bar=SC.BAR[form])


@pytest.mark.parametrize("form", list(FORMS))
def test_a_tenth_of_the_bank_covers_it(dev, form):
    """ratio = 0.1, dim = 0, the bank's own rows as queries.  With c the nearest pick of row x among the QUANTISED rows,
    |q_x - q_c| = sqrt(min_d2); each quantised row is off its fp32 row by at most sqrt(E) * 2^-15 in norm after the
    division by 2^14, so |x - c| <= sqrt(min_d2) / 2^14 + sqrt(E) * 2^-14, and on unit rows 1 - cos = |x - c|^2 / 2."""
    N, E, P = 2738, 128, 1369
    bank_rows = CC.case("clusters", N, E)
    full = engine.support_bank([tokens_of(bank_rows, P, dev)], form)
    core = engine.support_bank_coreset([tokens_of(bank_rows, P, dev)], form, 0.1, dim=0)
    n = 274
    assert core.rows[0].shape == (n, E) and core.index[0].shape == (n,) and core.radius2[0].shape == (n + 1,)
    q, norm2 = CC.quantised("clusters", N, E)
    picks, radius2, kept = CC.reference("clusters", N, E, 0)
    assert np.array_equal(core.index[0].cpu().numpy(), picks[:n]) and np.array_equal(core.radius2[0], radius2[:n + 1])
    qd = T(np.array(bank_rows)).to(dev)
    cos_f = engine.support_nearest(qd, full.rows[0])[0].cpu().numpy().astype(np.float64)
    cos_c, idx_c = engine.support_nearest(qd, core.rows[0])
    cos_c = cos_c.cpu().numpy().astype(np.float64)
    bar = SC.BAR[form]
    over = float((cos_c - cos_f).max())
    assert over <= bar                                                          # a part of the bank cannot be nearer
    bound = (np.sqrt(kept[n].astype(np.float64)) / 2 ** 14 + np.sqrt(E) * 2.0 ** -14) ** 2 / 2
    slack = float(((1 - cos_c) - bound).max())
    print(f"coreset bank {form}, ratio 0.1: max (cos_coreset - cos_full) {over:.3e}, max (1 - cos_coreset - bound) {slack:.3e}, "
          f"largest bound {bound.max():.3e}")
    assert slack <= bar
    assert int(idx_c.min()) >= 0 and int(idx_c.max()) < n
    record(f"coreset_bank.ratio0.1.{form}", max_over_full=over, max_over_bound=slack, bar=bar)


def test_the_projected_selection(dev):
    """dim = 128: the projected rows are unit within 1e-5, and the selection on them is the definition applied to their
    quantised bytes read back"""
    N, E, P, dim = 2738, 768, 1369, 128
    bank_rows = SC.case("planted", 1, N, E)[1]
    d = T(np.array(bank_rows)).to(dev)
    proj = engine.coreset_projected_rows(d, dim, seed=0)
    assert proj.shape == (N, dim) and proj.dtype == torch.float32
    host = proj.cpu().numpy().astype(np.float64)
    off = float(np.abs(np.linalg.norm(host, axis=1) - 1).max())
    w = engine.coreset_projection(E, dim, 0).numpy().astype(np.float64)
    want = SC.unit(bank_rows.astype(np.float64) @ w.T)
    perr = float(np.abs(host - want).max())
    print(f"projected rows: max | |row| - 1 | {off:.3e}, max |row - fp64| {perr:.3e}")
    assert off <= 1e-5 and perr <= 1e-4                       # the fp32 GEMM's standing bar on values of magnitude <= 1
    q, norm2 = engine.coreset_rows(proj)
    hq = q.cpu().numpy()
    assert np.array_equal(hq, CC.quantise(proj.cpu().numpy())[0])
    core = engine.support_bank_coreset([tokens_of(bank_rows, P, dev)], "fp32", 0.1, dim=dim)
    n = 274
    want_p, want_r, _, _ = CC.definition_gram(hq, n, 0)
    assert core.dim == dim and np.array_equal(core.index[0].cpu().numpy(), want_p) and np.array_equal(core.radius2[0], want_r)
    assert torch.equal(core.rows[0], d[core.index[0].long()])                     # the ORIGINAL rows of the picks
    again = engine.support_bank_coreset([tokens_of(bank_rows, P, dev)], "fp32", 0.1, dim=dim)
    assert torch.equal(again.index[0], core.index[0])
    # dim >= E selects on the rows themselves
    same = engine.support_bank_coreset([tokens_of(bank_rows, P, dev)], "fp32", 0.01, dim=768)
    assert same.dim == 0 and np.array_equal(same.index[0].cpu().numpy(), planted_selection(N, E)[0][:28])
    with pytest.raises(ValueError, match="dim"):
        engine.support_bank_coreset([tokens_of(bank_rows, P, dev)], "fp32", 0.1, dim=100)
    record("coreset_projection.dim128", max_norm_off=off, max_abs_err=perr, bars=dict(norm=1e-5, value=1e-4))


def test_duplicate_rows_truncate_the_bank(dev):
    rows = CC.case("duplicates", 20, 128)
    core = engine.support_bank_coreset([tokens_of(rows, 4, dev)], "fp32", 1.0, dim=0)
    assert core.rows[0].shape == (5, 128) and sorted(int(i) % 5 for i in core.index[0].cpu()) == [0, 1, 2, 3, 4]
    assert core.radius2[0].shape == (6,) and core.radius2[0][5] == 0 and core.radius2[0][4] > 0 and core.shots == 5
    cos, _ = engine.support_nearest(T(np.array(rows)).to(dev), core.rows[0])
    assert float((1 - cos).abs().max()) <= SC.BAR["fp32"]                      # every row has its duplicate in the bank


# ---------------------------------------------------------------------------------------------------- end to end
def test_harness_with_a_coreset_bank(dev, tmp_path):
    """The synthetic tree and reduced model of test_gpu_support.test_harness_with_a_support_bank, two shots per class"""
    import dataset as D
    import eval_coreset as EC
    import eval_last as EL
    import eval_support as ES
    import forward_utils as FU
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
    plain = (model, sets, anchors, dev, S, "MVTec")
    P = (S // cfg.patch_size) ** 2
    for device_metrics in (False, True):
        how = dict(batch_size=4, use_iqm=False, device_metrics=device_metrics)
        # without a coreset: eval_support's rows exactly
        assert EC.evaluate(*plain, **how, f1_max=True, support=2) == ES.evaluate(*plain, **how, f1_max=True, support=2)
        assert EC.evaluate(*plain, **how) == ES.evaluate(*plain, **how)
        rows, details = EC.evaluate(*plain, **how, f1_max=True, return_masks=True, support=2, coreset=0.25, coreset_dim=0)
        assert len(rows) == 3 and rows[-1]["class name"] == "Average"
        banks, evaluated = EL.support_banks(model, sets, 2, dev, S, coreset=0.25, coreset_dim=0)
        for c in classes:
            bank = banks[c]
            assert isinstance(bank, engine.CoresetBank) and bank.shots == 2 and bank.patches == P and len(bank.rows) == 2
            near = details[c]["support nearest"]
            assert len(near) == 2 and all(n.shape == (len(evaluated[c]), P, 2) and n.dtype == np.int32 for n in near)
            for l, n in enumerate(near):
                index = bank.index[l].cpu().numpy()
                assert 1 <= len(index) <= -(-2 * P // 4) and bank.rows[l].shape[0] == len(index)
                assert n[..., 0].min() >= 0 and n[..., 0].max() < 2 and n[..., 1].min() >= 0 and n[..., 1].max() < P
                assert np.isin(n[..., 0] * P + n[..., 1], index).all()            # every pair names a kept row
    with pytest.raises(ValueError, match="support"):
        EC.evaluate(*plain, batch_size=4, use_iqm=False, coreset=0.25)
