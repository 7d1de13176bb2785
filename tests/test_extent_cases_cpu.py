"""tests/extent_cases.py proven without a GPU: the period and crossing arithmetic of every case, the closed-form counts,
the weighted curve reference against metrics_device_cases.curve_metrics on the expanded arrays, the refusal table
against csrc/capi.hip (complete, and every call refused by the library's host-side checks with the limit's message),
and where a row offset truncated to 32 bits would land -- the evidence that tests/test_gpu_extent.py notices one."""
import numpy as np
import pytest
import torch

import extent_cases as EC
import metrics_device_cases as MD
from aaclip_hip import _lib

P = EC.P
G2, G4 = 1 << 31, 1 << 32


def all_cases():
    """(name, rows, operands) of every case of groups 1 and 2"""
    out = [(name, rows, ops) for name, (rows, ops, _) in EC.ROW_CASES.items()]
    out += [(f"gemm.{code}.{epi}", rows, ops) for (code, epi), (rows, ops) in EC.GEMM_CASES.items()]
    out += [(f"gemm_fused.{name}", rows, ops) for name, (rows, ops) in EC.FUSED_CASES.items()]
    out.append(("gemm_wgrad",) + EC.WGRAD_CASE)
    out.append(("drop_cls_rows.src",) + EC.DROP_CLS_CASE[:2])
    out.append(("drop_cls_rows.dst",) + EC.DROP_CLS_CASE[2:])
    return out


def test_period_is_odd_and_every_row_count_is_ragged():
    assert P % 2 == 1 and all(P % q for q in range(3, 32, 2)) and EC.MP % 2 == 1
    for name, rows, _ in all_cases():
        if name.endswith("_max"):                 # a row count set by the limit it sits on: 2^24 - 1 workgroups
            assert rows % P and rows in (EC.ROWS4_MAX, EC.GRID_MAX - 1, EC.HEAD_MAX_ROWS), (name, rows)
        else:
            assert EC.ragged(rows), (name, rows)
    assert EC.ROWS4_MAX == 2 ** 26 - 4 and (EC.ROWS4_MAX + 3) // 4 == EC.GRID_MAX - 1 == (EC.ROWS4_REFUSED + 3) // 4 - 1
    assert 3 * EC.HEAD_MAX_ROWS == EC.GRID_MAX - 1
    assert EC.ROWS * EC.WIDTH * 4 == G4 + (8 << 20) + 4096 * 3           # 4 GiB + 8 MiB (and three rows)


@pytest.mark.parametrize("name,rows,ops", all_cases(), ids=[c[0] for c in all_cases()])
def test_extents_and_crossings(name, rows, ops):
    """every operand that scales passes 2^31 bytes, every fp32 one 2^32 (`narrow` operands: a few bytes per row, or the
    unexpanded side of the head entries, which no shape of the case brings there); the row at each crossing is not the
    start of a period, so the row a wrapped offset lands on -- the crossing row minus 2^31 or 2^32 bytes -- has another
    phase, and so have the rows on either side of the crossing"""
    wide = [o for o in ops if not o.narrow]
    assert wide, name
    assert any(o.fp32 and rows * o.row_bytes > G4 for o in ops) or not any(o.fp32 for o in wide), name
    for o in wide:
        extent = rows * o.row_bytes
        assert extent > G2, (name, o.name, extent)
        assert not o.fp32 or extent > G4, (name, o.name, extent)
        cross = EC.crossings(rows, o.row_bytes)
        assert set(cross) == {lim for lim in EC.LIMITS if extent > lim} and cross
        for lim, c in cross.items():
            assert 0 < c < rows and c % P != 0 and (c - 1) % P != c % P, (name, o.name, lim, c)
            w = -(-lim // o.row_bytes)                    # the first row that STARTS at or behind the limit
            landed = EC.wrapped_offset(w * o.row_bytes, 32 if lim == G4 else 31) // o.row_bytes
            assert w < rows and landed < w and landed % P != w % P, (name, o.name, lim, w, landed)


def test_no_fp32_operand_of_groups_1_to_4_stays_below_4_gib():
    for name, rows, ops in all_cases():
        for o in ops:
            if o.fp32 and not o.narrow:
                assert rows * o.row_bytes > G4, (name, o.name)
    # the metrics chain: 4-byte scores and keys.  n = 2^31 - 1, the stated limit, is 8 GiB - 4 bytes; n = 2^29 + 3 is the
    # workload size the chain is used at (above one dataset's 4.6e8 pixels) and passes 2^31 bytes by 12
    big = max(EC.METRIC_SIZES)
    assert big == G2 - 1 and 4 * big > G4 and 4 * min(EC.METRIC_SIZES) > G2
    for (n, kind), (rows, ops) in EC.METRIC_CASES.items():
        assert rows == n and n % EC.MP and n % (3 * EC.MP) and n % 2048


def test_attention_cases_sit_at_the_limit_and_cross_on_another_phase():
    L, H, period = EC.ATTN_SHORT
    image = L * 3 * 64 * H * 4
    assert image == 2113896960 < G2 and (L + 1) * 3 * 64 * H * 4 >= G2 and H == 65535 and H % period
    assert 2 * image > G2 and 3 * image > G4 and 3 * image // 2 > G2          # fp32 / split: 2^32 at B = 3; 16-bit: 2^31
    for B, lim in ((2, G2), (3, G4)):
        assert EC.attention_phase_at(lim, B, L, H, period) != EC.attention_phase_at(0, B, L, H, period) == 0
        assert EC.attention_phase_at(lim, B, L, H, period, 128) != 0           # split16 rows: 128-byte planes per head
    Ll, Hl, pl = EC.ATTN_LONG
    assert Ll * 3 * 64 * Hl * 4 < G2 <= Ll * 3 * 64 * (Hl + 1) * 4 and Hl % pl and pl % 2 == 1
    for form, lim in (("split16", G4), ("qk8", G4), ("f16", G2)):             # at B = 3
        assert 3 * Ll * EC.attention_row_bytes(form, Hl)[0] > lim
    assert 2 * Ll * EC.attention_row_bytes("qk8", Hl)[0] > G2                  # B = 2: the 4- and 3.3-byte forms pass 2^31
    for form in ("f32", "f16", "bf16", "split16", "qk8"):
        assert form in EC.ATTN_TOL
    # the long rows' crossings: the split16 rows against period 127, the 640 H byte record rows against the period of 3
    # that the record form runs with.  A period of 3 leaves check (b) blind to a displacement by a multiple of 3 heads
    # WITHIN a token row; a 32-bit wrap displaces by 2^31 or 2^32 bytes, which is also another token row and another
    # plane: the byte at the crossing and the byte a wrapped offset reaches come from different places of the base, and
    # so do the bytes of the 64 heads behind them
    p3 = EC.ATTN_QK8_PERIOD
    assert p3 % 2 == 1 and Hl % p3 == 2
    for B, lim in ((2, G2), (3, G4)):
        assert EC.attention_phase_at(lim, B, Ll, Hl, pl, 128) != EC.attention_phase_at(0, B, Ll, Hl, pl, 128)
        assert B * Ll * 640 * Hl > lim
        for k in range(64):
            at = EC.attention_slot_at(lim + 128 * k, B, Ll, Hl, p3, 128, 640 * Hl)
            landed = EC.attention_slot_at(128 * k, B, Ll, Hl, p3, 128, 640 * Hl)
            assert at[1:3] != landed[1:3], (B, k, at, landed)            # another token row or plane, whatever the phase
    q = EC.attention_heads(5, 3, True)
    ref = EC.attention_reference(q, 5, 3, True)
    f = q.double().view(3, 5, 3, 64)
    one = torch.softmax((f[1, :, 0] * EC.LN2) @ f[1, :, 1].t(), -1) @ f[1, :, 2]
    assert torch.allclose(ref[1], one, rtol=1e-12, atol=1e-14)


def test_counts_are_the_closed_form():
    for rows in (1, P - 1, P, P + 1, 5 * P + 17, EC.ROWS, EC.WGRAD_ROWS):
        c = EC.counts(rows)
        assert int(c.sum()) == rows and c.max() - c.min() <= 1
        if rows < 10 * P:
            assert np.array_equal(c, np.bincount(np.arange(rows) % P, minlength=P))
    n = 2 ** 20
    s, l = EC.metric_base("plain")
    pos, neg = EC.pair_counts(n, l)
    scores, labels = EC.expand(n, s, l)
    idx = np.arange(n) % EC.MP
    assert np.array_equal(pos, np.bincount(idx, weights=labels != 0, minlength=EC.MP).astype(np.int64))
    assert np.array_equal(pos + neg, np.bincount(idx, minlength=EC.MP)) and int((pos + neg).sum()) == n


def test_reduction_references_are_the_expanded_sums():
    rows = 3 * P + 11
    dz, want = EC.bias_grad_base(rows)
    full = dz.double()[torch.arange(rows) % P]
    assert torch.equal(full.sum(0), want) and torch.equal(dz, dz.round())
    x, dy, (dw, db), _ = EC.ln_param_grad_base(rows)
    assert torch.equal(dy, dy.round()) and torch.equal(db, dy.double()[torch.arange(rows) % P].sum(0))
    xf, df = x.double()[torch.arange(rows) % P].requires_grad_(False), dy.double()[torch.arange(rows) % P]
    w = torch.ones(EC.WIDTH, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(EC.WIDTH, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(xf, (EC.WIDTH,), w, b, EC.LN_EPS).backward(df)
    assert torch.allclose(w.grad, dw, rtol=1e-9, atol=1e-9) and torch.allclose(b.grad, db, rtol=1e-9, atol=1e-9)
    dzw, u, exact = EC.wgrad_base()
    r = EC.WGRAD_ROWS
    c = torch.from_numpy(EC.counts(r)).double()
    assert float(exact.abs().max()) < 2 ** 24 and torch.equal(exact, exact.round())
    assert torch.equal(exact, torch.einsum("j,jo,ji->oi", c, dzw.double(), u.double()))


def test_a_wrapped_row_offset_changes_the_exact_reductions():
    """bias_grad's dz and layernorm_param_grad's x / d_y are fp32 rows of 4 KiB: a byte offset truncated to 32 bits
    makes rows [2^20, rows) read rows [0, 2051).  Applied to the references: the integer sums (db, d_b) change in almost
    every column, so equality sees it; d_w moves by some 10^-5 of its summation bound, which is why d_w is not what pins
    the addressing (the bound is the rule's, 6 % of the sum of magnitudes at this row count, and is not tightened)."""
    rows, wrap = EC.ROWS, (1 << 32) // (4 * EC.WIDTH)
    assert wrap == 2 ** 20 < rows and np.array_equal(EC.wrapped_counts(rows, rows), EC.counts(rows))
    moved = EC.wrapped_counts(rows, wrap) - EC.counts(rows)
    assert int(moved.sum()) == 0 and int(np.abs(moved).sum()) == 18           # nine rows leave phases 9 .. 17 for 0 .. 8
    _, want = EC.bias_grad_base(rows)
    _, wrapped = EC.bias_grad_base(rows, wrap)
    assert int((wrapped != want).sum()) > 0.9 * EC.WIDTH
    _, _, (dw, db), mag = EC.ln_param_grad_base(rows)
    _, _, (dw_w, db_w), _ = EC.ln_param_grad_base(rows, wrap)
    assert int((db_w != db).sum()) > 0.9 * EC.WIDTH
    bound = EC.reduction_bound(rows, mag, EC.IQB_MAX_CHUNKS)
    assert float(((dw_w - dw).abs() / bound).max()) < 1e-3 and bool((bound < 0.07 * mag).all())
    lost = EC.ln_param_grad_base(rows - rows // 8)[2][0]                        # an eighth of the rows left out
    assert bool(((lost - dw).abs() > bound).all())
    # an int ELEMENT offset r * 1024 stays below 2^31 up to row 2^21: at this row count only byte offsets wrap
    assert EC.wrapped_offset((rows - 1) * EC.WIDTH, 32, True) == (rows - 1) * EC.WIDTH


def test_drop_cls_rows_map_is_the_kernels():
    B, L, rpi, off = 3, 5, 9, 2
    dst = np.full(B * rpi, -1)
    for b in range(B):
        for t in range(L - 1):
            dst[b * rpi + off + t] = b * L + 1 + t
    written, source = EC.drop_cls_source(np.arange(B * rpi), B, L, 8, rpi, off)
    assert np.array_equal(written, dst >= 0) and np.array_equal(source[written], dst[written])
    c = EC.DROP_CLS
    assert c["rows_per_image"] >= c["row_off"] + c["L"] - 1 and c["L"] % P and c["rows_per_image"] % P


@pytest.mark.parametrize("kind", EC.METRIC_KINDS)
@pytest.mark.parametrize("n", [200003, 2 ** 20])
def test_weighted_curve_reference_is_curve_metrics(n, kind):
    """EC.curve_metrics_weighted on (value, count) pairs against MD.curve_metrics and forward_utils.f1max_eval on the
    expanded arrays: integers and the threshold equal, AP within 1e-10"""
    import forward_utils as FU
    s, l = EC.metric_base(kind)
    scores, labels = EC.expand(n, s, l)
    want = MD.curve_metrics(scores, labels)
    values = MD.normalise(s)
    assert np.array_equal(want["normalised"], values[np.arange(n) % EC.MP])
    got = EC.curve_metrics_weighted(values, *EC.pair_counts(n, l))
    assert (got["num"], got["P"], got["N"], got["groups"]) == (want["num"], want["P"], want["N"], want["groups"])
    assert got["auroc"] == want["auroc"] and abs(got["ap"] - want["ap"]) <= 1e-10
    f = FU.f1max_eval(labels, want["normalised"])
    assert (got["tp"], got["fp"], got["fn"], got["groups"]) == (f.tp, f.fp, f.fn, f.groups)
    assert np.float32(got["threshold"]).view(np.uint32) == np.float32(f.threshold).view(np.uint32)
    assert got["start"] == n - f.tp - f.fp and got["f1"] == f.f1
    if kind == "passthrough":
        assert want["packed"] is False and s.max() == 1 and (s < 0).any()
        zeros = s[s == 0].view(np.uint32)
        assert set(zeros.tolist()) == {0, 0x80000000} and got["groups"] == EC.MP - 1      # the two zeros are one group
    else:
        assert want["packed"] is True


# ------------------------------------------------------------------------------------------------ refusals
def test_refusal_table_covers_every_limit_of_capi():
    literals = EC.limit_messages()
    assert len(literals) >= 30
    covered = {r[3] for r in EC.REFUSALS}
    assert covered == set(literals), (sorted(set(literals) - covered), sorted(covered - set(literals)))
    assert len({r[0] for r in EC.REFUSALS}) == len(EC.REFUSALS)
    for word in EC.LIMIT_WORDS:
        assert any(word in lit for lit in literals), word


@pytest.mark.parametrize("case", EC.REFUSALS, ids=[r[0] for r in EC.REFUSALS])
def test_every_refusal_is_decided_on_the_host(case):
    """the checks run before the first launch, so the same call is refused without a GPU -- which is also what makes it
    safe to send with small buffers on one"""
    lib = _lib.load()
    rid, entry, args, literal, prefix = case
    bases = (0x10000000, 0x20000000, 0x30000000)          # never read: every one of these calls ends in its checks
    if torch.cuda.is_available():                         # with a device present the stand-ins are real, if small, buffers
        held = [torch.zeros(8 * EC.REFUSAL_SLOT, dtype=torch.uint8, device="cuda:0") for _ in bases]
        bases = tuple(t.data_ptr() for t in held)
    a, keep = EC.refusal_arguments(args, *bases)
    rc = getattr(lib, entry)(*a)
    msg = lib.aaclip_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else msg
    assert rc == -1 and msg == prefix + literal, (rid, rc, msg)


def test_the_last_allowed_sizes_are_what_the_gpu_cases_run():
    """one step below each refusal that a GPU case sits on: the metrics sizes end at 2^31 - 1, and the long-row attention
    refusal is one head above the largest head count whose rows fit"""
    assert max(EC.METRIC_SIZES) + 1 == EC.N31
    span = [r for r in EC.REFUSALS if r[0] == "attention_split.span_long"][0][2]
    L, H = span[3], span[4]
    assert L * 3 * 64 * H * 4 >= G2 > L * 3 * 64 * (H - 1) * 4
    L, H = [r for r in EC.REFUSALS if r[0] == "attention.span"][0][2][4:6]
    assert L * 3 * 64 * H * 4 >= G2 > (L - 1) * 3 * 64 * H * 4


# ------------------------------------------------------------------------------------------------ truncated offsets
def test_where_a_truncated_row_offset_lands():
    """The three mutations the extent tests are meant to catch, emulated on the index alone.
    layernorm_kernel, split output (`out + row * 2 * D` in halves): as an int the offset turns negative from row 2^20 on,
    so rows [2^20, rows) are never written and check (b) finds their fill; the fp32 forms' element offsets stay below
    2^31, but their byte offset truncated to 32 bits sends row 2^20 (phase 9) onto row 0 (phase 0): checks (a) and (b).
    epi_store (`row * ldc`, ldc = 16384): negative as an int from row 2^17 on -- rows [2^17, M) keep their fill.
    sort_scatter_kernel (`chunk * SORT_CHUNK`): the largest chunk base of n = 2^31 - 1 is 2^31 - 2048, which an int
    holds: the truncation changes nothing at any permitted n.  What a 32-bit BYTE offset would do is caught: from chunk
    2^19 on it reads the keys of chunk - 2^19, whose values differ (2^30 is no multiple of 65537), so the counts of the
    distinct keys come out wrong."""
    rows, D = EC.ROWS, EC.WIDTH
    first_bad = min(r for r in (2 ** 20 - 1, 2 ** 20, rows - 1) if EC.wrapped_offset(r * 2 * D, 32, True) != r * 2 * D)
    assert first_bad == 2 ** 20 and EC.wrapped_offset((rows - 1) * 2 * D, 32, True) < 0
    assert EC.wrapped_offset((rows - 1) * D, 32, True) == (rows - 1) * D                 # fp32 / 16-bit rows: no wrap
    assert EC.wrapped_offset(2 ** 20 * 4 * D, 32) == 0 and 2 ** 20 % P == 9
    M, ld = EC.GEMM_M16, EC.GEMM_LD
    assert EC.wrapped_offset(2 ** 17 * ld, 32, True) < 0 <= EC.wrapped_offset((2 ** 17 - 1) * ld, 32, True) and M > 2 ** 17
    assert EC.wrapped_offset((EC.GEMM_M32 - 1) * ld, 32, True) == (EC.GEMM_M32 - 1) * ld  # fp32 A: caught at M16 only
    chunk = 2048
    for n in EC.METRIC_SIZES:
        last = (n + chunk - 1) // chunk - 1
        assert EC.wrapped_offset(last * chunk + chunk - 1, 32, True) == last * chunk + chunk - 1
    n = max(EC.METRIC_SIZES)
    i = 2 ** 19 * chunk
    assert 4 * i == G4 and i < n and EC.wrapped_offset(4 * i, 32) == 0 and i % EC.MP != 0
