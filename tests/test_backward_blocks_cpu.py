"""CPU side of the building-block tests (tests/backward_blocks_cases.py): the weight-gradient GEMM's chunk table, the case
lists' coverage, the formulas behind the term sums against fp64 autograd, the measured constants against the fp32
evaluation they were measured on, and the sensitivity of the zero-kink cases.  Nothing here launches a kernel."""
import torch

import backward_blocks_cases as BB
from aaclip_hip import _lib

P = 0x7f0000001000      # a plausible, 16-byte aligned device address: nothing here may be dereferenced


# ---------------------------------------------------------------------------------------------- gemm_wgrad
def test_wgrad_chunk_table():
    """The numbers of wgrad_chunking's docstring; a change of the rule in csrc/text_backward.hip moves the edges the row
    counts were chosen for."""
    assert BB.WGRAD_TABLE == {1: (16, 1), 15: (16, 1), 16: (16, 1), 17: (32, 1), 128: (128, 1), 129: (80, 2),
                              2047: (128, 16), 2048: (128, 16), 2049: (144, 15), 2176: (144, 16)}
    last = {r: r - (nc - 1) * rpc for r, (rpc, nc) in BB.WGRAD_TABLE.items()}
    assert last[129] == 49 and last[2047] == 127 and last[2048] == 128 and last[2049] == 33 and last[2176] == 16
    for rows in list(range(1, 4500)) + [5000, 10 ** 6, 2 ** 31 - 1]:
        rpc, nc = BB.wgrad_chunking(rows)
        assert rpc % 16 == 0 and 1 <= nc <= BB.WGRAD_MAX_CHUNKS and (nc - 1) * rpc < rows <= nc * rpc, rows


def test_wgrad_chunk_rule_is_the_librarys():
    """The library refuses a workspace one byte short of chunks * O * I floats, and only asks for one above one chunk
    (every check precedes the launch; a call that passed them all would launch, so none is made here)."""
    lib = _lib.load()
    for rows in (129, 2047, 2048, 2049, 2176):
        O, I = 256, 1024
        need = 4 * BB.wgrad_ws_floats(rows, O, I)
        assert need == 4 * BB.WGRAD_TABLE[rows][1] * O * I
        rc = lib.aaclip_gemm_wgrad(P, O, P, I, P, rows, O, I, P, need - 1, None)
        assert rc < 0 and b"workspace too small" in lib.aaclip_last_error(), rows
    for rows in (1, 15, 16, 17, 128):
        assert BB.wgrad_ws_floats(rows, 256, 1024) == 0
    # the strides of the strided cases pass the stride check and fail on the workspace, the check behind it
    rc = lib.aaclip_gemm_wgrad(P, 256 + BB.WGRAD_PAD_Z, P, 1024 + BB.WGRAD_PAD_U, P, 129, 256, 1024, P, 16, None)
    assert rc < 0 and b"workspace too small" in lib.aaclip_last_error()


def test_wgrad_case_lists():
    rows_seen = {r for r, O, I in BB.WGRAD_CASES if O != I}
    assert rows_seen == set(BB.WGRAD_ROWS)                                  # every row count with a non-square shape
    for shape in ((128, 128), (256, 1024), (1024, 256), (1024, 1024)):
        assert any((O, I) == shape and BB.WGRAD_TABLE[r][1] > 1 for r, O, I in BB.WGRAD_CASES), shape
    assert sorted(r for r, O, I in BB.WGRAD_CASES if (O, I) == (1024, 1024)) == [129, 2049]
    assert [BB.WGRAD_TABLE[r][1] > 1 for r, _, _ in BB.WGRAD_EXACT_CASES] == [False, True]
    assert all(O != I for _, O, I in BB.WGRAD_EXACT_CASES + BB.WGRAD_STRIDED_CASES)
    assert BB.WGRAD_OFF_Z % 4 == 0 and BB.WGRAD_OFF_U % 4 == 0             # 16-byte aligned windows
    assert BB.WGRAD_OFF_Z <= BB.WGRAD_PAD_Z and BB.WGRAD_OFF_U <= BB.WGRAD_PAD_U


def test_wgrad_exact_cases_are_integers_below_2_24():
    for case in BB.WGRAD_EXACT_CASES:
        dz, u, want = BB.wgrad_exact_case(*case)
        assert torch.equal(dz, dz.round()) and torch.equal(u, u.round())
        assert float(want.abs().max()) < 2 ** 24 and torch.equal(want, want.round())
        assert not torch.equal(dz, dz.flip(0)) and not torch.equal(dz, dz.flip(1))
        assert not torch.equal(u, u.flip(0)) and not torch.equal(u, u.flip(1))


def test_wgrad_bound_holds_for_fp32_on_the_cpu():
    """The derived bound is not a measured one: torch's fp32 product must sit far inside it."""
    for case in [(17, 1024, 256), (129, 256, 1024), (2049, 256, 1024)]:
        dz, u, want, mag = BB.wgrad_case(*case)
        err = ((dz.t() @ u).double() - want).abs()
        assert bool((err <= BB.wgrad_bound(case[0], mag)).all())


# ---------------------------------------------------------------------------------------------- row kernels
def test_formulas_are_the_references():
    """The formulas the term sums are built from, in fp64, against fp64 torch autograd: a ratio of 1e-3 is 6e-11 of the
    term sum (fp64 itself gives ~1e-6)."""
    for case in BB.LN_CASES:
        (x, w, b, dy, dr), want = BB.ln_case(*case)
        got = BB.ln_backward_formula(x.double(), w.double(), dy.double(), dr.double())[0]
        assert BB.ratio(got, *want["resid"]) < 1e-3, case
    for case in BB.MIX_CASES + BB.MIX_ZERO_CASES:
        (u, z, dy), want, terms = BB.mix_case(*case)
        got = BB.mix_backward_formula(u.double(), z.double(), dy.double(), case[3])[:2]
        assert BB.ratio(got[0], want[0], terms[0]) < 1e-3 and BB.ratio(got[1], want[1], terms[1]) < 1e-3, case
    for name, (B, L, D, E, act, _) in BB.ALL_HEAD_CASES.items():
        t, want, terms = BB.head_case(name)
        got = BB.head_formula({k: v.double() for k, v in t.items()}, B, L, act)
        for k in BB.HEAD_OUTPUTS:
            assert BB.ratio(got[k], want[k], terms[k]) < 1e-3, (name, k)
    for name in BB.ROW_HEAD_ZERO_CASES:
        t, want, terms = BB.row_head_case(name)
        got = BB.row_head_formula({k: (v.double() if v.is_floating_point() else v) for k, v in t.items()}, name)
        for k in BB.ROW_HEAD_OUTPUTS:
            assert BB.ratio(got[k], want[k], terms[k]) < 1e-3, (name, k)


def test_row_kernel_constants():
    """K is 8 x the fp32 evaluation's own largest ratio: the constants may not drop below what they were measured on,
    and they are not padded beyond the stated 1.1 and the rounding either."""
    for measured, const, k in ((BB.ln_ref_ratio(), BB.LN_REF_RATIO, BB.LN_K), (BB.mix_ref_ratio(), BB.MIX_REF_RATIO, BB.MIX_K),
                               (BB.head_ref_ratio(), BB.HEAD_REF_RATIO, BB.HEAD_K)):
        print("fp32 reference ratio", measured, "constant", const)
        assert measured <= const <= 1.5 * measured, (measured, const)
        assert k == 8 * const


def test_row_kernel_case_lists():
    for cases in (BB.LN_CASES, BB.MIX_CASES):
        assert {c[0] for c in cases} == {256, 768, 1024} and {c[1] for c in cases} == {1, 5, 131}
    assert {(c[0], c[3]) for c in BB.MIX_CASES} == {(D, m) for D in BB.WIDTHS for m in (0.1, 0.9)}
    shapes = {(c[0], c[1], c[2], c[3]) for c in BB.HEAD_CASES.values()}
    assert {(B, L, D, E) for B, L in ((1, 2), (3, 5)) for D in BB.WIDTHS for E in BB.WIDTHS} <= shapes
    # the element-wise kernels' guard: n / 4 no multiple of 256, and exact multiples
    n4 = sorted(c[0] * c[3] // 4 for c in BB.ROW_HEAD_ZERO_CASES.values())             # act' over [n, E]
    assert n4 == [256, 256, 960]
    add4 = {c[0] * c[1] * c[2] // 4 for c in BB.HEAD_CASES.values()}                   # d_ln + d_ln2 over [B L, D]
    assert any(v % 256 for v in add4) and any(v % 256 == 0 for v in add4)


def test_ln_edge_rows_are_what_they_claim():
    x = BB.ln_inputs(1024, 131, "edges")[0].double()
    mean, var = x.mean(dim=-1), x.var(dim=-1, unbiased=False)
    assert abs(float(mean[1]) - 50) < 0.1 and 0.005 < float(var[1]) < 0.02
    assert float(var[2]) < 1e-2 * BB.LN_EPS and float(var[2]) > 0
    assert float(var[3]) == 0.0 and float(mean[3]) == 1.25


# ---------------------------------------------------------------------------------------------- LeakyReLU at zero
def test_zero_kink_cases_tell_the_two_conventions_apart():
    """Where z is exactly 0 the reference (torch's leaky_relu: slope 0.01) and a slope of 1 differ by a factor of 100;
    99 times the reference must break the bound there, or the case could not notice."""
    for case in BB.MIX_ZERO_CASES:
        (u, z, dy), want, terms = BB.mix_case(*case)
        at = z == 0
        assert bool(at.any()) and bool((99 * want[0][at].abs() > BB.MIX_K * BB.EPS24 * terms[0][at]).all()), case
        # ... and autograd did take 0.01 there
        got = BB.mix_backward_formula(u.double(), z.double(), dy.double(), case[3])[0]
        assert BB.ratio(got, want[0], terms[0]) < 1e-3
    for name, (B, L, D, E, act, row) in BB.HEAD_ZERO_CASES.items():
        if act != BB.LEAKY:
            continue
        t, want, terms = BB.head_case(name)
        for k in ("d_proj_w", "d_det_w"):
            assert bool((99 * want[k][row].abs() > BB.HEAD_K * BB.EPS24 * terms[k][row]).any()), (name, k)
    for name, c in BB.ROW_HEAD_ZERO_CASES.items():
        t, want, terms = BB.row_head_case(name)
        row = c[5]
        assert bool((99 * want["d_proj_w"][row].abs() > BB.HEAD_K * BB.EPS24 * terms["d_proj_w"][row]).any()), name


# ---------------------------------------------------------------------------------------------- attention
def test_attention_cases_and_bars():
    assert {c[0] for c in BB.ATTN_CASES if c[2] is None} == {2, 63, 64, 65, 127}
    assert {c[0] for c in BB.ATTN_CASES if c[2] is not None} == {65, 128}
    assert all((L, causal, p) in BB.ATTN_CASES for L, _, p in BB.ATTN_CASES for causal in (True, False))
    assert {(c[0], c[2] is not None) for c in BB.ATTN_CASES} == set(BB.ATTN_SEG_REF)
    for (L, peaked), const in BB.ATTN_SEG_REF.items():
        measured = BB.attention_ref_segment_error(L, peaked)
        print("fp32 segment error", L, peaked, measured, "constant", const)
        assert measured <= const <= 1.5 * measured, (L, peaked, measured, const)
        assert BB.attention_segment_bar(L, BB.ATTN_PEAK if peaked else None) == 8 * const


def test_peaked_rows_underflow():
    """peak = 40: in every row most of expf(s - m) is below fp32's smallest normal number relative to the row sum."""
    qkv, _, _ = BB.attention_case(128, False, BB.ATTN_PEAK)
    D = 64 * BB.ATTN_H
    q, k = (t.double().reshape(BB.ATTN_B, 128, BB.ATTN_H, 64).transpose(1, 2) for t in (qkv[:, :D], qkv[:, D:2 * D]))
    s = q @ k.transpose(-1, -2)
    assert abs(float(s.amax(dim=-1).max()) - BB.ATTN_PEAK) < 1e-3
    small = (torch.exp(s - s.amax(dim=-1, keepdim=True)) < 1e-7).double().mean()
    assert float(small) > 0.5, float(small)
