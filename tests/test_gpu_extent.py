"""Entry points on operands whose extent passes 2^31 and 2^32 bytes, at the size limits include/aaclip.h states, and one
step past them (tests/extent_cases.py holds the cases, the period arithmetic, the references and the refusal table;
tests/test_extent_cases_cpu.py pins them on the CPU).

Every operand that grows with the row count is periodic with the odd period P = 1021 (the metrics: 65537 values, labels
of period 3 x 65537), gathered on the device from a P-row base: nothing of full size exists on the host.  A case checks
(a) rows [0, P) against the fp64 reference at the tolerance of the entry's existing test, named in extent_cases.py and
beside each test here, (b) every later row r against row r % P byte for byte, in slabs of at most 256 MiB on the device
-- every kernel here forms a row from that row alone (read in csrc/rowops.hip, csrc/iqm.hip, csrc/text_backward.hip,
csrc/iqm_query_backward.hip, csrc/split3_rows.hip; a GEMM row from its A row and the shared weight) -- and that the 4 KiB
guards on both sides of every output, and the gap columns of a strided output, still hold their fill.  Reductions over
rows are compared with sum_j count_j term_j in fp64.  An allocation that fails FAILS the test with its byte count: a
skip would hide the gap.  These pin addressing that is correct today: they are expected to pass."""
import contextlib
import ctypes
import time

import numpy as np
import pytest
import torch

import backward_blocks_cases as BB
import backward_bf16x3_cases as BC
import extent_cases as EC
import fused_epilogue_cases as FC
import metrics_device_cases as MD
import placement_cases as PC
from aaclip_hip import _lib, engine

pytestmark = pytest.mark.gpu
F32, F16, BF16, F16X2 = _lib.F32, _lib.F16, _lib.BF16, _lib.F16X2
TDT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
NAME = {F32: "fp32", F16: "fp16", BF16: "bf16", F16X2: "fp16x2"}
GUARD, GUARD_BYTE, FILL_BYTE = PC.GUARD, 0xA5, 0xFF         # tests/test_gpu_placement.py's constants
FILL_WORD = -1                                              # eight FILL_BYTEs as an int64: a NaN in every float type
SLAB = 256 << 20
P = EC.P


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    d = torch.device("cuda:0")
    torch.zeros(1, device=d)                  # the allocator's statistics exist once the device has been used
    yield d
    torch.cuda.empty_cache()


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@contextlib.contextmanager
def measured(dev, group, what):
    """prints the peak of reserved memory and the wall time of one case; the cache is released behind it, so that the
    next case's peak is its own"""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    try:
        yield
    finally:
        torch.cuda.synchronize(dev)
        print(f"extent {group} {what}: peak reserved {torch.cuda.max_memory_reserved(dev) / 2 ** 30:.2f} GiB, "
              f"{time.perf_counter() - t0:.2f} s")
        torch.cuda.empty_cache()


def alloc(dev, nbytes, what):
    try:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    except Exception as e:      # no skip: a skip would hide the gap
        pytest.fail(f"{what}: {nbytes} bytes could not be allocated: {e}")


class Guarded:
    """nbytes on the device (a multiple of 8) between two guards of GUARD bytes"""
    def __init__(self, dev, nbytes, what, fill=FILL_BYTE):
        assert nbytes % 8 == 0
        self.what, self.nbytes = what, nbytes
        self.buf = alloc(dev, nbytes + 2 * GUARD, what)
        self.buf[:GUARD] = GUARD_BYTE
        self.buf[GUARD + nbytes:] = GUARD_BYTE
        self.body = self.buf[GUARD:GUARD + nbytes]
        if fill is not None:
            self.body.fill_(fill)

    def ptr(self):
        return self.body.data_ptr()

    def words(self, row_bytes):
        """the body as int64 [rows, row_bytes / 8]"""
        return self.body.view(torch.int64).view(-1, row_bytes // 8)

    def check_guards(self):
        assert bool((self.buf[:GUARD] == GUARD_BYTE).all()), f"{self.what}: the guard in front was written"
        assert bool((self.buf[GUARD + self.nbytes:] == GUARD_BYTE).all()), f"{self.what}: the guard behind was written"

    def check_untouched(self):
        self.check_guards()
        assert bool((self.body.view(torch.int64) == FILL_WORD).all()), f"{self.what}: a refused call wrote its output"


def row_slabs(rows, row_bytes, start=0):
    step = max(1, SLAB // row_bytes)
    for r0 in range(start, rows, step):
        yield r0, min(rows, r0 + step)


def as_words(t):
    """host or device tensor [rows, cols] of any type -> int64 [rows, row_bytes / 8]"""
    t = t.contiguous()
    return t.view(torch.uint8).view(t.shape[0], -1).view(torch.int64)


def fill_periodic(words, base_words):
    """words [rows, ld / 8] (device): columns [0, w) of row r <- base_words[r % P] (device, [P, w])"""
    rows, w = words.shape[0], base_words.shape[1]
    for r0, r1 in row_slabs(rows, 8 * w):
        idx = torch.arange(r0, r1, device=words.device) % base_words.shape[0]
        if w == words.shape[1]:
            torch.index_select(base_words, 0, idx, out=words[r0:r1])
        else:
            words[r0:r1, :w] = base_words[idx]


def check_periodic(words, w, what):
    """rows [P, rows) of columns [0, w) equal row r % P byte for byte, and the gap columns [w, ld) of EVERY row still hold
    the fill -> the first P rows of columns [0, w) on the host (int64)"""
    rows, ld = words.shape
    first = words[:P, :w].clone()
    for r0, r1 in row_slabs(rows, 8 * ld):
        got = words[r0:r1]
        if r1 > P:
            a = max(r0, P)
            idx = torch.arange(a, r1, device=words.device) % P
            same = got[a - r0:, :w] == first[idx]
            if not bool(same.all()):
                bad = a + int((~same.all(dim=1)).nonzero()[0])
                raise AssertionError(f"{what}: row {bad} differs from row {bad % P} (its phase)")
        if ld > w and not bool((got[:, w:] == FILL_WORD).all()):
            bad = r0 + int((got[:, w:] != FILL_WORD).any(dim=1).nonzero()[0])
            raise AssertionError(f"{what}: the gap columns of row {bad} were written")
    return first.cpu()


def assert_close(a, b, atol, rtol, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite output"
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} outside {atol}+{rtol}*|ref|; "
                           f"max err {err.max().item():.3e} at ref {b.flatten()[err.argmax()].item():.3e}")


def check_ratio(what, got, want, terms, K):
    r = BB.ratio(got.double(), want, terms)
    print(what, "largest |err| / (2^-24 terms):", r, "of", K)
    assert r <= K, (what, r, K)


def decode(words, dtype):
    """int64 [rows, w] (host) -> [rows, 8 w / itemsize] of dtype"""
    return words.contiguous().view(torch.uint8).view(words.shape[0], -1).view(dtype)


# ----------------------------------------------------------------------------------------------------------------
# group 1: row and element entry points at rows = 2^20 + 2051, D = 1024
# ----------------------------------------------------------------------------------------------------------------
def run_row_case(dev, name, bases, call, vectors=()):
    """bases: name -> host tensor [P, cols] of every 'in' / 'inout' operand of EC.ROW_CASES[name]; vectors: small
    operands, uploaded as they are; call(ptr: name -> address, rows) -> rc.  -> name -> the first P rows (host, int64
    words) of every 'out' / 'inout' operand, after the checks every case shares"""
    lib = _lib.load()
    rows, ops, _ = EC.ROW_CASES[name]
    bufs, small = {}, {k: v.to(dev).contiguous() for k, v in dict(vectors).items()}
    for o in ops:
        g = Guarded(dev, rows * o.row_bytes, f"{name} {o.name}", fill=None if o.role != "out" else FILL_BYTE)
        if o.role != "out":
            fill_periodic(g.words(o.row_bytes), as_words(bases[o.name]).to(dev))
        bufs[o.name] = g
    ptr = {k: g.ptr() for k, g in bufs.items()}
    ptr.update({k: v.data_ptr() for k, v in small.items()})
    rc = call(ptr, rows)
    assert rc == 0, f"{name}: rc {rc}: {lib.aaclip_last_error()}"
    torch.cuda.synchronize(dev)
    first = {}
    for o in ops:
        bufs[o.name].check_guards()
        if o.role != "in":
            first[o.name] = check_periodic(bufs[o.name].words(o.row_bytes), o.row_bytes // 8, f"{name} {o.name}")
    return first


@pytest.mark.parametrize("code", [F32, F16, BF16])
def test_layernorm(dev, code):
    """(a): tests/test_gpu_parity.py test_layernorm -- 2e-6 + 1e-5 |ref| (fp32), 2e-3 / 2e-2 + 1e-2 |ref| (fp16 / bf16)"""
    lib = _lib.load()
    name = "layernorm_" + ("f32" if code == F32 else NAME[code].replace("fp", "f"))
    x, w, b, ref = EC.ln_base()
    with measured(dev, "group1", name):
        first = run_row_case(dev, name, {"x": x}, lambda p, rows: lib.aaclip_layernorm(
            p["x"], p["w"], p["b"], p["out"], code, rows, EC.WIDTH, EC.LN_EPS, stream(dev)), {"w": w, "b": b})
    assert_close(decode(first["out"], TDT[code]).float(), ref, *EC.LN_TOL[name], name)


@pytest.mark.parametrize("hi8", [1, 0])
def test_layernorm_split(dev, hi8):
    """(a): tests/test_gpu_split.py test_layernorm_split_output -- hi + lo8 within 6e-6 + 2^-14 |ref|, the hi8 plane
    within 2^-4 |ref| + 2^-9; hi8 = 0 leaves that plane unwritten (tests/test_gpu_fused_epilogues.py)"""
    lib = _lib.load()
    name = "layernorm_split_hi8" if hi8 else "layernorm_split_no_hi8"
    x, w, b, ref = EC.ln_base()
    D = EC.WIDTH
    with measured(dev, "group1", name):
        first = run_row_case(dev, name, {"x": x}, lambda p, rows: lib.aaclip_layernorm_split(
            p["x"], p["w"], p["b"], p["out"], rows, D, EC.LN_EPS, hi8, stream(dev)), {"w": w, "b": b})
    out = decode(first["out"], torch.uint8)
    assert_close(engine.join_split8(out, D), ref, *EC.SPLIT_LN_TOL, name)
    if hi8:
        plane = out[:, 3 * D:].contiguous().view(torch.float8_e4m3fn).double()
        assert float(((plane - ref).abs() / (ref.abs() * 2.0 ** -4 + 2.0 ** -9)).max()) <= 1.0
    else:
        assert bool((out[:, 3 * D:] == FILL_BYTE).all()), "hi8 = 0 wrote the hi8 plane"


def test_split_rows(dev):
    """(a): tests/test_gpu_fused_epilogues.py test_layernorm_and_split_rows_without_hi8 -- engine.split_rows' bytes"""
    lib = _lib.load()
    x = EC.ln_base()[0]
    with measured(dev, "group1", "split_rows"):
        first = run_row_case(dev, "split_rows", {"src": x}, lambda p, rows: lib.aaclip_split_rows(
            p["src"], p["dst"], rows, EC.WIDTH, 1, stream(dev)))
        want = engine.split_rows(x.to(dev)).cpu()
    assert torch.equal(decode(first["dst"], torch.uint8), want)


def test_split3_rows(dev):
    """(a): tests/test_gpu_backward_bf16x3.py test_split3_rows_bit_for_bit -- split_planes' bits"""
    lib = _lib.load()
    x = EC.ln_base()[0]
    with measured(dev, "group1", "split3_rows"):
        first = run_row_case(dev, "split3_rows", {"src": x}, lambda p, rows: lib.aaclip_split3_rows(
            p["src"], p["dst"], rows, EC.WIDTH, stream(dev)))
    assert torch.equal(decode(first["dst"], torch.int16), BC.split_planes(x).view(torch.int16))


def test_adapter_mix(dev):
    """(a): tests/test_gpu_parity.py test_adapter_mix -- 1e-5 + 1e-5 |ref|"""
    lib = _lib.load()
    x, a, ref = EC.mix_base()
    with measured(dev, "group1", "adapter_mix"):
        first = run_row_case(dev, "adapter_mix", {"x": x, "a": a}, lambda p, rows: lib.aaclip_adapter_mix(
            p["x"], p["a"], rows, EC.WIDTH, EC.MIX_WEIGHT, stream(dev)))
    assert_close(decode(first["x"], torch.float32), ref, 1e-5, 1e-5, "adapter_mix")


def test_adapter_mix_fold(dev):
    """(a): tests/test_gpu_fused_epilogues.py test_adapter_mix_fold_every_row_kind -- x bit-equal to aaclip_adapter_mix,
    out16 bit-equal to its rounding, (rstd, b) of the rounded rows inside FC.ab_bounds"""
    lib = _lib.load()
    x, a, _ = EC.mix_base()
    D = EC.WIDTH
    with measured(dev, "group1", "adapter_mix_fold_f16"):
        first = run_row_case(dev, "adapter_mix_fold_f16", {"x": x, "a": a}, lambda p, rows: lib.aaclip_adapter_mix_fold(
            F16, p["x"], p["a"], rows, D, EC.MIX_WEIGHT, p["out16"], p["row_ab"], stream(dev)))
        want, ad = x.to(dev), a.to(dev)
        _lib.check(lib.aaclip_adapter_mix(want.data_ptr(), ad.data_ptr(), P, D, EC.MIX_WEIGHT, stream(dev)))
        want = want.cpu()
    assert torch.equal(decode(first["x"], torch.float32), want), "x differs from aaclip_adapter_mix"
    o16 = decode(first["out16"], torch.float16)
    assert torch.equal(o16.view(torch.int16), want.half().view(torch.int16)), "out16 is not the rounding of x"
    ab64, kappa = FC.finalize64(FC.slice_stats64(o16)[0], D)
    got = decode(first["row_ab"], torch.float32)
    assert torch.isfinite(got).all()
    assert bool(((got.double() - ab64).abs() / FC.ab_bounds(ab64, kappa) <= 1.0).all())


def test_ln_stats_finalize(dev):
    """(a): tests/test_gpu_fused_epilogues.py test_ln_stats_finalize_every_row_kind -- fp64 on the same partials, inside
    FC.ab_bounds"""
    lib = _lib.load()
    D = EC.WIDTH
    part = FC.slice_stats_emulated(FC.round16(FC.rows("plain", P, D), "fp16"))
    with measured(dev, "group1", "ln_stats_finalize"):
        first = run_row_case(dev, "ln_stats_finalize", {"partials": part.view(P, -1)},
                             lambda p, rows: lib.aaclip_ln_stats_finalize(p["partials"], p["row_ab"], rows, D, FC.EPS,
                                                                          stream(dev)))
    ab64, kappa = FC.finalize64(part, D)
    got = decode(first["row_ab"], torch.float32)
    assert torch.isfinite(got).all()
    assert bool(((got.double() - ab64).abs() / FC.ab_bounds(ab64, kappa) <= 1.0).all())


def test_residual_layernorm_and_combine3(dev):
    """(a): tests/test_gpu_iqm.py test_residual_layernorm_combine_smallk_dropcls -- 1e-5 + 1e-5 |ref| and
    1e-6 + 1e-6 |ref|; aaclip_combine3 takes the [rows, 1024] operands as flat n"""
    lib = _lib.load()
    a, b, c, w, bias, ln_ref, c3_ref = EC.combine_base()
    with measured(dev, "group1", "residual_layernorm"):
        first = run_row_case(dev, "residual_layernorm", {"a": a, "b": b}, lambda p, rows: lib.aaclip_residual_layernorm(
            p["a"], p["b"], p["w"], p["bias"], p["out"], rows, EC.WIDTH, 1e-12, stream(dev)), {"w": w, "bias": bias})
    assert_close(decode(first["out"], torch.float32), ln_ref, 1e-5, 1e-5, "residual_layernorm")
    with measured(dev, "group1", "combine3"):
        first = run_row_case(dev, "combine3", {"a": a, "b": b, "c": c}, lambda p, rows: lib.aaclip_combine3(
            p["a"], p["b"], p["c"], 0.4, 0.3, 0.3, p["out"], rows * EC.WIDTH, stream(dev)))
    assert_close(decode(first["out"], torch.float32), c3_ref, 1e-6, 1e-6, "combine3")


def test_layernorm_backward(dev):
    """(a): tests/test_gpu_backward_blocks.py test_layernorm_backward_per_element -- BB.LN_K 2^-24 terms"""
    lib = _lib.load()
    (x, w, dy, dr), want, terms = EC.ln_backward_base()
    with measured(dev, "group1", "layernorm_backward"):
        first = run_row_case(dev, "layernorm_backward", {"x": x, "d_y": dy, "d_resid": dr},
                             lambda p, rows: lib.aaclip_layernorm_backward(p["x"], p["w"], p["d_y"], p["d_resid"], p["d_x"],
                                                                           rows, EC.WIDTH, BB.LN_EPS, stream(dev)), {"w": w})
    check_ratio("extent layernorm_backward", decode(first["d_x"], torch.float32), want, terms, BB.LN_K)


def test_adapter_mix_backward(dev):
    """(a): tests/test_gpu_backward_blocks.py test_adapter_mix_backward_per_element -- BB.MIX_K 2^-24 terms"""
    lib = _lib.load()
    (u, z, dy), want, terms = EC.mix_backward_base()
    with measured(dev, "group1", "adapter_mix_backward"):
        first = run_row_case(dev, "adapter_mix_backward", {"u": u, "z": z, "d_y": dy},
                             lambda p, rows: lib.aaclip_adapter_mix_backward(p["u"], p["z"], p["d_y"], p["d_z"], p["d_u"],
                                                                             rows, EC.WIDTH, EC.MIX_WEIGHT, stream(dev)))
    check_ratio("extent adapter_mix_backward d_z", decode(first["d_z"], torch.float32), want[0], terms[0], BB.MIX_K)
    check_ratio("extent adapter_mix_backward d_u", decode(first["d_u"], torch.float32), want[1], terms[1], BB.MIX_K)


@pytest.mark.parametrize("act", [3, 2])
def test_act_backward(dev, act):
    """(a): tests/test_gpu_iqm_query_backward.py test_entry_against_fp64 -- relative Frobenius error 1e-4; a ReLU output
    of exactly 0 gives exactly 0 (test_exact_zeros).  The third activation code of the header, LeakyReLU, is refused by
    this entry (GELU and RELU only): its derivative runs inside aaclip_adapter_mix_backward, above."""
    lib = _lib.load()
    name = "act_backward_gelu" if act == 3 else "act_backward_relu"
    zy, dy, want = EC.act_base(act)
    with measured(dev, "group1", name):
        first = run_row_case(dev, name, {"zy": zy, "d_y": dy}, lambda p, rows: lib.aaclip_act_backward(
            act, p["zy"], p["d_y"], p["d_z"], rows * EC.WIDTH, stream(dev)))
    got = decode(first["d_z"], torch.float32)
    assert torch.isfinite(got).all()
    assert float((got.double() - want).norm() / want.norm()) <= 1e-4
    if act == 2:
        assert not got[zy == 0].any() and torch.equal(got[zy > 0], dy[zy > 0])


@pytest.mark.parametrize("code", [F32, F16])
def test_linear_smallk(dev, code):
    """R * N = 2^30 + 2.1 M elements.  (a): tests/test_gpu_iqm.py test_residual_layernorm_combine_smallk_dropcls --
    1e-6 + 1e-6 |ref| (fp32), 2e-3 + 2e-3 |ref| (fp16)"""
    lib = _lib.load()
    name = "linear_smallk_f32" if code == F32 else "linear_smallk_f16"
    x, W, bias, ref = EC.smallk_base()
    with measured(dev, "group1", name):
        first = run_row_case(dev, name, {"x": x}, lambda p, rows: lib.aaclip_linear_smallk(
            code, p["x"], p["W"], p["bias"], p["y"], rows, EC.WIDTH, 2, stream(dev)), {"W": W, "bias": bias})
    tol = 1e-6 if code == F32 else 2e-3
    assert_close(decode(first["y"], TDT[code]).float(), ref, tol, tol, name)


def test_head_expand_and_head_diag(dev):
    """H = 16, D = 1024: the expanded operand [rows * 16, 1024] fp32 is 4 GiB + 2.3 MiB, rows * H < 2^31.  head_expand
    (a): test_cross_rows_equals_projected_cross_attention's allclose at 1e-7 (+ 1e-5 |ref|); head_diag copies: equality"""
    lib = _lib.load()
    q, want, full, diag = EC.head_base()
    H, D = EC.HEAD_H, EC.WIDTH
    with measured(dev, "group1", "head_expand"):
        first = run_row_case(dev, "head_expand", {"q": q}, lambda p, rows: lib.aaclip_head_expand(
            F32, p["q"], p["qm"], rows, H, D, (D // H) ** -0.5, stream(dev)))
    assert_close(decode(first["qm"], torch.float32), want, 1e-7, 1e-5, "head_expand")
    with measured(dev, "group1", "head_diag"):
        first = run_row_case(dev, "head_diag", {"full": full}, lambda p, rows: lib.aaclip_head_diag(
            p["full"], p["ctx"], rows, H, D, stream(dev)))
    assert torch.equal(decode(first["ctx"], torch.float32), diag)


def test_largest_grids_that_remain_allowed(dev):
    """A launch covers its grid below 2^24 workgroups of 256 threads only; beyond, it silently runs the count modulo
    2^24 (found here: aaclip_metrics_range with 107 374 183 images of 5 summed 1 / 16 of them; aaclip_head_expand with
    2^24 + 4096 rows wrote 4096).  The per-row entries now refuse such counts (group 5); this runs them AT the limit:
    head_expand with rows * H = 2^24 - 1, head_diag with rows = 2^24 - 1, layernorm with rows = 2^26 - 4 (the last
    workgroup, number 2^24 - 2, holds rows 2^26 - 8 .. 2^26 - 5): every row written, and right."""
    lib = _lib.load()
    D, H = EC.HEAD_MAX_D, 3
    q, want, _, _ = EC.head_base(D, H)
    with measured(dev, "group1", "head_expand_max"):
        first = run_row_case(dev, "head_expand_max", {"q": q}, lambda p, rows: lib.aaclip_head_expand(
            F32, p["q"], p["qm"], rows, H, D, (D // H) ** -0.5, stream(dev)))
    assert_close(decode(first["qm"], torch.float32), want, 1e-7, 1e-5, "head_expand_max")
    _, _, full, diag = EC.head_base(128, 2)
    with measured(dev, "group1", "head_diag_max"):
        first = run_row_case(dev, "head_diag_max", {"full": full}, lambda p, rows: lib.aaclip_head_diag(
            p["full"], p["ctx"], rows, 2, 128, stream(dev)))
    assert torch.equal(decode(first["ctx"], torch.float32), diag)
    x = EC.rnd("ln.max.x", (P, 256), 3.0, 0.7)
    w, b = EC.rnd("ln.max.w", (256,), 0.2, 1.0), EC.rnd("ln.max.b", (256,), 0.2)
    with measured(dev, "group1", "layernorm_max"):
        first = run_row_case(dev, "layernorm_max", {"x": x}, lambda p, rows: lib.aaclip_layernorm(
            p["x"], p["w"], p["b"], p["out"], F16, rows, 256, EC.LN_EPS, stream(dev)), {"w": w, "b": b})
    ref = torch.nn.functional.layer_norm(x.double(), (256,), w.double(), b.double(), EC.LN_EPS)
    assert_close(decode(first["out"], torch.float16).float(), ref, 2e-3, 1e-2, "layernorm_max")


def test_drop_cls_rows(dev):
    """B = 1027 images of L = 1025 fp32 rows of 1024 into rows [2, 1026) of 1027: source and destination pass 2^32 bytes.
    A copy (tests/test_gpu_iqm.py asserts equality): EVERY destination row equals the base row of its source row's phase,
    byte for byte, and the rows that are not written keep their fill."""
    lib = _lib.load()
    c = EC.DROP_CLS
    src_rows, _, dst_rows, _ = EC.DROP_CLS_CASE
    base = EC.ln_base()[0]
    rb = 4 * c["E"]
    with measured(dev, "group1", "drop_cls_rows"):
        src, dst = Guarded(dev, src_rows * rb, "drop_cls src", fill=None), Guarded(dev, dst_rows * rb, "drop_cls dst")
        bw = as_words(base).to(dev)
        fill_periodic(src.words(rb), bw)
        rc = lib.aaclip_drop_cls_rows(F32, src.ptr(), dst.ptr(), c["B"], c["L"], c["E"], c["rows_per_image"], c["row_off"],
                                      stream(dev))
        assert rc == 0, f"drop_cls_rows: rc {rc}: {lib.aaclip_last_error()}"
        torch.cuda.synchronize(dev)
        src.check_guards()
        dst.check_guards()
        words = dst.words(rb)
        for r0, r1 in row_slabs(dst_rows, rb):
            written, source = EC.drop_cls_source(torch.arange(r0, r1, device=dev), **c)
            want = torch.where(written[:, None], bw[source % P], torch.full_like(bw[:1], FILL_WORD))
            if not torch.equal(words[r0:r1], want):
                bad = r0 + int((words[r0:r1] != want).any(dim=1).nonzero()[0])
                raise AssertionError(f"drop_cls_rows: destination row {bad} is not its source row (or was written)")


def reduction_workspace(dev, nbytes, what):
    return Guarded(dev, (nbytes + 7) // 8 * 8, what)


def test_bias_grad(dev):
    """a reduction over the rows on small integers: every partial sum is exact in fp32 in any order (the 64 chunk sums
    and the serial pass that adds them included), so db EQUALS sum_j count_j dz_j -- the summation bound of this row
    count, 6 % of the sum of magnitudes, would not see a wrapped row offset (tests/test_extent_cases_cpu.py)"""
    lib = _lib.load()
    dz, want = EC.bias_grad_base()
    N = EC.WIDTH
    with measured(dev, "group1", "bias_grad"):
        need = lib.aaclip_bias_grad_workspace_bytes(EC.ROWS, N)
        ws, db = reduction_workspace(dev, need, "bias_grad workspace"), Guarded(dev, 4 * N, "bias_grad db")
        run_row_case(dev, "bias_grad", {"dz": dz}, lambda p, rows: lib.aaclip_bias_grad(
            p["dz"], N, db.ptr(), rows, N, ws.ptr(), need, stream(dev)))
        ws.check_guards()
        db.check_guards()
        got = db.body.view(torch.float32).cpu()
    assert torch.equal(got.double(), want)


def test_layernorm_param_grad(dev):
    """d_b: integer d_y, EQUAL to sum_j count_j dy_j.  d_w = sum dy xhat cannot be made exact (xhat is the kernel's own
    fp32 value): terms of one sign, inside EC.reduction_bound = (rows + 64) 2^-24 sum |terms| -- BB.wgrad_bound's rule
    with the 64 partial sums of csrc/iqm_query_backward.hip -- which shows a lost sixteenth of the rows, not a wrapped
    offset; the addressing of x and d_y is pinned by d_b and by the row kernels that read the same way"""
    lib = _lib.load()
    x, dy, want, mag = EC.ln_param_grad_base()
    D = EC.WIDTH
    with measured(dev, "group1", "layernorm_param_grad"):
        need = lib.aaclip_layernorm_param_grad_workspace_bytes(EC.ROWS, D)
        ws = reduction_workspace(dev, need, "layernorm_param_grad workspace")
        d_w, d_b = Guarded(dev, 4 * D, "d_w"), Guarded(dev, 4 * D, "d_b")
        run_row_case(dev, "layernorm_param_grad", {"x": x, "d_y": dy}, lambda p, rows: lib.aaclip_layernorm_param_grad(
            p["x"], p["d_y"], d_w.ptr(), d_b.ptr(), rows, D, EC.LN_EPS, ws.ptr(), need, stream(dev)))
        for g in (ws, d_w, d_b):
            g.check_guards()
        got = [g.body.view(torch.float32).cpu() for g in (d_w, d_b)]
    assert torch.equal(got[1].double(), want[1]), "d_b"
    err = (got[0].double() - want[0]).abs()
    bound = EC.reduction_bound(EC.ROWS, mag, EC.IQB_MAX_CHUNKS)
    print("extent layernorm_param_grad d_w largest |err| / bound:", float((err / bound).max()))
    assert torch.isfinite(got[0]).all() and bool((err <= bound).all()), "d_w"


# ----------------------------------------------------------------------------------------------------------------
# group 2: products whose operands reach the extent through their row strides
# ----------------------------------------------------------------------------------------------------------------
def gemm_operand_rows(code):
    """-> (A rows as the kernel takes them [P, bytes], W, the A and W values the reference uses)"""
    A, W, _, _ = EC.gemm_base()
    if code == F16X2:
        return engine.split_rows(A), engine.split_rows(W, weight=True), A, W
    if code == F32:
        return A, W, A, W
    At, Wt = A.to(TDT[code]), W.to(TDT[code])
    return At, Wt, At.float(), Wt.float()


def gemm_output(code, epi, first):
    """the first P rows of the output (int64 words of its written columns) -> fp64 values"""
    N = EC.GEMM_N
    if epi in (EC.EPI_BIAS_RESID, EC.EPI_ACT_F32) or code == F32:
        return decode(first, torch.float32).double()
    if code != F16X2:
        return decode(first, TDT[code]).double()
    if epi == EC.EPI_BIAS:                                       # split16 rows: hi | lo
        h = decode(first, torch.float16).double()
        return h[:, :N] + h[:, N:]
    return engine.join_split8(decode(first, torch.uint8), N)     # split8 rows


def gemm_tolerance(code, epi):
    """tests/test_gpu_parity.py test_gemm_epilogues / tests/test_gpu_split.py test_gemm_split_epilogues"""
    if code == F16X2:
        return (EC.GEMM_SPLIT_TOL[0], EC.GEMM_SPLIT_TOL[1] + (2.0 ** -14 if epi == EC.EPI_BIAS_GELU else 0.0))
    if epi in (EC.EPI_BIAS_RESID, EC.EPI_ACT_F32):
        return EC.GEMM_F32_OUT_TOL
    return (EC.GEMM_ET[code], EC.GEMM_ET[code])


@pytest.mark.parametrize("code,variant", [(F32, 0), (F16, 0), (F16, 1), (BF16, 0), (BF16, 1), (F16X2, 0), (F16X2, 1)])
def test_gemm_strided(dev, code, variant):
    """aaclip_gemm, N = 256, K = 128, lda = ldc = 16384 elements: every epilogue, on the automatic route (16-bit and
    split operands: the 256-row tiles) and with the 128 x 128 tile forced.  (a): the tolerances of test_gemm_epilogues
    and test_gemm_split_epilogues (gemm_tolerance).  The gap columns of A hold NaN bytes, those of the output its fill."""
    lib = _lib.load()
    N, K, ld, M = EC.GEMM_N, EC.GEMM_K, EC.GEMM_LD, EC.gemm_rows(code)
    a_rows, w_rows, a_seen, w_seen = gemm_operand_rows(code)
    _, _, bias, resid = EC.gemm_base()
    a_es = 4 if code == F32 else 2
    assert lib.aaclip_set_gemm_variant(variant) == 0
    try:
        with measured(dev, "group2", f"gemm {NAME[code]} variant {variant}"):
            A = Guarded(dev, M * ld * a_es, "gemm A")
            fill_periodic(A.words(ld * a_es), as_words(a_rows).to(dev))
            Wd, bd = w_rows.to(dev).contiguous(), bias.to(dev)
            for epi in EC.GEMM_EPIS:
                what = f"gemm {NAME[code]} variant {variant} epilogue {epi}"
                o_rb = dict((o.name, o.row_bytes) for o in EC.GEMM_CASES[(code, epi)][1])["out"]
                out = Guarded(dev, M * o_rb, what)
                if epi == EC.EPI_BIAS_RESID:
                    fill_periodic(out.words(o_rb), as_words(resid).to(dev))
                act, cols, scale, bp = 0, 0, 1.0, bd.data_ptr()
                if epi == EC.EPI_BIAS:
                    cols, scale = 64, 0.125
                if epi == EC.EPI_ACT_F32:
                    act, bp = 1, None
                rc = lib.aaclip_gemm(code, epi, A.ptr(), ld, Wd.data_ptr(), bp, out.ptr(), ld, M, N, K, act, cols, scale,
                                     stream(dev))
                assert rc == 0, f"{what}: rc {rc}: {lib.aaclip_last_error()}"
                torch.cuda.synchronize(dev)
                out.check_guards()
                A.check_guards()
                o_es = 4 if (epi in (EC.EPI_BIAS_RESID, EC.EPI_ACT_F32) or code == F32) else 2
                width = N * o_es * (2 if (code == F16X2 and o_es == 2) else 1)
                first = check_periodic(out.words(o_rb), width // 8, what)
                ref = EC.gemm_reference(a_seen, w_seen, bias, resid, epi)
                assert_close(gemm_output(code, epi, first), ref, *gemm_tolerance(code, epi), what)
                del out
    finally:
        lib.aaclip_set_gemm_variant(0)


def test_gemm_wgrad_strided_exact_integers(dev):
    """aaclip_gemm_wgrad, O = I = 256, ldz = ldu = 16384: both operands 4 GiB + 18.8 MiB; small integers, so the check
    is equality with sum_j count_j dz_j^T u_j (tests/test_gpu_backward_blocks.py test_wgrad_exact_integers)"""
    lib = _lib.load()
    rows, O, I, ld = EC.WGRAD_ROWS, EC.WGRAD_O, EC.WGRAD_I, EC.WGRAD_LD
    dz, u, want = EC.wgrad_base()
    with measured(dev, "group2", "gemm_wgrad"):
        Z, U = Guarded(dev, rows * ld * 4, "wgrad dz"), Guarded(dev, rows * ld * 4, "wgrad u")
        fill_periodic(Z.words(4 * ld), as_words(dz).to(dev))
        fill_periodic(U.words(4 * ld), as_words(u).to(dev))
        need = lib.aaclip_text_backward_workspace_bytes(rows, I, 0)
        ws, dw = Guarded(dev, (need + 7) // 8 * 8, "wgrad workspace"), Guarded(dev, O * I * 4, "wgrad dw")
        rc = lib.aaclip_gemm_wgrad(Z.ptr(), ld, U.ptr(), ld, dw.ptr(), rows, O, I, ws.ptr(), need, stream(dev))
        assert rc == 0, f"gemm_wgrad: rc {rc}: {lib.aaclip_last_error()}"
        torch.cuda.synchronize(dev)
        for g in (Z, U, ws, dw):
            g.check_guards()
        got = dw.body.view(torch.float32).view(O, I).cpu()
    assert torch.equal(got.double(), want)


def fused_call(lib, dev, code, epi, A, W, bias, out, K, what, scale_cols=0, scale=1.0, **fields):
    """aaclip_gemm_fused at M = GEMM_M16, N = 256, lda = ldc = GEMM_LD on the automatic (256-row-tile) route"""
    f = _lib.GemmFusedArgs()
    for k, v in fields.items():
        setattr(f, k, v)
    rc = lib.aaclip_gemm_fused(code, epi, A.ptr(), EC.GEMM_LD, W.data_ptr(), bias.data_ptr(), out.ptr(), EC.GEMM_LD,
                               EC.GEMM_M16, EC.GEMM_N, K, 0, scale_cols, scale, ctypes.byref(f), stream(dev))
    assert rc == 0, f"{what}: rc {rc}: {lib.aaclip_last_error()}"
    torch.cuda.synchronize(dev)


def fused_buffers(dev, name, bases):
    """the guarded operands of EC.FUSED_CASES[name]: inputs periodic from `bases` (gap columns NaN bytes), outputs filled"""
    rows, ops = EC.FUSED_CASES[name]
    bufs = {}
    for o in ops:
        g = Guarded(dev, rows * o.row_bytes, f"gemm_fused {name} {o.name}")
        if o.role == "in":
            fill_periodic(g.words(o.row_bytes), as_words(bases[o.name]).to(dev))
        bufs[o.name] = g
    return bufs, {o.name: o.row_bytes for o in ops}


def test_gemm_fused_out16_and_stats(dev):
    """EPI_BIAS_RESID reading `resid` (placed at the stride of out) and writing out16 / stats_out, fp16.  (a), as
    tests/test_gpu_fused_epilogues.py test_resid_epilogue_out16_and_slice_statistics and test_gemm_epilogues: the fp32
    rows within 2e-5 + 1e-5 |ref| of fp64, out16 bit-equal to their rounding, every (sum, sumsq) slot within
    64 * 2^-24 * sum |r| (sum r^2) of the fp64 sums of the rounded values; `resid` is left as it was"""
    lib = _lib.load()
    A, W, bias, resid = EC.gemm_base()
    A16, W16 = A.half(), W.half()
    N, K = EC.GEMM_N, EC.GEMM_K
    with measured(dev, "group2", "gemm_fused out16_stats"):
        bufs, rb = fused_buffers(dev, "out16_stats", {"A": A16, "resid": resid})
        fused_call(lib, dev, F16, EC.EPI_BIAS_RESID, bufs["A"], W16.to(dev), bias.to(dev), bufs["out"], K, "out16_stats",
                   resid=bufs["resid"].ptr(), out16=bufs["out16"].ptr(), stats_out=bufs["stats_out"].ptr())
        first = {}
        for name, width in (("out", 4 * N), ("resid", 4 * N), ("out16", 2 * N), ("stats_out", N // 64 * 8), ("A", 2 * K)):
            bufs[name].check_guards()
            first[name] = check_periodic(bufs[name].words(rb[name]), width // 8, f"gemm_fused out16_stats {name}")
    out = decode(first["out"], torch.float32)
    assert torch.equal(decode(first["resid"], torch.float32), resid), "resid was modified"
    assert_close(out, EC.gemm_reference(A16.float(), W16.float(), bias, resid, EC.EPI_BIAS_RESID), *EC.GEMM_F32_OUT_TOL,
                 "out16_stats: fp32 rows")
    o16 = decode(first["out16"], torch.float16)
    assert torch.equal(o16.view(torch.int16), out.half().view(torch.int16)), "out16 is not the rounding of the fp32 rows"
    r = o16.double().view(P, N // 64, 64)
    got = decode(first["stats_out"], torch.float32).double().view(P, N // 64, 2)
    assert torch.isfinite(got).all()
    tol = 64 * 2.0 ** -24
    assert bool(((got[..., 0] - r.sum(-1)).abs() <= tol * r.abs().sum(-1)).all())
    assert bool(((got[..., 1] - (r * r).sum(-1)).abs() <= tol * (r * r).sum(-1)).all())


def test_gemm_fused_row_ab_col_s(dev):
    """EPI_BIAS_GELU with row_ab / col_s, fp16: LayerNorm folded into the product.  (a): test_folded_chain_against_fp64_
    and_the_layernorm_route on 'plain' rows -- fp64 gelu(LN(x16) W^T + bias) within test_gemm_epilogues' output rounding,
    1.5e-3 + 1.5e-3 |ref|"""
    lib = _lib.load()
    x16, ab, wf, col_s, fb, ref = EC.fused_fold_base()
    with measured(dev, "group2", "gemm_fused row_ab_col_s"):
        bufs, rb = fused_buffers(dev, "row_ab_col_s", {"A": x16, "row_ab": ab})
        cs = col_s.to(dev)
        fused_call(lib, dev, F16, EC.EPI_BIAS_GELU, bufs["A"], wf.to(dev), fb.to(dev), bufs["out"], EC.GEMM_K,
                   "row_ab_col_s", row_ab=bufs["row_ab"].ptr(), col_s=cs.data_ptr())
        for g in bufs.values():
            g.check_guards()
        first = check_periodic(bufs["out"].words(rb["out"]), 2 * EC.GEMM_N // 8, "gemm_fused row_ab_col_s out")
    assert_close(decode(first, torch.float16).float(), ref, FC.ET["fp16"], FC.ET["fp16"], "row_ab_col_s")


def test_gemm_fused_out_qk8(dev):
    """split fp16 EPI_BIAS with out_qk8 = 128 of N = 256 columns.  (a): test_out_qk8_records_byte_for_byte -- exact
    operands, every byte of the row (fp16 plane, [lo8 | hi8] records) is FC.qk8_records_cols'; the rest of the 32 KiB
    row keeps its fill"""
    lib = _lib.load()
    A, W, bias, want = EC.fused_qk8_base()
    with measured(dev, "group2", "gemm_fused out_qk8"):
        bufs, rb = fused_buffers(dev, "out_qk8", {"A": engine.split_rows(A)})
        fused_call(lib, dev, F16X2, EC.EPI_BIAS, bufs["A"], engine.split_rows(W, weight=True).to(dev), bias.to(dev),
                   bufs["out"], EC.GEMM_K, "out_qk8", scale_cols=64, scale=0.5, out_qk8=EC.FUSED_QK8)
        for g in bufs.values():
            g.check_guards()
        first = check_periodic(bufs["out"].words(rb["out"]), want.shape[1] // 8, "gemm_fused out_qk8 out")
    assert torch.equal(decode(first, torch.uint8), want)


# ----------------------------------------------------------------------------------------------------------------
# group 3: attention at its stated limit -- the extent is reached through the head count, the period runs over heads
# ----------------------------------------------------------------------------------------------------------------
def attention_planes(form, L, period):
    """-> (input planes, the values the kernel sees [period * L, 192] fp32, log2q): a plane is a uint8 tensor
    [period, L, bytes per head]; a packed row is its planes in order, each [H, bytes per head]"""
    log2q = form != "f32"
    # the record form's heads are the rows of the existing record test itself, FC.attention_inputs(3, 1, 513)
    qkv = FC.attention_inputs(period, 1, L) if form == "qk8" else EC.attention_heads(L, period, log2q)
    if form in ("f32", "f16", "bf16"):
        t = qkv if form == "f32" else qkv.to(torch.float16 if form == "f16" else torch.bfloat16)
        rows, seen, width = t.contiguous().view(torch.uint8).view(period * L, -1), t.float(), t.element_size() * 64
    elif form == "split16":
        rows, seen, width = engine.split16_rows(qkv).view(torch.uint8).view(period * L, -1), qkv.clone(), 128
        if L >= 512:                                    # long rows: v in fp16 (tests/test_gpu_split.py test_attention_split)
            seen[:, 128:] = seen[:, 128:].half().float()
    else:
        rec = FC.qk8_records(qkv, 1)                    # [hi q k v: 3 x 128 B][q: lo8 | hi8][k: lo8 | hi8]
        rows, seen, width = rec, FC.qk8_join(rec, 1).float(), 128
    planes = [rows[:, o:o + width].reshape(period, L, width).contiguous() for o in range(0, rows.shape[1], width)]
    return planes, seen, log2q


def head_phases(dev, b, H, period):
    return (b * H + torch.arange(H, device=dev)) % period


def run_attention(dev, form, B, L, H, period):
    lib = _lib.load()
    planes, seen, log2q = attention_planes(form, L, period)
    in_rb, out_rb = EC.attention_row_bytes(form, H)
    assert in_rb == sum(p.shape[2] for p in planes) * H
    what = f"attention {form} B={B} L={L} H={H}"
    qkv, ctx = Guarded(dev, B * L * in_rb, what + " qkv", fill=None), Guarded(dev, B * L * out_rb, what + " ctx")
    rows = qkv.body.view(B, L, in_rb)
    off = 0
    for p in planes:
        pd, w = p.to(dev), p.shape[2]
        for b in range(B):
            rows[b, :, off:off + H * w].view(L, H, w).copy_(pd[head_phases(dev, b, H, period)].permute(1, 0, 2))
        off += H * w
    if form == "f32":
        rc = lib.aaclip_attention(F32, qkv.ptr(), ctx.ptr(), B, L, H, 0, stream(dev))
    elif form in ("f16", "bf16"):
        rc = lib.aaclip_attention_log2q(F16 if form == "f16" else BF16, qkv.ptr(), ctx.ptr(), B, L, H, 0, stream(dev))
    else:
        rc = lib.aaclip_attention_split(qkv.ptr(), ctx.ptr(), B, L, H, 0, 1, int(form == "qk8"), 1, stream(dev))
    assert rc == 0, f"{what}: rc {rc}: {lib.aaclip_last_error()}"
    torch.cuda.synchronize(dev)
    qkv.check_guards()
    ctx.check_guards()
    del qkv
    # the context row's planes: one of 64 values per head, or split8's hi | lo8 | hi8
    widths = {"f32": [256], "f16": [128], "bf16": [128]}.get(form, [128, 64, 64])
    out, off, first = ctx.body.view(B, L, out_rb), 0, []
    for w in widths:
        plane = [out[b, :, off:off + H * w].view(L, H, w) for b in range(B)]
        head0 = plane[0][:, :period].permute(1, 0, 2).contiguous()                  # [period, L, w]: phases 0 .. period - 1
        for b in range(B):
            want = head0[head_phases(dev, b, H, period)].permute(1, 0, 2)
            if not torch.equal(plane[b], want):
                bad = int((plane[b] != want).any(dim=2).any(dim=0).nonzero()[0])
                raise AssertionError(f"{what}: head {bad} of image {b} differs from the head of its phase "
                                     f"{(b * H + bad) % period}")
        first.append(head0.cpu())
        off += H * w
    if form in ("f32", "f16", "bf16"):
        got = first[0].view({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[form]).double()
    else:
        got = (first[0].view(torch.float16).double()
               + first[1].view(torch.float8_e4m3fn).double() / float(2 ** engine.SPLIT8_ACT_LO_EXP))
    assert_close(got, EC.attention_reference(seen, L, period, log2q), *EC.ATTN_TOL[form], what)


@pytest.mark.parametrize("B", EC.ATTN_BATCHES)
@pytest.mark.parametrize("form", ["f32", "f16", "bf16", "split16"])
def test_attention_short_rows_at_the_head_limit(dev, form, B):
    """(B, 42, 65535): aaclip_attention (fp32), aaclip_attention_log2q (16-bit), aaclip_attention_split.  (a): the
    tolerances of test_attention / test_attention_log2q_variant / test_attention_split (EC.ATTN_TOL); (b): every head of
    every image equals, byte for byte, the head of its phase among the first 1021 of image 0 -- a workgroup forms one
    head of one image from that head's slice alone (csrc/attention.hip)"""
    L, H, period = EC.ATTN_SHORT
    with measured(dev, "group3", f"attention {form} B={B} L={L} H={H}"):
        run_attention(dev, form, B, L, H, period)


@pytest.mark.parametrize("B", EC.ATTN_BATCHES)
@pytest.mark.parametrize("form", ["f16", "bf16", "split16", "qk8"])
def test_attention_long_rows_within_one_head_of_the_limit(dev, form, B):
    """(B, 513, 5450): the kernels for 512 keys and more, a period of 127 heads.  B = 2 passes 2^31 bytes in the split
    and record forms, B = 3 passes 2^32 in those and 2^31 in the 16-bit ones.
    qk8: the e4m3 records of FC.qk8_records against the values the records hold, and the heads are the three images of
    test_qk8_attention_on_host_built_records' own case (3, 1, 513), a period of 3 (5450 = 2 mod 3): check (a) is then
    that test's check on that test's values.  Measured with 127 freshly drawn heads instead (same scaling, 4 169 664
    elements against that test's 98 496): 2 elements outside 4e-4 + 1e-3 |ref|, the largest error 5.5e-4 -- the tail of
    the record format's 2^-15 per operand on peaked rows, the same in every head of a phase, nothing of the extent."""
    L, H, period = EC.ATTN_LONG
    if form == "qk8":
        period = EC.ATTN_QK8_PERIOD
    with measured(dev, "group3", f"attention {form} B={B} L={L} H={H}"):
        run_attention(dev, form, B, L, H, period)


# ----------------------------------------------------------------------------------------------------------------
# group 4: the metrics chain at n = 2^29 + 3 and n = 2^31 - 1
# ----------------------------------------------------------------------------------------------------------------
MP = EC.MP
ITEMS = 1 << 26                                             # elements per slab of the flat checks


def flat_slabs(n, start=0):
    for a in range(start, n, ITEMS):
        yield a, min(n, a + ITEMS)


def periodic_flat(dev, base, n, what):
    """base (host, 1-D) -> device tensor [n] of base[i % len(base)]"""
    bd = torch.from_numpy(np.ascontiguousarray(base)).to(dev)
    out = alloc(dev, n * bd.element_size(), what).view(bd.dtype)
    for a, b in flat_slabs(n):
        torch.index_select(bd, 0, torch.arange(a, b, device=dev) % bd.numel(), out=out[a:b])
    return out


def check_flat_periodic(got, base_dev, what):
    """got[i] == base[i % len(base)], bit for bit (both viewed as int32 / uint8)"""
    for a, b in flat_slabs(got.numel()):
        want = base_dev[torch.arange(a, b, device=got.device) % base_dev.numel()]
        if not torch.equal(got[a:b], want):
            bad = a + int((got[a:b] != want).nonzero()[0])
            raise AssertionError(f"{what}: element {bad} differs from its phase {bad % base_dev.numel()}")


def guarded_ws(dev, nbytes, what):
    assert nbytes > 0 and nbytes % 8 == 0, (what, nbytes)
    return Guarded(dev, nbytes, what, fill=GUARD_BYTE)


def metrics_range(dev, lib, scores, labels, n, per_image):
    need = lib.aaclip_metrics_range_workspace_bytes(n, per_image)
    ws, rec = guarded_ws(dev, need, "metrics_range workspace"), Guarded(dev, 24, "range record")
    imax = Guarded(dev, (n // per_image * 4 + 7) // 8 * 8, "image_max") if per_image else None
    rc = lib.aaclip_metrics_range(scores.data_ptr(), labels.data_ptr(), n, per_image, imax.ptr() if imax else None,
                                  rec.ptr(), ws.ptr(), need, stream(dev))
    assert rc == 0, f"metrics_range: rc {rc}: {lib.aaclip_last_error()}"
    torch.cuda.synchronize(dev)
    for g in (ws, rec) + ((imax,) if imax else ()):
        g.check_guards()
    return rec, imax


@pytest.mark.parametrize("kind", EC.METRIC_KINDS)
@pytest.mark.parametrize("n", EC.METRIC_SIZES)
def test_metrics_range_and_normalise(dev, n, kind):
    """tests/test_gpu_metrics_device.py test_range_and_normalise_are_numpys: the record and every normalised word EQUAL
    numpy's (MD.normalise of the whole array is that of its 65537 values: every value occurs); image maxima of 35 scores
    each at n = 2^29 + 3 (EC.METRIC_PER_IMAGE; 2^31 - 1 is prime: no per_image divides it)"""
    lib = _lib.load()
    with measured(dev, "group4", f"range_normalise n={n} {kind}"):
        s, l = EC.metric_base(kind)
        scores, labels = periodic_flat(dev, s, n, "scores"), periodic_flat(dev, l, n, "labels")
        pos, _ = EC.pair_counts(n, l)
        per_image = EC.METRIC_PER_IMAGE[n]
        rec, imax = metrics_range(dev, lib, scores, labels, n, per_image)
        r = engine.metrics_range_host(rec.body.view(torch.int64))
        assert r == {"min": float(s.min()), "max": float(s.max()), "nonfinite": 0, "positives": int(pos.sum())}
        sd = torch.from_numpy(s).to(dev)
        if per_image:
            got = imax.body.view(torch.float32)[:n // per_image]
            for a, b in flat_slabs(n // per_image):
                k = torch.arange(a, b, device=dev) * per_image
                want = sd[k % MP]
                for j in range(1, per_image):
                    want = torch.maximum(want, sd[(k + j) % MP])
                assert torch.equal(got[a:b], want), "image_max"
        want_bits = torch.from_numpy(MD.normalise(s).view(np.int32)).to(dev)
        out = Guarded(dev, (4 * n + 7) // 8 * 8, "normalised scores")
        rc = lib.aaclip_metrics_normalise(scores.data_ptr(), out.ptr(), n, rec.ptr(), stream(dev))
        assert rc == 0, lib.aaclip_last_error()
        torch.cuda.synchronize(dev)
        out.check_guards()
        check_flat_periodic(out.body.view(torch.int32)[:n], want_bits, "normalise, out of place")
        del out
        rc = lib.aaclip_metrics_normalise(scores.data_ptr(), scores.data_ptr(), n, rec.ptr(), stream(dev))
        assert rc == 0, lib.aaclip_last_error()
        check_flat_periodic(scores.view(torch.int32), want_bits, "normalise, in place")
        if kind == "passthrough":
            assert np.array_equal(MD.normalise(s).view(np.uint32), s.view(np.uint32))


def signed_order(keys):
    """uint32 keys held in an int32 tensor -> int32 values in the same order, in place"""
    return keys.bitwise_xor_(-0x80000000)


def check_sorted(keys_signed, what):
    prev = None
    for a, b in flat_slabs(keys_signed.numel()):
        k = keys_signed[a:b]
        ok = bool((k[1:] >= k[:-1]).all()) and (prev is None or bool(k[0] >= prev))
        assert ok, f"{what}: the keys descend inside [{a}, {b})"
        prev = k[-1].clone()


def cumulative_counts(keys_signed, distinct_u32):
    """-> int64 [len(distinct)]: how many keys are <= each distinct key (host)"""
    d = torch.from_numpy((np.asarray(distinct_u32, np.uint32) ^ np.uint32(0x80000000)).view(np.int32)).to(keys_signed.device)
    return torch.searchsorted(keys_signed, d, right=True).cpu().numpy().astype(np.int64)


def positives_at(labels_sorted, ends):
    """-> int64: the number of non-zero labels in [0, e) for every e of the ascending host array `ends`, by cumulative
    sums of slabs with a carry"""
    out, carry = np.zeros(len(ends), np.int64), 0
    for a, b in flat_slabs(labels_sorted.numel()):
        cs = torch.cumsum((labels_sorted[a:b] != 0).to(torch.int64), 0)
        sel = np.nonzero((ends > a) & (ends <= b))[0]
        if sel.size:
            idx = torch.from_numpy(ends[sel] - a - 1).to(labels_sorted.device)
            out[sel] = carry + cs[idx].cpu().numpy()
        carry += int(cs[-1])
    out[ends == 0] = 0
    return out


@pytest.mark.parametrize("kind,packed", [("plain", 1), ("plain", 0), ("passthrough", 0)])
@pytest.mark.parametrize("n", EC.METRIC_SIZES)
def test_metrics_sort_curve_f1max_threshold(dev, n, kind, packed):
    """aaclip_metrics_sort -> aaclip_metrics_curve, aaclip_metrics_f1max -> aaclip_metrics_threshold against
    EC.curve_metrics_weighted under the rules of tests/test_gpu_metrics_device.py and tests/test_gpu_f1max_device.py:
    integers and the threshold EQUAL, AUROC within 1e-12, AP within 1e-10.  The sorted keys are checked as a whole:
    non-decreasing, the cumulative count of every distinct key (packed: of every (value, label) pair) exact, the
    positives of every run exact."""
    lib = _lib.load()
    with measured(dev, "group4", f"sort_curve_f1max n={n} {kind} packed={packed}"):
        s, l = EC.metric_base(kind)
        values = MD.normalise(s)                                   # the chain sorts normalised scores
        pos, neg = EC.pair_counts(n, l)
        want = EC.curve_metrics_weighted(values, pos, neg)
        scores, labels = periodic_flat(dev, values, n, "scores"), periodic_flat(dev, l, n, "labels")
        keys = Guarded(dev, (4 * n + 7) // 8 * 8, "keys")
        labs = None if packed else Guarded(dev, (n + 7) // 8 * 8, "labels_sorted")
        outside = Guarded(dev, 8, "out_of_range")
        need = lib.aaclip_metrics_sort_workspace_bytes(n)
        ws = guarded_ws(dev, need, "metrics_sort workspace")
        rc = lib.aaclip_metrics_sort(scores.data_ptr(), labels.data_ptr(), n, packed, keys.ptr(),
                                     labs.ptr() if labs else None, outside.ptr(), ws.ptr(), need, stream(dev))
        assert rc == 0, f"metrics_sort: rc {rc}: {lib.aaclip_last_error()}"
        torch.cuda.synchronize(dev)
        for g in (keys, outside, ws) + ((labs,) if labs else ()):
            g.check_guards()
        assert int(outside.body.view(torch.int64)[0]) == 0
        del ws
        # the records, on the keys as the sort left them
        need = lib.aaclip_metrics_curve_workspace_bytes(n)
        ws, crec = guarded_ws(dev, need, "metrics_curve workspace"), Guarded(dev, 40, "curve record")
        rc = lib.aaclip_metrics_curve(keys.ptr(), labs.ptr() if labs else None, n, packed, crec.ptr(), ws.ptr(), need,
                                      stream(dev))
        assert rc == 0, f"metrics_curve: rc {rc}: {lib.aaclip_last_error()}"
        torch.cuda.synchronize(dev)
        ws.check_guards()
        crec.check_guards()
        c = crec.body.view(torch.int64).cpu()
        assert [int(v) for v in c[:4]] == [want["num"], want["P"], want["N"], want["groups"]]
        ap = float(c[4:5].view(torch.float64)[0])
        d_auc, d_ap = abs(int(c[0]) / (2 * int(c[1]) * int(c[2])) - want["auroc"]), abs(ap - want["ap"])
        print(f"extent curve n={n} {kind} packed={packed}: auroc diff {d_auc}, ap diff {d_ap}")
        assert d_auc <= 1e-12 and d_ap <= 1e-10
        del ws
        need = lib.aaclip_metrics_f1max_workspace_bytes(n)
        ws, frec = guarded_ws(dev, need, "metrics_f1max workspace"), Guarded(dev, 8 * engine.F1MAX_RECORD_WORDS, "f1max record")
        rc = lib.aaclip_metrics_f1max(keys.ptr(), labs.ptr() if labs else None, n, packed, frec.ptr(), ws.ptr(), need,
                                      stream(dev))
        assert rc == 0, f"metrics_f1max: rc {rc}: {lib.aaclip_last_error()}"
        torch.cuda.synchronize(dev)
        ws.check_guards()
        frec.check_guards()
        f = engine.f1max_record_host(frec.body.view(torch.int64))
        assert (f["tp"], f["fp"], f["P"] - f["tp"], f["groups"], f["start"]) == \
            (want["tp"], want["fp"], want["fn"], want["groups"], want["start"]), (f, {k: want[k] for k in ("tp", "fp", "fn")})
        assert np.float32(f["threshold"]).view(np.uint32) == np.float32(want["threshold"]).view(np.uint32)
        tkey = int(MD.make_keys(np.float32([want["threshold"]]), [0], bool(packed))[0])
        assert f["key"] == (tkey >> 1 if packed else tkey)
        del ws
        # the mask and the totals at that threshold, from the scores themselves
        need = lib.aaclip_metrics_threshold_workspace_bytes(n, 0)
        ws, tot = guarded_ws(dev, need, "metrics_threshold workspace"), Guarded(dev, 32, "threshold totals")
        mask = Guarded(dev, (n + 7) // 8 * 8, "mask")
        rc = lib.aaclip_metrics_threshold(scores.data_ptr(), labels.data_ptr(), n, 0, None, frec.ptr(), mask.ptr(), None,
                                          tot.ptr(), ws.ptr(), need, stream(dev))
        assert rc == 0, f"metrics_threshold: rc {rc}: {lib.aaclip_last_error()}"
        torch.cuda.synchronize(dev)
        for g in (ws, tot, mask):
            g.check_guards()
        assert tot.body.view(torch.int64).cpu().tolist() == [want["tp"], want["fp"], want["fn"], want["N"] - want["fp"]]
        flagged = torch.from_numpy((values >= np.float32(want["threshold"])).astype(np.uint8)).to(dev)
        check_flat_periodic(mask.body[:n], flagged, "mask at the threshold")
        del ws, mask, scores
        # the sorted keys as a whole
        k = signed_order(keys.body.view(torch.int32)[:n])
        check_sorted(k, "metrics_sort")
        gp, gn, uk = want["group_pos"], want["group_neg"], want["keys"].astype(np.uint64)
        if packed:
            bits = uk ^ np.uint64(0x80000000)                          # normalised scores are >= 0: key = bits ^ 2^31
            pairs = np.stack([bits << np.uint64(1), (bits << np.uint64(1)) | np.uint64(1)], 1).reshape(-1)
            cnt = np.stack([gn, gp], 1).reshape(-1)
            live = cnt > 0
            got = cumulative_counts(k, pairs[live].astype(np.uint32))
            assert np.array_equal(got, np.cumsum(cnt[live])), "the count of a (value, label) pair is wrong"
        else:
            ends = np.cumsum(gp + gn)
            assert np.array_equal(cumulative_counts(k, uk.astype(np.uint32)), ends), "the count of a key is wrong"
            before = positives_at(labs.body[:n], ends)
            assert np.array_equal(np.diff(np.concatenate([[0], before])), gp), "the positives of a run are wrong"


@pytest.mark.parametrize("n", EC.METRIC_SIZES)
def test_metrics_sort_pairs(dev, n):
    """aaclip_metrics_sort_pairs with value i beside score i ('passthrough': negatives and zeros of both signs): keys
    non-decreasing with exact cumulative counts, every key the key of ITS value's score, and equal keys in input order"""
    lib = _lib.load()
    with measured(dev, "group4", f"sort_pairs n={n}"):
        s, l = EC.metric_base("passthrough")
        want = EC.curve_metrics_weighted(s, *EC.pair_counts(n, l))
        scores = periodic_flat(dev, s, n, "scores")
        vals = alloc(dev, 4 * n, "values").view(torch.int32)
        for a, b in flat_slabs(n):
            torch.arange(a, b, dtype=torch.int32, device=dev, out=vals[a:b])
        keys, vs = Guarded(dev, (4 * n + 7) // 8 * 8, "keys"), Guarded(dev, (4 * n + 7) // 8 * 8, "values_sorted")
        need = lib.aaclip_metrics_sort_pairs_workspace_bytes(n)
        ws = guarded_ws(dev, need, "metrics_sort_pairs workspace")
        rc = lib.aaclip_metrics_sort_pairs(scores.data_ptr(), vals.data_ptr(), n, keys.ptr(), vs.ptr(), ws.ptr(), need,
                                           stream(dev))
        assert rc == 0, f"metrics_sort_pairs: rc {rc}: {lib.aaclip_last_error()}"
        torch.cuda.synchronize(dev)
        for g in (keys, vs, ws):
            g.check_guards()
        del ws, scores, vals
        k, v = signed_order(keys.body.view(torch.int32)[:n]), vs.body.view(torch.int32)[:n]
        check_sorted(k, "metrics_sort_pairs")
        assert np.array_equal(cumulative_counts(k, want["keys"]), np.cumsum(want["group_pos"] + want["group_neg"]))
        base_keys = torch.from_numpy((MD.make_keys(s, np.zeros(MP, np.uint8), False) ^ np.uint32(0x80000000)).view(np.int32)).to(dev)
        prev_k = prev_v = None
        for a, b in flat_slabs(n):
            ks, vv = k[a:b], v[a:b]
            assert torch.equal(ks, base_keys[vv.to(torch.int64) % MP]), "a key is not the key of the value beside it"
            ok = bool(((ks[1:] != ks[:-1]) | (vv[1:] > vv[:-1])).all())
            if prev_k is not None:
                ok = ok and bool((ks[0] != prev_k) | (vv[0] > prev_v))
            assert ok, "equal keys are not in input order"
            prev_k, prev_v = ks[-1].clone(), vv[-1].clone()


# ----------------------------------------------------------------------------------------------------------------
# group 5: one step past every stated limit is refused, and nothing is written
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EC.REFUSALS, ids=[r[0] for r in EC.REFUSALS])
def test_refusal_past_the_limit(dev, case):
    """a negative code, the limit's message, and the poisoned outputs and workspace untouched (a refused call launches
    nothing; tests/test_extent_cases_cpu.py makes the same calls without a GPU)"""
    lib = _lib.load()
    rid, entry, args, literal, prefix = case
    ins = torch.zeros(8 * EC.REFUSAL_SLOT, dtype=torch.uint8, device=dev)
    outs, ws = Guarded(dev, 8 * EC.REFUSAL_SLOT, rid + " outputs"), Guarded(dev, EC.REFUSAL_SLOT, rid + " workspace")
    a, keep = EC.refusal_arguments(args, ins.data_ptr(), outs.ptr(), ws.ptr())
    rc = getattr(lib, entry)(*a)
    msg = lib.aaclip_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else msg
    torch.cuda.synchronize(dev)
    assert rc < 0 and msg == prefix + literal, (rid, rc, msg)
    outs.check_untouched()
    ws.check_untouched()
    assert not ins.any()
    del keep
