"""GPU tests of the V-V ("surgery") block path of aaclip_blocks (csrc/capi.hip block_impl, AACLIP_ATTN_VV_BATCH; the vv_*
kernels of csrc/rowops.hip) in every precision: against the fp64 restatement of the reference on the same fp32 inputs and
weights, and against its twin -- an ordinary block that computes the same function on permuted rows.  Cases, reference,
twin and bars: tests/vv_block_cases.py; what they rest on is checked without a GPU in tests/test_vv_block_cpu.py.

Every comparison is element-wise, |got - ref| <= atol + rtol * |ref|, at the project's own bar of the precision
(vv_block_cases.BARS).  The worst error of every case is recorded under vv_block.* (conftest.PARITY_ERRORS; the committed
copy is profiles/vv_block_parity_errors.json)."""
import functools
from types import SimpleNamespace

import pytest
import torch

import vv_block_cases as VC
from aaclip_hip import _lib, engine
from aaclip_hip._lib import BF16, F16, F16X2, F32
from conftest import PARITY_ERRORS

pytestmark = pytest.mark.gpu

CODES = {"fp32": F32, "fp16x2": F16X2, "fp16": F16, "bf16": BF16}
PRECISIONS = list(CODES)
LARGE = (VC.BIG_TILE, VC.STRIDE)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(shape, form="as_drawn"):
    """Block (on the device, flagged V-V), input and fp64 reference of a case, computed once and shared by the tests.
    The reference runs on the CPU; for the two large shapes the same function runs in fp64 on the device
    (test_reference_on_the_device_equals_the_cpu_one ties the two)."""
    dev = torch.device("cuda:0")
    B, L, D = shape
    blk = VC.make_block(D, form)
    x = VC.make_input(shape)
    if shape in LARGE:
        blk = blk.to(dev)
        x = x.to(dev)
        ref = VC.reference(x, VC.block_sd(blk, dev), B, L)
        twin = None
    else:
        ref = VC.reference(x, VC.block_sd(blk), B, L).to(dev)
        twin = VC.make_twin(blk).to(dev)
        blk = blk.to(dev)
        x = x.to(dev)
    blk.surgery = True
    return SimpleNamespace(shape=shape, B=B, L=L, D=D, H=D // 64, blk=blk, twin=twin, x=x, ref=ref)


def run_vv(c, prec, x=None):
    """one V-V block: reads x, writes a NaN-filled output tensor"""
    x = c.x if x is None else x
    keep = x.clone()
    out = torch.full_like(x, float("nan"))
    with torch.no_grad():
        engine.run_blocks(x, [c.blk], c.B, c.L, c.H, CODES[prec], x_out=out)
    assert torch.equal(x, keep), "the V-V block wrote the buffer it reads"
    return out


def run_twin(c, prec):
    xt = VC.to_twin_rows(c.x, c.B, c.L)
    out = torch.full_like(xt, float("nan"))
    with torch.no_grad():
        engine.run_blocks(xt, [c.twin], c.L, c.B, c.H, CODES[prec], causal=False, x_out=out)
    return VC.from_twin_rows(out, c.B, c.L)


def over_bar(a, b, ref, bar):
    """max |a - b| / (atol + rtol |ref|)"""
    return float(((a.double() - b.double()).abs() / (bar[0] + bar[1] * ref.abs())).max())


def check(key, got, ref, prec, what=None):
    """finite, element-wise inside the bar of `prec` around ref; recorded under vv_block.<key>"""
    what = what or key
    bar = VC.BARS[prec]
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    worst, over = VC.bar_excess(got, ref, bar)
    PARITY_ERRORS[f"vv_block.{key}"] = {"max_abs_err": worst, "max_err_over_bar": over, "atol": bar[0], "rtol": bar[1]}
    print(f"vv_block.{key}: max |err| {worst:.3e} = {over:.3f} x ({bar[0]} + {bar[1]} |ref|)")
    assert over <= 1.0, f"{what}: max err {worst:.3e} is {over:.2f} x the bar {bar[0]}+{bar[1]}*|ref|"
    return over


def test_reference_on_the_device_equals_the_cpu_one(dev):
    shape = VC.FORMS_SMALL
    B, L, D = shape
    blk, x = VC.make_block(D), VC.make_input(shape)
    cpu = VC.reference(x, VC.block_sd(blk), B, L)
    gpu = VC.reference(x.to(dev), VC.block_sd(blk, dev), B, L).cpu()
    assert float((cpu - gpu).abs().max() / cpu.abs().max()) <= 1e-12
    tw = VC.block_sd(VC.make_twin(blk))
    gpu = VC.twin_reference(x.to(dev), {k: v.to(dev) for k, v in tw.items()}, B, L).cpu()
    assert float((cpu - gpu).abs().max() / cpu.abs().max()) <= 1e-12


# ---- 1. every precision at the attention kernels' image counts and at the other widths
@pytest.mark.parametrize("shape", VC.SMALL, ids=VC.name)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_vv_block_vs_fp64(dev, prec, shape):
    c = case(shape)
    check(f"fp64.{prec}.{VC.name(shape)}", run_vv(c, prec), c.ref, prec)


# ---- 2. the twin: both inside the bar of fp64, and within one bar of each other
# of each other.  Whether the bits agree is recorded (vv_block.twin.*.bit_identical); in fp32 (same k order, same
# attention kernel) they do and it is asserted
@pytest.mark.parametrize("shape", VC.SMALL, ids=VC.name)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_vv_block_vs_twin(dev, prec, shape):
    c = case(shape)
    vv, twin = run_vv(c, prec), run_twin(c, prec)
    key = f"twin.{prec}.{VC.name(shape)}"
    check(key + ".vv", vv, c.ref, prec)
    check(key + ".twin", twin, c.ref, prec)
    d = over_bar(vv, twin, c.ref, VC.BARS[prec])
    PARITY_ERRORS[f"vv_block.{key}"] = {"vv_minus_twin_over_bar": d, "bit_identical": bool(torch.equal(vv, twin))}
    assert d <= 1.0, f"{key}: V-V and twin differ by {d:.2f} bars"
    if prec == "fp32":      # measured: the same bits in every case (the value product's tiles do not depend on N here)
        assert torch.equal(vv, twin), f"{key}: V-V and twin differ in fp32"


# ---- 3. fp16x2 weight forms: the value-only product reads its weight at an offset of 4 or 3 bytes per element inside
# the packed in_proj weight, and the hi8 switches of layernorm (in_proj exact) and attention (out_proj exact) disagree
# in the two mixed forms
@pytest.mark.parametrize("shape", [VC.FORMS_SMALL, VC.BIG_TILE], ids=VC.name)     # 128-tile / 256-tile GEMM kernels
@pytest.mark.parametrize("form", list(VC.FORMS))
def test_vv_block_fp16x2_weight_forms(dev, form, shape):
    c = case(shape, form)
    w, refs = engine.pack_block(c.blk, F16X2, None)
    assert w.exact16 == VC.FORMS[form], (form, w.exact16)
    planes = 3 if VC.FORMS[form] & _lib.EXACT16_QKV else 4
    assert engine.CACHE.get(c.blk.attn.in_proj_weight, F16X2, "plain+exact").shape == (3 * c.D, planes * c.D)
    del refs
    check(f"forms.{form}.{VC.name(shape)}", run_vv(c, "fp16x2"), c.ref, "fp16x2")


# ---- 4. the 256-tile GEMM kernels inside a V-V block (ragged last tile; a weight pointer inside an allocation), and a
# second pass of the vv_* kernels' grid-stride loops at full width
@pytest.mark.parametrize("shape", LARGE, ids=VC.name)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_vv_block_large_vs_fp64(dev, prec, shape):
    c = case(shape)
    got = run_vv(c, prec)
    if shape == VC.STRIDE:
        # rows of the last image at l >= 1000: written by the second grid-stride pass of vv_spread* (source rows past
        # 16384) -- on their own, so that a failure names them
        lo = (c.B - 1) * c.L + 1000
        check(f"fp64.{prec}.{VC.name(shape)}.second_pass_rows", got[lo:], c.ref[lo:], prec,
              f"{prec} {VC.name(shape)}: rows l >= 1000 of the last image (second grid-stride pass)")
    check(f"fp64.{prec}.{VC.name(shape)}", got, c.ref, prec)


# ---- 5. runs and taps
@functools.lru_cache(maxsize=None)
def tower():
    """Three blocks [ordinary, V-V, V-V] at D = 256 with BIG_TILE's rows, and the fp64 chain of their outputs"""
    from model.transformer import Transformer
    B, L, D = VC.BIG_TILE
    tr = Transformer(D, 3, D // 64)
    g = torch.Generator().manual_seed(77)
    for blk in tr.resblocks:
        VC.init_block(blk, g)
    x = VC.make_input(VC.BIG_TILE, salt=1)
    sds = [VC.block_sd(b) for b in tr.resblocks]
    r1 = VC.reference_plain(x, sds[0], B, L)
    r2 = VC.reference(r1, sds[1], B, L)
    r3 = VC.reference(r2, sds[2], B, L)
    tr.resblocks[1].surgery = True
    tr.resblocks[2].surgery = True
    dev = torch.device("cuda:0")
    return tr.to(dev).eval(), x.to(dev), [r.to(dev) for r in (r1, r2, r3)]


@pytest.mark.parametrize("prec", ["fp16", "fp16x2"])
def test_vv_blocks_in_a_tower_with_taps(dev, prec):
    """Transformer.run over [ordinary, V-V, V-V] with a tap after every block, at 4114 rows (the 256-tile kernels: the
    row count from which the fp16 path folds LayerNorm into its products and hands 16-bit rows from block to block, the
    first V-V block of the run included).  Every tap inside the bar of the fp64 chain; the
    V-V run reads the tapped buffer and writes others; nothing writes a tapped buffer again."""
    tr, x0, refs = tower()
    B, L, D = VC.BIG_TILE
    code = CODES[prec]
    x = x0.clone()
    with torch.no_grad():
        last, taps = tr.run(x, B, L, code, False, out_layers=[1, 2, 3])
    for i, (t, r) in enumerate(zip(taps, refs)):
        check(f"tower.{prec}.tap{i + 1}", t, r, prec)
    # the ordinary block runs in place on x; each V-V block reads the buffer before it and writes a fresh one
    ptrs = [t.data_ptr() for t in taps]
    assert ptrs[0] == x.data_ptr() and len(set(ptrs)) == 3 and last.data_ptr() == ptrs[2]
    # tap 1 is what the ordinary block alone leaves (bit for bit): the V-V run behind it did not write its input
    blocks = list(tr.resblocks)
    xa = x0.clone()
    with torch.no_grad():
        engine.run_blocks(xa, blocks[:1], B, L, tr.heads, code)
    assert torch.equal(taps[0], xa)
    # block by block: a tapped buffer is bit-equal before and after the run that reads it
    o1, o2 = torch.full_like(xa, float("nan")), torch.full_like(xa, float("nan"))
    with torch.no_grad():
        engine.run_blocks(xa, blocks[1:2], B, L, tr.heads, code, x_out=o1)
        s1 = o1.clone()
        engine.run_blocks(o1, blocks[2:3], B, L, tr.heads, code, x_out=o2)
    assert torch.equal(xa, taps[0]) and torch.equal(o1, s1)
    # two V-V blocks in one call (the tower's) against two single-block calls
    bar = VC.BARS[prec]
    d2, d3 = over_bar(taps[1], o1, refs[1], bar), over_bar(taps[2], o2, refs[2], bar)
    PARITY_ERRORS[f"vv_block.tower.{prec}.one_call_vs_two"] = {
        "tap2_over_bar": d2, "tap3_over_bar": d3,
        "bit_identical": bool(torch.equal(taps[1], o1) and torch.equal(taps[2], o2))}
    assert d2 <= 1.0 and d3 <= 1.0, (d2, d3)
    check(f"tower.{prec}.single_calls.tap3", o2, refs[2], prec)
    # the next run of the tower (other images, same workspace) leaves the first run's taps alone
    snap = [t.clone() for t in taps]
    x2 = VC.make_input(VC.BIG_TILE, salt=2).to(dev)
    with torch.no_grad():
        _, taps2 = tr.run(x2, B, L, code, False, out_layers=[1, 2, 3])
    assert all(torch.equal(a, b) for a, b in zip(taps, snap))
    assert not torch.equal(taps2[2], taps[2])


# ---- 6. permuting the images of a batch permutes the output images
@pytest.mark.parametrize("shape", [VC.FORMS_SMALL, (5, 9, 768)], ids=VC.name)
@pytest.mark.parametrize("prec", ["fp32", "fp16x2"])
def test_vv_block_batch_equivariance(dev, prec, shape):
    c = case(shape)
    B, L, D = shape
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to(dev)
    assert not torch.equal(perm, torch.arange(B, device=dev))
    pick = lambda t: t.view(B, L, D)[perm].reshape(B * L, D).contiguous()
    got, got_p = run_vv(c, prec), run_vv(c, prec, pick(c.x))
    check(f"equivariance.{prec}.{VC.name(shape)}.permuted_vs_fp64", got_p, pick(c.ref), prec)
    d = over_bar(got_p, pick(got), pick(c.ref), VC.BARS[prec])
    PARITY_ERRORS[f"vv_block.equivariance.{prec}.{VC.name(shape)}"] = {
        "over_bar": d, "bit_identical": bool(torch.equal(got_p, pick(got)))}
    assert d <= 1.0, d


# ---- 7. determinism
def test_vv_block_stride_is_deterministic(dev):
    c = case(VC.STRIDE)
    assert torch.equal(run_vv(c, "fp16x2"), run_vv(c, "fp16x2"))


# ---- 8. refusals (F < 4*D and attn_mode = 3: tests/test_gpu_parity.py test_surgery_needs_wide_workspace)
def test_run_blocks_refuses_mixed_modes_and_a_mask(dev):
    c = case(VC.FORMS_SMALL)
    plain = VC.make_block(c.D).to(dev)
    x = c.x.clone()
    with pytest.raises(ValueError, match="attention mode changes"):
        engine.run_blocks(x, [plain, c.blk], c.B, c.L, c.H, F16X2)
    assert torch.equal(x, c.x)
    with pytest.raises(ValueError, match="attention mode changes"):
        engine.run_blocks(x, [c.blk, plain], c.B, c.L, c.H, F32)
    assert torch.equal(x, c.x)
    with pytest.raises(ValueError, match="no mask"):
        engine.run_blocks(x, [c.blk], c.B, c.L, c.H, F16, causal=True)
    assert torch.equal(x, c.x)
