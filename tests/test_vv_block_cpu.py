"""What the GPU tests of the V-V block (tests/test_gpu_vv_block.py) rest on, checked without a GPU: the cases'
reference is the restatement pinned to the reference's golden vectors, the twin computes the same function, the inputs
put real softmax mass off the diagonal, the shapes reach the code paths they are named after, and the outputs depend on
the batch composition far above the bars."""
import os

import numpy as np
import pytest
import torch

import vv_block_cases as VC
from aaclip_hip import synth
from oracle import aaclip_oracle as O


@pytest.fixture(scope="module")
def blocks():
    """one block and its fp64 state dict per width"""
    out = {}
    for D in (256, 768, 1024):
        blk = VC.make_block(D)
        out[D] = (blk, VC.block_sd(blk))
    return out


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_reference_is_the_restatement_pinned_to_the_golden():
    """surgery.npz, B = 3, DPAM_layer = 2: the last block of the reduced model runs V-V.  The cases' reference applied to
    the stream before it (tap 2) with that block's weights gives the stream after it (tap 3): the oracle's own tap in
    fp64, and the reference's recorded tap within the bound of tests/test_oracle_golden.py."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "surgery.npz"))
    cfg = synth.tiny_cfg()
    sd = synth.synth_clip_state_dict(cfg, seed=7)
    img = synth.synth_images(3, cfg.image_size, seed=7)
    _, taps = O.encode_image(img, sd, cfg.vision.heads, [2, 3], dtype=torch.float64, dpam_layer=2)
    B, L, D = taps[0].shape
    assert D // 64 == cfg.vision.heads
    p = f"visual.transformer.resblocks.{cfg.vision.layers - 1}."
    bsd = {k[len(p):]: v.double() for k, v in sd.items() if k.startswith(p)}
    got = VC.reference(taps[0].reshape(B * L, D), bsd, B, L).view(B, L, D)
    assert torch.equal(got, taps[1])
    assert torch.allclose(got.float(), torch.from_numpy(g["b3.dpam2.tap3"]), atol=2e-5, rtol=1e-5)
    # and it is not the ordinary block
    assert not torch.allclose(VC.reference_plain(taps[0].reshape(B * L, D), bsd, B, L).view(B, L, D), taps[1], atol=1e-3)


@pytest.mark.parametrize("shape", VC.SMALL + [VC.FORMS_SMALL, (16, 40, 1024)], ids=VC.name)
def test_twin_equals_reference_in_fp64(blocks, shape):
    B, L, D = shape
    blk, sd = blocks[D]
    x = VC.make_input(shape)
    ref = VC.reference(x, sd, B, L)
    twin = VC.twin_reference(x, VC.block_sd(VC.make_twin(blk)), B, L)
    assert rel(twin, ref) <= 1e-12, rel(twin, ref)
    # the row maps are inverse permutations and really move rows
    r = torch.arange(B * L, dtype=torch.float32)[:, None]
    assert torch.equal(VC.from_twin_rows(VC.to_twin_rows(r, B, L), B, L), r)
    assert float(VC.to_twin_rows(r, B, L)[min(1, B * L - 1), 0]) == (L if B > 1 else 1) % (B * L)


@pytest.mark.parametrize("shape", [s for s in VC.SMALL + [VC.FORMS_SMALL, VC.BIG_TILE] if s[0] >= 2], ids=VC.name)
def test_softmax_mass_off_the_diagonal(blocks, shape):
    """A condition on the cases, not a measurement of the kernels."""
    B, L, D = shape
    m = VC.off_diagonal_mass(VC.make_input(shape), blocks[D][1], B, L)
    print(f"{VC.name(shape)}: mean off-diagonal mass {m:.3f}")
    assert m >= VC.MIN_OFF_DIAGONAL, m


def test_stride_rows_keep_the_condition(blocks):
    """STRIDE itself is too large for a CPU test: the same generator on its last 60 token positions' worth of rows"""
    B, L, D = VC.STRIDE
    shape = (B, 60, D)
    assert VC.off_diagonal_mass(VC.make_input(shape), blocks[D][1], B, 60) >= VC.MIN_OFF_DIAGONAL


def test_noise_level_is_part_of_the_case(blocks, monkeypatch):
    shape = (2, 7, 256)
    monkeypatch.setattr(VC, "NOISE", 1.0)
    assert VC.off_diagonal_mass(VC.make_input(shape), blocks[256][1], 2, 7) < VC.MIN_OFF_DIAGONAL


def test_shapes_reach_the_paths_they_are_named_after():
    B, L, D = VC.BIG_TILE
    assert B * L >= 4096 and (B * L) % 256 != 0                 # the 256-tile GEMM kernels, ragged last tile
    B, L, D = VC.STRIDE
    assert B * L * D // 4 > VC.VV_MAX_WORKGROUPS * VC.VV_THREADS                       # vv_spread*: a second pass ...
    assert VC.grid_stride_passes(B * L * D // 4) == 2
    first = VC.VV_MAX_WORKGROUPS * VC.VV_THREADS // (D // 4)                           # rows of the first pass
    assert B * L - first > 1000                                                        # ... over more than 1000 rows,
    assert (B - 1) * L + 1000 >= first and L > 1000              # the last image's rows l >= 1000 among them
    assert VC.grid_stride_passes(B * L * D // 2) == 3                                  # the split regroup: a third
    assert B * L >= 4096 and D == 1024
    assert sorted(b for b, _, _ in VC.BATCH_EDGES) == [1, 2, 3, 16, 17, 63, 64, 65, 129]
    assert sorted(d for _, _, d in VC.WIDTHS) == [768, 1024]
    B, L, D = VC.FORMS_SMALL
    assert B * L < 4096 and D % 256 == 0                        # 128-tile kernels; the 3-plane weight form needs K % 256 == 0


@pytest.mark.parametrize("shape", [(2, 7, 256), (3, 7, 256), (17, 7, 256), (5, 9, 768)], ids=VC.name)
def test_output_depends_on_the_batch_composition(blocks, shape):
    """Replacing image 1 moves the reference's output rows of image 0 by more than 100 fp32 bars: a test on these inputs
    notices attention over the wrong axis, or over the wrong images."""
    B, L, D = shape
    sd = blocks[D][1]
    x, x2 = VC.make_input(shape), VC.make_input(shape, replace_image=1)
    assert torch.equal(x[:L], x2[:L]) and not torch.equal(x[L:2 * L], x2[L:2 * L])
    a, b = VC.reference(x, sd, B, L)[:L], VC.reference(x2, sd, B, L)[:L]
    atol, rtol = VC.BARS["fp32"]
    moved = float(((a - b).abs() / (atol + rtol * a.abs())).max())
    print(f"{VC.name(shape)}: image 0 moves by {moved:.0f} fp32 bars")
    assert moved > 100
    # the ordinary block does not see the other images at all
    assert torch.equal(VC.reference_plain(x, sd, B, L)[:L], VC.reference_plain(x2, sd, B, L)[:L])


def test_weight_forms_round_what_they_say():
    for form, bits in VC.FORMS.items():
        blk = VC.make_block(256, form)
        exact = lambda p: bool((p.half().float() == p).all())
        got = (exact(blk.attn.in_proj_weight) * 1 + exact(blk.attn.out_proj.weight) * 2 + exact(blk.mlp.c_fc.weight) * 4
               + exact(blk.mlp.c_proj.weight) * 8)
        assert got == bits, (form, got)
