"""Cases of the V-V ("surgery") residual block, shared by tests/test_vv_block_cpu.py and tests/test_gpu_vv_block.py.

A block flagged by VisionTransformer.DAPM_replace runs AACLIP_ATTN_VV_BATCH (include/aaclip.h): q = k = v, and the
softmax runs over the BATCH axis, separately per token position and head (reference model/transformer.py:102-152 as
executed).  Here: the block and input generator, the fp64 reference (oracle.aaclip_oracle.resblock(surgery=True), pinned
to the reference's own output by tests/golden/surgery.npz), the "twin" (an ordinary block that computes the same
function on permuted rows), and the shapes.

Inputs.  For independent random rows the V-V softmax is dominated by its diagonal (the self score |v|^2 / 8 is far above
the cross scores), the context is close to v itself, and an error in WHICH images are mixed stays below a 16-bit bar.
The images of a batch therefore share a base: x[b, l] = base[l] + 0.5 * noise[b, l].  The 0.5 is part of the case
definition: test_vv_block_cpu.py asserts that at least 0.25 of a softmax row's mass lies off the diagonal on average.
"""
import torch

from oracle import aaclip_oracle as O

# (B, L, D); H = D / 64, F = 4 D
BATCH_EDGES = [(B, 7, 256) for B in (1, 2, 3, 16, 17, 63, 64, 65, 129)]   # image counts at the attention kernels' switches
WIDTHS = [(5, 9, 768), (5, 9, 1024)]                                       # the other row widths
SMALL = BATCH_EDGES + WIDTHS
FORMS_SMALL = (17, 7, 256)       # the fp16x2 weight forms on the 128-tile GEMM kernels
BIG_TILE = (17, 242, 256)        # 4114 rows: at least 4096 and no multiple of 256 -- the 256-tile kernels, ragged last tile
STRIDE = (16, 1100, 1024)        # 17600 rows at full width: a second pass of the vv_* kernels' grid-stride loops

VV_MAX_WORKGROUPS, VV_THREADS = 16384, 256     # csrc/rowops.hip: vv_blocks() and the kernels' launch bounds
NOISE = 0.5
MIN_OFF_DIAGONAL = 0.25

# fp16x2 weight forms -> the aaclip_block_weights.exact16 bits engine.pack_block must set (QKV 1, OUT 2, FC 4, PROJ 8)
FORMS = {"as_drawn": 0, "in_proj_fp16": 1, "out_proj_fp16": 2, "all_fp16": 15}

# |got - ref| <= atol + rtol * |ref|, element-wise; the project's own bars per precision: fp32 of test_lnd_block_api,
# fp16x2 of test_block_long_rows_take_the_e4m3_attention_form, fp16 / bf16 test_gpu_parity.TOL with the x4 on atol
# that the tap tests use for stream values
BARS = {"fp32": (2e-4, 1e-3), "fp16x2": (4e-4, 5e-4), "fp16": (4e-3, 1e-2), "bf16": (4e-2, 5e-2)}


def name(shape):
    return "x".join(str(s) for s in shape)


def _seed(shape, salt):
    B, L, D = shape
    return ((B * 1009 + L) * 4099 + D) * 16 + salt


def make_block(D, form="as_drawn", seed=5):
    """A fresh model.transformer.ResidualAttentionBlock(D, D / 64) on the CPU: matrices N(0, 0.7 / sqrt(fan_in)),
    vectors N(0, 0.3), +1 on the LayerNorm weights.  The draw depends on (D, seed) only; `form` rounds matrices through
    fp16 afterwards.  Every call builds a new module: engine.CACHE keys on the parameter object."""
    from model.transformer import ResidualAttentionBlock
    blk = ResidualAttentionBlock(D, D // 64)
    init_block(blk, torch.Generator().manual_seed(seed * 8191 + D))
    round16 = {"as_drawn": [], "in_proj_fp16": [blk.attn.in_proj_weight], "out_proj_fp16": [blk.attn.out_proj.weight],
               "all_fp16": [blk.attn.in_proj_weight, blk.attn.out_proj.weight, blk.mlp.c_fc.weight,
                            blk.mlp.c_proj.weight]}[form]
    with torch.no_grad():
        for p in round16:
            p.copy_(p.half().float())
    return blk.eval()


def init_block(blk, g):
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (0.7 * p.shape[1] ** -0.5))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        blk.ln_1.weight.add_(1.0)
        blk.ln_2.weight.add_(1.0)


def make_input(shape, salt=0, replace_image=None):
    """[B*L, D] fp32, rows b*L + l: x[b, l] = base[l] + NOISE * noise[b, l], column 3 shifted by +2.
    replace_image = b: that image is drawn again, base included (an unrelated image in the same batch)."""
    B, L, D = shape
    g = torch.Generator().manual_seed(_seed(shape, salt))
    base = torch.randn(L, D, generator=g)
    x = base[None] + NOISE * torch.randn(B, L, D, generator=g)
    if replace_image is not None:
        g2 = torch.Generator().manual_seed(_seed(shape, salt) + 7)
        x[replace_image] = torch.randn(L, D, generator=g2) + NOISE * torch.randn(L, D, generator=g2)
    x[:, :, 3] += 2.0
    return x.reshape(B * L, D).contiguous()


def block_sd(blk, device="cpu"):
    """The block's parameters in fp64 under the reference's state-dict key names (what oracle.resblock takes)"""
    return {k: v.detach().to(device=device, dtype=torch.float64) for k, v in blk.state_dict().items()}


def reference(x, sd, B, L):
    """The V-V block in fp64: x [B*L, D] (any float dtype, any device; sd on the same device) -> [B*L, D] fp64"""
    D = x.shape[1]
    return O.resblock(x.double().view(B, L, D), sd, "", D // 64, None, surgery=True).reshape(B * L, D)


def reference_plain(x, sd, B, L):
    """The ordinary block (full attention over the L rows of each of the B batches) in fp64"""
    D = x.shape[1]
    return O.resblock(x.double().view(B, L, D), sd, "", D // 64, None).reshape(B * L, D)


def off_diagonal_mass(x, sd, B, L):
    """Mean over (position, head, query image) of the fp64 softmax mass that the reference's V-V attention puts on the
    OTHER images of the batch"""
    D = x.shape[1]
    H = D // 64
    h = O.layer_norm(x.double().view(B, L, D), sd["ln_1.weight"], sd["ln_1.bias"])
    v = (h @ sd["attn.in_proj_weight"].t() + sd["attn.in_proj_bias"])[..., 2 * D:].view(B, L, H, 64).permute(1, 2, 0, 3)
    p = torch.softmax((v @ v.transpose(-1, -2)) * 0.125, dim=-1)                    # [L, H, B, B]
    return float((1.0 - torch.diagonal(p, dim1=-2, dim2=-1)).mean())


# ---- the twin: the same block with the q and k thirds of in_proj replaced by the v third, run in the ordinary mode on
# the permuted rows l*B + b with the extents swapped (B' = L, L' = B).  Its output, permuted back, is the V-V block's
# output in exact arithmetic.
def make_twin(blk):
    """A fresh module (see make_block) with blk's parameters, q and k projections := the v projection"""
    from model.transformer import ResidualAttentionBlock
    D = blk.ln_1.weight.shape[0]
    twin = ResidualAttentionBlock(D, D // 64)
    twin.load_state_dict(blk.state_dict())
    with torch.no_grad():
        w, b = twin.attn.in_proj_weight, twin.attn.in_proj_bias
        for third in (0, 1):
            w[third * D:(third + 1) * D].copy_(w[2 * D:])
            b[third * D:(third + 1) * D].copy_(b[2 * D:])
    return twin.eval()


def to_twin_rows(x, B, L):
    """rows b*L + l -> rows l*B + b"""
    return x.view(B, L, -1).transpose(0, 1).reshape(B * L, -1).contiguous()


def from_twin_rows(y, B, L):
    """rows l*B + b -> rows b*L + l"""
    return y.view(L, B, -1).transpose(0, 1).reshape(B * L, -1).contiguous()


def twin_reference(x, twin_sd, B, L):
    return from_twin_rows(reference_plain(to_twin_rows(x, B, L), twin_sd, L, B), B, L)


def grid_stride_passes(n_items):
    """passes of a vv_* kernel's grid-stride loop over n_items work items (4 elements each)"""
    per_pass = VV_MAX_WORKGROUPS * VV_THREADS
    return -(-n_items // per_pass)


def bar_excess(got, ref, bar):
    """(max |got - ref|, max |got - ref| / (atol + rtol |ref|)) in fp64 on ref's device"""
    atol, rtol = bar
    got = got.detach().to(device=ref.device, dtype=torch.float64)
    err = (got - ref).abs()
    return float(err.max()), float((err / (atol + rtol * ref.abs())).max())
