"""The fp64 references of tests/entry_edge_cases.py against the oracle (oracle/aaclip_oracle.py, itself pinned to the
reference by tests/test_oracle_golden.py), stock torch ops and the golden vectors, and the case tables against the C
ABI's stated limits.  This pins what tests/test_gpu_entry_edges.py compares the HIP kernels with."""
import math

import pytest
import torch
import torch.nn.functional as F

import entry_edge_cases as EC
from aaclip_hip import synth
from oracle import aaclip_oracle as O

T = torch.from_numpy


def maxerr(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a.double() - b.double()).abs().max())


# ---- patch embed
def test_patch_ref_equals_visual_stem_on_a_square_image():
    ps, D, g = 14, 256, 3
    img = EC.randn("cpu.pe.img", (2, 3, g * ps, g * ps))
    sd = {"visual.conv1.weight": EC.randn("cpu.pe.w", (D, 3, ps, ps), 0.05),
          "visual.class_embedding": EC.randn("cpu.pe.cls", (D,)),
          "visual.positional_embedding": EC.randn("cpu.pe.pos", (g * g + 1, D)),
          "visual.ln_pre.weight": EC.randn("cpu.pe.lnw", (D,), 0.1, 1.0), "visual.ln_pre.bias": EC.randn("cpu.pe.lnb", (D,), 0.1)}
    sd = {k: v.double() for k, v in sd.items()}
    ref = EC.patch_embed_ref(img, sd["visual.conv1.weight"], sd["visual.class_embedding"],
                             sd["visual.positional_embedding"], sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"])
    assert maxerr(ref, O.visual_stem(img.double(), sd)) <= 1e-12


@pytest.mark.parametrize("name", list(EC.PATCH_CASES))
def test_patch_ref_equals_a_convolution(name):
    """rows/columns split, the floor and the class row: against F.conv2d element by element, then the stem's tail"""
    ps, H, W, D, _modes = EC.PATCH_CASES[name]
    img, w, cls, pos, lw, lb = EC.patch_inputs(name)
    ref = EC.patch_embed_ref(img, w, cls, pos, lw, lb)
    gh, gw = H // ps, W // ps
    assert ref.shape == (EC.PATCH_B, gh * gw + 1, D)
    y = F.conv2d(img.double(), w.double(), stride=ps)
    assert y.shape[-2:] == (gh, gw)
    for b, py, px in ((0, 0, 0), (1, gh - 1, gw - 1), (1, gh - 1, 0), (0, 0, gw - 1)):
        row = O.layer_norm(y[b, :, py, px] + pos[1 + py * gw + px].double(), lw.double(), lb.double())
        assert maxerr(ref[b, 1 + py * gw + px], row) <= 1e-12
        patch = img[b, :, py * ps:(py + 1) * ps, px * ps:(px + 1) * ps].double()
        assert maxerr(y[b, :, py, px], (w.double() * patch).sum(dim=(1, 2, 3))) <= 1e-12
    assert maxerr(ref[:, 0], O.layer_norm(cls.double() + pos[0].double(), lw.double(), lb.double()).expand(EC.PATCH_B, D)) <= 1e-12
    # the surplus pixels of a size that is no multiple of ps do not reach the result
    img2 = img.clone()
    img2[:, :, gh * ps:, :] = 1e6
    img2[:, :, :, gw * ps:] = -1e6
    assert torch.equal(EC.patch_embed_ref(img2, w, cls, pos, lw, lb), ref)


# ---- heads
def test_head_ref_equals_the_oracle_chain():
    """ln_post -> projection -> normalise -> CLS dropped -> det mean, as O.adapted_visual_forward spells it"""
    x, lw, lb, w, wd = EC.head_inputs("ragged_slices")
    for act in (0, 1):
        seg, det = EC.head_ref(x, lw, lb, w, wd, act)
        t = O.layer_norm(x.double()[:, 1:], lw.double(), lb.double())
        s, d = t @ w.double().t(), t @ wd.double().t()
        if act:
            s, d = O.leaky_relu(s), O.leaky_relu(d)
        assert maxerr(seg, F.normalize(s, dim=-1)) <= 1e-14
        assert maxerr(det, F.normalize(d, dim=-1).mean(dim=1)) <= 1e-14
        assert maxerr(seg.norm(dim=-1), torch.ones(seg.shape[:2], dtype=torch.float64)) <= 1e-12


def test_head_ref_degenerate_row_is_zero():
    x, lw, lb, w, wd = EC.head_inputs("ragged_slices", degenerate=True)
    _c, b, t = EC.HEAD_DEGENERATE
    seg, det = EC.head_ref(x, lw, lb, w, wd, 0)
    assert bool((seg[b, t - 1] == 0).all())
    others = torch.cat([seg[b, : t - 1], seg[b, t:]])
    n = x.shape[1] - 1
    x2, *_ = EC.head_inputs("ragged_slices")
    assert not torch.equal(x, x2)
    zd = F.normalize(O.layer_norm(x.double(), lw.double(), lb.double())[b, 1:] @ wd.double().t(), dim=-1)
    assert maxerr(det[b], (zd.sum(0) - zd[t - 1]) / n) <= 1e-14 and others.shape[0] == n - 1


def test_row_head_ref_equals_golden_pooled(golden_tiny):
    """mode 1 (CLS row): ln_post + visual.proj on the reference's own tap = the reference's pooled output"""
    cfg = synth.tiny_cfg()
    sd = synth.synth_clip_state_dict(cfg, seed=7)
    x = T(golden_tiny["tiny.tap3"])
    ref = EC.row_head_ref(x, EC.row_pick(None, x.shape[0], 1), sd["visual.ln_post.weight"], sd["visual.ln_post.bias"],
                          sd["visual.proj"].t().contiguous(), 0)
    g = T(golden_tiny["tiny.pooled"]).double()
    assert float(((ref - g).abs() / (2e-5 + 1e-5 * g.abs())).max()) <= 1.0     # the golden is fp32


def test_row_pick_equals_argmax():
    for names in [n for sets in EC.ROW_TOKEN_SETS.values() for n in sets]:
        tok = EC.row_tokens(names)
        pick = EC.row_pick(tok, len(names), 0)
        assert torch.equal(pick, tok.long().argmax(dim=-1))
        assert pick.tolist() == [EC.ROW_TOKENS[k][1] for k in names]
    tie = EC.row_tokens(("tie",))[0]
    assert int((tie == tie.max()).sum()) > 1 and int(tie.long().argmax()) == 1
    assert EC.row_pick(None, 3, 1).tolist() == [0, 0, 0]


def test_row_head_ref_equals_oracle_text_tail():
    """mode 0: ln_final, EOT row, projection, as O.encode_text ends"""
    D, E, n = 256, 256, 3
    x, lw, lb, w = EC.row_inputs(D, E, n)
    tok = EC.row_tokens(EC.ROW_TOKEN_SETS[3][0])
    ref = EC.row_head_ref(x, EC.row_pick(tok, n, 0), lw, lb, w, 0)
    ln = O.layer_norm(x.double(), lw.double(), lb.double())
    want = ln[torch.arange(n), tok.long().argmax(dim=-1)] @ w.double().t()
    assert maxerr(ref, want) <= 1e-13
    # neighbouring rows give grossly different outputs: an off-by-one pick cannot hide inside any mode's bar
    other = ln[torch.arange(n), (tok.long().argmax(dim=-1) + 1) % EC.ROW_T] @ w.double().t()
    assert float((other - want).abs().max()) > 1.0


@pytest.mark.parametrize("shape", EC.EMBED_SHAPES)
def test_embed_ref_equals_nn_embedding(shape):
    tok, table, pos = EC.embed_inputs(*shape)
    assert 0 in tok.tolist()[0] and EC.EMBED_VOCAB - 1 in tok.flatten().tolist()
    want = torch.nn.functional.embedding(tok.long(), table) + pos[: shape[1]]
    assert torch.equal(EC.embed_ref(tok, table, pos), want.reshape(-1, shape[2]))


# ---- maps
@pytest.mark.parametrize("domain,ksize,sigma", [("Industrial", 7, 1.0), ("Medical", 9, 1.5)])
def test_map_ref_equals_oracle(golden_tiny, domain, ksize, sigma):
    pf, tf = T(golden_tiny["map.pf"]).double(), T(golden_tiny["map.tf"]).double()
    assert maxerr(EC.anomaly_map_ref([pf], tf, 70, ksize, sigma), O.similarity_map(pf, tf, 70, test=True, domain=domain)[:, 0]) <= 1e-12
    segs, anchors = EC.map_inputs("g5_s100_scaled")
    segs = [s.double() for s in segs]
    assert maxerr(EC.anomaly_map_ref(segs, anchors.double(), 100, ksize, sigma), O.anomaly_map(segs, anchors.double(), 100, domain)) <= 1e-10
    assert maxerr(EC.train_map_ref(pf, tf, 70), O.similarity_map(pf, tf, 70, test=False)) <= 1e-14
    assert maxerr(EC.train_map_ref(pf, tf, 70), T(golden_tiny["map.train"])) <= 1e-5       # the reference's own output


@pytest.mark.parametrize("name", ["g1_s13", "g2_s3", "g40_s79", "g2_s100", "g1_s1"])
def test_map_ref_without_blur_equals_interpolate(name):
    B, g, S, E, NL, ksize, _sigma, _per, _sc = EC.MAP_CASES[name]
    assert ksize == 1
    segs, anchors = EC.map_inputs(name)
    want = 0
    for seg in segs:
        s = 100.0 * torch.matmul(seg.double(), anchors.double())
        m = ((s[..., 1] + 1 - s[..., 0]) / 2).view(B, 1, g, g)
        want = want + F.interpolate(m, size=(S, S), mode="bilinear", align_corners=True)[:, 0]
    assert maxerr(EC.anomaly_map_ref(segs, anchors, S, 1, 1.0), want) <= 1e-11


def test_even_ksize_blur_is_the_oracle_taps_over_the_kernel_window():
    """ksize 4: taps exp(-x^2 / 2 s^2) at x = -1.5, -0.5, 0.5, 1.5 over columns i-2 .. i+1, reflect border"""
    m = EC.randn("cpu.blur", (1, 1, 5, 5)).double()
    k = O.gaussian_kernel1d(4, 1.0, torch.float64)
    assert maxerr(k, torch.exp(-torch.tensor([-1.5, -0.5, 0.5, 1.5], dtype=torch.float64) ** 2 / 2) / float(
        torch.exp(-torch.tensor([-1.5, -0.5, 0.5, 1.5], dtype=torch.float64) ** 2 / 2).sum())) <= 1e-15
    refl = lambda i, n: (-i if i < 0 else (2 * (n - 1) - i if i >= n else i))
    rows = torch.stack([sum(k[j] * m[0, 0][:, refl(x + j - 2, 5)] for j in range(4)) for x in range(5)], dim=1)
    want = torch.stack([sum(k[j] * rows[refl(y + j - 2, 5)] for j in range(4)) for y in range(5)], dim=0)
    assert maxerr(EC.blur(m, 4, 1.0)[0, 0], want) <= 1e-14
    odd = EC.randn("cpu.blur3", (2, 1, 5, 5)).double()
    assert torch.equal(EC.blur(odd, 9, 1.5), O.gaussian_blur2d(odd, 9, 1.5))


# ---- attention
def test_attn_ref_equals_torch_attention():
    B, L, H = 2, 9, 2
    D = 64 * H
    qkv = EC.attn_inputs(B, L, H).double()
    q, k, v = qkv.view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    for causal in (0, 1):
        want = F.scaled_dot_product_attention(q, k, v, is_causal=bool(causal), scale=1.0)
        assert maxerr(EC.attn_ref(qkv, B, L, H, causal), want.transpose(1, 2).reshape(B * L, D)) <= 1e-13


# ---- case tables
def test_case_tables_stay_inside_the_abi_limits():
    for name, (ps, H, W, D, modes) in EC.PATCH_CASES.items():
        kpad = (3 * ps * ps + 63) // 64 * 64
        assert kpad <= 640 and D in EC.ROW_WIDTHS and H >= ps and W >= ps, name
        assert "fp16x2" not in modes or kpad % 128 == 0, name
    a, b, c, d = (EC.PATCH_CASES[k] for k in "abcd")
    assert (a[1] // 14, a[2] // 14) == (2, 3) == (b[1] // 14, b[2] // 14) and b[1] % 14 and b[2] % 14
    assert 3 * 14 * 14 == 588 and 3 * 8 * 8 == 192 and 3 * 2 * 2 == 12
    rj = EC.PATCH_REJECTS
    assert (3 * rj["kpad_768"][0] ** 2 + 63) // 64 * 64 > 640 and (3 * rj["fp16x2_kpad_192"][0] ** 2) % 128 != 0
    for name, (B, L, D, E, modes, acts) in EC.HEAD_CASES.items():
        assert L > 1 and D in EC.ROW_WIDTHS and E in EC.ROW_WIDTHS and E % 128 == 0, name
    assert {a for c in EC.HEAD_CASES.values() for a in c[5]} == {0, 1}
    # the clamp case: the narrow region of ws_layout holds fewer than 32 slices of B * E floats (fp16: 2 bytes)
    B, L, D, E = EC.HEAD_CASES["clamped_slices"][:4]
    narrow_floats = (B * L * max(D, 640) * 2 + 255) // 256 * 256 // 4
    n, fit = L - 1, narrow_floats // (B * E)
    assert fit < min(32, n)
    slices = lambda first: math.ceil(n / math.ceil(n / first))            # launch_det_mean: rps, then the slice count
    assert slices(fit) != slices(min(32, n))                               # the clamp changes the launch ...
    assert B * slices(min(32, n)) * E > narrow_floats >= B * slices(fit) * E   # ... and without it the sums do not fit
    B, L, D, E = EC.HEAD_CASES["ragged_slices"][:4]
    assert math.ceil((L - 1) / 32) == 2 and math.ceil((L - 1) / 2) == 17 and (L - 1) % 2 == 1
    for D, E in EC.ROW_SHAPES:
        assert D in EC.ROW_WIDTHS and E % 128 == 0
    for n, T_, D in EC.EMBED_SHAPES:
        assert D % 4 == 0
    assert any(D > 256 and D % 256 for _n, _t, D in EC.EMBED_SHAPES)           # more than one 256-float stride, ragged
    for name, (B, g, S, E, NL, ksize, sigma, per, sc) in EC.MAP_CASES.items():
        assert 1 <= B <= 65535 and 1 <= g <= 40 and S >= 1 and E in EC.ROW_WIDTHS and 1 <= NL <= 4, name
        assert 1 <= ksize <= 15 and ksize // 2 < g and sigma > 0 and (sc is None or sc < NL), name
    cases = list(EC.MAP_CASES.values())
    assert {c[1] for c in cases} == {1, 2, 5, 40} and {c[3] for c in cases} == set(EC.ROW_WIDTHS)
    assert {c[4] for c in cases} == {1, 2, 3, 4} and {1, 3, 4, 15} <= {c[5] for c in cases}
    for g in (1, 2, 5, 40):
        assert {1, 3, g, 2 * g - 1, 13, 100} <= {c[2] for c in cases if c[1] == g}, g
    assert any(c[0] == 5 and c[1] == 1 for c in cases) and any(c[1] == 5 and c[5] == 9 for c in cases)
    assert any(c[7] for c in cases) and any(c[8] is not None for c in cases) and 15 <= len(cases) <= 25
    for name, (g, NL, ksize, sigma, short) in EC.MAP_REJECTS.items():
        assert g > 40 or NL > 4 or ksize > 15 or ksize // 2 >= g or sigma <= 0 or short, name
    assert {63, 64, 127, 128} == set(EC.ATTN_F32_L) and {511, 512, 513, 128, 256} <= set(EC.ATTN_16_L)


def test_emulation_figures_match_a_recomputation():
    got = EC.compute_emu_errors()
    assert set(got) == set(EC.EMU_ERR)
    for k, v in got.items():
        assert abs(v - EC.EMU_ERR[k]) <= 0.02 * EC.EMU_ERR[k], (k, v, EC.EMU_ERR[k])
    for k in EC.EMU_ERR:
        assert EC.bar(k) <= 4 * EC.EMU_ERR[k] and EC.bar(k) > 0
    # the emulation is an emulation of the right thing: it agrees with the fp64 reference to the format's precision
    assert all(v < 2.0 ** -18 for k, v in EC.EMU_ERR.items() if ".fp32" in k)
