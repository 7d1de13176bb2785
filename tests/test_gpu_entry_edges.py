"""C ABI entry points on their own, at edge shapes, against the fp64 references of tests/entry_edge_cases.py (pinned on
the CPU by tests/test_entry_edges_cpu.py): aaclip_patch_embed, aaclip_tap_head / _keep_rows / aaclip_det_head,
aaclip_row_head, aaclip_text_embed, aaclip_anomaly_map / aaclip_similarity_map_train, and aaclip_attention at the
lengths where launch_attention changes kernels.  Tiny shapes only; every output buffer starts as NaN (0xAA bytes for
split rows), so an element nobody wrote fails.

Bars: patch embed, heads and row head -- 4 x the CPU emulation's error of the mode's arithmetic, capped at the TOL of
tests/test_gpu_parity.py (entry_edge_cases.py, module docstring and EMU_ERR); maps and attention -- the tolerances of
the existing map and attention tests; bit-identity, exact zero and torch.equal are exact.  The measured maxima go to
PARITY_ERRORS under `edge.` keys (committed: profiles/entry_edges_parity_errors.json)."""
import ctypes as C

import pytest
import torch

import entry_edge_cases as EC
from aaclip_hip import _lib, engine
from conftest import PARITY_ERRORS
from oracle import aaclip_oracle as O

pytestmark = pytest.mark.gpu
TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
ALL_MODES = ("fp32", "fp16", "bf16", "fp16x2")
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def assert_close(a, b, atol, rtol, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite output"
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} outside {atol}+{rtol}*|ref|; "
                           f"max err {err.max().item():.3e} at ref {b.flatten()[err.argmax()].item():.3e}")


def maxerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max())


def assert_bar(got, ref, key, what):
    """max |got - ref| <= 4 x EMU_ERR[key], and inside TOL elementwise; the figure is printed and recorded first"""
    mode = key.rsplit(".", 2)[-2] if key.startswith("head.") else key.rsplit(".", 1)[-1]
    err = maxerr(got, ref)
    print(f"{what} [{key}]: max |err| {err:.3e}, bar {EC.bar(key):.3e} (emulation {EC.EMU_ERR[key]:.3e})")
    PARITY_ERRORS[f"edge.{what}"] = {"max_abs_err": err, "bar": EC.bar(key)}
    assert_close(got, ref, *EC.TOL[mode], what)
    assert err <= EC.bar(key), (what, err, EC.bar(key))


def nan_f32(dev, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def workspace(dev, nbytes, fill=0xFF):
    return torch.full((int(nbytes) + 256,), fill, dtype=torch.uint8, device=dev)


def weight(w, mode, dev, kind="plain"):
    """the matrix weight as the engine hands it to the library in this mode"""
    return engine.CACHE.get(w.to(dev), EC.MODES[mode], kind)


# ----------------------------------------------------------------------------------------------------------------
# 1. patch embed
# ----------------------------------------------------------------------------------------------------------------
def run_patch_embed(lib, dev, args, mode, ws_fill=0xFF, surplus_nan=False):
    img, w, cls, pos, lw, lb = args
    B, _, H, W = img.shape
    D, ps = w.shape[0], w.shape[-1]
    L = (H // ps) * (W // ps) + 1
    code = EC.MODES[mode]
    imgd = img.clone()
    if surplus_nan:                      # pixels behind the last whole patch: reading one shows
        imgd[:, :, (H // ps) * ps:, :] = NAN
        imgd[:, :, :, (W // ps) * ps:] = NAN
    x = nan_f32(dev, B * L, D)
    ws = workspace(dev, lib.aaclip_workspace_bytes(code, B * L, D, 4 * D, 0), ws_fill)
    keep = [t.to(dev).contiguous() for t in (imgd, cls, pos, lw, lb)] + [weight(w, mode, dev, "conv")]
    rc = lib.aaclip_patch_embed(keep[0].data_ptr(), keep[5].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                                keep[3].data_ptr(), keep[4].data_ptr(), x.data_ptr(), B, H, W, ps, D, code,
                                ws.data_ptr(), ws.numel(), stream(dev))
    torch.cuda.synchronize(dev)
    return rc, x.view(B, L, D), ws


@pytest.mark.parametrize("name,mode", [(n, m) for n, c in EC.PATCH_CASES.items() for m in c[4]])
def test_patch_embed_vs_convolution(dev, name, mode):
    """im2col + GEMM + class row + positional embedding + ln_pre against F.conv2d in fp64, on non-square grids, sizes
    that are no multiple of ps (the surplus pixels are NaN: none may be read) and every Kpad.
    Zero padding of K..Kpad: engine.WeightCache('conv') zero-pads the weight, as include/aaclip.h asks of the caller,
    so the weight's padded columns are the caller's duty; the library's own half is shown instead: the workspace is
    poisoned (0xFF bytes: NaN in every format) in one run and zeroed in the other, and the results must be the same
    bits and finite -- im2col writes its zero columns itself."""
    lib = _lib.load()
    args = EC.patch_inputs(name)
    rc, x, _ws = run_patch_embed(lib, dev, args, mode, ws_fill=0xFF, surplus_nan=True)
    assert rc == 0, lib.aaclip_last_error()
    assert_bar(x, EC.patch_embed_ref(*args, mode), f"patch.{name}.{mode}", f"patch_embed.{name}.{mode}")
    rc, x0, _ws = run_patch_embed(lib, dev, args, mode, ws_fill=0x00, surplus_nan=True)
    assert rc == 0 and torch.equal(x, x0)


@pytest.mark.parametrize("name", list(EC.PATCH_REJECTS))
def test_patch_embed_rejects_before_launching(dev, name):
    """rc < 0, and nothing was enqueued: the output is still NaN and the poisoned workspace, where im2col would have
    written the patch rows, still holds its 0xFF bytes"""
    lib = _lib.load()
    mode = EC.PATCH_REJECTS[name][4]
    rc, x, ws = run_patch_embed(lib, dev, EC.patch_inputs(name), mode)
    assert rc < 0 and lib.aaclip_last_error()
    assert bool(torch.isnan(x).all())
    assert bool((ws == 0xFF).all())


# ----------------------------------------------------------------------------------------------------------------
# 2. heads
# ----------------------------------------------------------------------------------------------------------------
def run_heads(lib, dev, x, lw, lb, w, wd, act, mode, what):
    """what: 'tap' -> (seg, det); 'keep' -> (seg, det, rows); 'det' -> det; 'seg' -> seg (det_w = NULL)"""
    B, L, D = x.shape
    E = w.shape[0]
    code = EC.MODES[mode]
    keep = [t.to(dev).contiguous() for t in (x, lw, lb)] + [weight(w, mode, dev), weight(wd, mode, dev)]
    xd, lwd, lbd, wq, wdq = keep
    seg, det = nan_f32(dev, B, L - 1, E), nan_f32(dev, B, E)
    ws = workspace(dev, lib.aaclip_workspace_bytes(code, B * L, D, 0, E))
    tail = (B, L, D, E, code, ws.data_ptr(), ws.numel(), stream(dev))
    rows = None
    if what == "det":
        rc = lib.aaclip_det_head(xd.data_ptr(), lwd.data_ptr(), lbd.data_ptr(), wdq.data_ptr(), act, det.data_ptr(), *tail)
    elif what == "keep":
        rows = (torch.full((B * L, 4 * D), 0xAA, dtype=torch.uint8, device=dev) if mode == "fp16x2"
                else torch.full((B * L, D), NAN, dtype=TDT[mode], device=dev))
        rc = lib.aaclip_tap_head_keep_rows(xd.data_ptr(), lwd.data_ptr(), lbd.data_ptr(), wq.data_ptr(), act,
                                           seg.data_ptr(), wdq.data_ptr(), det.data_ptr(), rows.data_ptr(), *tail)
    else:
        rc = lib.aaclip_tap_head(xd.data_ptr(), lwd.data_ptr(), lbd.data_ptr(), wq.data_ptr(), act, seg.data_ptr(),
                                 wdq.data_ptr() if what == "tap" else None, det.data_ptr() if what == "tap" else None,
                                 *tail)
    _lib.check(rc, what)
    torch.cuda.synchronize(dev)
    return {"tap": (seg, det), "keep": (seg, det, rows), "det": det, "seg": seg}[what]


@pytest.mark.parametrize("name,mode", [(n, m) for n, c in EC.HEAD_CASES.items() for m in c[4]])
def test_heads_vs_reference(dev, name, mode):
    """tap_head against the fp64 chain (CLS row dropped: the CLS rows of x are far from the patch rows, so row 0 of the
    output must be patch 1), unit rows, det_head == tap_head's det and keep_rows == tap_head bit for bit, the kept rows
    == aaclip_layernorm bit for bit.  Cases: one patch; 33 patches (rps 2, 17 slices, a last slice of one row); the
    clamp branch of launch_det_mean (entry_edge_cases.HEAD_CASES); B = 5."""
    lib = _lib.load()
    B, L, D, E, _modes, acts = EC.HEAD_CASES[name]
    args = EC.head_inputs(name)
    x, lw, lb = args[:3]
    for act in acts:
        seg, det = run_heads(lib, dev, *args, act, mode, "tap")
        rseg, rdet = EC.head_ref(*args, act, mode)
        assert_bar(seg, rseg, f"head.{name}.{mode}.seg", f"tap_head.{name}.{mode}.act{act}.seg")
        assert_bar(det, rdet, f"head.{name}.{mode}.det", f"tap_head.{name}.{mode}.act{act}.det")
        assert float((seg.double().norm(dim=-1) - 1).abs().max()) <= 1e-6
        assert torch.equal(run_heads(lib, dev, *args, act, mode, "det"), det)
        assert torch.equal(run_heads(lib, dev, *args, act, mode, "seg"), seg)
        kseg, kdet, rows = run_heads(lib, dev, *args, act, mode, "keep")
        assert torch.equal(kseg, seg) and torch.equal(kdet, det)
        ln = engine.layernorm(x.view(B * L, D).to(dev), lw.to(dev), lb.to(dev), out_code=EC.MODES[mode])
        assert torch.equal(rows.view(torch.uint8).reshape(B * L, -1), ln.view(torch.uint8).reshape(B * L, -1))
        ref_ln = O.layer_norm(x.double(), lw.double(), lb.double()).view(B * L, D)
        if mode == "fp16x2":
            joined = engine.join_split8(rows, D)
            hi = rows[:, : 2 * D].cpu().contiguous().view(torch.float16).double()
            assert_close(joined, ref_ln, 6e-6, 2.0 ** -14, "kept split8 rows")         # tests/test_gpu_split.py
            # join_split8 is hi + lo8 * 2^-10, the value a product sees; the fp16 half alone is hi = fp16(v), so the
            # two differ by the correction itself and equality is not the check: |hi - joined| = |lo8| <= half an ulp
            # of fp16 (2^-11 |v|) plus the e4m3 rounding of that rest (1/16 of it), asserted at 2^-10
            assert bool(((hi - joined).abs() <= 2.0 ** -10 * joined.abs() + 2.0 ** -24).all())
        else:
            assert_close(rows.float(), ref_ln, {"fp32": 2e-6, "fp16": 2e-3, "bf16": 2e-2}[mode],
                         1e-5 if mode == "fp32" else 1e-2, "kept rows")                # tests/test_gpu_parity.py


@pytest.mark.parametrize("mode", ALL_MODES)
def test_heads_image_alone_equals_image_in_batch(dev, mode):
    """image i's seg and det at B = 1 and inside a batch are the same bits (launch_det_mean: the slice count must not
    depend on B).  What can show a slice count that depends on B is a case with more patches than slices: five images
    of 33 patches (B = 5: 32 / B would give 6 slices instead of 32) and the two of 'ragged_slices'; 'batch5' (5 patches,
    fewer than any slice count) only covers the GEMM and the normalise at another width."""
    lib = _lib.load()
    _x, lw, lb, w, wd = EC.head_inputs("ragged_slices")
    x5 = EC.randn("hd.alone_vs_batch.x", (5, 34, 256), 1.5, 0.3)
    cases = [(x5, lw, lb, w, wd, 1), EC.head_inputs("ragged_slices") + (1,), EC.head_inputs("batch5") + (1,)]
    for x, lw, lb, w, wd, act in cases:
        seg, det = run_heads(lib, dev, x, lw, lb, w, wd, act, mode, "tap")
        for i in range(x.shape[0]):
            s1, d1 = run_heads(lib, dev, x[i:i + 1].contiguous(), lw, lb, w, wd, act, mode, "tap")
            assert torch.equal(s1[0], seg[i]) and torch.equal(d1[0], det[i]), (tuple(x.shape), i)


@pytest.mark.parametrize("mode", ALL_MODES)
def test_heads_degenerate_row(dev, mode):
    """a token row whose elements are all equal, ln_post bias zero: LayerNorm gives exact zeros, the projection too, and
    fmaxf(norm, 1e-12) turns 0 / 0 into an exactly zero, finite seg row; the det mean still divides by n"""
    lib = _lib.load()
    name, b, t = EC.HEAD_DEGENERATE
    args = EC.head_inputs(name, degenerate=True)
    seg, det = run_heads(lib, dev, *args, 0, mode, "tap")
    assert bool((seg[b, t - 1] == 0).all()) and bool(torch.isfinite(seg).all())
    rseg, rdet = EC.head_ref(*args, 0, mode)
    assert_bar(seg, rseg, f"head.{name}.{mode}.seg", f"tap_head.degenerate.{mode}.seg")
    assert_bar(det, rdet, f"head.{name}.{mode}.det", f"tap_head.degenerate.{mode}.det")


# ----------------------------------------------------------------------------------------------------------------
# 3. row head and text embed
# ----------------------------------------------------------------------------------------------------------------
def run_row_head(lib, dev, x, tokens, lw, lb, w, act, flag, mode, want_ws=False, E=None):
    n, T, D = x.shape
    E_buf = w.shape[0]
    E = E_buf if E is None else E
    code = EC.MODES[mode]
    keep = [t.to(dev).contiguous() for t in (x, lw, lb)] + [weight(w, mode, dev)]
    tk = tokens.to(dev).contiguous() if tokens is not None else None
    out = nan_f32(dev, n, E_buf)
    ws = workspace(dev, lib.aaclip_workspace_bytes(code, n * T + n, D, 0, E_buf))
    rc = lib.aaclip_row_head(keep[0].data_ptr(), None if tk is None else tk.data_ptr(), keep[1].data_ptr(),
                             keep[2].data_ptr(), keep[3].data_ptr(), act, out.data_ptr(), n, T, D, E, flag, code,
                             ws.data_ptr(), ws.numel(), stream(dev))
    torch.cuda.synchronize(dev)
    return (rc, out, ws) if want_ws else (rc, out)


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("shape", EC.ROW_SHAPES)
def test_row_head_forward(dev, shape, mode):
    """LayerNorm, row pick, projection against fp64.  Mode 0: maximum first, last, twice (the FIRST must win, as
    torch.argmax picks on the CPU) and all tokens equal; mode 1 with tokens = NULL.  Every row of x has its own
    direction, so a pick that is off by one row misses every mode's bar."""
    lib = _lib.load()
    D, E = shape
    key = f"row.{D}x{E}.{mode}"
    worst = 0.0
    for n in EC.ROW_NS:
        x, lw, lb, w = EC.row_inputs(D, E, n)
        for act in (0, 1):
            for names in EC.ROW_TOKEN_SETS[n] + (None,):
                tok = EC.row_tokens(names) if names else None
                flag = 0 if names else 1
                rc, out = run_row_head(lib, dev, x, tok, lw, lb, w, act, flag, mode)
                assert rc == 0, lib.aaclip_last_error()
                pick = tok.long().argmax(dim=-1) if names else torch.zeros(n, dtype=torch.long)
                ref = EC.row_head_ref(x, pick, lw, lb, w, act, mode)
                assert_close(out, ref, *EC.TOL[mode], f"row_head {shape} {mode} n={n} act={act} {names}")
                e = maxerr(out, ref)
                assert e <= EC.bar(key), (names, n, act, e, EC.bar(key))
                worst = max(worst, e)
    print(f"row_head [{key}]: max |err| {worst:.3e}, bar {EC.bar(key):.3e} (emulation {EC.EMU_ERR[key]:.3e})")
    PARITY_ERRORS[f"edge.row_head.{D}x{E}.{mode}"] = {"max_abs_err": worst, "bar": EC.bar(key)}


def test_row_head_rejects_eot_mode_without_tokens(dev):
    lib = _lib.load()
    x, lw, lb, w = EC.row_inputs(256, 256, 1)
    rc, out, ws = run_row_head(lib, dev, x, None, lw, lb, w, 0, 0, "fp32", want_ws=True)
    assert rc < 0 and b"tokens" in lib.aaclip_last_error()
    assert bool(torch.isnan(out).all()) and bool((ws == 0xFF).all())


def test_row_head_rejects_before_launching(dev):
    """a projection the GEMM refuses (no output features) is rejected before LayerNorm and the row gather run: the
    poisoned workspace they would have written still holds its 0xFF bytes"""
    lib = _lib.load()
    x, lw, lb, w = EC.row_inputs(256, 256, 3)
    tok = EC.row_tokens(EC.ROW_TOKEN_SETS[3][0])
    rc, out, ws = run_row_head(lib, dev, x, tok, lw, lb, w, 0, 0, "fp32", want_ws=True, E=0)
    assert rc < 0 and b"gemm" in lib.aaclip_last_error()
    assert bool(torch.isnan(out).all()) and bool((ws == 0xFF).all())


def run_text_embed(lib, dev, tok, table, pos, vocab):
    n, T = tok.shape
    D = table.shape[1]
    x = nan_f32(dev, n * T, D)
    td, tb, ps = tok.to(dev).contiguous(), table.to(dev).contiguous(), pos.to(dev).contiguous()
    _lib.check(lib.aaclip_text_embed(td.data_ptr(), tb.data_ptr(), ps.data_ptr(), x.data_ptr(), n, T, D, vocab,
                                     stream(dev)), "text_embed")
    return x.cpu()


@pytest.mark.parametrize("shape", EC.EMBED_SHAPES)
def test_text_embed_is_one_fp32_add(dev, shape):
    """D = 4 (one lane), 260 (a second, ragged stride of 256 floats) and 768; ids 0 and vocab - 1 present"""
    lib = _lib.load()
    tok, table, pos = EC.embed_inputs(*shape)
    assert torch.equal(run_text_embed(lib, dev, tok, table, pos, EC.EMBED_VOCAB), EC.embed_ref(tok, table, pos))


def test_text_embed_clamps_out_of_range_ids(dev):
    """what the kernel does today, stated in include/aaclip.h: ids below 0 read row 0, ids >= vocab read row
    vocab - 1 (the reference's nn.Embedding raises instead)"""
    lib = _lib.load()
    tok, table, pos = EC.embed_inputs(2, 5, 4)
    tok[0, 1], tok[1, 2] = -1, EC.EMBED_VOCAB
    got = run_text_embed(lib, dev, tok, table, pos, EC.EMBED_VOCAB)
    assert torch.equal(got, EC.embed_ref(tok.clamp(0, EC.EMBED_VOCAB - 1), table, pos))


# ----------------------------------------------------------------------------------------------------------------
# 4. maps
# ----------------------------------------------------------------------------------------------------------------
def call_anomaly_map(lib, dev, segs, anchors, S, ksize, sigma, g=None, ws_short=0):
    B, P, E = segs[0].shape
    g = g if g is not None else int(round(P ** 0.5))
    segd = [s.to(dev).contiguous() for s in segs]
    td = anchors.to(dev).contiguous()
    out = nan_f32(dev, B, S, S)
    need = len(segs) * B * g * g * 4
    ws = workspace(dev, need)
    arr = (C.c_void_p * len(segs))(*[s.data_ptr() for s in segd])
    rc = lib.aaclip_anomaly_map(arr, len(segs), td.data_ptr(), 0 if td.dim() == 2 else 2 * E, out.data_ptr(), B, g, E,
                                S, ksize, float(sigma), ws.data_ptr(), need - ws_short, stream(dev))
    torch.cuda.synchronize(dev)
    return rc, out


def call_train_map(lib, dev, seg, anchors, S):
    B, P, E = seg.shape
    g = int(round(P ** 0.5))
    sd, td = seg.to(dev).contiguous(), anchors.to(dev).contiguous()
    out = nan_f32(dev, B, 2, S, S)
    ws = workspace(dev, 2 * B * P * 4)
    _lib.check(lib.aaclip_similarity_map_train(sd.data_ptr(), td.data_ptr(), 0 if td.dim() == 2 else 2 * E,
                                               out.data_ptr(), B, g, E, S, ws.data_ptr(), ws.numel(), stream(dev)),
               "similarity_map_train")
    torch.cuda.synchronize(dev)
    return out


@pytest.mark.parametrize("name", list(EC.MAP_CASES))
def test_maps_vs_reference(dev, name):
    """test-mode map (all levels, blur, upsample, level sum) and train-mode map (level 0) against fp64 at g = 1 ...
    40, S = 1 ... 100 (below g, below the 14 bands), every row width and level count, odd and even ksize, reflection
    to depth g - 1, per-image anchors that differ per image, and one level at x30 (a dropped level shows in the sum).
    Even ksize: the reference's kornia takes odd sizes only; the expectation is the oracle's taps over the kernel's
    window (entry_edge_cases.blur), which pins kernel and oracle to each other, not to the reference.
    Per-image anchors: also B separate B = 1 calls with that image's pair as shared anchors -- the same bits."""
    lib = _lib.load()
    B, g, S, E, NL, ksize, sigma, per_image, _scaled = EC.MAP_CASES[name]
    segs, anchors = EC.map_inputs(name)
    rc, out = call_anomaly_map(lib, dev, segs, anchors, S, ksize, sigma)
    assert rc == 0, lib.aaclip_last_error()
    ref = EC.anomaly_map_ref(segs, anchors, S, ksize, sigma)
    tol = (1e-3, 1e-4) if ksize > 1 else (1e-4, 1e-5)           # tests/test_gpu_parity.py: with / without blur
    e_test = maxerr(out, ref)
    train = call_train_map(lib, dev, segs[0], anchors, S)
    tref = EC.train_map_ref(segs[0], anchors, S)
    e_train = maxerr(train, tref)
    print(f"maps {name}: test-mode max |err| {e_test:.3e} (|ref| <= {float(ref.abs().max()):.1f}), train-mode {e_train:.3e}")
    PARITY_ERRORS[f"edge.map.{name}"] = {"test_max_abs_err": e_test, "train_max_abs_err": e_train}
    assert_close(out, ref, *tol, f"anomaly map {name}")
    assert_close(train, tref, 1e-5, 1e-5, f"train map {name}")  # tests/test_gpu_parity.py test_similarity_maps
    if per_image:
        assert not torch.equal(anchors[0], anchors[1])
        for b in range(B):
            rc, one = call_anomaly_map(lib, dev, [s[b:b + 1] for s in segs], anchors[b], S, ksize, sigma)
            assert rc == 0 and torch.equal(one[0], out[b]), (name, b)
            assert torch.equal(call_train_map(lib, dev, segs[0][b:b + 1], anchors[b], S)[0], train[b]), (name, b)


def test_engine_map_wrappers_take_the_same_path(dev):
    """engine.anomaly_map / engine.similarity_map_train (what forward_utils calls) == the raw calls above"""
    lib = _lib.load()
    for name in ("g5_s9_deep", "g2_s13"):
        B, g, S, E, NL, ksize, sigma, _p, _s = EC.MAP_CASES[name]
        segs, anchors = EC.map_inputs(name)
        rc, out = call_anomaly_map(lib, dev, segs, anchors, S, ksize, sigma)
        assert torch.equal(engine.anomaly_map([s.to(dev) for s in segs], anchors.to(dev), S, ksize, sigma), out)
        assert torch.equal(engine.similarity_map_train(segs[0].to(dev), anchors.to(dev), S),
                           call_train_map(lib, dev, segs[0], anchors, S))


@pytest.mark.parametrize("name", list(EC.MAP_REJECTS))
def test_anomaly_map_rejections(dev, name):
    lib = _lib.load()
    g, NL, ksize, sigma, short = EC.MAP_REJECTS[name]
    gbuf = min(g, 40)
    segs = [torch.zeros(1, gbuf * gbuf, 256) for _ in range(NL)]
    rc, out = call_anomaly_map(lib, dev, segs, torch.zeros(256, 2), 3, ksize, sigma, g=g, ws_short=short)
    assert rc < 0 and lib.aaclip_last_error()
    assert bool(torch.isnan(out).all())
    if short:                                                   # the exact size passes
        rc, out = call_anomaly_map(lib, dev, segs, torch.zeros(256, 2), 3, ksize, sigma, g=g)
        assert rc == 0 and bool(torch.isfinite(out).all())


# ----------------------------------------------------------------------------------------------------------------
# 5. attention lengths at the kernel switches
# ----------------------------------------------------------------------------------------------------------------
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


def run_attention(lib, dev, mode, B, L, H, causal, log2q):
    """-> (context as fp64 [B*L, D], fp64 reference), inputs and reference as tests/test_gpu_parity.py test_attention /
    test_attention_log2q_variant and tests/test_gpu_split.py test_attention_split build them"""
    D = 64 * H
    qkv = EC.attn_inputs(B, L, H)
    if log2q:
        qkv[:, :D] *= LOG2E
    fn = lib.aaclip_attention_log2q if log2q else lib.aaclip_attention
    if mode == "fp16x2":
        qd = engine.split16_rows(qkv.to(dev))
        ctx = torch.full((B * L, 4 * D), 0xAA, dtype=torch.uint8, device=dev)
        f = qkv.clone()
        if L >= 512:                      # long rows: v in fp16
            f[:, 2 * D:] = f[:, 2 * D:].half().float()
    else:
        q16 = qkv.to(TDT[mode])
        qd = q16.to(dev)
        ctx = torch.full((B * L, D), NAN, dtype=TDT[mode], device=dev)
        f = q16.float()
    _lib.check(fn(EC.MODES[mode], qd.data_ptr(), ctx.data_ptr(), B, L, H, causal, stream(dev)), "attention")
    torch.cuda.synchronize(dev)
    if log2q:
        f[:, :D] *= LN2
    got = engine.join_split8(ctx, D) if mode == "fp16x2" else ctx.double().cpu()
    return got, EC.attn_ref(f, B, L, H, causal)


ATTN_TOL = {"fp32": (2e-5, 1e-5), "fp16": (3e-3, 1e-2), "bf16": (2.5e-2, 3e-2), "fp16x2": (4e-4, 1e-3)}


@pytest.mark.parametrize("L", EC.ATTN_F32_L)
def test_attention_fp32_at_the_64_switch(dev, L):
    """63: the VALU kernel; 64: the MFMA kernel; 127 / 128: a ragged and a full 128-query tile"""
    lib = _lib.load()
    for causal in (0, 1):
        got, ref = run_attention(lib, dev, "fp32", 1, L, 1, causal, 0)
        PARITY_ERRORS[f"edge.attn.fp32.L{L}.causal{causal}"] = maxerr(got, ref)
        assert_close(got, ref, *ATTN_TOL["fp32"], f"attention fp32 L={L} causal={causal}")


@pytest.mark.parametrize("mode", ["fp16", "bf16", "fp16x2"])
@pytest.mark.parametrize("cfg", [(1, 1, L) for L in EC.ATTN_16_L] + [EC.ATTN_BATCHED])
def test_attention_16bit_at_the_512_switch(dev, mode, cfg):
    """both sides of L = 512, exact multiples of the 128- and 256-query tiles, and (B, H, L) = (3, 1, 513): 9 tiles on
    a grid of 16 (plain 16-bit) / 15 on 16 (split); aaclip_attention and aaclip_attention_log2q, causal and not"""
    lib = _lib.load()
    B, H, L = cfg
    for causal in (0, 1):
        for log2q in (0, 1):
            got, ref = run_attention(lib, dev, mode, B, L, H, causal, log2q)
            PARITY_ERRORS[f"edge.attn.{mode}.B{B}.L{L}.causal{causal}.log2q{log2q}"] = maxerr(got, ref)
            assert_close(got, ref, *ATTN_TOL[mode], f"attention {mode} {cfg} causal={causal} log2q={log2q}")
