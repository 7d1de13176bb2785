"""Case table of the stream contract (include/aaclip.h: "`stream` is a hipStream_t passed as void*; every call only
enqueues work on it"), shared by tests/test_gpu_streams.py (which runs every case on the default stream, on a side
stream, under capture and as a replayed graph) and tests/test_stream_cases_cpu.py (which proves that the table covers
the header).

A case is built by make(dev) -> Case:
  call(stream_handle) -> rc   one ctypes call (aaclip_optim_adam_step: the grad-norm call and the step, one sequence)
                              with every pointer bound in advance; it allocates nothing and copies nothing
  inputs    device tensors the call only reads, each with two host value sets X and Y of the same shape and kind
  state     device tensors the call updates in place, with their initial host values
  outputs   device tensors the call writes; `fixed` outputs are compared like the others but need not differ between
            X and Y (a count that is zero by construction)
  scratch   the workspace, at exactly the size the entry's *_workspace_bytes function (or the header's formula) gives

Shapes are the smallest the existing GPU tests of each entry use; values come from synth.randn with seeds 1 (X) and 2
(Y).  Where an input must be in a format another entry writes (region ids, for one), make() runs that entry once on
the default stream and keeps its result as host bytes."""
import ctypes as C

import torch
import torch.nn.functional as F

from aaclip_hip import _lib, engine, synth

F32, F16, BF16, F16X2 = _lib.F32, _lib.F16, _lib.BF16, _lib.F16X2
TDT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
SEEDS = (1, 2)
POISON = 0xFF


class Case:
    def __init__(self, dev):
        self.dev = dev
        self.inputs, self.state, self.outputs, self.fixed, self.scratch = [], [], [], [], []
        self.keep = []          # ctypes structs and arrays the call points into
        self.call = None

    # ---- inputs
    def inp(self, x, y):
        """device tensor with the two host value sets x and y"""
        x, y = x.contiguous(), y.contiguous()
        assert x.shape == y.shape and x.dtype == y.dtype
        t = torch.empty(x.shape, dtype=x.dtype, device=self.dev)
        self.inputs.append((t, x, y))
        return t

    def rnd(self, key, shape, std=1.0, mean=0.0, f=None):
        """synth.randn values (seed 1 / seed 2), optionally mapped through f (a format conversion on the host)"""
        pair = [synth.randn(key, shape, std, s, mean) for s in SEEDS]
        if f is not None:
            pair = [f(t) for t in pair]
        return self.inp(*pair)

    def ints(self, key, shape, lo, hi, dtype=torch.int32):
        pair = [torch.randint(lo, hi, shape, generator=synth._gen(key, s)).to(dtype) for s in SEEDS]
        return self.inp(*pair)

    def st(self, key, shape, std=1.0, mean=0.0, f=None):
        v = synth.randn(key, shape, std, 3, mean)
        v = (f(v) if f is not None else v).contiguous()
        t = torch.empty(v.shape, dtype=v.dtype, device=self.dev)
        self.state.append((t, v))
        return t

    # ---- outputs and scratch
    def out(self, shape, dtype=torch.float32, fixed=False):
        t = torch.empty(shape, dtype=dtype, device=self.dev)
        (self.fixed if fixed else self.outputs).append(t)
        return t

    def ws(self, nbytes):
        nbytes = int(nbytes)
        assert nbytes > 0, "the workspace function refused the case's shape"
        t = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self.scratch.append(t)
        return t

    def ptrs(self, tensors):
        arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        self.keep.append(arr)
        return arr

    def load(self, which):
        """copy value set 0 (X) or 1 (Y) and the initial state into the bound buffers, on the current stream"""
        for t, x, y in self.inputs:
            t.copy_(y if which else x)
        for t, v in self.state:
            t.copy_(v)

    def poison(self):
        for t in self.outputs + self.fixed + self.scratch:
            t.view(torch.uint8).fill_(POISON)

    def results(self):
        """(tensors that must differ between X and Y, tensors that need not)"""
        return self.outputs + [t for t, _ in self.state], self.fixed


def p(t):
    return None if t is None else t.data_ptr()


def unit(t):
    return F.normalize(t, dim=-1)


# ----------------------------------------------------------------------------------------------------------------
# block weights
# ----------------------------------------------------------------------------------------------------------------
MATS = ("qkv_w", "out_w", "fc_w", "proj_w")


def block_host(key, D, Fw, seed):
    """host fp32 parameters of one block with its adapter, scaled like synth's towers"""
    r = lambda n, shape, std, mean=0.0: synth.randn(f"{key}.{n}", shape, std, seed, mean)
    return {"ln1_w": r("ln1_w", (D,), 0.1, 1.0), "ln1_b": r("ln1_b", (D,), 0.05),
            "qkv_w": r("qkv_w", (3 * D, D), D ** -0.5), "qkv_b": r("qkv_b", (3 * D,), 0.02),
            "out_w": r("out_w", (D, D), D ** -0.5), "out_b": r("out_b", (D,), 0.02),
            "ln2_w": r("ln2_w", (D,), 0.1, 1.0), "ln2_b": r("ln2_b", (D,), 0.05),
            "fc_w": r("fc_w", (Fw, D), D ** -0.5), "fc_b": r("fc_b", (Fw,), 0.02),
            "proj_w": r("proj_w", (D, Fw), Fw ** -0.5), "proj_b": r("proj_b", (D,), 0.02),
            "adapter_w": r("adapter_w", (D, D), D ** -0.5)}


def block_struct(c, hosts, conv):
    """BlockWeights over inputs whose X / Y values are conv(field name, host value) of hosts[0] / hosts[1]; a field conv
    maps to None stays NULL"""
    w = _lib.BlockWeights()
    for name in hosts[0]:
        pair = [conv(name, h[name]) for h in hosts]
        if pair[0] is not None:
            setattr(w, name, c.inp(*pair).data_ptr())
    return w


def blocks_array(c, key, n, D, Fw, code):
    """n blocks with their adapters, the matrix weights in the dtype of `code` (fp32, fp16 or bf16)"""
    arr = (_lib.BlockWeights * n)()
    for i in range(n):
        hosts = [block_host(f"{key}.{i}", D, Fw, s) for s in SEEDS]
        arr[i] = block_struct(c, hosts, lambda name, v: v.to(TDT[code]) if name in MATS + ("adapter_w",) else v)
    c.keep.append(arr)
    return arr


BLK = dict(B=2, L=5, D=256, H=4, Fw=1024)      # the tiny tower's block at five tokens


def make_block_family(entry, code=F16):
    def make(dev):
        lib, c = _lib.load(), Case(dev)
        B, L, D, H, Fw = (BLK[k] for k in ("B", "L", "D", "H", "Fw"))
        n = 1 if entry == "aaclip_block" else 2
        arr = blocks_array(c, entry, n, D, Fw, code)
        ws = c.ws(lib.aaclip_workspace_bytes(code, B * L, D, Fw, 0))
        tail = (B, L, D, H, Fw, 0, code, ws.data_ptr(), ws.numel())
        if entry in ("aaclip_block", "aaclip_blocks"):
            x = c.st(f"{entry}.x", (B * L, D))
            if entry == "aaclip_block":
                c.call = lambda s: lib.aaclip_block(x.data_ptr(), arr, 0.1, *tail, s)
            else:
                c.call = lambda s: lib.aaclip_blocks(x.data_ptr(), arr, n, 0.1, *tail, s)
        elif entry == "aaclip_blocks_to":
            x_in, x = c.rnd(f"{entry}.x", (B * L, D)), c.out((B * L, D))
            c.call = lambda s: lib.aaclip_blocks_to(x_in.data_ptr(), x.data_ptr(), arr, n, 0.1, *tail, s)
        else:
            x_in = c.rnd(f"{entry}.x", (B * L, D))
            outs = c.ptrs([c.out((B * L, D)) for _ in range(n)])
            c.call = lambda s: lib.aaclip_blocks_taps(x_in.data_ptr(), outs, arr, n, 0.1, *tail, s)
        return c
    return make


def make_block_backward(entry):
    """aaclip_block_backward / _long (fp32 structs w, wt) and _long_bf16x3 (w, w3, wt3)"""
    def make(dev):
        lib, c = _lib.load(), Case(dev)
        B, L, D, H, Fw = (BLK[k] for k in ("B", "L", "D", "H", "Fw"))
        hosts = [block_host(entry, D, Fw, s) for s in SEEDS]
        x_in, d_out = c.rnd(f"{entry}.x", (B * L, D)), c.rnd(f"{entry}.d_out", (B * L, D), 0.1)
        d_in, d_aw = c.out((B * L, D)), c.out((D, D))
        if entry == "aaclip_block_backward_long_bf16x3":
            vec = ("ln1_w", "ln1_b", "out_b", "ln2_w", "ln2_b", "fc_b", "proj_b", "adapter_w")
            w = block_struct(c, hosts, lambda n, v: v if n in vec else None)

            def conv3(n, v):
                if n == "qkv_w":
                    return engine.split3_weight(v, q_rows=D)
                if n == "qkv_b":
                    v = v.clone()
                    v[:D] *= 0.125
                    return v
                return engine.split3_weight(v) if n in MATS else None

            def convt3(n, v):
                if n == "adapter_w":
                    return v.t().contiguous()
                return engine.split3_weight(v.t()) if n in MATS else None
            w3, wt3 = block_struct(c, hosts, conv3), block_struct(c, hosts, convt3)
            ws = c.ws(lib.aaclip_block_backward_long_bf16x3_workspace_bytes(B, L, D, Fw))
            c.keep += [w, w3, wt3]
            c.call = lambda s: lib.aaclip_block_backward_long_bf16x3(
                x_in.data_ptr(), C.byref(w), C.byref(w3), C.byref(wt3), 0.1, B, L, D, H, Fw, 0, d_out.data_ptr(),
                d_in.data_ptr(), d_aw.data_ptr(), ws.data_ptr(), ws.numel(), s)
            return c
        w = block_struct(c, hosts, lambda n, v: v)
        wt = block_struct(c, hosts, lambda n, v: v.t().contiguous() if n in MATS + ("adapter_w",) else None)
        c.keep += [w, wt]
        if entry == "aaclip_block_backward":
            fn, ws = lib.aaclip_block_backward, c.ws(lib.aaclip_text_backward_workspace_bytes(B * L, D, Fw))
        else:
            fn, ws = lib.aaclip_block_backward_long, c.ws(lib.aaclip_block_backward_long_workspace_bytes(B, L, D, Fw))
        c.call = lambda s: fn(x_in.data_ptr(), C.byref(w), C.byref(wt), 0.1, B, L, D, H, Fw, 0, d_out.data_ptr(),
                              d_in.data_ptr(), d_aw.data_ptr(), ws.data_ptr(), ws.numel(), s)
        return c
    return make


# ----------------------------------------------------------------------------------------------------------------
# embed, heads, maps
# ----------------------------------------------------------------------------------------------------------------
def make_patch_embed(dev):
    lib, c = _lib.load(), Case(dev)
    B, ps, H, W, D = 2, 2, 4, 6, 256                    # entry_edge_cases PATCH_CASES "d": K = 12 padded to 64
    L, K = (H // ps) * (W // ps) + 1, 3 * ps * ps
    img = c.rnd("pe.img", (B, 3, H, W), 1.2, 0.1)
    w = c.rnd("pe.w", (D, K), K ** -0.5, f=lambda t: F.pad(t, (0, 64 - K)))
    cls, pos = c.rnd("pe.cls", (D,), 0.5), c.rnd("pe.pos", (L, D), 0.3)
    lw, lb = c.rnd("pe.lnw", (D,), 0.1, 1.0), c.rnd("pe.lnb", (D,), 0.05)
    x, ws = c.out((B * L, D)), c.ws(lib.aaclip_workspace_bytes(F32, B * L, D, 4 * D, 0))
    c.call = lambda s: lib.aaclip_patch_embed(img.data_ptr(), w.data_ptr(), cls.data_ptr(), pos.data_ptr(), lw.data_ptr(),
                                              lb.data_ptr(), x.data_ptr(), B, H, W, ps, D, F32, ws.data_ptr(),
                                              ws.numel(), s)
    return c


def make_head(entry):
    def make(dev):
        lib, c = _lib.load(), Case(dev)
        B, L, D, E = 3, 2, 256, 256                     # entry_edge_cases HEAD_CASES "one_patch"
        x = c.rnd("hd.x", (B * L, D), 1.5, 0.3)
        lw, lb = c.rnd("hd.lnw", (D,), 0.1, 1.0), c.rnd("hd.lnb", (D,), 0.05)
        w, wd = c.rnd("hd.w", (E, D), D ** -0.5), c.rnd("hd.wd", (E, D), D ** -0.5)
        ws = c.ws(lib.aaclip_workspace_bytes(F32, B * L, D, 0, E))
        tail = (B, L, D, E, F32, ws.data_ptr(), ws.numel())
        det = c.out((B, E))
        if entry == "aaclip_det_head":
            c.call = lambda s: lib.aaclip_det_head(x.data_ptr(), lw.data_ptr(), lb.data_ptr(), wd.data_ptr(), 1,
                                                   det.data_ptr(), *tail, s)
            return c
        seg = c.out((B, L - 1, E))
        if entry == "aaclip_tap_head":
            c.call = lambda s: lib.aaclip_tap_head(x.data_ptr(), lw.data_ptr(), lb.data_ptr(), w.data_ptr(), 1,
                                                   seg.data_ptr(), wd.data_ptr(), det.data_ptr(), *tail, s)
        else:
            rows = c.out((B * L, D))
            c.call = lambda s: lib.aaclip_tap_head_keep_rows(x.data_ptr(), lw.data_ptr(), lb.data_ptr(), w.data_ptr(), 1,
                                                             seg.data_ptr(), wd.data_ptr(), det.data_ptr(),
                                                             rows.data_ptr(), *tail, s)
        return c
    return make


MAP = dict(B=2, g=5, S=9, E=256, NL=2, ksize=3, sigma=1.0)


def make_anomaly_map(dev):
    lib, c = _lib.load(), Case(dev)
    B, g, S, E, NL, ks, sg = (MAP[k] for k in ("B", "g", "S", "E", "NL", "ksize", "sigma"))
    segs = c.ptrs([c.rnd(f"am.seg{l}", (B, g * g, E), f=unit) for l in range(NL)])
    t = c.rnd("am.t", (2, E), f=lambda v: unit(v).t())            # anchors [E, 2] with unit columns
    out, ws = c.out((B, S, S)), c.ws(NL * B * g * g * 4)
    c.call = lambda s: lib.aaclip_anomaly_map(segs, NL, t.data_ptr(), 0, out.data_ptr(), B, g, E, S, ks, sg,
                                              ws.data_ptr(), ws.numel(), s)
    return c


def make_support_map(dev):
    lib, c = _lib.load(), Case(dev)
    B, g, S, NL, ks, sg = (MAP[k] for k in ("B", "g", "S", "NL", "ksize", "sigma"))
    cos = c.ptrs([c.rnd(f"sm.cos{l}", (B * g * g,), 0.3, 0.5) for l in range(NL)])
    base = c.rnd("sm.base", (B, S, S))                  # with a base and a weight the last stage (the add) is no identity
    out, ws = c.out((B, S, S)), c.ws(NL * B * g * g * 4)
    c.call = lambda s: lib.aaclip_support_map(cos, NL, base.data_ptr(), 0.7, out.data_ptr(), B, g, S, ks, sg,
                                              ws.data_ptr(), ws.numel(), s)
    return c


def make_iqm_map(dev):
    lib, c = _lib.load(), Case(dev)
    B, g, S, E, NL = (MAP[k] for k in ("B", "g", "S", "E", "NL"))
    segs = c.ptrs([c.rnd(f"im.seg{l}", (B, g * g, E)) for l in range(NL)])
    q, base = c.rnd("im.q", (B, 2, E)), c.rnd("im.base", (B, S, S))
    out, ws = c.out((B, S, S)), c.ws(NL * B * g * g * 4)
    c.call = lambda s: lib.aaclip_iqm_map(segs, NL, q.data_ptr(), base.data_ptr(), out.data_ptr(), B, g, E, S, 0.6, 0.4,
                                          ws.data_ptr(), ws.numel(), s)
    return c


def make_train_map(dev):
    lib, c = _lib.load(), Case(dev)
    B, g, S, E = (MAP[k] for k in ("B", "g", "S", "E"))
    seg = c.rnd("tm.seg", (B, g * g, E), f=unit)
    t = c.rnd("tm.t", (2, E), f=lambda v: unit(v).t())
    out, ws = c.out((B, 2, S, S)), c.ws(2 * B * g * g * 4)
    c.call = lambda s: lib.aaclip_similarity_map_train(seg.data_ptr(), t.data_ptr(), 0, out.data_ptr(), B, g, E, S,
                                                       ws.data_ptr(), ws.numel(), s)
    return c


def make_train_map_backward(dev):
    lib, c = _lib.load(), Case(dev)
    B, g, S, E = (MAP[k] for k in ("B", "g", "S", "E"))
    seg = c.rnd("tmb.seg", (B, g * g, E), f=unit)
    t = c.rnd("tmb.t", (2, E), f=lambda v: unit(v).t())
    preds = c.rnd("tmb.preds", (B, 2, S, S), f=lambda v: torch.softmax(v, dim=1))
    d_preds = c.rnd("tmb.d_preds", (B, 2, S, S), 0.1)
    d_t, d_seg = c.out((E, 2)), c.out((B, g * g, E))
    ws = c.ws(lib.aaclip_similarity_map_train_backward_workspace_bytes(B, g, S))
    c.call = lambda s: lib.aaclip_similarity_map_train_backward(
        seg.data_ptr(), t.data_ptr(), 0, preds.data_ptr(), d_preds.data_ptr(), d_t.data_ptr(), d_seg.data_ptr(), B, g, E,
        S, ws.data_ptr(), ws.numel(), s)
    return c


def make_iqm_map_train_backward(dev):
    lib, c = _lib.load(), Case(dev)
    B, g, S, E = (MAP[k] for k in ("B", "g", "S", "E"))
    seg, q = c.rnd("imb.seg", (B, g * g, E)), c.rnd("imb.q", (B, 2, E))
    grid = c.rnd("imb.grid", (B, g * g), f=torch.sigmoid)
    d_preds = c.rnd("imb.d_preds", (B, 2, S, S), 0.1)
    d_seg, d_q = c.out((B, g * g, E)), c.out((B, 2, E))
    ws = c.ws(lib.aaclip_iqm_map_train_backward_workspace_bytes(B, g, E, S))
    c.call = lambda s: lib.aaclip_iqm_map_train_backward(seg.data_ptr(), q.data_ptr(), grid.data_ptr(), d_preds.data_ptr(),
                                                         d_seg.data_ptr(), d_q.data_ptr(), B, g, E, S, ws.data_ptr(),
                                                         ws.numel(), s)
    return c


def make_iqm_map_train(dev):
    lib, c = _lib.load(), Case(dev)
    B, g, S, E = (MAP[k] for k in ("B", "g", "S", "E"))
    seg, q = c.rnd("imt.seg", (B, g * g, E)), c.rnd("imt.q", (B, 2, E))
    grid, out = c.out((B, g * g)), c.out((B, 2, S, S))
    c.call = lambda s: lib.aaclip_iqm_map_train(seg.data_ptr(), q.data_ptr(), grid.data_ptr(), out.data_ptr(), B, g, E, S,
                                                s)
    return c


def make_seg_loss(dev):
    lib, c = _lib.load(), Case(dev)
    B, S = 2, 10
    P = S * S
    preds = c.rnd("sl.preds", (B, 2, S, S), f=lambda v: torch.softmax(v, dim=1))
    mask = c.rnd("sl.mask", (B, P), f=lambda v: (v > 0.8).float())
    loss, coef, ws = c.out((4,)), c.out((B, 4)), c.ws(lib.aaclip_seg_loss_workspace_bytes(B))
    c.call = lambda s: lib.aaclip_seg_loss(preds.data_ptr(), 2 * P, P, mask.data_ptr(), _lib.SEG_LOSS_ALL,
                                           loss.data_ptr(), coef.data_ptr(), B, P, ws.data_ptr(), ws.numel(), s)
    return c


# ----------------------------------------------------------------------------------------------------------------
# backward building blocks
# ----------------------------------------------------------------------------------------------------------------
def make_gemm_wgrad(dev):
    lib, c = _lib.load(), Case(dev)
    rows, O, I = 37, 128, 128
    dz, u, dw = c.rnd("wg.dz", (rows, O)), c.rnd("wg.u", (rows, I)), c.out((O, I))
    ws = c.ws(lib.aaclip_text_backward_workspace_bytes(rows, I, 0))
    c.call = lambda s: lib.aaclip_gemm_wgrad(dz.data_ptr(), O, u.data_ptr(), I, dw.data_ptr(), rows, O, I, ws.data_ptr(),
                                             ws.numel(), s)
    return c


def attn_qkv(c, key, B, L, H, f=None):
    def scale(v):
        v = v.clone()
        v[:, : H * 64] *= 0.6                          # logits O(5), tests/test_gpu_parity.py test_attention
        return v if f is None else f(v)
    return c.rnd(key, (B * L, 3 * H * 64), f=scale)


def make_attention_backward(entry):
    def make(dev):
        lib, c = _lib.load(), Case(dev)
        B, H = 2, 2
        L, causal = (7, 1) if entry == "aaclip_attention_backward" else (70, 0)
        qkv, d_ctx = attn_qkv(c, f"{entry}.qkv", B, L, H), c.rnd(f"{entry}.d_ctx", (B * L, H * 64), 0.1)
        d_qkv = c.out((B * L, 3 * H * 64))
        if entry == "aaclip_attention_backward":
            c.call = lambda s: lib.aaclip_attention_backward(qkv.data_ptr(), d_ctx.data_ptr(), d_qkv.data_ptr(), B, L, H,
                                                             causal, 0.125, s)
            return c
        fn = getattr(lib, entry)
        ws = c.ws(getattr(lib, entry + "_workspace_bytes")(B, L, H))
        c.call = lambda s: fn(qkv.data_ptr(), d_ctx.data_ptr(), d_qkv.data_ptr(), B, L, H, causal, 0.125, ws.data_ptr(),
                              ws.numel(), s)
        return c
    return make


def row_tokens(c, key, n, T):
    """token rows whose maximum (the EOT row) sits elsewhere in X than in Y"""
    pair = []
    for shift in (1, 3):
        tok = torch.arange(1, n * T + 1, dtype=torch.int32).view(n, T) % 5
        for i in range(n):
            tok[i, (i + shift) % T] = 9
        pair.append(tok)
    return c.inp(*pair)


def make_row_head(dev):
    lib, c = _lib.load(), Case(dev)
    n, T, D, E = 3, 7, 256, 256                         # entry_edge_cases ROW_SHAPES[0]
    x, tok = c.rnd("rh.x", (n * T, D), 2.0, 0.5), row_tokens(c, "rh.tok", n, T)
    lw, lb, w = c.rnd("rh.lnw", (D,), 0.1, 1.0), c.rnd("rh.lnb", (D,), 0.05), c.rnd("rh.w", (E, D), D ** -0.5)
    out, ws = c.out((n, E)), c.ws(lib.aaclip_workspace_bytes(F32, n * T + n, D, 0, E))
    c.call = lambda s: lib.aaclip_row_head(x.data_ptr(), tok.data_ptr(), lw.data_ptr(), lb.data_ptr(), w.data_ptr(), 1,
                                           out.data_ptr(), n, T, D, E, 0, F32, ws.data_ptr(), ws.numel(), s)
    return c


def make_row_head_backward(dev):
    lib, c = _lib.load(), Case(dev)
    n, T, D, E = 3, 7, 256, 256
    x, tok = c.rnd("rhb.x", (n * T, D), 2.0, 0.5), row_tokens(c, "rhb.tok", n, T)
    lw, lb = c.rnd("rhb.lnw", (D,), 0.1, 1.0), c.rnd("rhb.lnb", (D,), 0.05)
    hw = [synth.randn("rhb.w", (E, D), D ** -0.5, s) for s in SEEDS]
    w, wt = c.inp(*hw), c.inp(*[h.t().contiguous() for h in hw])
    d_out = c.rnd("rhb.d_out", (n, E), 0.1)
    d_x, d_w = c.out((n * T, D)), c.out((E, D))
    ws = c.ws(lib.aaclip_text_backward_workspace_bytes(n * T, D, 0))
    c.call = lambda s: lib.aaclip_row_head_backward(x.data_ptr(), tok.data_ptr(), lw.data_ptr(), lb.data_ptr(),
                                                    w.data_ptr(), wt.data_ptr(), 1, d_out.data_ptr(), d_x.data_ptr(),
                                                    d_w.data_ptr(), n, T, D, E, 0, ws.data_ptr(), ws.numel(), s)
    return c


def make_tap_head_backward(dev):
    lib, c = _lib.load(), Case(dev)
    B, L, D, E = 2, 3, 256, 256
    x = c.rnd("thb.x", (B * L, D), 1.5, 0.3)
    lw, lb = c.rnd("thb.lnw", (D,), 0.1, 1.0), c.rnd("thb.lnb", (D,), 0.05)
    hw = [synth.randn("thb.w", (E, D), D ** -0.5, s) for s in SEEDS]
    hd = [synth.randn("thb.wd", (E, D), D ** -0.5, s) for s in SEEDS]
    w, wt = c.inp(*hw), c.inp(*[h.t().contiguous() for h in hw])
    wd, wdt = c.inp(*hd), c.inp(*[h.t().contiguous() for h in hd])
    d_seg, d_det = c.rnd("thb.d_seg", (B, L - 1, E), 0.1), c.rnd("thb.d_det", (B, E), 0.1)
    d_x, d_w, d_wd = c.out((B * L, D)), c.out((E, D)), c.out((E, D))
    ws = c.ws(lib.aaclip_tap_head_backward_workspace_bytes(B, L, D, E))
    c.call = lambda s: lib.aaclip_tap_head_backward(
        x.data_ptr(), lw.data_ptr(), lb.data_ptr(), w.data_ptr(), wt.data_ptr(), 1, d_seg.data_ptr(), wd.data_ptr(),
        wdt.data_ptr(), d_det.data_ptr(), d_x.data_ptr(), d_w.data_ptr(), d_wd.data_ptr(), B, L, D, E, ws.data_ptr(),
        ws.numel(), s)
    return c


def make_layernorm_param_grad(dev):
    lib, c = _lib.load(), Case(dev)
    rows, D = 37, 256
    x, d_y, d_w, d_b = c.rnd("lpg.x", (rows, D)), c.rnd("lpg.d_y", (rows, D)), c.out((D,)), c.out((D,))
    ws = c.ws(lib.aaclip_layernorm_param_grad_workspace_bytes(rows, D))
    c.call = lambda s: lib.aaclip_layernorm_param_grad(x.data_ptr(), d_y.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), rows,
                                                       D, 1e-5, ws.data_ptr(), ws.numel(), s)
    return c


def make_bias_grad(dev):
    lib, c = _lib.load(), Case(dev)
    rows, N = 37, 128
    dz, db, ws = c.rnd("bg.dz", (rows, N)), c.out((N,)), c.ws(lib.aaclip_bias_grad_workspace_bytes(rows, N))
    c.call = lambda s: lib.aaclip_bias_grad(dz.data_ptr(), N, db.data_ptr(), rows, N, ws.data_ptr(), ws.numel(), s)
    return c


def make_linear_smallk_backward(dev):
    lib, c = _lib.load(), Case(dev)
    R, N, K = 37, 256, 2
    x, d_y, d_w, d_b = c.rnd("lsb.x", (R, K)), c.rnd("lsb.d_y", (R, N)), c.out((N, K)), c.out((N,))
    ws = c.ws(lib.aaclip_linear_smallk_backward_workspace_bytes(R, N, K))
    c.call = lambda s: lib.aaclip_linear_smallk_backward(x.data_ptr(), d_y.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), R,
                                                         N, K, ws.data_ptr(), ws.numel(), s)
    return c


# ----------------------------------------------------------------------------------------------------------------
# cross rows
# ----------------------------------------------------------------------------------------------------------------
def make_cross_rows(backward):
    def make(dev):
        lib, c = _lib.load(), Case(dev)
        B, R, Lk, Dk = 2, 4, 10, 256
        qt, x = c.rnd("cr.qt", (B, R, Dk), 0.1), c.rnd("cr.x", (B * Lk, Dk))
        if not backward:
            out, ws = c.out((B, R, Dk)), c.ws(lib.aaclip_cross_rows_workspace_bytes(B, R, Lk, Dk))
            c.call = lambda s: lib.aaclip_cross_rows(F32, qt.data_ptr(), x.data_ptr(), out.data_ptr(), B, R, Lk, Dk,
                                                     ws.data_ptr(), ws.numel(), s)
            return c
        d_out, d_qt, d_x = c.rnd("cr.d_out", (B, R, Dk), 0.1), c.out((B, R, Dk)), c.out((B * Lk, Dk))
        ws = c.ws(lib.aaclip_cross_rows_backward_workspace_bytes(B, R, Lk, Dk))
        c.call = lambda s: lib.aaclip_cross_rows_backward(F32, qt.data_ptr(), x.data_ptr(), d_out.data_ptr(),
                                                          d_qt.data_ptr(), d_x.data_ptr(), 0, 0, B, R, Lk, Dk,
                                                          ws.data_ptr(), ws.numel(), s)
        return c
    return make


def make_cross_rows_levels(backward):
    def make(dev):
        lib, c = _lib.load(), Case(dev)
        B, R, nseg, Lk, Dk = 2, 4, 2, 9, 768
        rpi, row0 = Lk + 1, 1
        qt = c.rnd("crl.qt", (B, R, nseg, Dk), 0.05)
        xs = c.ptrs([c.rnd(f"crl.x{i}", (B * rpi, Dk), f=lambda v: v.half()) for i in range(nseg)])
        if not backward:
            out, ws = c.out((B, R, nseg, Dk)), c.ws(lib.aaclip_cross_rows_levels_workspace_bytes(B, nseg, Lk, Dk))
            c.call = lambda s: lib.aaclip_cross_rows_levels(F16, qt.data_ptr(), xs, nseg, out.data_ptr(), B, R, rpi, row0,
                                                            Lk, Dk, Dk, ws.data_ptr(), ws.numel(), s)
            return c
        d_out, d_qt = c.rnd("crl.d_out", (B, R, nseg, Dk), 0.1), c.out((B, R, nseg, Dk))
        d_xs = c.ptrs([c.out((B * rpi, Dk)) for _ in range(nseg)])     # the CLS rows are never written: they stay poison
        ws = c.ws(lib.aaclip_cross_rows_levels_backward_workspace_bytes(B, R, nseg, Lk, Dk))
        c.call = lambda s: lib.aaclip_cross_rows_levels_backward(
            F16, qt.data_ptr(), xs, nseg, d_out.data_ptr(), d_qt.data_ptr(), d_xs, 0, B, R, rpi, row0, Lk, Dk, Dk,
            ws.data_ptr(), ws.numel(), s)
        return c
    return make


# ----------------------------------------------------------------------------------------------------------------
# input pipeline, metrics, support, coreset, optimiser
# ----------------------------------------------------------------------------------------------------------------
def make_color_jitter(dev):
    lib, c = _lib.load(), Case(dev)
    B, H, W = 2, 5, 7
    src = c.ints("cj.src", (B, H, W, 3), 0, 256, torch.uint8)
    fac = c.rnd("cj.fac", (3 * B,), 0.2, 1.0)
    apply = c.inp(torch.full((B,), 7, dtype=torch.int32), torch.full((B,), 7, dtype=torch.int32))
    dst, ws = c.out((B, H, W, 3), torch.uint8), c.ws(lib.aaclip_color_jitter_workspace_bytes(B, H, W))
    c.call = lambda s: lib.aaclip_color_jitter(src.data_ptr(), dst.data_ptr(), B, H, W, fac.data_ptr(), apply.data_ptr(),
                                               ws.data_ptr(), ws.numel(), s)
    return c


N_SCORES, PER_IMAGE = 1000, 100


def scores01(c, key):
    """scores in [0, 1) and 0/1 labels"""
    sc = [torch.rand(N_SCORES, generator=synth._gen(key, s)) for s in SEEDS]
    lab = [(torch.rand(N_SCORES, generator=synth._gen(key + ".lab", s)) < 0.3).to(torch.uint8) for s in SEEDS]
    return sc, lab


def packed_keys(sc, lab):
    """aaclip_metrics_sort's packed keys: fp32 bits << 1 | label, ascending (include/aaclip.h)"""
    k = (sc.view(torch.int32).to(torch.int64) << 1) | lab.to(torch.int64)
    return k.sort().values.to(torch.uint32)


def make_metrics_range(dev):
    lib, c = _lib.load(), Case(dev)
    sc, lab = scores01(c, "mr")
    scores, labels = c.inp(*sc), c.inp(*lab)
    image_max, rec = c.out((N_SCORES // PER_IMAGE,)), c.out((24,), torch.uint8)
    ws = c.ws(lib.aaclip_metrics_range_workspace_bytes(N_SCORES, PER_IMAGE))
    c.call = lambda s: lib.aaclip_metrics_range(scores.data_ptr(), labels.data_ptr(), N_SCORES, PER_IMAGE,
                                                image_max.data_ptr(), rec.data_ptr(), ws.data_ptr(), ws.numel(), s)
    return c


def make_metrics_sort(dev):
    lib, c = _lib.load(), Case(dev)
    sc, lab = scores01(c, "ms")
    scores, labels = c.inp(*sc), c.inp(*lab)
    keys = c.out((N_SCORES,), torch.uint32)
    oor = c.out((8,), torch.uint8, fixed=True)          # every score is inside [0, 1]: the count is 0 for X and for Y
    ws = c.ws(lib.aaclip_metrics_sort_workspace_bytes(N_SCORES))
    c.call = lambda s: lib.aaclip_metrics_sort(scores.data_ptr(), labels.data_ptr(), N_SCORES, 1, keys.data_ptr(), None,
                                               oor.data_ptr(), ws.data_ptr(), ws.numel(), s)
    return c


def make_metrics_sort_pairs(dev):
    lib, c = _lib.load(), Case(dev)
    scores = c.rnd("msp.scores", (N_SCORES,))
    values = c.ints("msp.values", (N_SCORES,), 0, 1 << 20, torch.uint32)
    keys, vs = c.out((N_SCORES,), torch.uint32), c.out((N_SCORES,), torch.uint32)
    ws = c.ws(lib.aaclip_metrics_sort_pairs_workspace_bytes(N_SCORES))
    c.call = lambda s: lib.aaclip_metrics_sort_pairs(scores.data_ptr(), values.data_ptr(), N_SCORES, keys.data_ptr(),
                                                     vs.data_ptr(), ws.data_ptr(), ws.numel(), s)
    return c


def make_metrics_curve(entry, rec_bytes):
    def make(dev):
        lib, c = _lib.load(), Case(dev)
        sc, lab = scores01(c, entry)
        keys = c.inp(*[packed_keys(a, b) for a, b in zip(sc, lab)])
        rec = c.out((rec_bytes,), torch.uint8)
        fn, ws = getattr(lib, entry), c.ws(getattr(lib, entry + "_workspace_bytes")(N_SCORES))
        c.call = lambda s: fn(keys.data_ptr(), None, N_SCORES, 1, rec.data_ptr(), ws.data_ptr(), ws.numel(), s)
        return c
    return make


def make_metrics_threshold(dev):
    lib, c = _lib.load(), Case(dev)
    sc, lab = scores01(c, "mt")
    scores, labels = c.inp(*sc), c.inp(*lab)
    recs = []
    for thr in (0.4, 0.6):                              # aaclip_metrics_f1max_record: `threshold` is its last field
        r = torch.zeros(56, dtype=torch.uint8)
        r[52:56] = torch.tensor([thr], dtype=torch.float32).view(torch.uint8)
        recs.append(r)
    f1 = c.inp(*recs)
    mask = c.out((N_SCORES,), torch.uint8)
    counts, totals = c.out((N_SCORES // PER_IMAGE, 4), torch.uint32), c.out((32,), torch.uint8)
    ws = c.ws(lib.aaclip_metrics_threshold_workspace_bytes(N_SCORES, PER_IMAGE))
    c.call = lambda s: lib.aaclip_metrics_threshold(scores.data_ptr(), labels.data_ptr(), N_SCORES, PER_IMAGE, None,
                                                    f1.data_ptr(), mask.data_ptr(), counts.data_ptr(), totals.data_ptr(),
                                                    ws.data_ptr(), ws.numel(), s)
    return c


REG = dict(images=2, H=9, W=11)


def region_masks():
    """X: 40 % anomalous pixels, Y: 20 % -- other region counts per image, so every output of the table differs"""
    n = REG["images"] * REG["H"] * REG["W"]
    return [(torch.rand(n, generator=synth._gen("reg.mask", s)) < d).to(torch.uint8) for s, d in zip(SEEDS, (0.4, 0.2))]


def make_metrics_regions(dev):
    lib, c = _lib.load(), Case(dev)
    im, H, W = REG["images"], REG["H"], REG["W"]
    n = im * H * W
    mask = c.inp(*region_masks())
    region, area, rec = c.out((n,), torch.uint32), c.out((n,), torch.uint32), c.out((24,), torch.uint8)
    ws = c.ws(lib.aaclip_metrics_regions_workspace_bytes(im, H, W))
    c.call = lambda s: lib.aaclip_metrics_regions(mask.data_ptr(), im, H, W, 8, region.data_ptr(), area.data_ptr(),
                                                  rec.data_ptr(), ws.data_ptr(), ws.numel(), s)
    return c


def make_region_table(dev):
    """region / area as aaclip_metrics_regions leaves them: make() runs that entry once per value set on the default
    stream and keeps the host copies"""
    lib, c = _lib.load(), Case(dev)
    im, H, W = REG["images"], REG["H"], REG["W"]
    n = im * H * W
    pre = make_metrics_regions(dev)
    sets = []
    for which in (0, 1):
        pre.load(which)
        rc = pre.call(torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0, lib.aaclip_last_error()
        torch.cuda.synchronize(dev)
        sets.append((pre.outputs[0].cpu(), pre.outputs[1].cpu()))
    region, area = c.inp(sets[0][0], sets[1][0]), c.inp(sets[0][1], sets[1][1])
    scores = c.rnd("rt.scores", (n,))
    cap = n                                               # no more regions than pixels: nothing is dropped
    rows = c.out((cap, 12), torch.uint32)                 # rows behind the kept ones are not touched: they stay poison
    offs, kept, rec = c.out((im + 1,), torch.int32), c.out((n,), torch.uint8), c.out((32,), torch.uint8)
    ws = c.ws(lib.aaclip_region_table_workspace_bytes(im, H, W))
    c.call = lambda s: lib.aaclip_region_table(region.data_ptr(), area.data_ptr(), scores.data_ptr(), None, None, im, H, W,
                                               1, cap, rows.data_ptr(), offs.data_ptr(), kept.data_ptr(), rec.data_ptr(),
                                               ws.data_ptr(), ws.numel(), s)
    return c


def make_metrics_pro_curve(dev):
    """sorted keys with the area of the pixel's region beside them (0 = a normal pixel), as the pair sort leaves them"""
    lib, c = _lib.load(), Case(dev)
    keys = c.inp(*[torch.randint(0, 1 << 31, (N_SCORES,), generator=synth._gen("pc.keys", s)).sort().values
                   .to(torch.uint32) for s in SEEDS])
    areas = c.inp(*[(torch.randint(0, 3, (N_SCORES,), generator=synth._gen("pc.areas", s)) * 5).to(torch.uint32)
                    for s in SEEDS])
    rr = c.inp(*[torch.tensor([7 + i, 600, 400], dtype=torch.int64).view(torch.uint8) for i in (0, 1)])
    rec, ws = c.out((40,), torch.uint8), c.ws(lib.aaclip_metrics_pro_curve_workspace_bytes(N_SCORES))
    c.call = lambda s: lib.aaclip_metrics_pro_curve(keys.data_ptr(), areas.data_ptr(), N_SCORES, rr.data_ptr(), 0.3,
                                                    rec.data_ptr(), ws.data_ptr(), ws.numel(), s)
    return c


def make_support_nearest(dev):
    lib, c = _lib.load(), Case(dev)
    M, N, E = 37, 50, 64
    q, bank = c.rnd("sn.q", (M, E), f=unit), c.rnd("sn.bank", (N, E), f=unit)     # AACLIP_SUPPORT_FP32: a copy of the rows
    cos, idx = c.out((M,)), c.out((M,), torch.int32)
    ws = c.ws(lib.aaclip_support_nearest_workspace_bytes(M, N, E, _lib.SUPPORT_FP32))
    c.call = lambda s: lib.aaclip_support_nearest(q.data_ptr(), M, bank.data_ptr(), N, E, _lib.SUPPORT_FP32,
                                                  cos.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), s)
    return c


def make_coreset_select(dev):
    lib, c = _lib.load(), Case(dev)
    N, E, n = 50, 32, 5

    def quant(v):                                         # aaclip_coreset_rows on unit rows (norm2 ~ 2^28 < 2^29)
        return torch.round(unit(v) * 16384.0).clamp(-32767, 32767).to(torch.int16)
    hq = [quant(synth.randn("cs.rows", (N, E), 1.0, s)) for s in SEEDS]
    q = c.inp(*hq)
    norm2 = c.inp(*[(h.to(torch.int64) ** 2).sum(dim=1).to(torch.int32) for h in hq])
    picks, rad, mind = c.out((n,), torch.int32), c.out((n + 1,), torch.uint32), c.out((N,), torch.uint32)
    ws = c.ws(lib.aaclip_coreset_select_workspace_bytes(N, E, n))
    c.call = lambda s: lib.aaclip_coreset_select(q.data_ptr(), norm2.data_ptr(), N, E, n, 0, picks.data_ptr(),
                                                 rad.data_ptr(), mind.data_ptr(), ws.data_ptr(), ws.numel(), s)
    return c


def make_optim(step):
    """aaclip_optim_grad_norm alone, or followed in the same call sequence by the aaclip_optim_adam_step that reads its
    clipping record on the device"""
    def make(dev):
        lib, c = _lib.load(), Case(dev)
        sizes = (1000, 37)
        rows = []
        for i, n in enumerate(sizes):
            g = c.rnd(f"opt.g{i}", (n,), 2.0)
            if step:
                prm, m = c.st(f"opt.p{i}", (n,)), c.st(f"opt.m{i}", (n,), 0.1)
                v = c.st(f"opt.v{i}", (n,), 0.1, f=torch.abs)
                rows.append((prm.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 0))
            else:
                rows.append((None, g.data_ptr(), None, None, n, 0))
        items = (_lib.OptimTensor * len(rows))(*rows)
        ts = _lib.OptimTensors(items=items, count=len(rows))
        groups = (_lib.OptimGroup * 1)((1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 3))
        c.keep += [items, ts, groups]
        rec, ws = c.out((2,)), c.ws(lib.aaclip_optim_grad_norm_workspace_bytes(C.byref(ts)))

        def call(s):
            rc = lib.aaclip_optim_grad_norm(C.byref(ts), 1.0, rec.data_ptr(), ws.data_ptr(), ws.numel(), s)
            if rc == 0 and step:
                rc = lib.aaclip_optim_adam_step(C.byref(ts), groups, 1, rec.data_ptr(), s)
            return rc
        c.call = call
        return c
    return make


# ----------------------------------------------------------------------------------------------------------------
# entries without a workspace that launch several kernels, issue a memset or select among kernels
# ----------------------------------------------------------------------------------------------------------------
def make_text_embed(dev):
    lib, c = _lib.load(), Case(dev)
    n, T, D, vocab = 2, 5, 260, 11
    tok = c.ints("te.tok", (n, T), 0, vocab)
    table, pos, x = c.rnd("te.table", (vocab, D), 0.7), c.rnd("te.pos", (T, D), 0.3), c.out((n * T, D))
    c.call = lambda s: lib.aaclip_text_embed(tok.data_ptr(), table.data_ptr(), pos.data_ptr(), x.data_ptr(), n, T, D,
                                             vocab, s)
    return c


def make_adapter_mix_fold(dev):
    lib, c = _lib.load(), Case(dev)
    rows, D = 37, 256
    x, a = c.st("amf.x", (rows, D)), c.rnd("amf.a", (rows, D))
    out16, ab = c.out((rows, D), torch.float16), c.out((rows, 2))
    c.call = lambda s: lib.aaclip_adapter_mix_fold(F16, x.data_ptr(), a.data_ptr(), rows, D, 0.1, out16.data_ptr(),
                                                   ab.data_ptr(), s)
    return c


def make_layernorm_split(dev):
    lib, c = _lib.load(), Case(dev)
    rows, D = 37, 256
    x, w, b = c.rnd("lns.x", (rows, D), 1.5, 0.3), c.rnd("lns.w", (D,), 0.1, 1.0), c.rnd("lns.b", (D,), 0.05)
    out = c.out((rows, 4 * D), torch.uint8)
    c.call = lambda s: lib.aaclip_layernorm_split(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), rows, D, 1e-5,
                                                  1, s)
    return c


def make_gemm(code, M, N, K, epi=_lib.EPI_ACT_F32):
    """aaclip_gemm.  M = 4100: the 256-row-tile kernels for the 16-bit dtypes (16 tiles and 4 ragged rows); M = 200:
    the 128-tile kernel.  AACLIP_F16X2: split8 operands, split16 output rows behind the bias epilogue."""
    def make(dev):
        lib, c = _lib.load(), Case(dev)
        key = f"gemm.{code}.{M}.{epi}"
        if code == F16X2:
            A = c.rnd(key + ".A", (M, K), f=engine.split_rows)                               # uint8 [M, 4K]
            W = c.rnd(key + ".W", (N, K), K ** -0.5, f=lambda v: engine.split_rows(v, weight=True))
            bias, out = c.rnd(key + ".b", (N,), 0.1), c.out((M, 2 * N), torch.float16)
            lda, ldc, e = 2 * K, 2 * N, _lib.EPI_BIAS
        else:
            A = c.rnd(key + ".A", (M, K), f=lambda v: v.to(TDT[code]))
            W = c.rnd(key + ".W", (N, K), K ** -0.5, f=lambda v: v.to(TDT[code]))
            lda, ldc, e = K, N, epi
            if epi == _lib.EPI_BIAS_RESID:
                bias, out = c.rnd(key + ".b", (N,), 0.1), c.st(key + ".resid", (M, N))
            else:
                bias, out = None, c.out((M, N))
        c.call = lambda s: lib.aaclip_gemm(code, e, A.data_ptr(), lda, W.data_ptr(), p(bias), out.data_ptr(), ldc, M, N, K,
                                           0, 0, 1.0, s)
        return c
    return make


def make_attention(code, L):
    def make(dev):
        lib, c = _lib.load(), Case(dev)
        B, H = 1, 2
        if code == F16X2:
            qkv = attn_qkv(c, f"attn.x2.{L}", B, L, H, engine.split16_rows)
            ctx = c.out((B * L, 4 * H * 64), torch.uint8)
            c.call = lambda s: lib.aaclip_attention_split(qkv.data_ptr(), ctx.data_ptr(), B, L, H, 0, 0, 0, 1, s)
        else:
            qkv = attn_qkv(c, f"attn.{code}.{L}", B, L, H, lambda v: v.to(TDT[code]))
            ctx = c.out((B * L, H * 64), TDT[code])
            c.call = lambda s: lib.aaclip_attention(code, qkv.data_ptr(), ctx.data_ptr(), B, L, H, 0, s)
        return c
    return make


# entry point -> {case name: make}
CASES = {
    "aaclip_patch_embed": {"k12": make_patch_embed},
    "aaclip_block": {"fp16": make_block_family("aaclip_block")},
    "aaclip_blocks": {"fp16": make_block_family("aaclip_blocks")},
    "aaclip_blocks_to": {"fp16": make_block_family("aaclip_blocks_to")},
    "aaclip_blocks_taps": {"fp16": make_block_family("aaclip_blocks_taps"),
                           "fp32": make_block_family("aaclip_blocks_taps", F32)},
    "aaclip_tap_head": {"one_patch": make_head("aaclip_tap_head")},
    "aaclip_tap_head_keep_rows": {"one_patch": make_head("aaclip_tap_head_keep_rows")},
    "aaclip_det_head": {"one_patch": make_head("aaclip_det_head")},
    "aaclip_anomaly_map": {"g5": make_anomaly_map},
    "aaclip_similarity_map_train": {"g5": make_train_map},
    "aaclip_similarity_map_train_backward": {"g5": make_train_map_backward},
    "aaclip_iqm_map_train": {"g5": make_iqm_map_train},
    "aaclip_iqm_map_train_backward": {"g5": make_iqm_map_train_backward},
    "aaclip_seg_loss": {"all_terms": make_seg_loss},
    "aaclip_gemm_wgrad": {"rows37": make_gemm_wgrad},
    "aaclip_attention_backward": {"l7_causal": make_attention_backward("aaclip_attention_backward")},
    "aaclip_attention_backward_long": {"l70": make_attention_backward("aaclip_attention_backward_long")},
    "aaclip_attention_backward_long_bf16x3": {"l70": make_attention_backward("aaclip_attention_backward_long_bf16x3")},
    "aaclip_block_backward": {"l5": make_block_backward("aaclip_block_backward")},
    "aaclip_block_backward_long": {"l5": make_block_backward("aaclip_block_backward_long")},
    "aaclip_block_backward_long_bf16x3": {"l5": make_block_backward("aaclip_block_backward_long_bf16x3")},
    "aaclip_row_head": {"eot": make_row_head},
    "aaclip_row_head_backward": {"eot": make_row_head_backward},
    "aaclip_tap_head_backward": {"seg_det": make_tap_head_backward},
    "aaclip_color_jitter": {"all_steps": make_color_jitter},
    "aaclip_metrics_range": {"per_image": make_metrics_range},
    "aaclip_metrics_sort": {"packed": make_metrics_sort},
    "aaclip_metrics_curve": {"packed": make_metrics_curve("aaclip_metrics_curve", 40)},
    "aaclip_metrics_f1max": {"packed": make_metrics_curve("aaclip_metrics_f1max", 56)},
    "aaclip_metrics_threshold": {"per_image": make_metrics_threshold},
    "aaclip_metrics_regions": {"conn8": make_metrics_regions},
    "aaclip_metrics_sort_pairs": {"n1000": make_metrics_sort_pairs},
    "aaclip_metrics_pro_curve": {"n1000": make_metrics_pro_curve},
    "aaclip_region_table": {"conn8": make_region_table},
    "aaclip_support_nearest": {"fp32": make_support_nearest},
    "aaclip_support_map": {"g5": make_support_map},
    "aaclip_coreset_select": {"n5": make_coreset_select},
    "aaclip_optim_grad_norm": {"two_tensors": make_optim(False)},
    "aaclip_optim_adam_step": {"clipped": make_optim(True)},
    "aaclip_cross_rows": {"fp32": make_cross_rows(False)},
    "aaclip_cross_rows_backward": {"fp32": make_cross_rows(True)},
    "aaclip_cross_rows_levels": {"two_segments": make_cross_rows_levels(False)},
    "aaclip_cross_rows_levels_backward": {"two_segments": make_cross_rows_levels(True)},
    "aaclip_layernorm_param_grad": {"rows37": make_layernorm_param_grad},
    "aaclip_bias_grad": {"rows37": make_bias_grad},
    "aaclip_linear_smallk_backward": {"k2": make_linear_smallk_backward},
    "aaclip_iqm_map": {"g5": make_iqm_map},
    "aaclip_text_embed": {"d260": make_text_embed},
    "aaclip_adapter_mix_fold": {"fp16": make_adapter_mix_fold},
    "aaclip_layernorm_split": {"rows37": make_layernorm_split},
    "aaclip_gemm": {"fp32_m4100": make_gemm(F32, 4100, 128, 64),
                    "fp16_m4100": make_gemm(F16, 4100, 256, 128),
                    "fp16x2_m4100": make_gemm(F16X2, 4100, 256, 256),
                    "fp16_m200": make_gemm(F16, 200, 256, 128),
                    "fp16_m200_resid": make_gemm(F16, 200, 256, 128, _lib.EPI_BIAS_RESID)},
    "aaclip_attention": {f"{n}_l{L}": make_attention(code, L)
                         for n, code in (("fp32", F32), ("fp16", F16), ("bf16", BF16)) for L in (130, 600)},
    "aaclip_attention_split": {f"l{L}": make_attention(F16X2, L) for L in (130, 600)},
}

# single-kernel entry points without a workspace: name -> why no case
_ONE = "one elementwise or per-row kernel, launched once on the caller's stream"
EXEMPT = {
    "aaclip_seg_loss_backward": _ONE,
    "aaclip_layernorm_backward": _ONE,
    "aaclip_adapter_mix_backward": _ONE,
    "aaclip_split3_rows": _ONE,
    "aaclip_preprocess": "one kernel (both resize passes in it), no workspace, no memset",
    "aaclip_mask_preprocess": _ONE,
    "aaclip_augment_geometric": _ONE,
    "aaclip_metrics_normalise": _ONE,
    "aaclip_support_bank_rows": _ONE,
    "aaclip_coreset_rows": _ONE,
    "aaclip_coreset_unit_rows": _ONE,
    "aaclip_layernorm": _ONE,
    "aaclip_attention_log2q": "aaclip_attention's launcher with one template flag; aaclip_attention has six cases",
    "aaclip_adapter_mix": "the kernel of aaclip_adapter_mix_fold, which has a case",
    "aaclip_gemm_fused": "aaclip_gemm's launcher with epilogue fields; aaclip_gemm has five cases",
    "aaclip_ln_stats_finalize": _ONE,
    "aaclip_split_rows": _ONE,
    "aaclip_small_attention": "one kernel, one workgroup per (head, image)",
    "aaclip_small_attention_backward": "one kernel, one workgroup per (head, image)",
    "aaclip_head_expand": _ONE,
    "aaclip_head_diag": _ONE,
    "aaclip_residual_layernorm": _ONE,
    "aaclip_combine3": _ONE,
    "aaclip_linear_smallk": _ONE,
    "aaclip_act_backward": _ONE,
    "aaclip_drop_cls_rows": _ONE,
}


def case_ids():
    return [(e, n) for e, cs in CASES.items() for n in cs]
