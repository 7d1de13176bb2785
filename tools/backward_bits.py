"""One sha256 per output tensor of the attention backward and the block backward, in both backward arithmetics, on the
inputs of the test cases (tests/visual_backward_cases.py, tests/backward_bf16x3_cases.py): the pin for a change that must
not move a bit.  Run it once per library, one fresh process each (AACLIP_LIB selects the library), then compare:

    AACLIP_LIB=/path/to/parent/libaaclip_hip.so python tools/backward_bits.py --out parent.json
    python tools/backward_bits.py --out new.json
    python tools/backward_bits.py --compare parent.json new.json --out profiles/backward_skeleton_bits.json

--compare exits 1 unless the two runs hold the same keys with the same hashes."""
import argparse
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "aa-clip-iqm_amd"), os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def write(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")


def compare(a_path, b_path, out):
    a, b = (json.load(open(p)) for p in (a_path, b_path))
    ha, hb = a["sha256"], b["sha256"]
    differing = sorted(k for k in set(ha) | set(hb) if ha.get(k) != hb.get(k))
    result = {"device": a["device"], "tensors": len(ha), "equal": not differing, "differing": differing, "sha256": ha}
    print(json.dumps({k: v for k, v in result.items() if k != "sha256"}, sort_keys=True))
    if out:
        write(out, result)
    return 0 if ha and not differing else 1


def hashes():
    import torch

    import backward_bf16x3_cases as BC
    import visual_backward_cases as VB
    from aaclip_hip import engine

    dev = torch.device("cuda:0")
    out = {}

    def put(key, t):
        if t is not None:
            out[key] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    # ---- attention backward: the tiled entries at every L (long_rows forces them for fp32)
    def attention(key, qkv, d_ctx, B, H, L, causal, **kw):
        for mode in engine.BACKWARD_PRECISIONS:
            put(f"attention.{mode}.{key}", engine.attention_backward(qkv.to(dev), d_ctx.to(dev), B, L, H, causal,
                                                                      long_rows=True, precision=mode, **kw))

    for B, H, L in BC.ATTENTION_CASES:
        qkv, d_ctx = VB.attention_inputs(B, H, L)
        for causal in (False, True):
            attention(f"{'causal' if causal else 'full'}.B{B}.H{H}.L{L}", qkv, d_ctx, B, H, L, causal)
    B, H, L, _ = BC.PEAKED
    attention("peaked", *BC.peaked_case()[:2], B, H, L, False)
    B, H, L, _ = BC.RANGE
    attention("range", *BC.range_case()[:2], B, H, L, False)
    attention("dq_scale", *VB.attention_inputs(2, 4, 160), 2, 4, 160, False, dq_scale=0.125)

    # ---- block backward
    blocks = {}

    def model(width):
        if width not in blocks:
            cfg = BC.block_cfg(width)
            blocks[width] = (cfg, BC.build_clip(cfg, "fp32", 7)[1].to(dev).eval().visual.transformer.resblocks[0])
        return blocks[width]

    def block(key, width, x, d_out, B, L, causal, modes, **kw):
        cfg, blk = model(width)
        for mode in modes:
            d_in, d_aw = engine.block_backward(x.to(dev), blk, B, L, cfg.vision.heads, d_out.to(dev).clone(), causal=causal,
                                               precision=mode, **kw)
            put(f"block.{mode}.{key}.d_in", d_in)
            put(f"block.{mode}.{key}.d_adapter_w", d_aw)

    for case, (width, B, L, causal) in BC.PLAIN_BLOCK_CASES.items():
        D = BC.block_cfg(width).vision.width
        block(case, width, BC.rnd(f"blk.x.{case}", (B * L, D)), BC.rnd(f"blk.do.{case}", (B * L, D)), B, L, causal,
              engine.BACKWARD_PRECISIONS)
    c = BC.ADAPTER_CASE
    _, _, x, d_out, aw = BC.adapter_case()[:5]
    aw_dev = torch.nn.Parameter(aw.to(dev), requires_grad=False)
    for tag, kw in (("plain", {}), ("weight_only", dict(need_input_grad=False)), ("alias", dict(in_place=True))):
        block(f"adapter.{tag}", c["width"], x, d_out, c["B"], c["L"], False, engine.BACKWARD_PRECISIONS, adapter_weight=aw_dev,
              mix=c["mix"], long_rows=True, **kw)          # L = 33: long_rows keeps fp32 on the visual (long) entry
    # the short entry (the text tower's route): tiny width, B = 2, L = 77, causal
    B, L, D = 2, 77, BC.block_cfg("tiny").vision.width
    x, d_out = BC.rnd("bits.short.x", (B * L, D)), BC.rnd("bits.short.do", (B * L, D))
    aw_dev = torch.nn.Parameter(BC.rnd("bits.short.adapter", (D, D), D ** -0.5).to(dev), requires_grad=False)
    block("short.plain", "tiny", x, d_out, B, L, True, ("fp32",))
    block("short.adapter", "tiny", x, d_out, B, L, True, ("fp32",), adapter_weight=aw_dev, mix=0.1)
    torch.cuda.synchronize()
    return {"device": torch.cuda.get_device_name(0), "sha256": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, a.out))
    result = hashes()
    print(len(result["sha256"]), "tensors hashed")
    if a.out:
        write(a.out, result)


if __name__ == "__main__":
    main()
