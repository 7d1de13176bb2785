"""engine.block_backward on one visual-tower block, for a `rocprofv3 --kernel-trace --stats -- python ...` run:
B = 2 images of L = 1370 rows, D = 1024, 16 heads, F = 4096, with an adapter ("Timing")."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "aa-clip-iqm_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from aaclip_hip import engine, synth  # noqa: E402
from model.model import CLIP  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1370)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = synth.ClipCfg(embed_dim=256, image_size=70, vision=synth.TowerCfg(1024, 1, 16, 4096),
                        text=synth.TowerCfg(256, 1, 4, 1024))
    clip = CLIP(cfg.embed_dim, dict(image_size=70, layers=1, width=1024, patch_size=14),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=256, heads=4, layers=1), precision="fp32")
    clip.load_state_dict(synth.synth_clip_state_dict(cfg, seed=7), strict=True)
    block = clip.to(dev).eval().visual.transformer.resblocks[0]
    B, L, D = a.batch, a.rows, 1024
    x = synth.randn("pbb.x", (B * L, D), 1.0, 31).to(dev)
    d_out = synth.randn("pbb.d", (B * L, D), 1.0, 31).to(dev)
    aw = torch.nn.Parameter(synth._xavier("pbb.adapter", D, D, 31).to(dev), requires_grad=False)
    for _ in range(a.calls):
        engine.block_backward(x, block, B, L, 16, d_out, adapter_weight=aw, mix=0.1)
    torch.cuda.synchronize()
    print("block_backward calls:", a.calls)


if __name__ == "__main__":
    main()
