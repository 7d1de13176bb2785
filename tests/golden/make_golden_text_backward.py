#!/usr/bin/env python3
"""Golden vectors of the text-adapter gradients, made by RUNNING THE REFERENCE'S OWN AdaptedCLIP.encode_text
(reference model/adapter.py:273-304) in fp64 on the reduced synthetic model (aaclip_hip.synth tiny_cfg, seed 7,
text_adapt_until = 1), followed by the anchor rule of forward_utils.py:154-161, the reference's
calculate_similarity_map(test=False), calculate_seg_loss and the orthogonal term of train.py:89-96, with torch autograd
on the CPU.  The reference's method is called unbound on a holder with the attributes it reads: its constructor
hard-codes the full model's widths and its loop runs `range(12)` blocks, so the holder's block list pads the reduced
tower's 2 blocks with pass-through entries.

Records: the two sentences' token ids, the loss, and the gradient of every text_adapter tensor -- whole in fp32 and
every ROW_STEP-th row in fp64 (two fp64 [256, 256] tensors would not fit the 1 MB limit of a committed file).

Usage:  python tests/golden/make_golden_text_backward.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import text_backward_cases as TB  # noqa: E402

synth = MG.synth


class _Padded:
    """resblocks[i] of the reduced tower, and a pass-through for the indices the reference's range(12) asks beyond it"""

    def __init__(self, blocks):
        self.blocks = blocks

    def __getitem__(self, i):
        if i < len(self.blocks):
            return self.blocks[i]
        return lambda x, attn_mask=None: (x, None)


def main():
    A, C, M, TK, FU, CONST = MG._stub_and_import_reference()
    from model.adapter_modules import SimpleAdapter, SimpleProj
    cfg = synth.tiny_cfg()
    until = 1
    clip = M.CLIP(
        embed_dim=cfg.embed_dim,
        vision_cfg=dict(image_size=cfg.image_size, layers=cfg.vision.layers, width=cfg.vision.width,
                        patch_size=cfg.patch_size, head_width=64),
        text_cfg=dict(context_length=cfg.context_length, vocab_size=cfg.vocab_size, width=cfg.text.width,
                      heads=cfg.text.heads, layers=cfg.text.layers),
    ).eval()
    clip.load_state_dict(synth.synth_clip_state_dict(cfg, seed=7), strict=True)
    clip = clip.double()
    for p in clip.parameters():
        p.requires_grad_(False)
    d = cfg.text.width
    adapter = torch.nn.ModuleList([SimpleAdapter(d, d) for _ in range(until)] + [SimpleProj(d, cfg.embed_dim, relu=True)])
    adapter.load_state_dict(synth.synth_text_adapter_state_dict(cfg, until=until, seed=7), strict=True)
    adapter = adapter.double()
    holder = types.SimpleNamespace(
        clipmodel=types.SimpleNamespace(
            transformer=types.SimpleNamespace(get_cast_dtype=lambda: torch.float64,
                                              resblocks=_Padded(clip.transformer.resblocks)),
            token_embedding=clip.token_embedding, positional_embedding=clip.positional_embedding,
            attn_mask=clip.attn_mask, ln_final=clip.ln_final),
        text_adapt_until=until, text_adapter=adapter, t_w=0.1)
    tokens = TK.tokenize(TB.SENTENCES)
    emb = A.AdaptedCLIP.encode_text(holder, tokens)
    t = TB.anchors(emb[0:1], emb[1:2]).unsqueeze(0).expand(TB.BATCH, -1, -1)
    f, mask = TB.patch_inputs()
    loss = TB.stage1_loss(t, f, mask, TB.IMG, TB.NORM_WEIGHT, FU.calculate_similarity_map, FU.calculate_seg_loss)
    loss.backward()
    out = {"tokens": tokens.numpy().astype(np.int32), "loss": np.float64(loss.item()),
           "embeddings": emb.detach().numpy()}
    for name, p in adapter.state_dict(keep_vars=True).items():
        out[f"grad.{name}"] = p.grad.float().numpy()
        out[f"grad64.{name}"] = p.grad[::TB.ROW_STEP].numpy()
        print(name, tuple(p.shape), float(p.grad.norm()))
    print("loss", loss.item())
    np.savez_compressed(os.path.join(HERE, "text_backward.npz"), **out)


if __name__ == "__main__":
    main()
