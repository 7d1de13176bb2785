"""train.py with the optimizer step on the HIP path: its arguments and steps, plus

  --fused_optimizer     both optimizers from aaclip_hip.optim: FusedAdam for the text adapters, FusedAdamW in the
                        reference's two groups for the image adapters and the IQM branch.  One step is a handful of
                        multi-tensor launches (csrc/optim.hip) instead of torch's foreach passes.  The optimizer state
                        and the checkpoints keep torch's layout: a run started with train.py resumes here and the other
                        way round.
  --clip_grad_norm X    clip the stage-2 update to a gradient norm of X (needs --fused_optimizer).  The reference calls
                        clip_grad_norm_(model.parameters(), 1.0) on gradients it is about to discard, so its clipping
                        never acts; this one does, inside optimizer.step(): the norm over every trained parameter and the
                        coefficient min(1, X / (norm + 1e-6)) stay on the device, the gradients in memory are left as
                        they are.

Without the two flags it does exactly what train.py does.

python train_fused.py --dataset MVTec --training_mode full_shot --iqm_hidden_size 768 --save_path ckpt/run \
    --fused_optimizer --clip_grad_norm 1.0 [every argument of train.py]
"""
from __future__ import annotations

import argparse

import train as T


def build_parser() -> argparse.ArgumentParser:
    parser = T.build_parser()
    parser.add_argument("--fused_optimizer", action="store_true",
                        help="FusedAdam / FusedAdamW (aaclip_hip.optim) instead of torch.optim.Adam / AdamW")
    parser.add_argument("--clip_grad_norm", type=float, default=None, metavar="X",
                        help="clip the stage-2 step to a gradient norm of X, inside optimizer.step() "
                             "(needs --fused_optimizer)")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.clip_grad_norm is not None and not args.fused_optimizer:
        parser.error("--clip_grad_norm needs --fused_optimizer")
    if args.clip_grad_norm is not None and not args.clip_grad_norm > 0:
        parser.error("--clip_grad_norm must be above 0")
    T.host_threads()
    return T.run(args)


if __name__ == "__main__":
    main()
