"""The IQM map term of the stage-2 loss at the training shape (B = 2, g = 37, S = 518, E = 768, four tap levels), forward
plus backward, six rounds: the program for `rocprofv3 --kernel-trace --stats -- python tools/profile_iqm_loss.py`
("The IQM map term")."""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "aa-clip-iqm_amd"), REPO]
import torch
from aaclip_hip import engine, synth

dev = torch.device("cuda:0")
B, g, S, E = 2, 37, 518, 768
segs = [torch.nn.functional.normalize(synth.randn(f"prof.seg{i}", (B, g * g, E), 1.0, 5), dim=-1).to(dev) for i in range(4)]
q = synth.randn("prof.q", (B, 2, E), 1.0, 6).to(dev)
d = synth.randn("prof.d", (B, 2, S, S), 1.0, 7).to(dev)
for it in range(6):
    for s in segs:
        out, grid = engine.iqm_map_train(s, q, S)
        engine.iqm_map_train_backward(s, q, grid, d)
torch.cuda.synchronize()
print("done")
