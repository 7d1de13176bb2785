"""The fp64 restatement of the stage-1 training loss (tests/seg_loss_cases.py: similarity_map, seg_loss_terms) against
what the reference's own calculate_similarity_map(test=False) and calculate_seg_loss computed, with their autograd
gradients (tests/golden/seg_loss.npz, made by tests/golden/make_golden_seg_loss.py).  This pins the restatement the
GPU tests compare the HIP kernels with to the reference."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from seg_loss_cases import CASES, make_case, seg_loss_terms, seg_rows, similarity_map


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "seg_loss.npz"))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_reference(golden, name):
    B, g, S, _kinds, _shared = CASES[name]
    f, t, mask = make_case(name)
    f.requires_grad_(True)
    t.requires_grad_(True)
    focal, d0, d1 = seg_loss_terms(similarity_map(f, t, S), mask)
    loss = focal + d0 + d1
    loss.backward()
    assert abs(loss.item() - float(golden[f"{name}.loss"])) <= 1e-9 * abs(float(golden[f"{name}.loss"]))
    assert np.allclose([focal.item(), d0.item(), d1.item()], golden[f"{name}.terms"], rtol=1e-9, atol=0)
    assert rel(t.grad, golden[f"{name}.d_anchors"]) <= 1e-9
    assert rel(f.grad[:, seg_rows(g * g), :], golden[f"{name}.d_seg_rows"]) <= 1e-6   # stored in fp32


def test_cases_cover_the_issue_shapes():
    shapes = {(B, g, S) for B, g, S, _k, _s in CASES.values()}
    kinds = {k for _B, _g, _S, ks, _s in CASES.values() for k in ks}
    assert {(1, 37, 518), (4, 37, 518)} <= shapes and any(g == 5 and S == 33 for _B, g, S in shapes)
    assert {1, 4} <= {B for B, _g, _S in shapes}
    assert kinds == {"zero", "one", "rect"}
