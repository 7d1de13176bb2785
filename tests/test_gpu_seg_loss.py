"""Stage-1 training loss on the GPU (reference train.py:94-105): forward_utils.calculate_similarity_map(test=False)
and calculate_seg_loss, forward and backward through the HIP kernels of csrc/train_loss.hip, against the fp64
restatement (tests/seg_loss_cases.py, itself pinned to the reference by tests/test_seg_loss_cpu.py) and against what
the reference computed (tests/golden/seg_loss.npz).

Bars: loss and its three terms 1e-5 relative; gradients (anchors, patch features, d preds) 1e-4 relative Frobenius.
The kernels run in fp32 (the reference trains in fp32); the measured errors go to PARITY_ERRORS."""
import os

import numpy as np
import pytest
import torch

import forward_utils as FU
from aaclip_hip import _lib, engine
from conftest import GOLDEN, PARITY_ERRORS
from seg_loss_cases import CASES, make_case, seg_loss_terms, seg_rows, similarity_map

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "seg_loss.npz"))


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def hip_step(name, dev, need_seg=False):
    """one forward + backward on the GPU: -> (loss, d anchors, d patch features or None)"""
    f, t, mask = make_case(name)
    S = CASES[name][2]
    fd = f.float().to(dev).requires_grad_(need_seg)
    td = t.float().to(dev).requires_grad_(True)
    preds = FU.calculate_similarity_map(fd, td, S)
    loss = FU.calculate_seg_loss(preds, mask.float().to(dev))
    loss.backward()
    return loss.detach(), td.grad, fd.grad


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_gradients_match_reference(dev, golden, name):
    B, g, S, _k, _s = CASES[name]
    loss, d_t, d_f = hip_step(name, dev, need_seg=True)
    e_loss = abs(loss.item() - float(golden[f"{name}.loss"])) / abs(float(golden[f"{name}.loss"]))
    e_t = rel(d_t, golden[f"{name}.d_anchors"])
    e_f = rel(d_f[:, seg_rows(g * g), :], golden[f"{name}.d_seg_rows"])
    # the full patch-feature gradient against fp64 autograd of the restatement
    f, t, mask = make_case(name)
    f.requires_grad_(True)
    sum(seg_loss_terms(similarity_map(f, t, S), mask)).backward()
    e_f_full = rel(d_f, f.grad)
    PARITY_ERRORS[f"seg_loss.{name}"] = {"loss_rel": e_loss, "d_anchors_rel_fro": e_t, "d_seg_rows_rel_fro": e_f,
                                         "d_seg_rel_fro": e_f_full}
    assert e_loss <= 1e-5, e_loss
    assert e_t <= 1e-4, e_t
    assert e_f <= 1e-4 and e_f_full <= 1e-4, (e_f, e_f_full)


@pytest.mark.parametrize("name", ["b4_g37_mixed", "b4_g5_zero", "b4_g5_one", "b1_g5_mixed"])
def test_seg_loss_terms_and_backward(dev, golden, name):
    """calculate_seg_loss, FocalLoss and BinaryDiceLoss on fixed probabilities; d preds against fp64 autograd."""
    S = CASES[name][2]
    f, t, mask = make_case(name)
    p64 = similarity_map(f, t, S).detach()
    pd = p64.float().to(dev).requires_grad_(True)
    md = mask.float().to(dev)
    loss = FU.calculate_seg_loss(pd, md)
    loss.backward()
    p64.requires_grad_(True)
    terms = seg_loss_terms(p64, mask)
    sum(terms).backward()
    assert abs(loss.item() - sum(terms).item()) <= 1e-5 * abs(sum(terms).item())
    e_d = rel(pd.grad, p64.grad)
    PARITY_ERRORS[f"seg_loss.d_preds.{name}"] = e_d
    assert e_d <= 1e-4, e_d
    got = [FU.FocalLoss()(pd, md).item(), FU.BinaryDiceLoss()(pd[:, 0, :, :], 1 - md).item(),
           FU.BinaryDiceLoss()(pd[:, 1, :, :], md).item()]
    assert np.allclose(got, golden[f"{name}.terms"], rtol=1e-5, atol=1e-7), (got, golden[f"{name}.terms"])
    # the single-term wrappers are differentiable too: the dice gradient against fp64
    x = pd.detach()[:, 1].clone().requires_grad_(True)
    FU.BinaryDiceLoss()(x, md).backward()
    x64 = p64.detach()[:, 1].clone().requires_grad_(True)
    d1 = 1 - ((2 * (x64.reshape(x64.shape[0], -1) * mask.reshape(x64.shape[0], -1)).sum(1) + 1)
              / (x64.reshape(x64.shape[0], -1).sum(1) + mask.reshape(x64.shape[0], -1).sum(1) + 1)).sum() / x64.shape[0]
    d1.backward()
    assert rel(x.grad, x64.grad) <= 1e-4


def test_grad_enabled_map_is_bit_identical(dev):
    f, t, mask = make_case("b4_g37_mixed")
    fd, td = f.float().to(dev), t.float().to(dev)
    with torch.no_grad():
        ref = FU.calculate_similarity_map(fd, td, 518)
    out = FU.calculate_similarity_map(fd, td.clone().requires_grad_(True), 518)
    assert out.grad_fn is not None and ref.grad_fn is None
    assert torch.equal(out.detach(), ref)


def test_two_backward_passes_are_bit_identical(dev):
    a = hip_step("b4_g37_mixed", dev, need_seg=True)
    b = hip_step("b4_g37_mixed", dev, need_seg=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_saved_tensors_are_freed(dev):
    f, t, mask = make_case("b4_g37_mixed")
    fd, md = f.float().to(dev), mask.float().to(dev)
    td = t.float().to(dev).requires_grad_(True)
    hip_step("b4_g37_mixed", dev)          # warm the workspace
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    loss = FU.calculate_seg_loss(FU.calculate_similarity_map(fd, td, 518), md)
    assert torch.cuda.memory_allocated(dev) > base + 4 * 518 * 518 * 2 * 4 - 1    # the map is held by the graph
    loss.backward()
    del loss
    td.grad = None
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == base


def test_shared_anchor_pair_sums_over_images(dev):
    """anchors [E, 2] shared by the batch: the gradient is the sum of the per-image ones, in a fixed order."""
    f, t, mask = make_case("b3_g5_shared")
    fd, md = f.float().to(dev), mask.float().to(dev)
    t1 = t.float().to(dev).requires_grad_(True)
    FU.calculate_seg_loss(FU.calculate_similarity_map(fd, t1, 33), md).backward()
    tb = t.float().to(dev).unsqueeze(0).expand(3, -1, -1).contiguous().requires_grad_(True)
    FU.calculate_seg_loss(FU.calculate_similarity_map(fd, tb, 33), md).backward()
    assert rel(t1.grad, tb.grad.sum(0)) <= 1e-5


def test_abi_rejects_bad_shapes(dev):
    lib = _lib.load()
    x = torch.zeros(8, device=dev)
    rc = lib.aaclip_seg_loss(x.data_ptr(), 2, 1, x.data_ptr(), 0, x.data_ptr(), x.data_ptr(), 1, 1, x.data_ptr(),
                             4096, engine._stream(dev))
    assert rc < 0 and b"terms" in lib.aaclip_last_error()
    rc = lib.aaclip_similarity_map_train_backward(x.data_ptr(), x.data_ptr(), 0, x.data_ptr(), x.data_ptr(),
                                                  x.data_ptr(), None, 1, 41, 768, 33, x.data_ptr(), 1 << 20,
                                                  engine._stream(dev))
    assert rc < 0
