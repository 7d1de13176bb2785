"""The train-time input pipeline on the GPU (csrc/augment.hip): colour jitter against Pillow's ImageEnhance and the
mask resize against dataset.transform_mask, both bit for bit; the composed geometric gather against the sequential
fp32 torch path (tests/augment_cases.py); engine.train_preprocess against the host transform of dataset.BaseDataset;
dataset.device_batch; and train.run on a temporary tree with the reduced synthetic model.

Geometry bar: equal everywhere when the rotation is off or a multiple of 90 degrees.  Otherwise a pixel may differ only
where the fp64 source coordinate lies within 1e-3 of a half-integer (AC.BAND), and such pixels are at most 2 % of a
case (AC.BAND_CAP).  Every compared figure goes to PARITY_ERRORS under augment.* (profiles/augment_parity_errors.json)."""
import argparse
import logging

import numpy as np
import pytest
import torch
from PIL import Image

import augment_cases as AC
import dataset as D
import visual_backward_cases as VB
from aaclip_hip import engine, synth
from conftest import PARITY_ERRORS
from synth_dataset import write_tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


T = torch.from_numpy


# ------------------------------------------------------------------------------------------------------ colour
@pytest.mark.parametrize("name", AC.COLOR_CASES)
def test_color_jitter_is_pillow(dev, name):
    c = AC.color_case(name)
    want = AC.color_reference(name)
    src = T(c["src"]).to(dev)
    got = engine.color_jitter(src, T(c["factors"]), T(c["apply"]))
    assert torch.equal(src.cpu(), T(c["src"]))                           # out of place leaves the source alone
    differing = int((got.cpu().numpy() != want).sum())
    print(name, "differing bytes", differing)
    PARITY_ERRORS[f"augment.color.{name}"] = {"differing_bytes": differing}
    assert differing == 0
    assert torch.equal(engine.color_jitter(src, T(c["factors"]), T(c["apply"])), got)     # the same bits again
    work = src.clone()
    assert engine.color_jitter(work, T(c["factors"]), T(c["apply"]), out=work) is work
    assert torch.equal(work, got)                                        # in place equals out of place
    # the byte-wise path: the same frames at an address that is not 16-byte aligned
    flat = torch.empty(src.numel() + 16, dtype=torch.uint8, device=dev)
    odd = flat[3:3 + src.numel()].view(src.shape)
    odd.copy_(src)
    assert odd.data_ptr() % 16 != 0 and torch.equal(engine.color_jitter(odd, T(c["factors"]), T(c["apply"])), got)


def test_color_jitter_rejects_bad_input(dev):
    src = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        engine.color_jitter(torch.zeros(2, 8, 8, 4, dtype=torch.uint8, device=dev), torch.ones(2, 3), torch.zeros(2))
    with pytest.raises(ValueError):
        engine.color_jitter(src, torch.ones(3, 3), torch.zeros(2))
    with pytest.raises(ValueError):
        engine.color_jitter(src, torch.ones(2, 3), torch.zeros(2), out=torch.zeros(2, 8, 8, 3, device=dev))
    flat = torch.zeros(2 * src.numel(), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="color_jitter: dst must be src itself"):
        engine.color_jitter(flat[:src.numel()].view(src.shape), torch.ones(2, 3), torch.zeros(2),
                            out=flat[48:48 + src.numel()].view(src.shape))


# -------------------------------------------------------------------------------------------------------- mask
@pytest.mark.parametrize("name", AC.MASK_CASES)
def test_mask_preprocess_is_transform_mask(dev, name):
    masks, normal, S = AC.mask_case(name)
    want = AC.mask_reference(name)
    got = engine.mask_preprocess(T(masks).to(dev), S, T(normal) if normal.any() else None)
    differing = int((got.cpu() != want).sum())
    print(name, "differing pixels", differing)
    PARITY_ERRORS[f"augment.mask.{name}"] = {"differing_pixels": differing}
    assert got.shape == (len(masks), 1, S, S) and got.dtype == torch.float32 and differing == 0
    if name == "corners":
        assert all(got[b].any() for b in range(4))                       # 37x53 -> 28 keeps every corner pixel
    if name == "normal_between":
        assert not got[1].any() and got[0].any() and got[2].any()
        assert torch.equal(engine.mask_preprocess(T(masks).to(dev), S, T(normal).bool().to(dev)), got)
    assert torch.equal(engine.mask_preprocess(T(masks).to(dev), S, T(normal)), got)


# ---------------------------------------------------------------------------------------------------- geometry
def run_geometry(dev, name):
    image, mask, angle, shift, flags, want_image, want_mask, band = AC.geo_case(name)
    got_image, got_mask = engine.augment_geometric(image.to(dev), mask.to(dev), angle, shift, flags)
    again = engine.augment_geometric(image.to(dev), mask.to(dev), angle.to(dev), shift.to(dev), flags.to(dev))
    assert torch.equal(again[0], got_image) and torch.equal(again[1], got_mask)
    assert set(got_mask.unique().tolist()) <= {0.0, 1.0}                 # the mask channel stays in {0, 1}
    outside, inside, share = AC.compare_geometry(got_image.cpu(), got_mask.cpu(), want_image, want_mask, band)
    print(name, "differ outside the band", outside, "inside", inside, "band share", share)
    PARITY_ERRORS[f"augment.geometry.{name}"] = {"differ_outside_band": outside, "differ_inside_band": inside,
                                                 "band_share": share}
    return outside, inside, share


@pytest.mark.parametrize("name", list(AC.EXACT_CASES))
def test_geometry_exact(dev, name):
    outside, inside, share = run_geometry(dev, name)
    assert share == 0.0 and outside == 0 and inside == 0


@pytest.mark.parametrize("name", list(AC.ROTATED_CASES))
def test_geometry_rotated(dev, name):
    outside, inside, share = run_geometry(dev, name)
    assert outside == 0
    assert share <= AC.BAND_CAP


# ------------------------------------------------------------------------------------------- train_preprocess
def fixed_params():
    """five samples: colour only, shift + flips, everything with a rotation, text-style (nothing), rotation alone"""
    return {"color_factors": torch.tensor([[1.3, 0.7, 1.2], [0.6, 1.4, 0.9], [1.1, 1.2, 0.5], [1.0, 1.0, 1.0],
                                           [0.8, 0.9, 1.5]]),
            "color_apply": torch.tensor([7, 5, 7, 0, 2], dtype=torch.int32),
            "angle": torch.tensor([12.0, -5.0, 17.3, 0.0, -23.456]),
            "shift": torch.tensor([[0, 0], [10, -7], [-4, 9], [0, 0], [3, 3]], dtype=torch.int32),
            "flags": torch.tensor([0, D.GEO_SHIFT | D.GEO_HFLIP | D.GEO_VFLIP, 15, 0, D.GEO_ROTATE], dtype=torch.int32)}


def test_train_preprocess_is_the_host_transform(dev):
    H, W, S, n = 96, 80, 70, 5
    frames = AC.frames("train_preprocess", n, H, W)
    masks = np.zeros((n, H, W), np.uint8)
    for b in range(n):
        masks[b, 10 + 5 * b:50 + 5 * b, 8 * b:30 + 8 * b] = 255
    normal = torch.tensor([0, 0, 0, 1, 0], dtype=torch.int32)
    params = fixed_params()
    got_image, got_mask = engine.train_preprocess(T(frames).to(dev), T(masks).to(dev), normal.to(dev), params, S)
    got_image, got_mask = got_image.cpu(), got_mask.cpu()
    for b in range(n):
        want_image, want_mask = D.train_transform(Image.fromarray(frames[b]),
                                                  None if normal[b] else Image.fromarray(masks[b]), params, S, b)
        band = AC.boundary_band(S, float(params["angle"][b]), params["shift"][b].tolist(), int(params["flags"][b]))
        outside, inside, share = AC.compare_geometry(got_image[b:b + 1], got_mask[b:b + 1], want_image[None],
                                                     want_mask[None], band[None])
        print("train_preprocess sample", b, "differ outside the band", outside, "inside", inside, "band share", share)
        PARITY_ERRORS[f"augment.train_preprocess.sample{b}"] = {"differ_outside_band": outside,
                                                                "differ_inside_band": inside, "band_share": share}
        assert outside == 0 and share <= AC.BAND_CAP
        if not int(params["flags"][b]) & D.GEO_ROTATE:
            assert share == 0.0 and inside == 0
    assert not got_mask[3].any() and got_mask[0].any()


# ----------------------------------------------------------------------------------------------- device_batch
@pytest.fixture()
def tree(tmp_path, monkeypatch):
    """bottle at 96x96 and grid at 64x80, six samples each"""
    root = write_tree(str(tmp_path / "MVTec"), classes=("bottle",), size=(96, 96))
    write_tree(root, classes=("grid",), size=(64, 80), seed=5)
    meta = tmp_path / "meta"
    assert D.build_metadata(root, str(meta / "MVTec" / "full-shot.jsonl")) == 12
    monkeypatch.setitem(D.DATA_PATH, "MVTec", root)
    monkeypatch.setattr(D, "METADATA_ROOT", str(meta))
    return root


def test_device_batch_keeps_the_order(dev, tree):
    S = 70
    _, raw_set = D.get_train_datasets("MVTec", S, "full_shot", -1, device_augment=True)
    _, host_set = D.get_train_datasets("MVTec", S, "full_shot", -1)
    order = [3, 9, 0, 6, 1, 10]                          # the two frame sizes interleaved, normal and anomalous
    raw_set.generator = torch.Generator().manual_seed(11)
    host_set.generator = torch.Generator().manual_seed(11)                # the same numbers, sample by sample
    raw = D.collate_raw([raw_set[i] for i in order])
    assert len(raw["groups"]) == 2
    batch = D.device_batch(raw, dev)
    assert set(batch) >= {"image", "mask", "label", "class_name"}
    assert batch["image"].shape == (6, 3, S, S) and batch["mask"].shape == (6, 1, S, S) and batch["image"].is_cuda
    assert batch["class_name"] == [raw_set.meta[i]["class_name"] for i in order]
    assert batch["label"].tolist() == [raw_set.meta[i]["label"] for i in order]
    total_outside = 0
    for row, i in enumerate(order):
        item = host_set[i]
        assert item["file_name"] == batch["file_name"][row]
        g = next(g for g in raw["groups"] if row in g["index"].tolist())
        k = g["index"].tolist().index(row)
        band = AC.boundary_band(S, float(g["params"]["angle"][k]), g["params"]["shift"][k].tolist(),
                                int(g["params"]["flags"][k]))
        outside, inside, share = AC.compare_geometry(batch["image"][row:row + 1].cpu(), batch["mask"][row:row + 1].cpu(),
                                                     item["image"][None], item["mask"][None], band[None])
        PARITY_ERRORS[f"augment.device_batch.row{row}"] = {"differ_outside_band": outside, "differ_inside_band": inside,
                                                           "band_share": share}
        total_outside += outside
        assert share <= AC.BAND_CAP
    assert total_outside == 0


# -------------------------------------------------------------------------------------------------- train.run
class _Losses(logging.Handler):
    def __init__(self):
        super().__init__()
        self.values, self.epochs = [], []

    def emit(self, record):
        msg = record.getMessage()
        if msg.startswith("loss: "):
            self.values.append(float(msg[6:]))
        if msg.startswith("training "):
            self.epochs.append(msg)


def reduced_clip(model_name, img_size, device, pretrained, require_pretrained):
    """model_factory: the reduced synthetic CLIP of the GPU training tests at the size asked for"""
    assert pretrained == "openai" and require_pretrained
    cfg = synth.tiny_cfg()
    cfg.image_size = img_size
    return VB.build_clip(cfg, "fp32", 7)[1].to(device)


def run_args(save_path, device_augment):
    import train
    args = train.build_parser().parse_args([])
    vars(args).update(img_size=VB.TAPS_IMAGE, surgery_until_layer=3, dataset="MVTec", training_mode="full_shot",
                      text_batch_size=2, image_batch_size=2, text_epoch=1, image_epoch=1, save_path=str(save_path),
                      text_adapt_until=1, image_adapt_until=VB.TAPS_UNTIL, iqm_hidden_size=256,
                      device_augment=device_augment)
    assert isinstance(args, argparse.Namespace)
    return args


@pytest.mark.parametrize("device_augment", [False, True])
def test_train_run(dev, tree, tmp_path, device_augment):
    import train
    save = tmp_path / "ckpt"
    seen = _Losses()
    logger = logging.getLogger("train")
    logger.setLevel(logging.INFO)
    logger.addHandler(seen)
    try:
        model = train.run(run_args(save, device_augment), model_factory=reduced_clip, levels=VB.TAPS_LEVELS)
        first = (list(seen.values), list(seen.epochs))
        text_ckpt = torch.load(save / "text_adapter.pth")
        image_ckpt = torch.load(save / "image_adapter.pth")
        again = train.run(run_args(save, device_augment), model_factory=reduced_clip, levels=VB.TAPS_LEVELS)
    finally:
        logger.removeHandler(seen)
    print("device_augment", device_augment, "epoch losses", first[0])
    PARITY_ERRORS[f"augment.train_run.device_augment_{int(device_augment)}"] = {"text_loss": first[0][0],
                                                                               "image_loss": first[0][1]}
    assert first[1] == ["training text epoch 0:", "training image epoch 0:"]
    assert len(first[0]) == 2 and all(np.isfinite(v) for v in first[0])
    assert set(text_ckpt) == {"epoch", "text_adapter", "text_optimizer"} and text_ckpt["epoch"] == 1
    assert set(image_ckpt) == {"epoch", "image_adapter", "image_optimizer", "iqm_branch"} and image_ckpt["epoch"] == 1
    assert (save / "image_adapter_1.pth").exists()
    # the second run resumes at the stored epochs: nothing more is trained, and the weights are the checkpoint's
    assert (seen.values, seen.epochs) == first
    for k, v in image_ckpt["image_adapter"].items():
        assert torch.equal(again.image_adapter.state_dict()[k].cpu(), v.cpu()), k
    for k, v in text_ckpt["text_adapter"].items():
        assert torch.equal(again.text_adapter.state_dict()[k].cpu(), v.cpu()), k
    for k, v in image_ckpt["iqm_branch"]["iqm"].items():
        assert torch.equal(again.iqm.state_dict()[k].cpu(), v.cpu()) and torch.equal(model.iqm.state_dict()[k].cpu(), v.cpu()), k
