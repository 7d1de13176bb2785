"""CPU side of the train-time input pipeline: the new C ABI symbols and their argument checks on the built library,
the host transform of dataset.BaseDataset against Pillow's own ImageEnhance / Image.resize and against the torch
rotation path (tests/augment_cases.py), draw_augment_params, get_train_datasets / collate_raw on a temporary tree, and
train.py's parser against the reference's defaults."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import augment_cases as AC
import dataset as D
from aaclip_hip import _lib, engine
from synth_dataset import write_tree

NEW_SYMBOLS = ["aaclip_color_jitter_workspace_bytes", "aaclip_color_jitter", "aaclip_nearest_table",
               "aaclip_mask_preprocess", "aaclip_augment_geometric"]


# ------------------------------------------------------------------------------------------------- the library
def test_symbols_and_abi():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.aaclip_version() == 10
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aaclip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header


def err():
    return _lib.load().aaclip_last_error().decode()


P = 1 << 20          # a non-null, 16-byte aligned address: every call below is refused before anything reads it


def test_color_jitter_rejections():
    lib = _lib.load()
    need = lib.aaclip_color_jitter_workspace_bytes(2, 37, 53)
    assert need > 0 and lib.aaclip_color_jitter_workspace_bytes(0, 37, 53) == 0
    assert lib.aaclip_color_jitter_workspace_bytes(4, 37, 53) >= need
    far = P + (1 << 24)
    calls = [((None, P, 2, 37, 53, far, far, far, need, None), "null pointer"),
             ((P, far, 0, 37, 53, far, far, far, need, None), "bad frame shape"),
             ((P, far, 2, 0, 53, far, far, far, need, None), "bad frame shape"),
             ((P, far, 2, 37, 1 << 17, far, far, far, need, None), "bad frame shape"),
             ((P, P + 48, 2, 37, 53, far, far, far, need, None), "overlap"),
             ((P, far + (1 << 20), 2, 37, 53, far, far, far + 4, need, None), "8-byte aligned"),
             ((P, far + (1 << 20), 2, 37, 53, far, far, far, need - 1, None), "workspace too small")]
    for args, msg in calls:
        assert lib.aaclip_color_jitter(*args) == -1
        assert err().startswith("color_jitter:") and msg in err(), (err(), msg)


def test_mask_and_geometry_rejections():
    lib = _lib.load()
    far = P + (1 << 24)
    for args, msg in [((None, 2, 37, 53, 28, far, far, None, far, None), "null pointer"),
                      ((P, 2, 37, 53, 28, None, far, None, far, None), "null pointer"),
                      ((P, 0, 37, 53, 28, far, far, None, far, None), "bad source shape"),
                      ((P, 2, 37, 0, 28, far, far, None, far, None), "bad source shape"),
                      ((P, 2, 37, 53, 0, far, far, None, far, None), "output size"),
                      ((P, 2, 37, 53, 4097, far, far, None, far, None), "output size")]:
        assert lib.aaclip_mask_preprocess(*args) == -1
        assert err().startswith("mask_preprocess:") and msg in err(), (err(), msg)
    image, mask, oi, om, prm = P, P + (1 << 22), P + (2 << 22), P + (3 << 22), P + (4 << 22)
    for args, msg in [((image, None, 2, 16, prm, prm, prm, oi, om, None), "null pointer"),
                      ((image, mask, 0, 16, prm, prm, prm, oi, om, None), "batch"),
                      ((image, mask, 2, 0, prm, prm, prm, oi, om, None), "size"),
                      ((image, mask, 2, 4097, prm, prm, prm, oi, om, None), "size"),
                      ((image, mask, 2, 16, prm, prm, prm, image, om, None), "overlap"),
                      ((image, mask, 2, 16, prm, prm, prm, oi, mask, None), "overlap"),
                      ((image, mask, 2, 16, prm, prm, prm, image + 2 * 3 * 16 * 16 * 4 - 4, om, None), "overlap"),
                      ((image, mask, 2, 16, prm, prm, prm, oi, oi + 64, None), "overlap")]:
        assert lib.aaclip_augment_geometric(*args) == -1
        assert err().startswith("augment_geometric:") and msg in err(), (err(), msg)


def test_nearest_table_is_pillows():
    """The index map of Image.resize(NEAREST), read off a ramp image, for every axis the GPU tests use and more"""
    for n_in, n_out in [(37, 28), (53, 28), (20, 56), (28, 28), (96, 70), (80, 70), (12, 10), (1024, 518), (1, 5), (5, 1)]:
        ramp = np.arange(n_in)
        lo = Image.fromarray((ramp % 256).astype(np.uint8)[None, :].repeat(2, 0))
        hi = Image.fromarray((ramp // 256).astype(np.uint8)[None, :].repeat(2, 0))
        want = (np.asarray(lo.resize((n_out, 2), Image.NEAREST))[0].astype(int)
                + 256 * np.asarray(hi.resize((n_out, 2), Image.NEAREST))[0].astype(int))
        assert np.array_equal(engine.nearest_table(n_in, n_out).numpy(), want), (n_in, n_out)
    lib = _lib.load()
    buf = (ctypes.c_int32 * 4)()
    assert lib.aaclip_nearest_table(0, 4, ctypes.addressof(buf)) == -1 and "nearest_table" in err()
    assert lib.aaclip_nearest_table(4, 4, None) == -1


def test_wrappers_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.color_jitter(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.ones(1, 3), torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.mask_preprocess(torch.zeros(1, 4, 4, dtype=torch.uint8), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.augment_geometric(torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1), torch.zeros(1, 2),
                                 torch.zeros(1))


# ---------------------------------------------------------------------------------------- the host transform
@pytest.mark.parametrize("name", AC.COLOR_CASES)
def test_host_colour_is_image_enhance(name):
    c = AC.color_case(name)
    want = AC.color_reference(name)
    for b in range(len(c["src"])):
        got = D.jitter_image(Image.fromarray(c["src"][b]), c["factors"][b], int(c["apply"][b]))
        assert np.array_equal(np.asarray(got), want[b]), (name, b)


def test_rotated_cases_respect_the_cap():
    for name in AC.ROTATED_CASES:
        band = AC.geo_case(name)[7]
        assert float(band.float().mean()) <= AC.BAND_CAP, name
        for b in range(band.shape[0]):
            assert float(band[b].float().mean()) <= AC.BAND_CAP, (name, b)
    for name in AC.EXACT_CASES:
        S, frames = AC.EXACT_CASES[name]
        for b, (angle, shift, flags) in enumerate(frames):
            if flags & AC.ROTATE:                     # right angles never come near a boundary
                assert not AC.geo_case(name)[7][b].any(), (name, b)


@pytest.mark.parametrize("name", list(AC.EXACT_CASES) + list(AC.ROTATED_CASES))
def test_host_geometry_is_the_torch_path(name):
    image, mask, angle, shift, flags, want_image, want_mask, band = AC.geo_case(name)
    for b in range(image.shape[0]):
        got = D.geometric_transform(torch.cat([image[b], mask[b]]), float(angle[b]), shift[b].tolist(), int(flags[b]))
        assert torch.equal(got[0:3], want_image[b]) and torch.equal(got[3:4], want_mask[b])


def test_rotation_matches_the_fp64_formula_and_rot90():
    """The fp32 torch path against the fp64 source index, outside the band; +90 degrees is rot90(k=1)"""
    for name in AC.ROTATED_CASES:
        image, mask, angle, shift, flags, want_image, _, band = AC.geo_case(name)
        S = image.shape[-1]
        th = math.radians(float(angle[0]))            # frame 0 of every rotated case is the rotation alone
        y, x = torch.meshgrid(torch.arange(S, dtype=torch.float64), torch.arange(S, dtype=torch.float64), indexing="ij")
        xc, yc = x + 0.5 - S / 2, y + 0.5 - S / 2
        xs = torch.round(math.cos(th) * xc - math.sin(th) * yc + S / 2 - 0.5).long()
        ys = torch.round(math.sin(th) * xc + math.cos(th) * yc + S / 2 - 0.5).long()
        inside = (xs >= 0) & (xs < S) & (ys >= 0) & (ys < S)
        formula = torch.where(inside, image[0][:, ys.clamp(0, S - 1), xs.clamp(0, S - 1)], torch.zeros(()))
        differ = (formula != want_image[0]).any(dim=0)
        assert not (differ & ~band[0]).any(), name
    t = AC.geo_inputs(16, 1)[0][0]
    assert torch.equal(D.geometric_transform(t, 90.0, (0, 0), D.GEO_ROTATE), torch.rot90(t, 1, (1, 2)))
    assert torch.equal(D.geometric_transform(t, 0.0, (2, -3), D.GEO_SHIFT)[:, :-3, 2:], t[:, 3:, :-2])


def test_train_transform_is_resize_of_the_jittered_image():
    src = AC.frames("tt", 1, 96, 80)[0]
    m = np.zeros((96, 80), np.uint8)
    m[10:40, 20:50] = 255
    params = {"color_factors": torch.tensor([[1.3, 0.7, 1.2]]), "color_apply": torch.tensor([7], dtype=torch.int32),
              "angle": torch.tensor([0.0]), "shift": torch.tensor([[0, 0]], dtype=torch.int32),
              "flags": torch.tensor([D.GEO_HFLIP], dtype=torch.int32)}
    image, mask = D.train_transform(Image.fromarray(src), Image.fromarray(m), params, 70)
    jit = AC.enhance(Image.fromarray(src), [1.3, 0.7, 1.2], 7)
    assert torch.equal(image, D.transform_image(jit, 70).flip(-1))
    assert torch.equal(mask, D.transform_mask(Image.fromarray(m), 70).flip(-1))
    assert set(mask.unique().tolist()) <= {0.0, 1.0}
    image, mask = D.train_transform(Image.fromarray(src), None, params, 70)
    assert mask.shape == (1, 70, 70) and not mask.any()


# --------------------------------------------------------------------------------------- draw_augment_params
def test_draw_ranges_flags_and_repeat():
    n, S = 4000, 518
    a = D.draw_augment_params(torch.Generator().manual_seed(5), n, S, False)
    b = D.draw_augment_params(torch.Generator().manual_seed(5), n, S, False)
    assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == {"color_factors", "color_apply", "angle", "shift", "flags"}
    c = D.draw_augment_params(torch.Generator().manual_seed(6), n, S, False)
    assert not torch.equal(a["angle"], c["angle"])
    assert a["color_factors"].dtype == torch.float32 and a["color_factors"].shape == (n, 3)
    assert a["color_apply"].dtype == a["flags"].dtype == a["shift"].dtype == torch.int32 and a["shift"].shape == (n, 2)
    assert a["color_factors"].min() >= 0.5 and a["color_factors"].max() <= 1.5
    assert a["angle"].dtype == torch.float32 and a["angle"].abs().max() <= 30.0 + 1e-4 and a["angle"].abs().max() > 29
    m = int(round(0.15 * S))
    assert a["shift"].abs().max() <= m and a["shift"].min() < -m + 5 and a["shift"].max() > m - 5
    assert a["color_apply"].min() >= 0 and a["color_apply"].max() <= 7 and a["flags"].min() >= 0 and a["flags"].max() <= 15
    # empirical probabilities inside a 5-sigma binomial band
    for bits, p, word in [((1, 2, 4), 0.7, a["color_apply"]), ((1, 2, 4, 8), 0.5, a["flags"])]:
        for bit in bits:
            k = int(((word & bit) != 0).sum())
            assert abs(k - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (bit, k)
    t = D.draw_augment_params(torch.Generator().manual_seed(5), n, S, True)
    assert not t["color_apply"].any() and torch.equal(t["color_factors"], torch.ones(n, 3))
    assert t["flags"].any()


# ----------------------------------------------------------------------------------------------- the datasets
@pytest.fixture()
def tree(tmp_path, monkeypatch):
    """bottle at 96x96 and grid at 64x80, six samples each, with full-shot and 2-shot metadata"""
    root = write_tree(str(tmp_path / "MVTec"), classes=("bottle",), size=(96, 96))
    write_tree(root, classes=("grid",), size=(64, 80), seed=5)
    meta = tmp_path / "meta"
    n = D.build_metadata(root, str(meta / "MVTec" / "full-shot.jsonl"))
    assert n == 12
    rows = open(meta / "MVTec" / "full-shot.jsonl").read().splitlines()
    with open(meta / "MVTec" / "2-shot.jsonl", "w") as f:
        f.write("\n".join(rows[:2] + rows[-2:]) + "\n")
    monkeypatch.setitem(D.DATA_PATH, "MVTec", root)
    monkeypatch.setattr(D, "METADATA_ROOT", str(meta))
    return root


def test_get_train_datasets(tree):
    text, image = D.get_train_datasets("MVTec", 70, "full_shot", -1)
    assert len(text) == len(image) == 12 and text.text and not image.text and text.full_shot
    few_text, few_image = D.get_train_datasets("MVTec", 70, "few_shot", 2)
    assert len(few_text) == len(few_image) == 4 and not few_image.full_shot and few_image.shot == 2
    with pytest.raises(AssertionError):
        D.get_train_datasets("MVTec", 70, "few_shot", 0)
    with pytest.raises(AssertionError):
        D.get_train_datasets("nope", 70, "full_shot", -1)
    image.generator = torch.Generator().manual_seed(3)
    it = image[7]
    assert set(it) == {"image", "mask", "label", "file_name", "class_name"}
    assert it["image"].shape == (3, 70, 70) and it["image"].dtype == torch.float32 and it["mask"].shape == (1, 70, 70)
    assert int(it["label"]) == 1 and it["mask"].any()
    assert it["label"].dtype == torch.int64 and it["label"].dim() == 0 and set(it["mask"].unique().tolist()) <= {0.0, 1.0}
    # the item is train_transform of the decoded files for the numbers the generator gives
    params = D.draw_augment_params(torch.Generator().manual_seed(3), 1, 70, False)
    meta = image.meta[7]
    want = D.train_transform(Image.open(os.path.join(tree, meta["image_path"])).convert("RGB"),
                             Image.open(os.path.join(tree, meta["mask_path"])).convert("L") if meta["label"] else None,
                             params, 70)
    assert torch.equal(it["image"], want[0]) and torch.equal(it["mask"], want[1])
    loader = torch.utils.data.DataLoader(text, batch_size=5)          # the default collate serves the host mode
    batch = next(iter(loader))
    assert batch["image"].shape == (5, 3, 70, 70) and batch["label"].shape == (5,) and len(batch["class_name"]) == 5


def test_collate_raw_groups_by_frame_size(tree):
    _, image = D.get_train_datasets("MVTec", 70, "full_shot", -1, device_augment=True)
    image.generator = torch.Generator().manual_seed(3)
    order = [3, 9, 0, 6, 1, 10]                        # bottle good, grid good, bottle bad, grid bad, bottle bad, grid good
    items = [image[i] for i in order]
    assert items[0]["image"].dtype == torch.uint8 and items[0]["image"].shape == (96, 96, 3) and items[0]["mask"] is None
    assert items[3]["mask"].dtype == torch.uint8 and items[3]["mask"].shape == (64, 80)
    raw = D.collate_raw(items)
    assert raw["img_size"] == 70 and raw["class_name"] == [image.meta[i]["class_name"] for i in order]
    assert torch.equal(raw["label"], torch.tensor([image.meta[i]["label"] for i in order]))
    assert len(raw["groups"]) == 2
    seen = []
    for g in raw["groups"]:
        idx = g["index"].tolist()
        seen += idx
        n = len(idx)
        assert g["frames"].shape[0] == g["masks"].shape[0] == n and g["normal"].dtype == torch.int32
        assert g["frames"].shape[1:3] == g["masks"].shape[1:]
        for row, i in enumerate(idx):
            assert torch.equal(g["frames"][row], items[i]["image"])
            assert bool(g["normal"][row]) == (items[i]["mask"] is None)
            if items[i]["mask"] is not None:
                assert torch.equal(g["masks"][row], items[i]["mask"])
            for k, v in g["params"].items():
                assert v.shape[0] == n and torch.equal(v[row], items[i]["params"][k][0])
    assert sorted(seen) == list(range(6))
    only_normal = D.collate_raw([items[0], items[1]])
    assert len(only_normal["groups"]) == 2 and all(g["masks"].shape[1:] == (1, 1) for g in only_normal["groups"])


def test_get_dataset_train_still_raises(tree):
    with pytest.raises(NotImplementedError):
        D.get_dataset("MVTec", 70, "full_shot", -1, "train")


# -------------------------------------------------------------------------------------------------- the parser
REFERENCE_DEFAULTS = {
    "model_name": "ViT-L-14-336", "img_size": 518, "surgery_until_layer": 20, "relu": False, "dataset": "VisA",
    "training_mode": "few_shot", "shot": 32, "text_batch_size": 16, "image_batch_size": 2, "text_epoch": 5,
    "image_epoch": 20, "text_lr": 0.00001, "image_lr": 0.0005, "criterion": ["dice_loss", "focal_loss"], "seed": 111,
    "save_path": "ckpt/baseline", "text_norm_weight": 0.1, "text_adapt_weight": 0.1, "image_adapt_weight": 0.1,
    "text_adapt_until": 3, "image_adapt_until": 6, "iqm_hidden_size": 512, "iqm_num_layers": 2, "iqm_num_heads": 8,
    "iqm_weight": 0.4,
}


def test_parser_defaults_are_the_references():
    import train
    got = vars(train.build_parser().parse_args([]))
    assert got.pop("device_augment") is False
    assert got == REFERENCE_DEFAULTS
    args = train.build_parser().parse_args(["--device_augment", "--training_mode", "full_shot", "--relu"])
    assert args.device_augment and args.relu and args.training_mode == "full_shot"
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--training_mode", "zero_shot"])
    assert train.NUM_WORKERS == 4 and callable(train.main) and callable(train.run)
