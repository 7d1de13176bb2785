"""Datasets with the reference's names and item layout (reference dataset/__init__.py).

Test time (reference :123-272): BaseSingleClassDataset and get_dataset, stages "test" / "visualize".
Train time (reference :13-121, :224-238): BaseDataset and get_train_datasets (get_dataset keeps refusing stage
"train").  torchvision is not needed: both transforms are spelled out with Pillow and torch --
  image  [ColorJitter(brightness) / (contrast) / (saturation), each with p = 0.7, only when text=False]
         -> Resize((S,S), BICUBIC) -> ToTensor -> Normalize
  mask   Resize((S,S), NEAREST) -> ToTensor -> != 0 (all zeros for a normal sample)
  both   RandomRotation(+-30 deg, p = 0.5) -> RandomAffine(translate 0.15, p = 0.5) -> RandomHorizontalFlip
         -> RandomVerticalFlip on the [4,S,S] tensor: nearest sampling, zero fill
The random numbers of one sample are drawn by draw_augment_params (the reference's probabilities and ranges; its
stream inside the DataLoader workers cannot be reproduced) and then APPLIED by train_transform on the host, or, with
`device_augment=True`, by the HIP kernels: the dataset then returns the raw uint8 frame, the raw mask and the drawn
numbers, `collate_raw` groups a batch by frame size and `device_batch` runs aaclip_hip.engine.train_preprocess per
group.  For the same numbers the two agree (see the tests).

`device_preprocess=True` (test time) returns the decoded image as uint8 [H,W,3] instead, so that the caller
runs `aaclip_hip.engine.preprocess` on the GPU (bit-identical result, see tests); images of one
class must then share a size for the default DataLoader collate (true for MVTec-AD).
The reference also attaches a random normal "prompt_image" to anomalous samples
(dataset/__init__.py:112-119, :196-203); nothing in the reference reads it, so it is not produced here.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from PIL import Image
from torch.nn.functional import grid_sample
from torch.utils.data import Dataset

from .constants import CLASS_NAMES, DATA_PATH, DOMAINS  # noqa: F401

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
METADATA_ROOT = os.environ.get("AACLIP_METADATA_ROOT", "./dataset/metadata")


def transform_image(img: Image.Image, img_size: int) -> torch.Tensor:
    """Resize((S,S), BICUBIC) -> ToTensor -> Normalize (reference dataset/__init__.py:150-161)."""
    arr = np.asarray(img.resize((img_size, img_size), Image.BICUBIC))
    t = torch.from_numpy(arr.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return t.sub_(torch.tensor(CLIP_MEAN).view(-1, 1, 1)).div_(torch.tensor(CLIP_STD).view(-1, 1, 1))


def transform_mask(mask: Image.Image, img_size: int) -> torch.Tensor:
    """Resize NEAREST -> ToTensor -> (!= 0) (reference dataset/__init__.py:162-167,186-189) -> [1,S,S]."""
    arr = np.asarray(mask.resize((img_size, img_size), Image.NEAREST))
    return (torch.from_numpy(arr.copy()).to(torch.float32).div(255).unsqueeze(0) != 0).float()


class BaseSingleClassDataset(Dataset):
    def __init__(self, data_path: str, meta_path: str, img_size: int, class_name: str, logger=None, shot: int = -1,
                 device_preprocess: bool = False):
        assert class_name is not None, "class_name should be provided"
        self.data_path = data_path
        self.img_size = img_size
        self.shot = shot
        self.device_preprocess = device_preprocess
        self.full_shot = "full-shot" in meta_path
        self.meta, self.normal_meta = [], []
        with open(meta_path, "r") as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                m = json.loads(line)
                if m["class_name"] == class_name:
                    self.meta.append(m)
                    if m["label"] == 0:
                        self.normal_meta.append(m)
        if logger:
            logger.info(f"Class name: {class_name}")
            logger.info(f"Sample number: {len(self.meta)}")
            logger.info("=====================================")

    def __len__(self):
        return len(self.meta)

    def _with_meta(self, meta):
        """a dataset of the same settings over the given entries"""
        import copy
        other = copy.copy(self)
        other.meta = list(meta)
        other.normal_meta = [m for m in other.meta if m["label"] == 0]
        return other

    def support_split(self, k: int):
        """-> (support_dataset, eval_dataset) of the k-shot protocol: the support set is the first k entries of
        normal_meta in file order, and those images are REMOVED from the evaluated set (a test image that is in the
        bank has distance 0 to itself); the other entries keep their order.  k larger than the number of normal images
        (or below 1) raises ValueError."""
        if not 1 <= int(k) <= len(self.normal_meta):
            raise ValueError(f"support_split: k = {k}, but the class has {len(self.normal_meta)} normal images")
        support = self.normal_meta[:int(k)]
        taken = {id(m) for m in support}
        return self._with_meta(support), self._with_meta([m for m in self.meta if id(m) not in taken])

    def __getitem__(self, idx):
        meta = self.meta[idx]
        img = Image.open(os.path.join(self.data_path, meta["image_path"])).convert("RGB")
        if self.device_preprocess:
            image = torch.from_numpy(np.asarray(img).copy())
        else:
            image = transform_image(img, self.img_size)
        if meta["label"]:
            mask = transform_mask(Image.open(os.path.join(self.data_path, meta["mask_path"])).convert("L"),
                                  self.img_size)
        else:
            mask = torch.zeros([1, self.img_size, self.img_size])
        return {"image": image, "mask": mask, "label": meta["label"], "file_name": meta["image_path"],
                "class_name": meta["class_name"]}


def get_dataset(dataset_name: str, img_size: int, training_mode: Optional[str], shot: int = -1, stage: str = "train",
                logger=None, device_preprocess: bool = False) -> Dict[str, BaseSingleClassDataset]:
    """reference dataset/__init__.py:208-272; stages "test" and "visualize" (one dataset per class)."""
    if "Med" not in dataset_name:
        assert dataset_name in DATA_PATH, (
            f"Dataset {dataset_name} not found; available datasets: {list(DATA_PATH.keys())}")
    if stage not in ("test", "visualize"):
        raise NotImplementedError(
            "only the inference datasets are part of the MI355X path; training datasets (stage='train') are not")
    meta_path = os.path.join(METADATA_ROOT, dataset_name, "full-shot.jsonl")
    return {c: BaseSingleClassDataset(DATA_PATH[dataset_name], meta_path, img_size, c, logger=logger, shot=shot,
                                      device_preprocess=device_preprocess)
            for c in CLASS_NAMES[dataset_name]}


# ---------------------------------------------------------------------------------------------- train time
COLOR_P, GEOMETRY_P = 0.7, 0.5                   # RandomApply / flip probabilities (reference :38-58)
COLOR_RANGE = (0.5, 1.5)                         # ColorJitter(x=0.5): factor from U[max(0, 1 - 0.5), 1 + 0.5]
MAX_ANGLE = math.degrees(math.pi / 6)            # RandomRotation(degrees=30)
TRANSLATE = 0.15                                 # RandomAffine(translate=(0.15, 0.15))
COLOR_BRIGHTNESS, COLOR_CONTRAST, COLOR_SATURATION = 1, 2, 4      # bits of "color_apply"
GEO_ROTATE, GEO_SHIFT, GEO_HFLIP, GEO_VFLIP = 1, 2, 4, 8          # bits of "flags"


def draw_augment_params(generator: Optional[torch.Generator], n: int, img_size: int,
                        text: bool) -> Dict[str, torch.Tensor]:
    """The random numbers of n samples, with the reference's probabilities and ranges, in the layout the kernels take:
        color_factors fp32 [n,3]  brightness, contrast, saturation factor, each from U[0.5, 1.5]
        color_apply   int32 [n]   bit 0 / 1 / 2: that step runs (p = 0.7 each; never when text=True)
        angle         fp32 [n]    degrees from U[-30, 30], counter-clockwise
        shift         int32 [n,2] (tx, ty) = round(U(-0.15 S, 0.15 S))
        flags         int32 [n]   GEO_ROTATE | GEO_SHIFT | GEO_HFLIP | GEO_VFLIP, p = 0.5 each
    Every number is drawn whether or not its step runs, so the stream does not depend on the outcomes.
    generator None: torch's global generator (seeded per DataLoader worker), as torchvision uses it."""
    def uniform(shape, lo, hi):
        return torch.empty(shape, dtype=torch.float32).uniform_(lo, hi, generator=generator)

    def coin(p):
        return torch.rand(n, generator=generator) < p

    color_apply = torch.zeros(n, dtype=torch.int32)
    color_factors = uniform((n, 3), *COLOR_RANGE)
    for bit in (COLOR_BRIGHTNESS, COLOR_CONTRAST, COLOR_SATURATION):
        on = coin(COLOR_P)
        if not text:
            color_apply |= on.to(torch.int32) * bit
    if text:
        color_factors = torch.ones(n, 3, dtype=torch.float32)
    flags = torch.zeros(n, dtype=torch.int32)
    angle = uniform((n,), -MAX_ANGLE, MAX_ANGLE)
    flags |= coin(GEOMETRY_P).to(torch.int32) * GEO_ROTATE
    shift = torch.round(uniform((n, 2), -TRANSLATE * img_size, TRANSLATE * img_size)).to(torch.int32)
    for bit in (GEO_SHIFT, GEO_HFLIP, GEO_VFLIP):
        flags |= coin(GEOMETRY_P).to(torch.int32) * bit
    return {"color_factors": color_factors, "color_apply": color_apply, "angle": angle, "shift": shift, "flags": flags}


def jitter_image(img: Image.Image, factors, apply: int) -> Image.Image:
    """ColorJitter's three steps on a PIL RGB image for given factors: ImageEnhance.{Brightness, Contrast, Color} is
    Image.blend(degenerate, image, factor) with the degenerate black, the constant int(mean(L) + 0.5), and L."""
    if apply & COLOR_BRIGHTNESS:
        img = Image.blend(Image.new("RGB", img.size, 0), img, float(factors[0]))
    if apply & COLOR_CONTRAST:
        grey = np.asarray(img.convert("L"), dtype=np.int64)
        mean = int(int(grey.sum()) / grey.size + 0.5)
        img = Image.blend(Image.new("L", img.size, mean).convert("RGB"), img, float(factors[1]))
    if apply & COLOR_SATURATION:
        img = Image.blend(img.convert("L").convert("RGB"), img, float(factors[2]))
    return img


def _affine_sample(t: torch.Tensor, matrix) -> torch.Tensor:
    """torchvision's tensor affine for an inverse matrix [a, b, c, d, e, f] about the centre: fp32 base grid of pixel
    centres, one product with the matrix scaled to grid_sample's [-1, 1] coordinates, nearest sampling, zero fill."""
    _, h, w = t.shape
    theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
    base = torch.empty(1, h, w, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-w * 0.5 + 0.5, w * 0.5 + 0.5 - 1, steps=w))
    base[..., 1].copy_(torch.linspace(-h * 0.5 + 0.5, h * 0.5 + 0.5 - 1, steps=h).unsqueeze(-1))
    base[..., 2].fill_(1)
    grid = base.view(1, h * w, 3).bmm(theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h])).view(1, h, w, 2)
    return grid_sample(t.unsqueeze(0), grid, mode="nearest", padding_mode="zeros", align_corners=False)[0]


def geometric_transform(t: torch.Tensor, angle: float, shift, flags: int) -> torch.Tensor:
    """The reference's four random transforms on a [C,S,S] tensor for given numbers, one after the other."""
    if flags & GEO_ROTATE:
        rot = math.radians(angle)                # counter-clockwise; the inverse map rotates the output grid back
        t = _affine_sample(t, [math.cos(rot), -math.sin(rot), 0.0, math.sin(rot), math.cos(rot), 0.0])
    if flags & GEO_SHIFT:
        t = _affine_sample(t, [1.0, 0.0, -float(shift[0]), 0.0, 1.0, -float(shift[1])])
    if flags & GEO_HFLIP:
        t = t.flip(-1)
    if flags & GEO_VFLIP:
        t = t.flip(-2)
    return t


def train_transform(img: Image.Image, mask: Optional[Image.Image], params: Dict[str, torch.Tensor], img_size: int,
                    i: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Sample i of `params` applied on the host -> (image [3,S,S], mask [1,S,S]); mask None: a normal sample."""
    img = jitter_image(img, params["color_factors"][i].tolist(), int(params["color_apply"][i]))
    image = transform_image(img, img_size)
    m = transform_mask(mask, img_size) if mask is not None else torch.zeros([1, img_size, img_size])
    both = geometric_transform(torch.cat([image, m], dim=0), float(params["angle"][i]), params["shift"][i].tolist(),
                               int(params["flags"][i]))
    return both[0:3], both[3:4]


class BaseDataset(Dataset):
    """reference dataset/__init__.py:13-121: every row of the metadata file, all classes together."""

    def __init__(self, data_path: str, meta_path: str, img_size: int, text: bool = False, shot: int = -1,
                 device_augment: bool = False, generator: Optional[torch.Generator] = None):
        self.data_path = data_path
        self.img_size = img_size
        self.text = text
        self.shot = shot
        self.device_augment = device_augment
        self.generator = generator
        self.full_shot = "full-shot" in meta_path
        self.meta, self.normal_meta = [], []
        with open(meta_path, "r") as f:
            for line in f:
                if not line.strip():
                    continue
                m = json.loads(line)
                self.meta.append(m)
                if m["label"] == 0:
                    self.normal_meta.append(m)

    def __len__(self):
        return len(self.meta)

    def __getitem__(self, idx):
        meta = self.meta[idx]
        img = Image.open(os.path.join(self.data_path, meta["image_path"])).convert("RGB")
        mask = Image.open(os.path.join(self.data_path, meta["mask_path"])).convert("L") if meta["label"] else None
        params = draw_augment_params(self.generator, 1, self.img_size, self.text)
        item = {"label": torch.tensor(meta["label"]).to(torch.int64), "file_name": meta["image_path"],
                "class_name": meta["class_name"]}
        if self.device_augment:
            item.update(image=torch.from_numpy(np.asarray(img).copy()),
                        mask=None if mask is None else torch.from_numpy(np.asarray(mask).copy()),
                        params=params, img_size=self.img_size)
        else:
            item["image"], item["mask"] = train_transform(img, mask, params, self.img_size)
        return item


def collate_raw(items: List[dict]) -> dict:
    """collate_fn for `device_augment=True` items: frames of one size are stacked into one group (a batch of a mixed
    dataset holds several sizes).  A group is {"index": positions in the batch, "frames" uint8 [n,H,W,3], "masks" uint8
    [n,Hm,Wm], "normal" int32 [n], "params": the drawn numbers, stacked}; a normal sample has no mask file, so its row
    of "masks" is zeros and its "normal" entry is set.  Anomalous samples of one frame size whose masks differ in size
    go to separate groups."""
    groups: Dict[tuple, List[int]] = {}
    for i, it in enumerate(items):
        if it["mask"] is not None:
            groups.setdefault(tuple(it["image"].shape[:2]) + tuple(it["mask"].shape), []).append(i)
    for i, it in enumerate(items):
        if it["mask"] is None:
            hw = tuple(it["image"].shape[:2])
            key = next((k for k in groups if k[:2] == hw), hw + (1, 1))
            groups.setdefault(key, []).append(i)
    out = []
    for key, index in groups.items():
        index = sorted(index)
        masks = torch.zeros((len(index),) + key[2:], dtype=torch.uint8)
        for row, i in enumerate(index):
            if items[i]["mask"] is not None:
                masks[row] = items[i]["mask"]
        out.append({"index": torch.tensor(index), "frames": torch.stack([items[i]["image"] for i in index]),
                    "masks": masks,
                    "normal": torch.tensor([items[i]["mask"] is None for i in index], dtype=torch.int32),
                    "params": {k: torch.cat([items[i]["params"][k] for i in index]) for k in items[0]["params"]}})
    return {"groups": out, "img_size": items[0]["img_size"], "label": torch.stack([it["label"] for it in items]),
            "file_name": [it["file_name"] for it in items], "class_name": [it["class_name"] for it in items]}


def device_batch(raw_batch: dict, device) -> dict:
    """A collate_raw batch -> the {"image", "mask", "label", "class_name"} batch of the train loops, image and mask on
    `device` and in the batch's original order: aaclip_hip.engine.train_preprocess once per group."""
    from aaclip_hip import engine
    S, n = raw_batch["img_size"], len(raw_batch["class_name"])
    image = torch.empty(n, 3, S, S, dtype=torch.float32, device=device)
    mask = torch.empty(n, 1, S, S, dtype=torch.float32, device=device)
    for g in raw_batch["groups"]:
        im, mk = engine.train_preprocess(g["frames"].to(device), g["masks"].to(device), g["normal"].to(device),
                                         g["params"], S)
        index = g["index"].to(device)
        image[index] = im
        mask[index] = mk
    return {"image": image, "mask": mask, "label": raw_batch["label"], "class_name": raw_batch["class_name"],
            "file_name": raw_batch["file_name"]}


class DeviceAugmentLoader:
    """Wraps a DataLoader over a `device_augment=True` dataset (collate_fn=collate_raw): iterating yields device_batch
    of every raw batch."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, device

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for raw in self.loader:
            yield device_batch(raw, self.device)


def get_train_datasets(dataset_name: str, img_size: int, training_mode: Optional[str], shot: int, logger=None,
                       device_augment: bool = False) -> Tuple[BaseDataset, BaseDataset]:
    """reference dataset/__init__.py:224-238 (its get_dataset with stage "train") -> (text_dataset, image_dataset): the
    same rows, without and with the colour jitter."""
    if "Med" not in dataset_name:
        assert dataset_name in DATA_PATH, (
            f"Dataset {dataset_name} not found; available datasets: {list(DATA_PATH.keys())}")
    if training_mode == "few_shot":
        assert shot > 0, "shot should be positive"
        meta_path = os.path.join(METADATA_ROOT, dataset_name, f"{shot}-shot.jsonl")
    else:
        meta_path = os.path.join(METADATA_ROOT, dataset_name, "full-shot.jsonl")
    data_path = DATA_PATH[dataset_name.split("-")[0]]
    if logger:
        logger.info(f"train metadata: {meta_path}")
    return (BaseDataset(data_path, meta_path, img_size, text=True, shot=shot, device_augment=device_augment),
            BaseDataset(data_path, meta_path, img_size, text=False, shot=shot, device_augment=device_augment))


def build_metadata(data_path: str, out_path: str, class_names=None) -> int:
    """Write a full-shot.jsonl for an MVTec-AD style tree (<class>/test/<defect>/*.png with masks under
    <class>/ground_truth/<defect>/<stem>_mask.png; 'good' = normal).  Returns the number of rows.
    (The reference ships pre-made metadata files; this regenerates the same row format.)"""
    rows = []
    for c in sorted(class_names or os.listdir(data_path)):
        tdir = os.path.join(data_path, c, "test")
        if not os.path.isdir(tdir):
            continue
        for defect in sorted(os.listdir(tdir)):
            for fn in sorted(os.listdir(os.path.join(tdir, defect))):
                stem, ext = os.path.splitext(fn)
                if ext.lower() not in (".png", ".jpg", ".jpeg", ".bmp"):
                    continue
                good = defect == "good"
                rows.append({"image_path": f"{c}/test/{defect}/{fn}", "label": 0 if good else 1,
                             "mask_path": "" if good else f"{c}/ground_truth/{defect}/{stem}_mask.png",
                             "class_name": c})
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return len(rows)
