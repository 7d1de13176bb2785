"""Cases and reference evaluators of the train-time input pipeline (csrc/augment.hip, dataset.BaseDataset).

References, none of which touches the code under test:
  colour    Pillow's own ImageEnhance.{Brightness, Contrast, Color}, what torchvision's ColorJitter calls on a PIL image
  mask      dataset.transform_mask (Pillow's NEAREST resize), the test-time yardstick
  geometry  torchvision's tensor path restated in fp32 torch, one transform after the other: a base grid of pixel
            centres, one bmm with the inverse matrix, grid_sample(nearest, zeros, align_corners=False); flips are
            torch.flip.  `boundary_band` marks, in fp64, the pixels whose rotation source coordinate lies within
            BAND of a half-integer: only there may two correct evaluations pick different neighbours.
Everything is computed once (lru_cache) and never modified."""
import functools
import math

import numpy as np
import torch
from PIL import Image, ImageEnhance
from torch.nn.functional import grid_sample

ROTATE, SHIFT, HFLIP, VFLIP = 1, 2, 4, 8
BAND = 1e-3            # distance of a source coordinate from a half-integer below which the neighbour is undecided
BAND_CAP = 0.02        # largest share of such pixels a rotated case may have


def rng(name):
    return np.random.default_rng(abs(hash_name(name)))


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (2 ** 31)
    return h


# ------------------------------------------------------------------------------------------------------ colour
def frames(name, B, H, W):
    r = rng("frames." + name)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        base = 128 + 90 * np.sin(xx / (3.0 + b) + r.uniform(0, 3)) * np.cos(yy / (4.0 + b))
        out[b] = np.clip(base[..., None] + r.integers(-60, 60, (H, W, 3)), 0, 255).astype(np.uint8)
    return out


def _color(name, src, factors, apply):
    return {"src": src, "factors": np.asarray(factors, np.float32).reshape(len(src), 3),
            "apply": np.asarray(apply, np.int32)}


@functools.lru_cache(maxsize=None)
def color_case(name):
    r = rng("color." + name)
    if name == "masks8_37x53":                         # every apply mask, random factors, rows of 159 bytes
        return _color(name, frames(name, 8, 37, 53), r.uniform(0.5, 1.5, (8, 3)), list(range(8)))
    if name == "b3_64x64":                             # three frames, different factors and masks
        return _color(name, frames(name, 3, 64, 64), [[0.5, 1.5, 1.0], [1.5, 0.5, 0.5], [1.0, 1.0, 1.5]], [7, 5, 6])
    if name == "edges_37x53":                          # the ends and the middle of the factor range, all steps
        f = [[0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [1.5, 1.5, 1.5]]
        return _color(name, frames(name, 3, 37, 53), f, [7, 7, 7])
    if name == "b3_1x1":                               # three frames inside one 16-pixel group
        return _color(name, frames(name, 3, 1, 1), r.uniform(0.5, 1.5, (3, 3)), [7, 3, 6])
    if name == "black_white":                          # an all-black and an all-255 frame, then an ordinary one
        src = frames(name, 3, 37, 53)
        src[0], src[1] = 0, 255
        return _color(name, src, [[1.5, 1.5, 1.5], [1.5, 0.5, 1.5], [0.7, 1.3, 0.6]], [7, 7, 7])
    if name == "random_64x64":
        return _color(name, frames(name, 4, 64, 64), r.uniform(0.5, 1.5, (4, 3)), [7, 7, 2, 7])
    if name == "beyond_range_19x23":                   # factors outside [0.5, 1.5]: the clipping branch of the blend
        return _color(name, frames(name, 3, 19, 23), [[0.0, 2.5, 3.0], [2.0, 0.0, 0.0], [1.9, 1.9, 1.9]], [7, 7, 7])
    if name == "strided_sum_520x517":                  # more groups than one pass of the luma sum's 64 workgroups
        return _color(name, frames(name, 2, 520, 517), [[1.2, 0.8, 1.1], [0.9, 1.4, 0.7]], [7, 6])
    raise KeyError(name)


COLOR_CASES = ["masks8_37x53", "b3_64x64", "edges_37x53", "b3_1x1", "black_white", "random_64x64",
               "beyond_range_19x23", "strided_sum_520x517"]


def enhance(img, factors, apply):
    """torchvision's three ColorJitter steps on a PIL image, through Pillow's ImageEnhance"""
    if apply & 1:
        img = ImageEnhance.Brightness(img).enhance(float(factors[0]))
    if apply & 2:
        img = ImageEnhance.Contrast(img).enhance(float(factors[1]))
    if apply & 4:
        img = ImageEnhance.Color(img).enhance(float(factors[2]))
    return img


@functools.lru_cache(maxsize=None)
def color_reference(name):
    c = color_case(name)
    return np.stack([np.asarray(enhance(Image.fromarray(c["src"][b]), c["factors"][b], int(c["apply"][b])))
                     for b in range(len(c["src"]))])


# -------------------------------------------------------------------------------------------------------- mask
@functools.lru_cache(maxsize=None)
def mask_case(name):
    """-> (masks uint8 [B,Hm,Wm], normal int32 [B], S)"""
    r = rng("mask." + name)

    def blobs(B, H, W):
        m = np.zeros((B, H, W), np.uint8)
        for b in range(B):
            y0, x0 = r.integers(0, max(1, H // 2)), r.integers(0, max(1, W // 2))
            m[b, y0:y0 + max(1, H // 3), x0:x0 + max(1, W // 3)] = r.choice([1, 128, 255])
            m[b][r.random((H, W)) < 0.05] = 255
        return m
    if name == "37x53_to_28":
        return blobs(3, 37, 53), np.zeros(3, np.int32), 28
    if name == "20x20_to_56":
        return blobs(2, 20, 20), np.zeros(2, np.int32), 56
    if name == "28_to_28":
        return blobs(2, 28, 28), np.zeros(2, np.int32), 28
    if name == "normal_between":                       # the flagged frame's source is full of ones and must not be read
        m = blobs(3, 37, 53)
        m[1] = 255
        return m, np.array([0, 1, 0], np.int32), 28
    if name == "corners":                              # the only non-zero pixel sits in a corner
        m = np.zeros((4, 37, 53), np.uint8)
        m[0, 0, 0] = m[1, 0, -1] = m[2, -1, 0] = m[3, -1, -1] = 1
        return m, np.zeros(4, np.int32), 28
    raise KeyError(name)


MASK_CASES = ["37x53_to_28", "20x20_to_56", "28_to_28", "normal_between", "corners"]


@functools.lru_cache(maxsize=None)
def mask_reference(name):
    import dataset as D
    masks, normal, S = mask_case(name)
    return torch.stack([torch.zeros(1, S, S) if normal[b] else D.transform_mask(Image.fromarray(masks[b]), S)
                        for b in range(len(masks))])


# ---------------------------------------------------------------------------------------------------- geometry
def affine_sample(t, matrix):
    """torchvision's tensor affine / rotate for the inverse matrix [a, b, c, d, e, f], about the centre, in fp32"""
    _, h, w = t.shape
    theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
    base = torch.empty(1, h, w, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-w * 0.5 + 0.5, w * 0.5 + 0.5 - 1, steps=w))
    base[..., 1].copy_(torch.linspace(-h * 0.5 + 0.5, h * 0.5 + 0.5 - 1, steps=h).unsqueeze(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h])
    grid = base.view(1, h * w, 3).bmm(rescaled).view(1, h, w, 2)
    return grid_sample(t.unsqueeze(0), grid, mode="nearest", padding_mode="zeros", align_corners=False)[0]


def rotation_matrix(angle):
    rot = math.radians(angle)
    return [math.cos(rot), -math.sin(rot), 0.0, math.sin(rot), math.cos(rot), 0.0]


def sequential(t, angle, shift, flags):
    """rotation, shift, horizontal flip, vertical flip of a [C,S,S] tensor, one after the other"""
    if flags & ROTATE:
        t = affine_sample(t, rotation_matrix(angle))
    if flags & SHIFT:
        t = affine_sample(t, [1.0, 0.0, -float(shift[0]), 0.0, 1.0, -float(shift[1])])
    if flags & HFLIP:
        t = t.flip(-1)
    if flags & VFLIP:
        t = t.flip(-2)
    return t


def boundary_band(S, angle, shift, flags):
    """bool [S,S]: output pixels of the whole sequence whose rotation source coordinate, in fp64, lies within BAND of
    a half-integer (none when the rotation is off)"""
    if not flags & ROTATE:
        return torch.zeros(S, S, dtype=torch.bool)
    th = math.radians(angle)
    y, x = torch.meshgrid(torch.arange(S, dtype=torch.float64), torch.arange(S, dtype=torch.float64), indexing="ij")
    xc, yc = x + 0.5 - S / 2, y + 0.5 - S / 2
    xs = math.cos(th) * xc - math.sin(th) * yc + S / 2 - 0.5
    ys = math.sin(th) * xc + math.cos(th) * yc + S / 2 - 0.5

    def near_half(v):
        return ((v - torch.floor(v)) - 0.5).abs() < BAND
    band = (near_half(xs) | near_half(ys)).float().unsqueeze(0)
    return sequential(band, 0.0, shift, flags & ~ROTATE)[0] != 0


def geo_inputs(S, B):
    """image fp32 [B,3,S,S] with all-distinct values (a wrong neighbour cannot go unnoticed), mask of 0 / 1"""
    r = rng(f"geo.{S}.{B}")
    image = torch.from_numpy(r.permutation(B * 3 * S * S).astype(np.float32).reshape(B, 3, S, S) / 64 - 7)
    mask = torch.from_numpy((r.random((B, 1, S, S)) < 0.4).astype(np.float32))
    return image, mask


def max_shift(S):
    return int(round(0.15 * S))


def _exact_cases():
    cases = {}
    for S in (16, 21):
        m = max_shift(S)
        # (angle, (tx, ty), flags) per frame; three frames per case
        cases[f"right_angles_{S}"] = (S, [(0.0, (0, 0), ROTATE), (90.0, (0, 0), ROTATE), (-90.0, (0, 0), ROTATE)])
        cases[f"half_turn_{S}"] = (S, [(180.0, (0, 0), ROTATE), (180.0, (1, -1), ROTATE | SHIFT | HFLIP),
                                       (90.0, (-1, 1), ROTATE | SHIFT | VFLIP)])
        cases[f"flips_{S}"] = (S, [(0.0, (0, 0), HFLIP), (0.0, (0, 0), VFLIP), (0.0, (0, 0), HFLIP | VFLIP)])
        cases[f"identity_{S}"] = (S, [(0.0, (0, 0), 0), (25.0, (3, 3), 0), (0.0, (0, 0), SHIFT)])
        cases[f"shifts_small_{S}"] = (S, [(0.0, (1, 0), SHIFT), (0.0, (0, -1), SHIFT), (0.0, (-1, 1), SHIFT)])
        cases[f"shifts_max_{S}"] = (S, [(0.0, (m, -m), SHIFT), (0.0, (-m, m), SHIFT), (0.0, (m, m), SHIFT | HFLIP)])
        cases[f"shifts_max_neg_{S}"] = (S, [(0.0, (-m, -m), SHIFT | VFLIP), (17.0, (m, 0), SHIFT),     # angle unused
                                            (0.0, (0, -m), SHIFT | HFLIP | VFLIP)])
        cases[f"rotate_without_shift_{S}"] = (S, [(90.0, (m, m), ROTATE), (-90.0, (m, m), ROTATE | HFLIP),
                                                  (180.0, (-m, m), ROTATE | VFLIP)])
        cases[f"all_four_{S}"] = (S, [(90.0, (m, -1), 15), (-90.0, (-1, m), 15), (180.0, (1, 1), 15)])
    return cases


def _rotated_cases():
    cases = {}
    per_size = {16: [30.0, -30.0, 17.3, -23.456], 21: [17.3, 7.0], 64: [30.0, -30.0, 17.3, -23.456, 7.0]}
    for S, angles in per_size.items():
        m = max_shift(S)
        combos = [ROTATE, ROTATE | SHIFT, ROTATE | HFLIP | VFLIP, 15, ROTATE | SHIFT | VFLIP]
        shifts = [(m, -2), (-3, m), (1, 1), (-m, -m), (2, -1)]
        for k, a in enumerate(angles):
            # each angle alone and with a shift and both flips
            cases[f"rot_{S}_{a}"] = (S, [(a, (0, 0), ROTATE), (a, shifts[k], 15), (a, shifts[(k + 1) % 5], combos[k])])
    return cases


EXACT_CASES = _exact_cases()
ROTATED_CASES = _rotated_cases()


@functools.lru_cache(maxsize=None)
def geo_case(name):
    """-> (image, mask, angle fp32 [B], shift int32 [B,2], flags int32 [B], want_image, want_mask, band bool [B,S,S])"""
    S, frames_ = (EXACT_CASES if name in EXACT_CASES else ROTATED_CASES)[name]
    B = len(frames_)
    image, mask = geo_inputs(S, B)
    want = [sequential(torch.cat([image[b], mask[b]]), *frames_[b]) for b in range(B)]
    band = torch.stack([boundary_band(S, *frames_[b]) for b in range(B)])
    return (image, mask, torch.tensor([f[0] for f in frames_], dtype=torch.float32),
            torch.tensor([f[1] for f in frames_], dtype=torch.int32),
            torch.tensor([f[2] for f in frames_], dtype=torch.int32),
            torch.stack([w[0:3] for w in want]), torch.stack([w[3:4] for w in want]), band)


def compare_geometry(got_image, got_mask, want_image, want_mask, band):
    """-> (pixels that differ outside the band, pixels that differ inside it, share of band pixels)"""
    diff = ((got_image != want_image).any(dim=1) | (got_mask != want_mask).any(dim=1))
    return int((diff & ~band).sum()), int((diff & band).sum()), float(band.float().mean())
