"""Joint augmentation on the device: random crop, horizontal flip, colour jitter (image only) and a random affine map (image
and mask), in the order of the reference's JointTransform2D.__call__ (utils.py:70-98), which does them per item with
torchvision on the host -- and, not in the reference, U-Net's elastic deformation: a cubic B-spline free-form deformation
over a coarse grid of random displacements (`draw_field`), applied in front of the affine map, the image sampled bilinearly.

The host only DRAWS: `draw_record` turns the random numbers of one item into a record of `ops.augment_param_floats()` floats
(layout: include/medt_abi.h), `RawJointTransform2D` hands the dataset's decoded uint8 image and mask on untouched together
with that record, and `DeviceAugment` runs the two kernels (`ops.augment_batch`) on the uploaded uint8 batch.  What crosses
PCIe is the uint8 image, a quarter of the float32 batch the host transform builds.

Random streams: crop origin from torch.randint, flip from np.random.rand() -- the calls, in the order, of
medt_amd.data.JointTransform2D, so `--aug on` without jitter and affine sees the batches `--aug off` sees.  Jitter factors,
their order and the affine parameters follow from np.random (train.py seeds it); torchvision draws them from generators this
project does not have, so only the distributions are the reference's, not the streams.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops

PARAM_FLOATS = 20                     # == ops.augment_param_floats() (checked by DeviceAugment and the tests)
OP_NONE, OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3, 4
ELASTIC_SLOT = 18                     # != 0: the record's image gets the elastic deformation (include/medt_abi.h)
ELASTIC_MAX_GRID = 8


def inverse_affine_matrix(center, angle, translate, scale, shear):
    """torchvision.transforms.functional._get_inverse_affine_matrix: the map from OUTPUT to input coordinates of
    rotation by `angle`, shear (sx, sy), isotropic `scale` about `center`, then translation.  Angles in degrees."""
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def make_record(cy=0, cx=0, flip=False, matrix=None, ops_and_factors=(), elastic=False):
    """One record as a float32 numpy array.  matrix: the six entries of the inverse map, or None for the identity flag;
    ops_and_factors: up to four (operation code, factor) pairs in the order they apply; elastic: slot 18, the image is
    deformed by its control lattice (draw_field)."""
    if len(ops_and_factors) > 4:
        raise ValueError("a record holds at most four colour operations")
    r = np.zeros(PARAM_FLOATS, np.float32)
    r[0], r[1], r[2] = cy, cx, 1.0 if flip else 0.0
    if matrix is None:
        r[3] = 1.0
        r[4:10] = (1, 0, 0, 0, 1, 0)
    else:
        r[4:10] = matrix
    for k, (op, fac) in enumerate(ops_and_factors):
        r[10 + k], r[14 + k] = op, fac
    r[ELASTIC_SLOT] = 1.0 if elastic else 0.0
    return r


def draw_record(h, w, crop, p_flip=0.5, jitter=None, p_affine=0.0):
    """Draw the record of one (h, w) item: crop = (th, tw) or None, jitter = (brightness, contrast, saturation, hue) ranges
    of torchvision's ColorJitter or None, p_affine the probability of the reference's RandomAffine draw."""
    th, tw = crop if crop else (h, w)
    if th > h or tw > w:
        raise ValueError(f"crop {th} x {tw} is larger than the {h} x {w} image")
    cy = cx = 0
    if crop:                          # data.JointTransform2D.__call__'s draws, in its order
        cy = 0 if h == th else int(torch.randint(0, h - th + 1, (1,)).item())
        cx = 0 if w == tw else int(torch.randint(0, w - tw + 1, (1,)).item())
    flip = np.random.rand() < p_flip
    ops_and_factors = []
    if jitter and any(jitter):
        b, c, s, hue = jitter
        fac = {}
        for op, rng in ((OP_BRIGHTNESS, b), (OP_CONTRAST, c), (OP_SATURATION, s)):
            if rng:                   # ColorJitter: uniform(max(0, 1 - r), 1 + r); a zero range drops the operation
                fac[op] = np.random.uniform(max(0.0, 1.0 - rng), 1.0 + rng)
        if hue:
            fac[OP_HUE] = np.random.uniform(-hue, hue)
        order = np.random.permutation(4)
        ops_and_factors = [(op, fac[op]) for op in (int(k) + 1 for k in order) if op in fac]
    matrix = None
    if p_affine and np.random.rand() < p_affine:
        # RandomAffine.get_params((-90, 90), (1, 1), (2, 2), (-45, 45), size): the reference's call (utils.py:88)
        angle = np.random.uniform(-90.0, 90.0)
        tx = int(round(np.random.uniform(-tw, tw)))
        ty = int(round(np.random.uniform(-th, th)))
        scale = np.random.uniform(2.0, 2.0)
        shear = np.random.uniform(-45.0, 45.0)
        matrix = inverse_affine_matrix((tw * 0.5, th * 0.5), angle, (tx, ty), scale, (shear, 0.0))
    return make_record(cy, cx, flip, matrix, ops_and_factors)


def draw_field(G, sigma):
    """The control lattice of one elastic deformation over G x G cells: (2, G+3, G+3) float32 displacements in pixels
    (channel 0 = dx, channel 1 = dy), normal with standard deviation sigma, clipped to +-3 sigma -- U-Net's random
    displacement vectors on a coarse grid.  One np.random call."""
    if not 1 <= G <= ELASTIC_MAX_GRID:
        raise ValueError(f"an elastic grid of 1 .. {ELASTIC_MAX_GRID} cells per side expected, got {G}")
    return np.clip(np.random.normal(0.0, sigma, (2, G + 3, G + 3)), -3.0 * sigma, 3.0 * sigma).astype(np.float32)


def parse_jitter(text):
    """--aug_jitter "b,c,s,h": four non-negative ranges, hue at most 0.5 (ColorJitter's own limits)."""
    try:
        v = tuple(float(t) for t in text.split(","))
    except ValueError:
        raise ValueError("four comma-separated numbers expected, got %r" % text)
    if len(v) != 4:
        raise ValueError("four comma-separated numbers expected (brightness,contrast,saturation,hue), got %r" % text)
    if any(not math.isfinite(x) or x < 0 for x in v) or v[3] > 0.5:
        raise ValueError("non-negative finite ranges expected, hue at most 0.5, got %r" % text)
    return v


class RawJointTransform2D:
    """Dataset transform of the device path: (image, mask) -> (uint8 HWC image, uint8 HW mask, float32 record).  The draws
    happen here, per item, where data.JointTransform2D makes them; nothing is cropped, flipped or converted on the host.
    elastic = {"p", "grid", "sigma"}: a fourth element, the item's (2, grid+3, grid+3) control lattice -- drawn with
    probability p AFTER every other draw of the item (the record's slot 18 says so), all zeros otherwise."""

    def __init__(self, crop=None, p_flip=0.5, jitter=None, p_affine=0.0, elastic=None):
        self.crop, self.p_flip, self.jitter, self.p_affine, self.elastic = crop, p_flip, jitter, p_affine, elastic
        if elastic is not None and not 1 <= int(elastic["grid"]) <= ELASTIC_MAX_GRID:
            raise ValueError(f"an elastic grid of 1 .. {ELASTIC_MAX_GRID} cells per side expected, got {elastic['grid']}")

    def __call__(self, image, mask):
        image, mask = np.asarray(image), np.asarray(mask)
        if image.ndim == 2:
            image = image[:, :, None]
        h, w = image.shape[:2]
        rec = draw_record(h, w, self.crop, self.p_flip, self.jitter, self.p_affine)
        item = (torch.from_numpy(np.ascontiguousarray(image, np.uint8)),
                torch.from_numpy(np.ascontiguousarray(mask.reshape(h, w), np.uint8)), torch.from_numpy(rec))
        if self.elastic is None:
            return item
        G = int(self.elastic["grid"])
        if np.random.rand() < self.elastic["p"]:
            rec[ELASTIC_SLOT] = 1.0
            return item + (torch.from_numpy(draw_field(G, self.elastic["sigma"])),)
        return item + (torch.zeros((2, G + 3, G + 3), dtype=torch.float32),)


class DeviceAugment:
    """The device half: uint8 (N,H,W,C) images, uint8 (N,H,W) masks and the (N,P) record table, all on the device ->
    the float32 (N,C,th,tw) images and int64 (N,th,tw) masks TrainStep takes.  Holds the workspace of the contrast mean."""

    def __init__(self, crop=None):
        self.crop = crop
        self._ws = {}
        if ops.augment_param_floats() != PARAM_FLOATS:
            raise ops.L.MedtError("medt_amd.augment and the library disagree on the record length")

    def means(self, N, size):
        """The per-image grey means the last call's contrast operations used (0 when the batch had none)."""
        return self._ws[(N, tuple(size))][-N:]

    def __call__(self, img_u8, mask_u8, params, host_params=None, field=None):
        N, H, W = img_u8.shape[:3]
        size = tuple(self.crop) if self.crop else (H, W)
        key = (N, size)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.zeros(ops.augment_workspace(N, size), device=img_u8.device, dtype=torch.float32)
        return ops.augment_batch(img_u8, mask_u8, params, size, workspace=ws, host_params=host_params, field=field)
