"""Instance annotations for test.py: ground-truth label maps read from files (--instance_labels DIR) and label maps written as
16-bit PNGs (--write_instances on).  Host plumbing only: PIL + numpy."""
from __future__ import annotations

import os

import numpy as np
from PIL import Image

MAX_PNG_LABEL = 65535


def renumber(ids):
    """Integer id map (0 = background) -> (int32 label map with the ids replaced by 1..K in raster order of each id's first
    pixel, K)."""
    flat = np.asarray(ids).reshape(-1)
    values, first = np.unique(flat, return_index=True)
    keep = values != 0
    values, first = values[keep], first[keep]
    order = np.argsort(first, kind="stable")
    rank = np.zeros(len(values), np.int32)
    rank[order] = np.arange(1, len(values) + 1, dtype=np.int32)
    out = np.zeros(flat.shape, np.int32)
    if len(values):
        pos = np.searchsorted(values, flat)
        hit = (flat != 0)
        out[hit] = rank[np.minimum(pos, len(values) - 1)[hit]]
    return out.reshape(np.asarray(ids).shape), int(len(values))


def read_instances(direc, filename, shape):
    """The instance map of the image written as `filename`: <direc>/<stem>.png (8- or 16-bit, value = instance id, 0 =
    background) or <direc>/<stem>.npy, of the image's (H, W) -> (int32 labels 1..K in raster order of first pixel, K)."""
    stem = os.path.splitext(os.path.basename(filename))[0]
    png, npy = os.path.join(direc, stem + ".png"), os.path.join(direc, stem + ".npy")
    if os.path.exists(png):
        with Image.open(png) as im:
            if im.mode not in ("L", "P", "I;16", "I;16B", "I", "1"):
                raise SystemExit(f"--instance_labels: {png}: mode {im.mode}: an 8- or 16-bit single-channel PNG of instance ids expected")
            ids = np.array(im).astype(np.int64)
    elif os.path.exists(npy):
        ids = np.load(npy)
        if ids.dtype.kind not in "iub":
            raise SystemExit(f"--instance_labels: {npy}: dtype {ids.dtype}: an integer map of instance ids expected")
        ids = ids.astype(np.int64)
    else:
        raise SystemExit(f"--instance_labels: neither {png} nor {npy} exists")
    if ids.ndim != 2 or tuple(ids.shape) != tuple(shape):
        raise SystemExit(f"--instance_labels: {stem}: a map of {tuple(ids.shape)}, the image has {tuple(shape)}")
    if ids.min() < 0:
        raise SystemExit(f"--instance_labels: {stem}: negative instance ids")
    return renumber(ids)


def write_instances(path, labels):
    """int32 (H,W) label map -> a 16-bit grayscale PNG whose values are the labels."""
    labels = np.asarray(labels)
    if labels.size and int(labels.max()) > MAX_PNG_LABEL:
        raise SystemExit(f"--write_instances: {int(labels.max())} objects in {path}: a 16-bit PNG holds at most {MAX_PNG_LABEL}")
    Image.fromarray(labels.astype(np.uint16)).save(path)
