#!/usr/bin/env python
"""Splitting touching objects (DESIGN.md 'Splitting touching objects') of masks that are on the device, through the two paths:

  device  medt_amd.ops.split_markers (label, two distance-transform launches, component maxima, marker pass),
          medt_amd.ops.grow_labels from the labelled markers (with its pass count) and medt_amd.ops.split_objects (all of it);
  host    the masks copied to the CPU and the same definition from SciPy calls and vectorised numpy, per image:
          scipy.ndimage.label, scipy.ndimage.distance_transform_edt(return_indices=True) for exact squared depths,
          scipy.ndimage.maximum_filter(size=2r+1, mode="constant"), scipy.ndimage.maximum per component, the int64 predicate in
          numpy, scipy.ndimage.label of the markers, and a level-by-level breadth-first growth in numpy (np.minimum.reduce over
          the shifted frontier labels, one whole-image step per level).

Wall-clock per call (perf_counter around a window of --inner calls that ends in a device synchronisation), median of --repeats
windows after --warmup windows.  Cases: one 128^2 image, 4 x 128^2, one 1000^2 map of roughly 1300 overlapping blobs.  The label
maps of the two paths are compared as well.

    python scripts/split_time.py [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-transformer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402

from medt_amd import ops  # noqa: E402

EIGHT = np.ones((3, 3))
BIG = np.int64(2 ** 62)


def blobs(side, count, seed, rmin=6, rmax=14):
    g = np.random.default_rng(seed)
    yy, xx = np.indices((side, side))
    m = np.zeros((side, side), bool)
    for _ in range(count):
        cy, cx, r = int(g.integers(0, side)), int(g.integers(0, side)), int(g.integers(rmin, rmax + 1))
        y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, side), max(cx - r, 0), min(cx + r + 1, side)
        m[y0:y1, x0:x1] |= (yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2 <= r * r
    return m.astype(np.uint8) * np.uint8(255)


def host_markers(m, r, t):
    F = m != 0
    comp, k = ndimage.label(F, EIGHT)
    if F.all():
        d2 = np.full(F.shape, 2 ** 31 - 1, np.int64)
    else:
        iy, ix = ndimage.distance_transform_edt(F, return_distances=False, return_indices=True)
        yy, xx = np.indices(F.shape)
        d2 = ((iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2) * F
    M = ndimage.maximum_filter(d2, size=2 * r + 1, mode="constant", cval=0)
    cmax = np.zeros(k + 1, np.int64)
    if k:
        cmax[1:] = ndimage.maximum(d2, comp, np.arange(1, k + 1))
    e = M - d2 - t * t
    return F & ((e <= 0) | (e * e <= 4 * t * t * d2) | (d2 == cmax[comp]))


def host_grow(seeds, m):
    F = m != 0
    H, W = F.shape
    lab = np.where(F & (seeds > 0), seeds, 0).astype(np.int64)
    dist = np.where(lab > 0, 0, -1)
    level = 0
    while True:
        p = np.pad(np.where(dist == level, lab, BIG), 1, constant_values=BIG)
        cand = np.minimum.reduce([p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx])
        new = F & (dist < 0) & (cand < BIG)
        if not new.any():
            return lab.astype(np.int32)
        lab[new] = cand[new]
        dist[new] = level + 1
        level += 1


def host_split(masks, r, t):
    out = []
    for m in masks.cpu().numpy():
        seeds, _ = ndimage.label(host_markers(m, r, t), EIGHT)
        out.append(host_grow(seeds, m))
    return np.stack(out)


def windows(fn, inner, repeats, warmup):
    """median ms per call of fn over `repeats` windows of `inner` calls, each window closed by a synchronisation."""
    t = []
    for k in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        if k >= warmup:
            t.append((time.perf_counter() - t0) * 1e3 / inner)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--distance", type=int, default=7)
    ap.add_argument("--tolerance", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f"ms per call: median [min .. max] of {a.repeats} windows of {a.inner} calls after {a.warmup} warm-up windows; distance "
        f"{a.distance}, tolerance {a.tolerance}, connectivity 8; host path: SciPy {__import__('scipy').__version__}, numpy {np.__version__}")
    for N, side, count in ((1, 128, 22), (4, 128, 22), (1, 1000, 1300)):
        masks = torch.from_numpy(np.stack([blobs(side, count, 10 + n) for n in range(N)])).to(dev)
        labels, counts = ops.split_objects(masks, a.distance, a.tolerance, 8)
        comps = ops.label(masks, 8)[1]
        seeds = ops.label(ops.split_markers(masks, a.distance, a.tolerance, 8), 8)[0]
        _, passes = ops.grow_labels(seeds, masks, 8, return_passes=True)
        same = np.array_equal(labels.cpu().numpy(), host_split(masks, a.distance, a.tolerance))
        say(f"--- {N} x {side}^2, {count} discs per image: {comps.tolist()} components -> {counts.tolist()} objects, growth in "
            f"{passes} passes, label maps equal the host path's: {same}")
        rows = [("device: ops.split_markers", lambda: ops.split_markers(masks, a.distance, a.tolerance, 8)),
                ("device: ops.grow_labels (%d passes)" % passes, lambda: ops.grow_labels(seeds, masks, 8)),
                ("device: ops.split_objects", lambda: ops.split_objects(masks, a.distance, a.tolerance, 8)),
                ("host: copy + markers (SciPy)", lambda: [host_markers(m, a.distance, a.tolerance) for m in masks.cpu().numpy()]),
                ("host: copy + markers + label + numpy growth", lambda: host_split(masks, a.distance, a.tolerance))]
        for name, fn in rows:
            med, lo, hi = windows(fn, a.inner, a.repeats, a.warmup)
            say(f"{name:<50} {med:10.4f} [{lo:.4f} .. {hi:.4f}]")
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
