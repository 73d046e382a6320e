#!/usr/bin/env python
"""One training batch through the two input paths, decoded uint8 images in host memory -> what TrainStep takes on the device:

  host    medt_amd.data.JointTransform2D per item (crop, flip, to_tensor: float32 on the CPU), stacked into a pinned float32
          batch, copied to the device;
  device  medt_amd.augment.RawJointTransform2D per item (draws only), the uint8 images stacked into a pinned batch, copied
          with the record table, then augment_stats (when a record has contrast) + augment_apply.

Wall-clock per batch (perf_counter around a window of --inner batches that ends in a device synchronisation), median of
--repeats windows after --warmup windows; the device path's kernels alone by hipEvents, same medians.  Cases: 4 x 128^2
images as they are, and 4 crops of 128^2 out of 1000^2 images (the device path uploads the whole image).

    python scripts/augment_time.py [--out FILE]
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

from medt_amd import ops  # noqa: E402
from medt_amd.augment import DeviceAugment, RawJointTransform2D  # noqa: E402
from medt_amd.data import JointTransform2D  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N = a.batch
    lines = [f"batch of {N}, 3 channels, ms per batch: median [min .. max] of {a.repeats} windows of {a.inner} batches after {a.warmup} warm-up windows"]
    for side, crop in ((128, None), (1000, (128, 128))):
        rng = np.random.RandomState(0)
        imgs = [rng.randint(0, 256, (side, side, 3)).astype(np.uint8) for _ in range(N)]
        masks = [rng.randint(0, 2, (side, side)).astype(np.uint8) for _ in range(N)]
        size = crop or (side, side)
        np.random.seed(3000)
        torch.manual_seed(3000)

        host_tf = JointTransform2D(crop=crop, p_flip=0.5, color_jitter_params=None, long_mask=True)
        pin_x = torch.empty((N, 3) + size, dtype=torch.float32).pin_memory()
        pin_y = torch.empty((N,) + size, dtype=torch.int64).pin_memory()

        def host_path():
            for n in range(N):
                x, y = host_tf(imgs[n], masks[n])
                pin_x[n].copy_(x)
                pin_y[n].copy_(y)
            return pin_x.to(dev, non_blocking=True), pin_y.to(dev, non_blocking=True)

        pin_u = torch.empty((N, side, side, 3), dtype=torch.uint8).pin_memory()
        pin_m = torch.empty((N, side, side), dtype=torch.uint8).pin_memory()
        pin_r = torch.empty((N, ops.augment_param_floats()), dtype=torch.float32).pin_memory()
        aug = DeviceAugment(crop)
        st = {}

        def device_path(raw_tf):
            for n in range(N):
                u, m, r = raw_tf(imgs[n], masks[n])
                pin_u[n].copy_(u)
                pin_m[n].copy_(m)
                pin_r[n].copy_(r)
            st["in"] = (pin_u.to(dev, non_blocking=True), pin_m.to(dev, non_blocking=True), pin_r.to(dev, non_blocking=True))
            return aug(*st["in"], host_params=pin_r)

        plain = RawJointTransform2D(crop=crop, p_flip=0.5)
        full = RawJointTransform2D(crop=crop, p_flip=0.5, jitter=(0.2, 0.2, 0.2, 0.05), p_affine=0.5)
        rows = [("host: crop+flip on the CPU, float32 upload", host_path),
                ("device: uint8 upload + kernels, crop+flip", lambda: device_path(plain)),
                ("device: ... + jitter 0.2,0.2,0.2,0.05 + affine 0.5", lambda: device_path(full))]
        lines.append(f"--- {N} x {side}^2 images -> {size[0]} x {size[1]}: upload {N * 3 * size[0] * size[1] * 4 + N * size[0] * size[1] * 8} B (host path), "
                     f"{N * side * side * 4} B (device path)")
        for name, fn in rows:
            med, lo, hi = windows(fn, a.inner, a.repeats, a.warmup)
            lines.append(f"{name:<55} {med:9.3f} [{lo:.3f} .. {hi:.3f}]")
            print(lines[-1], flush=True)
        # the kernels alone, on the batch that is already on the device
        for name, tf in (("kernels alone, crop+flip (1 launch)", plain), ("kernels alone, jitter+affine (2 launches)", full)):
            device_path(tf)
            torch.cuda.synchronize()
            host_r = pin_r.clone()
            t = []
            for k in range(a.warmup + a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    aug(*st["in"], host_params=host_r)
                e1.record()
                e1.synchronize()
                if k >= a.warmup:
                    t.append(e0.elapsed_time(e1) / a.inner)
            lines.append(f"{name:<55} {statistics.median(t):9.4f} [{min(t):.4f} .. {max(t):.4f}]")
            print(lines[-1], flush=True)
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
