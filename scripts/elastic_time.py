#!/usr/bin/env python
"""The `apply` launch of the device-side joint augmentation alone, with and without the elastic deformation: medt_augment_apply
(the kernel every batch took before the elastic deformation existed: the baseline) and medt_augment_warp on the SAME batches, in
one process, in alternating windows, by hipEvents.  The records carry crop, flip, jitter without contrast (so neither launch
needs the statistics launch) and, for half the images, an affine map.

Batches: 4 x 128^2 images as they are, 4 crops of 128^2 out of 1000^2 images, one 1000^2 crop.  Flags all 1 and mixed [1,0,1,0]
(flag-0 blocks take apply's body inside the warp kernel).  ms per launch: median [min .. max] of --repeats windows of --inner
launches after --warmup windows, and the ratio of the medians.

    python scripts/elastic_time.py [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-transformer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from medt_amd import _lib as L, ops  # noqa: E402
from medt_amd.augment import OP_BRIGHTNESS, OP_HUE, OP_SATURATION, inverse_affine_matrix, make_record  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib, G = L.lib(), a.grid
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"3 channels, grid {G}, ms per launch: median [min .. max] of {a.repeats} windows of {a.inner} launches after {a.warmup} "
             f"warm-up windows, apply and warp alternating"]
    for N, side, crop in ((4, 128, 128), (4, 1000, 128), (1, 1000, 1000)):
        rng = np.random.RandomState(0)
        img = torch.from_numpy(rng.randint(0, 256, (N, side, side, 3)).astype(np.uint8)).to(dev)
        mask = torch.from_numpy(rng.randint(0, 2, (N, side, side)).astype(np.uint8)).to(dev)
        sigma = crop / 32.0
        field = torch.from_numpy(np.clip(rng.normal(0, sigma, (N, 2, G + 3, G + 3)), -3 * sigma, 3 * sigma).astype(np.float32)).to(dev)
        oi = torch.empty((N, 3, crop, crop), device=dev)
        om = torch.empty((N, crop, crop), device=dev, dtype=torch.int64)
        jit = [(OP_BRIGHTNESS, 1.1), (OP_SATURATION, 0.9), (OP_HUE, 0.03)]
        for flags in ([[1]] if N == 1 else [[1] * N, [1, 0, 1, 0][:N]]):
            recs = []
            for n in range(N):
                m = inverse_affine_matrix((crop * 0.5, crop * 0.5), 20.0, (3, -2), 1.2, (5.0, 0.0)) if n & 1 else None
                recs.append(make_record(int(rng.randint(0, side - crop + 1)), int(rng.randint(0, side - crop + 1)), bool(n & 1), m, jit,
                                        elastic=bool(flags[n])))
            params = torch.from_numpy(np.stack(recs)).to(dev)
            args = (N, side, side, 3, crop, crop, 0, stream)

            def apply():
                L.check(lib.medt_augment_apply(img.data_ptr(), mask.data_ptr(), params.data_ptr(), None, oi.data_ptr(), om.data_ptr(), *args),
                        "medt_augment_apply")

            def warp():
                L.check(lib.medt_augment_warp(img.data_ptr(), mask.data_ptr(), params.data_ptr(), field.data_ptr(), G, None, oi.data_ptr(),
                                              om.data_ptr(), *args), "medt_augment_warp")

            t = {"apply": [], "warp": []}
            for k in range(a.warmup + a.repeats):
                for name, fn in (("apply", apply), ("warp", warp)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.inner):
                        fn()
                    e1.record()
                    e1.synchronize()
                    if k >= a.warmup:
                        t[name].append(e0.elapsed_time(e1) / a.inner)
            med = {k: statistics.median(v) for k, v in t.items()}
            lines.append(f"--- {N} x {side}^2 -> {crop}^2, flags {flags}")
            for k in ("apply", "warp"):
                lines.append(f"{k:<6} {med[k]:9.4f} [{min(t[k]):.4f} .. {max(t[k]):.4f}]")
            lines.append(f"warp / apply {med['warp'] / med['apply']:.2f}")
            print("\n".join(lines[-4:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
