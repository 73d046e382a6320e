#!/usr/bin/env python
"""Surface-distance scores (HD, HD95, ASSD) of masks that are on the device, through the two paths:

  device  metrics.surface_scores: two medt_amd.ops.surface_d2 calls (distance transform of one border, read at the other),
          torch.sort and float64 roots on the device, a handful of scalars to the host;
  host    the masks copied to the CPU, SciPy's distance_transform_edt + binary_erosion per direction, numpy for the scores
          (what a user of the evaluation loop does today).  Without SciPy: the brute-force oracle of the tests, 128^2 only.

Wall-clock per call (perf_counter around a window of --inner calls that ends in a device synchronisation), median of --repeats
windows after --warmup windows; the two kernels of one surface_d2 and of one full edt_sq alone by hipEvents, same medians.
Cases: one 128^2 image, one 1000^2 image, a batch of 4 x 128^2.  Masks: seeded blobs (rng.random < --density, dilated --grow
times by the 3x3 cross), prediction and target from different seeds.  The scores of the two paths are compared as well.

    python scripts/surface_time.py [--out FILE]
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

import metrics  # noqa: E402
from medt_amd import ops  # noqa: E402

try:
    from scipy import ndimage
except ImportError:                                     # the brute-force oracle of the tests stands in, at 128^2 only
    ndimage = None
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import surface_oracle


def blobs(H, W, seed, density, grow):
    a = np.random.default_rng(seed).random((H, W)) < density
    for _ in range(grow):
        p = np.pad(a, 1)
        a = p[1:-1, 1:-1] | p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
    return a.astype(np.uint8) * np.uint8(255)


def host_scores(pred, target):
    """(N,3) float64 {hd, hd95, assd} of uint8 (N,H,W) device masks, on the host."""
    p, t = pred.cpu().numpy() != 0, target.cpu().numpy() != 0
    rows = []
    for a, b in zip(p, t):
        if ndimage is None:
            rows.append(surface_oracle.surface_scores(a, b)[:3])
            continue
        cross = ndimage.generate_binary_structure(2, 1)
        sa, sb = a & ~ndimage.binary_erosion(a, cross), b & ~ndimage.binary_erosion(b, cross)
        d_ab, d_ba = ndimage.distance_transform_edt(~sb)[sa], ndimage.distance_transform_edt(~sa)[sb]
        rows.append((max(d_ab.max(), d_ba.max()), np.percentile(np.hstack((d_ab, d_ba)), 95), (d_ab.mean() + d_ba.mean()) / 2))
    return np.asarray(rows, np.float64)


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


def events(fn, inner, repeats, warmup):
    t = []
    for k in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            t.append(e0.elapsed_time(e1) / inner)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.002)
    ap.add_argument("--grow", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    host_name = "SciPy %s" % __import__("scipy").__version__ if ndimage is not None else "brute-force oracle (no SciPy)"
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f"ms per call: median [min .. max] of {a.repeats} windows of {a.inner} calls after {a.warmup} warm-up windows; "
             f"masks: blobs, density {a.density}, grown {a.grow} times; host path: {host_name}")
    for N, side in ((1, 128), (1, 1000), (4, 128)):
        pred = torch.from_numpy(np.stack([blobs(side, side, 10 + n, a.density, a.grow) for n in range(N)])).to(dev)
        target = torch.from_numpy(np.stack([blobs(side, side, 110 + n, a.density, a.grow) for n in range(N)])).to(dev)
        say(f"--- {N} x {side}^2: foreground {float((pred != 0).float().mean()):.3f} / {float((target != 0).float().mean()):.3f} of the pixels")
        got = metrics.surface_scores(pred, target)
        say("    scores of image 0 (device): HD %.4f  HD95 %.4f  ASSD %.4f  valid %s" % (
            got["hd"][0], got["hd95"][0], got["assd"][0], got["valid"].tolist()))
        rows = [("device: metrics.surface_scores", lambda: metrics.surface_scores(pred, target), windows)]
        if ndimage is not None or side <= 128:
            want = host_scores(pred, target)
            dev_rows = np.stack([got[k].numpy() for k in ("hd", "hd95", "assd")], axis=1)
            say("    largest |device - host| over the scores: %.3e" % np.nanmax(np.abs(dev_rows - want)))
            rows.append(("host: copy to the CPU + " + host_name, lambda: host_scores(pred, target), windows))
        rows.append(("kernels alone: one surface_d2 (cols + rows)", lambda: ops.surface_d2(pred, target), events))
        rows.append(("kernels alone: one full edt_sq (cols + rows)", lambda: ops.edt_sq(target), events))
        for name, fn, timer in rows:
            med, lo, hi = timer(fn, a.inner, a.repeats, a.warmup)
            say(f"{name:<55} {med:9.4f} [{lo:.4f} .. {hi:.4f}]")
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
