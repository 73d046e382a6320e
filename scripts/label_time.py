#!/usr/bin/env python
"""Connected-component labelling and the object-level scores (object F1 / Dice, AJI, PQ) of masks that are on the device,
through the two paths:

  device  medt_amd.ops.label (six launches) and metrics.object_scores: both masks labelled, the area tables and the overlap
          table built on the device, those integer tables to the host, the scores there in float64;
  host    the masks copied to the CPU, scipy.ndimage.label for both, numpy bincounts for the same tables and the same table
          arithmetic (what a user of the evaluation loop does today).

Wall-clock per call (perf_counter around a window of --inner calls that ends in a device synchronisation), median of --repeats
windows after --warmup windows; one ops.label alone by hipEvents as well, same medians.  Cases: one 128^2 image, one 1000^2
image, a batch of 4 x 128^2.  Masks: seeded blobs (rng.random < --density, dilated --grow times by the 3x3 cross), prediction
and target from different seeds; for ops.label also a random map at density 0.59 (4-connected: long tangled components).  The
labels and scores of the two paths are compared as well.

    python scripts/label_time.py [--out FILE]
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

import metrics  # noqa: E402
from medt_amd import ops  # noqa: E402

KEYS = ("f1", "dice", "aji", "pq", "dq", "sq")
EIGHT = np.ones((3, 3))


def blobs(H, W, seed, density, grow):
    a = np.random.default_rng(seed).random((H, W)) < density
    for _ in range(grow):
        p = np.pad(a, 1)
        a = p[1:-1, 1:-1] | p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
    return a.astype(np.uint8) * np.uint8(255)


def host_scores(pred, target):
    """(N,6) float64 {f1, dice, aji, pq, dq, sq} of uint8 (N,H,W) device masks, on the host."""
    rows = []
    for a, b in zip(pred.cpu().numpy(), target.cpu().numpy()):
        lp, kp = ndimage.label(a, EIGHT)
        lg, kg = ndimage.label(b, EIGHT)
        ap, ag = np.bincount(lp.reshape(-1), minlength=kp + 1), np.bincount(lg.reshape(-1), minlength=kg + 1)
        both = (lp > 0) & (lg > 0)
        key, cnt = np.unique(lp[both].astype(np.int64) * (kg + 1) + lg[both], return_counts=True)
        triples = list(zip((key // (kg + 1)).tolist(), (key % (kg + 1)).tolist(), cnt.tolist()))
        rows.append(metrics._object_scores_image(ap[1:].tolist(), ag[1:].tolist(), triples))
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
    host_name = "SciPy %s" % __import__("scipy").__version__
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f"ms per call: median [min .. max] of {a.repeats} windows of {a.inner} calls after {a.warmup} warm-up windows; "
        f"masks: blobs, density {a.density}, grown {a.grow} times; host path: {host_name}")
    for N, side in ((1, 128), (1, 1000), (4, 128)):
        pred = torch.from_numpy(np.stack([blobs(side, side, 10 + n, a.density, a.grow) for n in range(N)])).to(dev)
        target = torch.from_numpy(np.stack([blobs(side, side, 110 + n, a.density, a.grow) for n in range(N)])).to(dev)
        tangle = torch.from_numpy((np.random.default_rng(5).random((N, side, side)) < 0.59).astype(np.uint8)).to(dev)
        got = metrics.object_scores(pred, target)
        say(f"--- {N} x {side}^2: {got['n_pred'].tolist()} predicted / {got['n_gt'].tolist()} target objects")
        say("    scores of image 0 (device): F1obj %.4f  Diceobj %.4f  AJI %.4f  PQ %.4f" % tuple(got[k][0] for k in KEYS[:4]))
        want = host_scores(pred, target)
        say("    largest |device - host| over the scores: %.3e" % np.nanmax(np.abs(np.stack([got[k].numpy() for k in KEYS], axis=1) - want)))
        labels, counts = ops.label(tangle, 4)
        same = all(np.array_equal(labels[n].cpu().numpy(), ndimage.label(tangle[n].cpu().numpy())[0]) for n in range(N))
        say(f"    random map at density 0.59, 4-connected: {counts.tolist()} components, labels equal SciPy's: {same}")
        rows = [("device: metrics.object_scores", lambda: metrics.object_scores(pred, target), windows),
                ("host: copy to the CPU + " + host_name + " + tables", lambda: host_scores(pred, target), windows),
                ("device: one ops.label, blobs, 8-connected", lambda: ops.label(pred, 8), windows),
                ("host: copy + ndimage.label, blobs, 8-connected", lambda: [ndimage.label(m, EIGHT) for m in pred.cpu().numpy()], windows),
                ("device: one ops.label, density 0.59, 4-connected", lambda: ops.label(tangle, 4), windows),
                ("host: copy + ndimage.label, density 0.59, 4-conn.", lambda: [ndimage.label(m) for m in tangle.cpu().numpy()], windows),
                ("kernels alone: one ops.label, blobs, 8-connected", lambda: ops.label(pred, 8), events),
                ("kernels alone: one ops.label, density 0.59, 4-conn.", lambda: ops.label(tangle, 4), events)]
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
