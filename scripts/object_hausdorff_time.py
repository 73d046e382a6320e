#!/usr/bin/env python
"""The object-level Hausdorff distance of GlaS (metrics.object_hausdorff) of masks that are on the device, through two paths:

  device  metrics.object_hausdorff: both masks labelled, area tables, overlap table and bounding boxes built on the device,
          those integer tables to the host, the matching there, the per-pair distances in two batched device calls
          (medt_amd.ops.pair_hausdorff_sq), roots and weighted sums on the host in float64;
  host    the masks copied to the CPU, scipy.ndimage.label for both, the same matching with the same bounding-box pruning,
          and one scipy.ndimage.distance_transform_edt per pair and direction on the crop that holds both objects.

Wall-clock per call (perf_counter around a window of --inner calls that ends in a device synchronisation), median of --repeats
windows after --warmup windows; the two batched device calls alone by hipEvents as well.  Cases: a GlaS-like 522 x 775 image
with about 30 blobs against a perturbed copy, one 1000^2 image with about 1300 small objects, a batch of 4 x 128^2.  The scores
of the two paths are compared as well.

    python scripts/object_hausdorff_time.py [--out FILE]
"""
import argparse
import math
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

EIGHT = np.ones((3, 3))


def blobs(H, W, seed, density, grow):
    a = np.random.default_rng(seed).random((H, W)) < density
    for _ in range(grow):
        p = np.pad(a, 1)
        a = p[1:-1, 1:-1] | p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
    return a.astype(np.uint8) * np.uint8(255)


def glands(H, W, seed, count=30):
    """About `count` elliptical blobs of 30..70 pixels per half axis, and a perturbed copy: shifted by a few pixels, eroded or
    dilated once, two glands dropped and two spurious ones added."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]

    def paint(centres):
        m = np.zeros((H, W), bool)
        for cy, cx, ry, rx in centres:
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        return m

    cs = [(rng.uniform(0, H), rng.uniform(0, W), rng.uniform(18, 45), rng.uniform(18, 45)) for _ in range(count)]
    target = paint(cs)
    moved = [(cy + rng.uniform(-6, 6), cx + rng.uniform(-6, 6), ry * rng.uniform(0.8, 1.2), rx * rng.uniform(0.8, 1.2)) for cy, cx, ry, rx in cs[2:]]
    moved += [(rng.uniform(0, H), rng.uniform(0, W), 12.0, 12.0) for _ in range(2)]
    pred = paint(moved)
    return pred.astype(np.uint8) * np.uint8(255), target.astype(np.uint8) * np.uint8(255)


def host_image(pred, target):
    """(hd, pairs evaluated) of one image on the host: SciPy labels, the matching of metrics.object_hausdorff with its pruning,
    one distance_transform_edt per pair and direction on the crop that holds both objects."""
    P, kp = ndimage.label(pred, EIGHT)
    G, kg = ndimage.label(target, EIGHT)
    if not kp or not kg:
        return float("nan"), 0
    sp, sg = ndimage.find_objects(P), ndimage.find_objects(G)
    ap, ag = np.bincount(P.reshape(-1), minlength=kp + 1), np.bincount(G.reshape(-1), minlength=kg + 1)
    bp = np.asarray([[s[0].start, s[1].start, s[0].stop - 1, s[1].stop - 1] for s in sp], np.int64)
    bg = np.asarray([[s[0].start, s[1].start, s[0].stop - 1, s[1].stop - 1] for s in sg], np.int64)
    both = (P > 0) & (G > 0)
    key, cnt = np.unique(P[both].astype(np.int64) * (kg + 1) + G[both], return_counts=True)
    part_g, part_p = {}, {}
    for j, i, I in zip((key // (kg + 1)).tolist(), (key % (kg + 1)).tolist(), cnt.tolist()):
        if i not in part_g or I > part_g[i][0]:
            part_g[i] = (I, j)
        if j not in part_p or I > part_p[j][0]:
            part_p[j] = (I, i)
    dist = {}

    def h2(j, i):
        if (j, i) not in dist:
            a, b = bp[j - 1], bg[i - 1]
            y0, x0, y1, x1 = min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]) + 1, max(a[3], b[3]) + 1
            A, B = P[y0:y1, x0:x1] == j, G[y0:y1, x0:x1] == i
            d = max(ndimage.distance_transform_edt(~B)[A].max(), ndimage.distance_transform_edt(~A)[B].max())
            dist[(j, i)] = int(round(float(d) ** 2))
        return dist[(j, i)]

    def nearest(box, others, h):
        bound = np.abs(others - box[None, :]).max(axis=1) ** 2
        k = int(np.argmin(bound))
        best = h(k + 1)
        ds = [(h(c + 1), c + 1) for c in np.nonzero(bound <= best)[0]]
        return min(ds)[1]

    hg = hp = 0.0
    for i in range(1, kg + 1):
        j = part_g[i][1] if i in part_g else nearest(bg[i - 1], bp, lambda jj: h2(jj, i))
        hg += (int(ag[i]) / int(ag[1:].sum())) * math.sqrt(float(h2(j, i)))
    for j in range(1, kp + 1):
        i = part_p[j][1] if j in part_p else nearest(bp[j - 1], bg, lambda ii: h2(j, ii))
        hp += (int(ap[j]) / int(ap[1:].sum())) * math.sqrt(float(h2(j, i)))
    return 0.5 * (hg + hp), 2 * len(dist)


def host_path(pred, target):
    return [host_image(a, b) for a, b in zip(pred.cpu().numpy(), target.cpu().numpy())]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_hausdorff.txt"))
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    import scipy
    lines = ["ms per call: median [min .. max] of %d windows of %d calls after %d warm-up windows (the host path of the 1000^2 case: "
             "3 windows of 1 call after 1); host path: SciPy %s" % (args.repeats, args.inner, args.warmup, scipy.__version__)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g_pred, g_target = glands(522, 775, 1)
    cases = [("1 x 522 x 775, gland-like blobs against a perturbed copy", g_pred[None], g_target[None], False),
             ("1 x 1000^2, small blobs (density 0.002, grown 6 times), independent seeds", blobs(1000, 1000, 1, 0.002, 6)[None],
              blobs(1000, 1000, 101, 0.002, 6)[None], True),
             ("4 x 128^2, small blobs, independent seeds", np.stack([blobs(128, 128, s, 0.002, 6) for s in range(1, 5)]),
              np.stack([blobs(128, 128, s, 0.002, 6) for s in range(101, 105)]), False)]
    for name, pred, target, slow_host in cases:
        p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev)
        got = metrics.object_hausdorff(p, t)
        off = metrics.object_hausdorff(p, t, prune=False)
        host = host_path(p, t)
        say("--- %s: %s predicted / %s target objects" % (name, got["n_pred"].tolist(), got["n_gt"].tolist()))
        say("    Hobj (device): %s   jobs with pruning %s, without %s, on the host path %s" % (
            ["%.4f" % v for v in got["hd"].tolist()], got["pairs"].tolist(), off["pairs"].tolist(), [k for _, k in host]))
        diff = max((abs(float(a) - b) for a, (b, _) in zip(got["hd"], host) if not math.isnan(b)), default=0.0)
        say("    largest |device - host|: %.3e   pruned == unpruned: %s" % (diff, got["hd"].tolist() == off["hd"].tolist()))
        w = (args.inner, args.repeats, args.warmup)
        say("device: metrics.object_hausdorff                           %.4f [%.4f .. %.4f]" % windows(lambda: metrics.object_hausdorff(p, t), *w))
        say("device: metrics.object_hausdorff, prune=False              %.4f [%.4f .. %.4f]" % windows(lambda: metrics.object_hausdorff(p, t, prune=False), *w))
        say("device: metrics.object_scores (labelling and tables alone)  %.4f [%.4f .. %.4f]" % windows(lambda: metrics.object_scores(p, t), *w))
        say("host: copy to the CPU + SciPy label + EDT per pair          %.4f [%.4f .. %.4f]" % windows(lambda: host_path(p, t), *((1, 3, 1) if slow_host else w)))
        # the distances alone: every overlapping pair as one batched call, kernels by hipEvents
        lp, cp = ops.label(p, 8)
        lg, cg = ops.label(t, 8)
        pairs = ops.label_overlaps(lp, cp, lg, cg)[:, :3].to(torch.int32).cpu()
        boxes = (ops.label_boxes(lp, cp).cpu(), ops.label_boxes(lg, cg).cpu())
        if len(pairs):
            ts = []
            for k in range(args.warmup + args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                ops.pair_hausdorff_sq(lp, cp, lg, cg, pairs, boxes=boxes)
                e1.record()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ts.append(e0.elapsed_time(e1))
            say("one ops.pair_hausdorff_sq of the %5d overlapping pairs, by events (job table built on the host inside)  %.4f [%.4f .. %.4f]"
                % (len(pairs), statistics.median(ts), min(ts), max(ts)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
