#!/usr/bin/env python
"""Step time of the replayed training step (TrainStep as a hipGraph, MedT 128, 4 images, bench.py's model and batch) with each
criterion of metrics.py: one variant per process, windows of --steps replays after --warmup, wall clock around a synchronized
window as bench.py measures it; the median and the fastest of --windows windows are reported.

    python scripts/seg_loss_time.py --variant {plain,weighted,dice,ce+dice} [--out FILE] [--label TEXT] [--pkg DIR]

  plain     LogNLLLoss()                      medt_ce_fwd / _bwd (the default criterion of train.py)
  weighted  LogNLLLoss(weight=[1, 3])         medt_seg_loss_fwd / _bwd, cross entropy only
  dice      DiceCELoss(ce=0)                  medt_seg_loss_fwd / _bwd, Dice only
  ce+dice   DiceCELoss(weight=[1, 3])         medt_seg_loss_fwd / _bwd, both terms

--pkg: the medical-transformer_amd directory of ANOTHER checkout (with its own built library) to import from, e.g. the parent
commit's for the plain figure on the same box.  Every variant is a command of its own: give each its own time limit and chain them
with &&, so that nothing more starts on the GPU after one of them has failed:

    timeout -k 10 150 python scripts/seg_loss_time.py --variant plain --out profiles/seg_loss.txt && \
    timeout -k 10 150 python scripts/seg_loss_time.py --variant weighted --out profiles/seg_loss.txt && ...
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", required=True, choices=["plain", "weighted", "dice", "ce+dice"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the result line to this file")
    ap.add_argument("--label", default="")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "medical-transformer_amd"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))

    import torch
    import lib as droplib
    import metrics
    from medt_amd.optim import FlatAdam
    from medt_amd.trainer import TrainStep

    dev = torch.device("cuda:0")
    torch.manual_seed(3000)
    model = droplib.models.axialnet.MedT(img_size=128, imgchan=3).to(dev).train()
    opt = FlatAdam(list(model.parameters()), lr=1e-3, weight_decay=1e-5)
    g = torch.Generator().manual_seed(3000)
    x = torch.rand(4, 3, 128, 128, generator=g).to(dev)
    y = torch.randint(0, 2, (4, 128, 128), generator=g).to(dev)
    w = torch.tensor([1.0, 3.0])
    crit = {"plain": lambda: metrics.LogNLLLoss(), "weighted": lambda: metrics.LogNLLLoss(weight=w),
            "dice": lambda: metrics.DiceCELoss(ce=0.0, dice=1.0), "ce+dice": lambda: metrics.DiceCELoss(weight=w)}[a.variant]().to(dev)
    step = TrainStep(model, opt, crit, use_graph=True)
    for _ in range(a.warmup):
        step(x, y)
    times = []
    for _ in range(a.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step(x, y)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / a.steps * 1e3)
    step.check_targets()
    line = (f"{a.variant:<9} {a.label:<14} ms/step median {statistics.median(times):.4f}  min {min(times):.4f}  "
            f"({a.windows} windows of {a.steps} replays after {a.warmup}; MedT 128, 4 images; loss {loss.item():.4f})")
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
