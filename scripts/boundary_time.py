#!/usr/bin/env python
"""What the boundary loss costs, in one process on one tree (after scripts/seg_loss_time.py):

  1. the replayed training step (TrainStep as a hipGraph, MedT 128, 4 images, bench.py's model and batch) with
     DiceCELoss(weight=[1, 3]) -- `--loss ce+dice`, code this feature does not touch;
  2. the same step with BoundaryLoss(weight=[1, 3], ce=1, dice=1) -- `--loss ce+dice+boundary`: + the signed distance map of
     the batch's masks (two launches), the boundary partial sums and finalize, the accumulating backward;
  3. ops.signed_edt_sq alone at 4 x 128^2 (a step's masks) and at 1 x 1000^2, next to ops.edt_sq on the same maps as uint8
     (the existing pair; it computes ONE unsigned map);
  4. the host path every SciPy pipeline takes for the same maps: device -> host copy + two distance_transform_edt calls.

The two steps are timed in alternating windows of --steps replays after --warmup (wall clock around a synchronized window, as
bench.py measures); the kernels in windows of --calls calls.  Medians (and the fastest window) of --windows windows.

    timeout -k 10 300 python scripts/boundary_time.py --out profiles/boundary.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def window(fn, reps, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "medical-transformer_amd"))

    import numpy as np
    import torch
    from scipy import ndimage
    import lib as droplib
    import metrics
    from medt_amd import ops
    from medt_amd.optim import FlatAdam
    from medt_amd.trainer import TrainStep

    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    lines = []

    def report(name, times, note):
        lines.append(f"{name:<28} ms median {statistics.median(times):.4f}  min {min(times):.4f}  ({note})")
        print(lines[-1], flush=True)

    # ---- 1, 2: the replayed step, the two criteria in alternating windows
    g = torch.Generator().manual_seed(3000)
    x = torch.rand(4, 3, 128, 128, generator=g).to(dev)
    y = torch.randint(0, 2, (4, 128, 128), generator=g)
    y[:, 32:96, 40:104] = 1                       # a gland-sized blob among the noise: distances of tens of pixels, as in a mask
    y = y.to(dev)
    w = torch.tensor([1.0, 3.0])
    steps, last = {}, {}
    for name, crit in (("ce+dice", metrics.DiceCELoss(weight=w)), ("ce+dice+boundary", metrics.BoundaryLoss(alpha=0.01, weight=w, dice=1.0))):
        torch.manual_seed(3000)
        model = droplib.models.axialnet.MedT(img_size=128, imgchan=3).to(dev).train()
        opt = FlatAdam(list(model.parameters()), lr=1e-3, weight_decay=1e-5)
        steps[name] = TrainStep(model, opt, crit.to(dev), use_graph=True)
        for _ in range(a.warmup):
            steps[name](x, y)
    times = {name: [] for name in steps}
    for _ in range(a.windows):
        for name, step in steps.items():
            def one(step=step, name=name):
                last[name] = step(x, y)
            times[name].append(window(one, a.steps, sync))
    for name, step in steps.items():
        step.check_targets()
        report("step " + name, times[name], f"{a.windows} alternating windows of {a.steps} replays after {a.warmup}; MedT 128, 4 images; "
                                            f"loss {last[name].item():.4f}")
    over = statistics.median(times["ce+dice+boundary"]) - statistics.median(times["ce+dice"])
    lines.append(f"{'step overhead':<28} ms {over:+.4f}  ({100.0 * over / statistics.median(times['ce+dice']):+.2f} % of the ce+dice step)")
    print(lines[-1], flush=True)

    # ---- 3, 4: the distance maps alone, and the host path
    for N, S in ((4, 128), (1, 1000)):
        gg = np.random.default_rng(7)
        coarse = gg.random((N, S // 8 + 1, S // 8 + 1)) < 0.3
        t = torch.from_numpy(np.repeat(np.repeat(coarse, 8, axis=1), 8, axis=2)[:, :S, :S].astype(np.int64)).to(dev)
        m = (t * 255).to(torch.uint8)
        out, out_u = torch.empty((N, S, S), dtype=torch.int32, device=dev), torch.empty((N, S, S), dtype=torch.int32, device=dev)
        for _ in range(10):
            ops.signed_edt_sq(t, out=out)
            ops.edt_sq(m, out=out_u)
        calls = a.calls if S <= 128 else max(10, a.calls // 10)
        ts = [window(lambda: ops.signed_edt_sq(t, out=out), calls, sync) for _ in range(a.windows)]
        tu = [window(lambda: ops.edt_sq(m, out=out_u), calls, sync) for _ in range(a.windows)]
        note = f"{N} x {S}^2, {a.windows} windows of {calls} calls, eager launches from Python"
        report(f"signed_edt_sq {N}x{S}^2", ts, note + "; two launches, both maps")
        report(f"edt_sq {N}x{S}^2", tu, note + "; the existing pair, one unsigned map")

        def host():
            f = t.cpu().numpy() == 1
            return [ndimage.distance_transform_edt(~f[n]) for n in range(N)], [ndimage.distance_transform_edt(f[n]) for n in range(N)]
        host()
        hcalls = 5 if S <= 128 else 2
        th = [window(host, hcalls, sync) for _ in range(a.windows)]
        report(f"SciPy host path {N}x{S}^2", th, f"copy to the host + two distance_transform_edt per image, {a.windows} windows of {hcalls} calls")
        want = np.stack([np.where(f, -np.rint(i ** 2), np.rint(o ** 2)) for f, o, i in zip((t.cpu().numpy() == 1), *host())])
        assert np.array_equal(out.cpu().numpy(), want.astype(np.int32)), "signed_edt_sq differs from SciPy"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
