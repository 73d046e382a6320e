#!/usr/bin/env python
"""What the border term for touching objects costs, in one process on one tree (after scripts/boundary_time.py):

  1. the replayed training step (TrainStep as a hipGraph, MedT 128, 4 images, bench.py's model and batch) with LogNLLLoss() --
     `--loss ce`, code this feature does not touch;
  2. the same step with BorderLoss(ce=1) -- `--loss ce+border`: + the uint8 mask of the foreground (torch), its connected
     components (ops.label), the two distance maps (ops.object_edt2_sq, two launches), the border partial sums and finalize, the
     accumulating backward;
  3. ops.label + ops.object_edt2_sq alone on blob maps of 4 x 128^2 (a step's masks) and 1 x 1000^2;
  4. the host path a SciPy pipeline takes for the same maps: device -> host copy, ndimage.label, one distance_transform_edt per
     object, a sort over the objects.

The two steps are timed in alternating windows of --steps replays after --warmup (wall clock around a synchronized window, as
bench.py measures); the kernels in windows of --calls calls.  Medians (and the fastest window) of --windows windows.

    timeout -k 10 300 python scripts/border_time.py --out profiles/border.txt
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

    def blobs(N, S, seed=7):
        """uint8 (N,S,S): square blocks of S / 16 pixels (S / 25 from 1000 on: the host path runs one transform per object) at
        30 %, with a one-pixel cut along every other block border: objects that merge, nearly touch, and lie apart."""
        gg = np.random.default_rng(seed)
        b = S // 16 if S < 1000 else S // 25
        coarse = gg.random((N, S // b + 1, S // b + 1)) < 0.3
        m = np.repeat(np.repeat(coarse, b, axis=1), b, axis=2)[:, :S, :S]
        m[:, ::2 * b, :] = False
        m[:, :, ::2 * b] = False
        return m.astype(np.uint8)

    # ---- 1, 2: the replayed step, the two criteria in alternating windows
    g = torch.Generator().manual_seed(3000)
    x = torch.rand(4, 3, 128, 128, generator=g).to(dev)
    y = torch.from_numpy(blobs(4, 128, 3000).astype(np.int64)).to(dev)            # gland-like masks: tens of objects per image
    steps, last = {}, {}
    for name, crit in (("ce", metrics.LogNLLLoss()), ("ce+border", metrics.BorderLoss(w0=10.0, sigma=5.0))):
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
    over = statistics.median(times["ce+border"]) - statistics.median(times["ce"])
    lines.append(f"{'step overhead':<28} ms {over:+.4f}  ({100.0 * over / statistics.median(times['ce']):+.2f} % of the ce step)")
    print(lines[-1], flush=True)

    # ---- 3, 4: labelling + the two distance maps alone, and the host path
    for N, S in ((4, 128), (1, 1000)):
        m = torch.from_numpy(blobs(N, S)).to(dev)
        lab = torch.empty((N, S, S), dtype=torch.int32, device=dev)
        d1, d2 = torch.empty_like(lab), torch.empty_like(lab)

        def device_path():
            ops.label(m, 8, out=lab)
            ops.object_edt2_sq(lab, out=(d1, d2))
        for _ in range(10):
            device_path()
        calls = a.calls if S <= 128 else max(10, a.calls // 10)
        td = [window(device_path, calls, sync) for _ in range(a.windows)]
        te = [window(lambda: ops.object_edt2_sq(lab, out=(d1, d2)), calls, sync) for _ in range(a.windows)]
        note = f"{N} x {S}^2, {int(lab.max())} objects at most per image, {a.windows} windows of {calls} calls, eager launches from Python"
        report(f"label+object_edt2 {N}x{S}^2", td, note)
        report(f"object_edt2_sq {N}x{S}^2", te, note + "; the two launches alone")

        def host():
            mm = m.cpu().numpy()
            out = []
            for n in range(N):
                lb, cnt = ndimage.label(mm[n], structure=np.ones((3, 3)))
                per = np.stack([ndimage.distance_transform_edt(lb != l) for l in range(1, cnt + 1)])
                out.append(np.sort(per, axis=0)[:2])
            return out
        want = host()
        hcalls = 2 if S <= 128 else 1
        th = [window(host, hcalls, sync) for _ in range(3 if S > 128 else a.windows)]
        report(f"SciPy host path {N}x{S}^2", th, f"copy to the host + ndimage.label + one distance_transform_edt per object + sort, "
                                                 f"{len(th)} windows of {hcalls} calls")
        for n in range(N):
            w = np.rint(want[n] ** 2).astype(np.int32)
            assert np.array_equal(d1[n].cpu().numpy(), w[0]) and np.array_equal(d2[n].cpu().numpy(), w[1]), "object_edt2_sq differs from SciPy"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
