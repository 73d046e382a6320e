#!/usr/bin/env python
"""What test-time augmentation (medt_amd.tta) costs next to the forward replays it drives.  MedT, d4 (8 views), per --gather:
  (a) TtaInfer on --n images: tta_expand, the replays with the copy of each replay's logits, tta_merge;
  (b) the same InferStep replays with the views built and merged by torch ops (flip / transpose / contiguous / stack,
      sequential adds and one division) -- what a user writes without this module;
  (c) the replays alone;
  (d) WindowInfer(tta=d4) against WindowInfer on one --H x --W image at --stride.
hipEvents around each call, median over --calls calls after --warmup.

    python scripts/tta_time.py [--size 128 --n 4 --H 1000 --W 1000 --stride 64 --calls 25 --warmup 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-transformer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import lib as droplib  # noqa: E402
from medt_amd.trainer import InferStep  # noqa: E402
from medt_amd.tta import VIEWS_D4, TtaInfer, view_codes  # noqa: E402
from medt_amd.window import WindowInfer  # noqa: E402


def timed(fn, calls, warmup):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for k in range(warmup + calls):
        a, b = ev[max(0, k - warmup)]
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def torch_views(x, codes):
    out = []
    for n in range(x.shape[0]):
        for v in codes:
            t = x[n].transpose(-1, -2) if v & 4 else x[n]
            dims = [d for b, d in ((2, -2), (1, -1)) if v & b]
            out.append((t.flip(dims) if dims else t).contiguous())
    return torch.stack(out)


def torch_merge(logits, codes):
    V = len(codes)
    merged = []
    for n in range(logits.shape[0] // V):
        acc = None
        for j, v in enumerate(codes):
            l = logits[n * V + j]
            dims = [d for b, d in ((2, -2), (1, -1)) if v & b]
            m = l.flip(dims) if dims else l
            m = m.transpose(-1, -2) if v & 4 else m
            acc = m.clone() if acc is None else acc + m
        merged.append(acc / float(V))
    merged = torch.stack(merged)
    return merged, (merged[:, 1] >= 0.5).to(torch.uint8) * 255


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--H", type=int, default=1000)
    ap.add_argument("--W", type=int, default=1000)
    ap.add_argument("--stride", type=int, default=64)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gathers", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(3000)
    S = a.size
    model = droplib.models.axialnet.MedT(img_size=S, imgchan=3).to(dev).eval()
    x = torch.rand(a.n, 3, S, S, device=dev)
    image = torch.rand(3, a.H, a.W, device=dev)
    codes = view_codes(VIEWS_D4)
    nv = a.n * len(codes)
    lines = [f"MedT {S}, fp32, d4 (8 views), median of {a.calls} calls after {a.warmup} (ms)",
             f"{'gather':>6} {'replays':>7} {'a_tta':>8} {'b_torch':>8} {'c_bare':>8} {'a-c':>8} {'b-c':>8} {'(a-c)/c':>8} "
             f"{'win_tta':>9} {'win':>9} {'ratio':>6}"]
    for g in a.gathers:
        R = -(-nv // g)
        tta = TtaInfer(model, VIEWS_D4, gather=g)
        bare = InferStep(model)
        xb = torch.rand(g, 3, S, S, device=dev)

        def do_torch():
            views = torch_views(x, codes)
            pad = R * g - nv
            if pad:
                views = torch.cat([views] + [views[-1:]] * pad)
            logits = torch.cat([bare(views[b:b + g])[:min(g, nv - b)].clone() for b in range(0, nv, g)])
            return torch_merge(logits, codes)

        def do_bare():
            for _ in range(R):
                bare(xb)

        got, want = tta(x), do_torch()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "TtaInfer and the torch composition disagree"
        ta, tb, tc = timed(lambda: tta(x), a.calls, a.warmup), timed(do_torch, a.calls, a.warmup), timed(do_bare, a.calls, a.warmup)
        wt, w0 = WindowInfer(model, S, gather=g, stride=a.stride, tta=VIEWS_D4), WindowInfer(model, S, gather=g, stride=a.stride)
        calls, warm = max(3, a.calls // 5), max(1, a.warmup // 2)
        tw, t0 = timed(lambda: wt(image), calls, warm), timed(lambda: w0(image), calls, warm)
        lines.append(f"{g:>6} {R:>7} {ta:>8.3f} {tb:>8.3f} {tc:>8.3f} {ta - tc:>8.3f} {tb - tc:>8.3f} {(ta - tc) / tc:>8.1%} "
                     f"{tw:>9.2f} {t0:>9.2f} {tw / t0:>6.2f}")
        print(lines[-1], flush=True)
    lines.append(f"a_tta: TtaInfer on {a.n} images ({nv} views); b_torch: the same replays with the views built and merged by torch ops; "
                 f"c_bare: the replays alone at that batch size; win_tta / win: WindowInfer with and without tta=d4 on one "
                 f"{a.H}x{a.W} image at stride {a.stride} (median of fewer calls); ratio: win_tta / win (8 views).")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
