#!/usr/bin/env python
"""Drop-in for the reference's test.py (reference test.py:28-146): same flags; loads a checkpoint written by
train.py (with or without DataParallel's "module." prefix), runs the network in eval mode and writes the
thresholded channel-1 prediction of every validation image as <direc>/<filename>.  The reference reads an
undefined args.aug (test.py:62) and dies; here the flag exists and is ignored.  --surface on adds the surface-distance scores
(HD, HD95, ASSD) of the written masks behind the F1 / mIoU / PA line."""
import argparse
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

import lib
import medt_amd
import metrics
from medt_amd.data import imwrite
from medt_amd.trainer import InferStep

parser = argparse.ArgumentParser(description='MedT')
parser.add_argument('-j', '--workers', default=16, type=int, metavar='N', help='number of data loading workers (default: 8)')
parser.add_argument('--epochs', default=100, type=int, metavar='N', help='number of total epochs to run(default: 1)')
parser.add_argument('--start-epoch', default=0, type=int, metavar='N', help='manual epoch number (useful on restarts)')
parser.add_argument('-b', '--batch_size', default=1, type=int, metavar='N', help='batch size (default: 8)')
parser.add_argument('--learning_rate', default=1e-3, type=float, metavar='LR', help='initial learning rate (default: 0.01)')
parser.add_argument('--momentum', default=0.9, type=float, metavar='M', help='momentum')
parser.add_argument('--weight-decay', '--wd', default=1e-5, type=float, metavar='W', help='weight decay (default: 1e-4)')
parser.add_argument('--train_dataset', type=str)
parser.add_argument('--val_dataset', type=str)
parser.add_argument('--save_freq', type=int, default=5)
parser.add_argument('--modelname', default='off', type=str, help='name of the model to load')
parser.add_argument('--cuda', default="on", type=str, help='switch on/off cuda option (default: off)')
parser.add_argument('--aug', default='off', type=str)
parser.add_argument('--direc', default='./results', type=str, help='directory to save')
parser.add_argument('--crop', type=int, default=None)
parser.add_argument('--device', default='cuda', type=str)
parser.add_argument('--loaddirec', default='load', type=str)
parser.add_argument('--imgsize', type=int, default=None)
parser.add_argument('--gray', default='no', type=str)
parser.add_argument('--gather', type=int, default=4,
                    help='(not in the reference) loader items run per forward replay: in eval mode every image is normalised '
                         'with the running statistics, so batching changes no result; 1 = one replay per image')
parser.add_argument('--window', default='off', choices=['off', 'on'],
                    help='(not in the reference) on: images of any size -- each is cut into overlapping --imgsize windows on the '
                         'device, the windows run --gather per replay and their logits are blended into a map of the '
                         "image's own size (medt_amd.window.WindowInfer)")
parser.add_argument('--window_stride', type=int, default=None, help='window step in pixels with --window on (default: imgsize / 2)')
parser.add_argument('--surface', default='off', choices=['off', 'on'],
                    help='(not in the reference) on: a second score line with the surface-distance scores of the written masks '
                         'against the label maps -- Hausdorff distance, its 95th percentile and the average symmetric surface '
                         'distance, in pixels, means over the images whose mask and label map both have foreground '
                         '(metrics.surface_scores: distance transforms on the device)')


def main():
    args = parser.parse_args()
    if args.gray == "yes":
        from utils_gray import JointTransform2D, ImageToImage2D
        imgchant = 1
    else:
        from utils import JointTransform2D, ImageToImage2D
        imgchant = 3
    crop = (args.crop, args.crop) if args.crop is not None else None
    tf_val = JointTransform2D(crop=crop, p_flip=0, color_jitter_params=None, long_mask=True)
    valloader = DataLoader(ImageToImage2D(args.val_dataset, tf_val), 1, shuffle=True)
    device = torch.device(args.device)
    if device.type == "cuda":
        device = torch.device("cuda", device.index or 0)
        torch.cuda.set_device(device)
    factories = {"axialunet": lib.models.axialunet, "MedT": lib.models.axialnet.MedT,
                 "gatedaxialunet": lib.models.axialnet.gated, "logo": lib.models.axialnet.logo}
    model = factories[args.modelname](img_size=args.imgsize, imgchan=imgchant).to(device)
    state = torch.load(args.loaddirec, map_location=device)
    state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    model.load_state_dict(state)
    model.eval()
    fulldir = args.direc + "/"
    os.makedirs(fulldir, exist_ok=True)
    scores = []
    surface = [] if args.surface == "on" else None     # per-batch metrics.surface_scores of (mask, target > 0), eager, behind the replay
    # forward + the device-side counts as ONE replayed hipGraph per image shape (medt_amd.trainer.InferStep): an eager
    # forward is ~110 dependent launches issued from Python and is host-bound
    infer = InferStep(model)
    # The reference's loop runs ONE image per forward (test.py:106-119, batch size 1).  One replay costs the local branch's
    # dependent chain whatever the batch (0.8 ms for one image, 0.74 ms for four: bench.py's fwd_ms_per_image_bs1 / fwd_ms_per_image),
    # and in eval mode the images of a batch do not interact -- so --gather loader items of the same shape share a replay.  The
    # last, shorter batch is padded with copies of its last image (same graph; the padding's outputs are dropped).
    def run(items):
        xs = torch.cat([it[0] for it in items] + [items[-1][0]] * (gather - len(items))).to(device)
        ys = torch.cat([it[1].long().reshape(1, *it[0].shape[2:]) for it in items] + [items[-1][1].long().reshape(1, *items[-1][0].shape[2:])] * (gather - len(items))).to(device)
        y_out, counts = infer(xs, ys)
        scores.append(counts[:len(items)].clone())
        if surface is not None:                        # the mask the PNG holds (same comparison, on the device) against target > 0
            surface.append(metrics.surface_scores((y_out[:len(items), 1] >= 0.5).to(torch.uint8) * 255,
                                                  (ys[:len(items)] > 0).to(torch.uint8)))
        yHaT = (y_out[:len(items)].detach().cpu().numpy() >= 0.5).astype(np.uint8) * 255
        for k, it in enumerate(items):
            imwrite(fulldir + it[2], yHaT[k, 1, :, :])

    gather = max(1, args.gather)
    pending = []
    if args.window == "on":
        # every loader item may have its own H x W: one image at a time, its windows `gather` per replay; the PNG has the
        # image's size and the counts are those of the whole image
        from medt_amd.window import WindowInfer
        winfer = WindowInfer(model, args.imgsize, gather=gather, stride=args.window_stride)
        for batch_idx, (X_batch, y_batch, *rest) in enumerate(valloader):
            image_filename = rest[0][0] if isinstance(rest[0][0], str) else '%s.png' % str(batch_idx + 1).zfill(3)
            target = y_batch.long().reshape(1, *X_batch.shape[2:]).to(device)
            _, mask, counts = winfer(X_batch.to(device), target)
            scores.append(counts)
            if surface is not None:
                surface.append(metrics.surface_scores(mask.unsqueeze(0), (target > 0).to(torch.uint8)))
            imwrite(fulldir + image_filename, mask.cpu().numpy())
        valloader = ()
    for batch_idx, (X_batch, y_batch, *rest) in enumerate(valloader):
        image_filename = rest[0][0] if isinstance(rest[0][0], str) else '%s.png' % str(batch_idx + 1).zfill(3)
        if pending and pending[0][0].shape != X_batch.shape:
            run(pending)
            pending = []
        pending.append((X_batch, y_batch, image_filename))
        if len(pending) == gather:
            run(pending)
            pending = []
    if pending:
        run(pending)
    if scores:
        f1, iou, pa = metrics.segmentation_scores(torch.cat(scores))
        print("images {}  F1 {:.4f}  mIoU {:.4f}  PA {:.4f}".format(len(f1), f1.mean().item(), iou.mean().item(),
                                                                   pa.mean().item()))
    if surface:
        valid = torch.cat([s["valid"] for s in surface])
        hd, hd95, assd = (torch.cat([s[k] for s in surface])[valid] for k in ("hd", "hd95", "assd"))
        print("surface images {}/{}  HD {:.4f}  HD95 {:.4f}  ASSD {:.4f}".format(
            int(valid.sum()), len(valid), *(v.mean().item() if len(v) else float("nan") for v in (hd, hd95, assd))))


if __name__ == "__main__":
    main()
