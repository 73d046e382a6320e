#!/usr/bin/env python
"""Drop-in for the reference's test.py (reference test.py:28-146): same flags; loads a checkpoint written by
train.py (with or without DataParallel's "module." prefix), runs the network in eval mode and writes the
thresholded channel-1 prediction of every validation image as <direc>/<filename>.  The reference reads an
undefined args.aug (test.py:62) and dies; here the flag exists and is ignored.  --surface on adds the surface-distance scores
(HD, HD95, ASSD) of the written masks behind the F1 / mIoU / PA line, --objects on the object-level scores (object F1 and Dice,
AJI, PQ) behind those, --object_hausdorff on the object-level Hausdorff distance of GlaS behind those; --fill_holes on and
--min_object AREA clean the masks on the device before they are written and scored; --tta flips|d4 averages the logits of the
mirrored (and rotated) views of every image or window before the mask is taken (medt_amd.tta)."""
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
parser.add_argument('--tta', default='off', choices=['off', 'flips', 'd4'],
                    help='(not in the reference) test-time augmentation: the network also runs on mirrored (flips: 4 views) or '
                         'mirrored and rotated (d4: 8 views, square inputs) copies of every image or window, the logits are '
                         'mapped back and averaged on the device, and every mask, PNG and score line describes the average '
                         '(medt_amd.tta.TtaInfer)')
parser.add_argument('--surface', default='off', choices=['off', 'on'],
                    help='(not in the reference) on: a second score line with the surface-distance scores of the written masks '
                         'against the label maps -- Hausdorff distance, its 95th percentile and the average symmetric surface '
                         'distance, in pixels, means over the images whose mask and label map both have foreground '
                         '(metrics.surface_scores: distance transforms on the device)')
parser.add_argument('--objects', default='off', choices=['off', 'on'],
                    help='(not in the reference) on: a further score line with the object-level scores of the written masks against '
                         'the label maps -- GlaS object F1 and object Dice, Aggregated Jaccard Index, panoptic quality -- means over '
                         'the images in which the mask or the label map has an object (metrics.object_scores: connected-component '
                         'labelling on the device)')
parser.add_argument('--object_hausdorff', default='off', choices=['off', 'on'],
                    help='(not in the reference) on: a further score line with the object-level Hausdorff distance of GlaS of the '
                         'written masks against the label maps, in pixels, averaged over the images in which both the mask and '
                         'the label map have an object (metrics.object_hausdorff: labelling and one distance transform per '
                         'object pair on the device); prints only its own line, --objects is not needed')
parser.add_argument('--connectivity', type=int, default=8, choices=[4, 8],
                    help="(not in the reference) connectivity of the objects of --objects, --object_hausdorff and --min_object "
                         "(8: MATLAB's bwlabel)")
parser.add_argument('--min_object', type=int, default=0, metavar='AREA',
                    help='(not in the reference) > 0: objects of fewer than AREA pixels are removed from every mask before it is '
                         'written and scored (medt_amd.ops.remove_small_objects)')
parser.add_argument('--fill_holes', default='off', choices=['off', 'on'],
                    help='(not in the reference) on: the holes of every mask are filled before small objects are removed and the '
                         'mask is written and scored (medt_amd.ops.fill_holes = scipy.ndimage.binary_fill_holes)')


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
    objects = [] if args.objects == "on" else None     # per-batch metrics.object_scores of the same pairs
    obj_hd = [] if args.object_hausdorff == "on" else None   # per-batch metrics.object_hausdorff of the same pairs
    scoring = surface is not None or objects is not None or obj_hd is not None
    cleaning = args.fill_holes == "on" or args.min_object > 0

    def clean(mask, target, like):
        """The clean-ups of a uint8 {0,255} mask batch on the device, holes first, and the {tp, fp, fn, tn} counts of the result
        against target > 0 in the layout and dtype of the replayed counts: every score line describes the files written."""
        from medt_amd import ops
        if args.fill_holes == "on":
            mask = ops.fill_holes(mask)
        if args.min_object > 0:
            mask = ops.remove_small_objects(mask, args.min_object, args.connectivity)
        p, t = (mask != 0).reshape(mask.shape[0], -1), (target > 0).reshape(mask.shape[0], -1)
        counts = torch.stack([(p & t).sum(1), (p & ~t).sum(1), (~p & t).sum(1), (~p & ~t).sum(1)], dim=1).to(like.dtype)
        return mask, counts

    def score(mask, target):
        t = (target > 0).to(torch.uint8)
        if surface is not None:
            surface.append(metrics.surface_scores(mask, t))
        if objects is not None:
            objects.append(metrics.object_scores(mask, t, args.connectivity))
        if obj_hd is not None:
            obj_hd.append(metrics.object_hausdorff(mask, t, args.connectivity))

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
        if tta_infer is not None:      # the views of the batch, `gather` per replay; logits and counts of their mean
            y_out, _, counts = tta_infer(xs[:len(items)], ys[:len(items)])
        else:
            y_out, counts = infer(xs, ys)
        if cleaning:
            mask, cleaned = clean((y_out[:len(items), 1] >= 0.5).to(torch.uint8) * 255, ys[:len(items)], counts)
            scores.append(cleaned)
            score(mask, ys[:len(items)])
            mask = mask.cpu().numpy()
            for k, it in enumerate(items):
                imwrite(fulldir + it[2], mask[k])
            return
        scores.append(counts[:len(items)].clone())
        if scoring:   # the mask the PNG holds (same comparison, on the device) against target > 0
            score((y_out[:len(items), 1] >= 0.5).to(torch.uint8) * 255, ys[:len(items)])
        yHaT = (y_out[:len(items)].detach().cpu().numpy() >= 0.5).astype(np.uint8) * 255
        for k, it in enumerate(items):
            imwrite(fulldir + it[2], yHaT[k, 1, :, :])

    gather = max(1, args.gather)
    pending = []
    tta_infer = None
    if args.tta != "off" and args.window != "on":
        from medt_amd.tta import TtaInfer
        tta_infer = TtaInfer(model, args.tta, gather=gather)
    if args.window == "on":
        # every loader item may have its own H x W: one image at a time, its windows `gather` per replay; the PNG has the
        # image's size and the counts are those of the whole image
        from medt_amd.window import WindowInfer
        winfer = WindowInfer(model, args.imgsize, gather=gather, stride=args.window_stride,
                             tta=None if args.tta == "off" else args.tta)
        for batch_idx, (X_batch, y_batch, *rest) in enumerate(valloader):
            image_filename = rest[0][0] if isinstance(rest[0][0], str) else '%s.png' % str(batch_idx + 1).zfill(3)
            target = y_batch.long().reshape(1, *X_batch.shape[2:]).to(device)
            _, mask, counts = winfer(X_batch.to(device), target)
            if cleaning:
                mask, counts = clean(mask.unsqueeze(0), target, counts)
                mask = mask[0]
            scores.append(counts)
            if scoring:
                score(mask.unsqueeze(0), target)
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
    if objects:
        valid = torch.cat([s["valid"] for s in objects])
        f1o, diceo, aji, pq = (torch.cat([s[k] for s in objects])[valid] for k in ("f1", "dice", "aji", "pq"))
        print("objects images {}/{}  F1obj {:.4f}  Diceobj {:.4f}  AJI {:.4f}  PQ {:.4f}".format(
            int(valid.sum()), len(valid), *(v.mean().item() if len(v) else float("nan") for v in (f1o, diceo, aji, pq))))
    if obj_hd:
        valid = torch.cat([s["valid"] for s in obj_hd])
        hobj = torch.cat([s["hd"] for s in obj_hd])[valid]
        print("object hausdorff images {}/{}  Hobj {:.4f}".format(int(valid.sum()), len(valid),
                                                                  hobj.mean().item() if len(hobj) else float("nan")))


if __name__ == "__main__":
    main()
