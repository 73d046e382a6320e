#!/usr/bin/env python
"""Drop-in for the reference's test.py (reference test.py:28-146): same flags; loads a checkpoint written by
train.py (with or without DataParallel's "module." prefix), runs the network in eval mode and writes the
thresholded channel-1 prediction of every validation image as <direc>/<filename>.  The reference reads an
undefined args.aug (test.py:62) and dies; here the flag exists and is ignored.  --surface on adds the surface-distance scores
(HD, HD95, ASSD) of the written masks behind the F1 / mIoU / PA line, --objects on the object-level scores (object F1 and Dice,
AJI, PQ) behind those, --object_hausdorff on the object-level Hausdorff distance of GlaS behind those; --fill_holes on and
--min_object AREA clean the masks on the device before they are written and scored; --tta flips|d4 averages the logits of the
mirrored (and rotated) views of every image or window before the mask is taken (medt_amd.tta); --split on splits touching
objects of the cleaned mask on the device before --objects and --object_hausdorff count them (medt_amd.ops.split_objects),
--instance_labels DIR gives those two scores ground-truth instances, --write_instances on writes the split label maps."""
import argparse
import os

import torch
from torch.utils.data import DataLoader

import lib
import medt_amd
import metrics
from medt_amd.data import imwrite, item_filename
from medt_amd.trainer import InferStep, padded_batch, run_padded

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
parser.add_argument('--split', default='off', choices=['off', 'on'],
                    help='(not in the reference) on: touching objects of every mask are split on the device -- peak markers of the '
                         'distance transform, marker-controlled growth (medt_amd.ops.split_objects) -- behind --fill_holes and '
                         '--min_object, at --connectivity; --objects and --object_hausdorff score the split label map.  The PNG, '
                         'the F1 / mIoU / PA line and --surface describe the same foreground and do not change')
parser.add_argument('--split_distance', type=int, default=None, metavar='R',
                    help='with --split on: radius of the window whose depth maximum makes a marker, 1 .. 32 pixels (default 7)')
parser.add_argument('--split_tolerance', type=int, default=None, metavar='T',
                    help='with --split on: a pixel within T pixels of depth of its window maximum is a marker, 0 .. 8 (default 1)')
parser.add_argument('--instance_labels', type=str, default=None, metavar='DIR',
                    help='(not in the reference) ground-truth instances for --objects and --object_hausdorff: DIR/<stem>.png (8- or '
                         '16-bit, value = instance id, 0 = background) or DIR/<stem>.npy of the image\'s size; ids are renumbered '
                         'in raster order of their first pixel.  Not with --crop')
parser.add_argument('--write_instances', default='off', choices=['off', 'on'],
                    help='(not in the reference) with --split on: also writes <stem>_inst.png, the split label map as a 16-bit PNG')

# the score lines behind "images ...": (line prefix = the flag's name with a blank for its underscore, metric of a {0,255} mask
# batch and a {0,1} target batch on the device -> per-batch dictionary with "valid", the keys the line shows, their labels)
SUMMARY = (("surface", lambda mask, t, conn: metrics.surface_scores(mask, t), ("hd", "hd95", "assd"), ("HD", "HD95", "ASSD")),
           ("objects", metrics.object_scores, ("f1", "dice", "aji", "pq"), ("F1obj", "Diceobj", "AJI", "PQ")),
           ("object hausdorff", metrics.object_hausdorff, ("hd",), ("Hobj",)))


def group_items(loader, gather):
    """The loader's items as (X, y, file name), in runs of at most `gather` consecutive items of equal image shape: what one
    forward replay takes.  gather = 1 gives single items."""
    pending = []
    for batch_idx, (X_batch, y_batch, *rest) in enumerate(loader):
        if pending and pending[0][0].shape != X_batch.shape:
            yield pending
            pending = []
        pending.append((X_batch, y_batch, item_filename(rest, batch_idx)))
        if len(pending) == gather:
            yield pending
            pending = []
    if pending:
        yield pending


def images_line(counts):
    f1, iou, pa = metrics.segmentation_scores(counts)
    return "images {}  F1 {:.4f}  mIoU {:.4f}  PA {:.4f}".format(len(f1), f1.mean().item(), iou.mean().item(), pa.mean().item())


def summary_line(prefix, keys, labels, batches, totals=False):
    """One line of SUMMARY from its per-batch dictionaries: the means over the valid images, nan when there is none.  totals:
    behind them the objects counted on either side, summed over all images (the object lines under --split on or
    --instance_labels, where the counts are what those flags change)."""
    valid = torch.cat([s["valid"] for s in batches])
    means = [v.mean().item() if len(v) else float("nan") for v in (torch.cat([s[k] for s in batches])[valid] for k in keys)]
    line = "{} images {}/{}".format(prefix, int(valid.sum()), len(valid)) + "".join(
        "  {} {:.4f}".format(label, m) for label, m in zip(labels, means))
    if totals:
        line += "  Npred {}  Ngt {}".format(*(int(torch.cat([s[k] for s in batches]).sum()) for k in ("n_pred", "n_gt")))
    return line


def split_options(args):
    """The checked --split* / --instance_labels / --write_instances flags -> (distance, tolerance) or None without --split on.
    Refusals leave through parser.error before any file or device is touched."""
    if args.split != "on":
        for flag in ("split_distance", "split_tolerance"):
            if getattr(args, flag) is not None:
                parser.error("--%s: add --split on" % flag)
        if args.write_instances == "on":
            parser.error("--write_instances: add --split on")
    distance = 7 if args.split_distance is None else args.split_distance
    tolerance = 1 if args.split_tolerance is None else args.split_tolerance
    if not 1 <= distance <= 32:
        parser.error("--split_distance: %d: 1 .. 32 pixels" % distance)
    if not 0 <= tolerance <= 8:
        parser.error("--split_tolerance: %d: 0 .. 8 pixels" % tolerance)
    if args.instance_labels is not None:
        if args.crop is not None:
            parser.error("--instance_labels: the instance maps have the images' own size: not with --crop")
        if not os.path.isdir(args.instance_labels):
            parser.error("--instance_labels: %s is not a directory" % args.instance_labels)
    return (distance, tolerance) if args.split == "on" else None


def main():
    args = parser.parse_args()
    split = split_options(args)
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
    gather = max(1, args.gather)
    scores = []
    # the score lines asked for, each with its per-batch dictionaries of (mask, target > 0): eager, behind the replay
    scored = [(row, []) for row in SUMMARY if getattr(args, row[0].replace(" ", "_")) == "on"]
    object_lines = any(row[0] != "surface" for row, _ in scored)      # the lines that count objects: what --split changes

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

    def label_maps(items):
        return torch.cat([it[1].long().reshape(1, *it[0].shape[2:]) for it in items])

    def to_mask(logits):
        return (logits[:, 1] >= 0.5).to(torch.uint8) * 255

    # One predictor: items (of group_items) -> the uint8 {0,255} mask (n,H,W) on the device, its (n,4) counts, the int64 label
    # maps (n,H,W) on the device.  Each runs forward + counts as replayed hipGraphs (medt_amd.trainer.InferStep): an eager
    # forward is ~110 dependent launches issued from Python and is host-bound.
    if args.window == "on":
        # every loader item may have its own H x W: one image at a time, its windows `gather` per replay; the PNG has the
        # image's size and the counts are those of the whole image
        from medt_amd.window import WindowInfer
        winfer = WindowInfer(model, args.imgsize, gather=gather, stride=args.window_stride,
                             tta=None if args.tta == "off" else args.tta)

        def predict(items):
            target = label_maps(items).to(device)
            _, mask, counts = winfer(items[0][0].to(device), target)
            return mask.unsqueeze(0), counts, target
    elif args.tta != "off":
        from medt_amd.tta import TtaInfer
        tta_infer = TtaInfer(model, args.tta, gather=gather)

        def predict(items):        # the views of the group, `gather` per replay; mask and counts of their mean
            target = label_maps(items).to(device)
            merged, _, counts = tta_infer(torch.cat([it[0] for it in items]).to(device), target)
            return to_mask(merged), counts, target
    else:
        # The reference's loop runs ONE image per forward (test.py:106-119, batch size 1).  One replay costs the local branch's
        # dependent chain whatever the batch (0.8 ms for one image, 0.74 ms for four: bench.py's fwd_ms_per_image_bs1 /
        # fwd_ms_per_image), and in eval mode the images of a batch do not interact -- so a group shares a replay, the counts
        # inside it.  A shorter group is padded with copies of its last image (same graph; the padding's outputs are dropped).
        infer = InferStep(model)

        def predict(items):
            n, shape = len(items), items[0][0].shape
            xs = padded_batch(n, gather, shape[1:], device)
            ys = padded_batch(n, gather, shape[2:], device, torch.int64)
            xs[:n].copy_(torch.cat([it[0] for it in items]))
            ys[:n].copy_(label_maps(items))
            logits, counts = run_padded(infer, xs, n, gather, ys)
            return to_mask(logits), counts, ys[:n]

    for items in group_items(valloader, 1 if args.window == "on" else gather):
        mask, counts, target = predict(items)
        if args.fill_holes == "on" or args.min_object > 0:
            mask, counts = clean(mask, target, counts)
        scores.append(counts)
        objects = None
        if split is not None and (object_lines or args.write_instances == "on"):
            # the same foreground, its touching objects apart: what the object-level lines count and --write_instances writes
            from medt_amd import ops
            objects, _ = ops.split_objects(mask, split[0], split[1], args.connectivity)
        if scored:                 # the mask the PNG holds against target > 0
            t = (target > 0).to(torch.uint8)
            instances = None
            if args.instance_labels is not None and object_lines:
                import numpy
                from medt_amd.instances import read_instances
                instances = torch.from_numpy(numpy.stack([read_instances(args.instance_labels, it[2], tuple(mask.shape[1:]))[0]
                                                          for it in items])).to(mask.device)
            for (name, metric, _, _), batches in scored:
                if name != "surface" and (objects is not None or instances is not None):
                    batches.append(metric(mask if objects is None else objects, t if instances is None else instances,
                                          args.connectivity, labelled=(objects is not None, instances is not None)))
                else:
                    batches.append(metric(mask, t, args.connectivity))
        mask = mask.cpu().numpy()
        for k, it in enumerate(items):
            imwrite(fulldir + it[2], mask[k])
        if args.write_instances == "on":
            from medt_amd.instances import write_instances
            objects = objects.cpu().numpy()
            for k, it in enumerate(items):
                write_instances(fulldir + os.path.splitext(it[2])[0] + "_inst.png", objects[k])
    if scores:
        print(images_line(torch.cat(scores)))
        for (prefix, _, keys, labels), batches in scored:
            print(summary_line(prefix, keys, labels, batches,
                               totals=prefix != "surface" and (split is not None or args.instance_labels is not None)))


if __name__ == "__main__":
    main()
