#!/usr/bin/env python
"""Drop-in for the reference's train.py: same flags, defaults, stdout lines and checkpoint paths
(reference train.py:30-66, 93-117, 126-217), driving the MI355X-native model.

Differences, all host-side plumbing:
  * data loading uses PIL/numpy (utils.py here) -- cv2/torchvision/skimage are not in the MI355X image;
  * --device is honoured (the reference hard-codes "cuda", train.py:93); the kernels need a GPU;
  * multi-GPU = one process per GPU under torchrun (torch.distributed, RCCL) with a single flat-bucket
    gradient all-reduce per step, instead of nn.DataParallel(device_ids=[0,1]) (train.py:104-107);
    --batch_size stays the GLOBAL batch and is split over the ranks, as DataParallel splits it;
  * batches are decoded, pinned and copied to the GPU one step ahead (medt_amd.data.DevicePrefetcher);
  * the step runs as a replayed hipGraph with a fused flat Adam (medt_amd.trainer); --eager disables it;
  * --synthetic N writes N synthetic PNG pairs into --train_dataset first (BASELINE.json config 1 plumbing);
  * --loss {ce,dice,ce+dice} and --class_weights "w0,w1" pick the criterion (metrics.DiceCELoss / LogNLLLoss(weight)); the
    defaults are the reference's LogNLLLoss();
  * --loss ce+boundary / dice+boundary / ce+dice+boundary add the boundary loss of Kervadec et al. (metrics.BoundaryLoss; the
    signed distance map is computed on the GPU from the batch's own masks); its weight starts at --boundary_alpha, grows by
    --boundary_step after every epoch up to --boundary_max, and is printed as `boundary alpha` before the epoch line;
  * --loss ce+border / dice+border / ce+dice+border add U-Net's border weight for touching objects as a term of the loss
    (metrics.BorderLoss; the objects are the connected components of the batch's own masks, labelled and measured on the GPU):
    --border_w0 is its weight, --border_sigma its width in pixels, --border_connectivity {4,8} what counts as one object
    (printed once as `border w0 .. sigma .. connectivity ..`);
  * --aug on moves the joint transform to the GPU (medt_amd.augment: the uint8 image is uploaded, two kernels crop, flip,
    jitter and map it); --aug_jitter "b,c,s,h" and --aug_affine P add the colour jitter and the random affine map the
    reference's JointTransform2D has and its train.py never enables; --aug off (the default) is the host transform as before;
  * --aug_elastic P adds U-Net's elastic deformation to --aug on: with probability P an item gets a cubic B-spline deformation
    over --aug_elastic_grid x --aug_elastic_grid cells of random displacements with standard deviation --aug_elastic_sigma
    pixels, the image sampled bilinearly, the mask nearest (printed once as `elastic p .. grid .. sigma ..`);
  * the per-step threshold-and-copy-to-host of the output (train.py:142-152) is dropped: its result is unused.
"""
import argparse
import os

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader

import lib
from metrics import BorderLoss, BoundaryLoss, DiceCELoss, LogNLLLoss
from medt_amd import dp
from medt_amd.data import DevicePrefetcher, imwrite, item_filename, make_synthetic_dataset
from medt_amd.optim import FlatAdam
from medt_amd.trainer import InferStep, TrainStep

parser = argparse.ArgumentParser(description='MedT')
parser.add_argument('-j', '--workers', default=16, type=int, metavar='N', help='number of data loading workers (default: 8)')
parser.add_argument('--epochs', default=400, type=int, metavar='N', help='number of total epochs to run(default: 400)')
parser.add_argument('--start-epoch', default=0, type=int, metavar='N', help='manual epoch number (useful on restarts)')
parser.add_argument('-b', '--batch_size', default=1, type=int, metavar='N', help='batch size (default: 1)')
parser.add_argument('--learning_rate', default=1e-3, type=float, metavar='LR', help='initial learning rate (default: 0.001)')
parser.add_argument('--momentum', default=0.9, type=float, metavar='M', help='momentum')
parser.add_argument('--weight-decay', '--wd', default=1e-5, type=float, metavar='W', help='weight decay (default: 1e-5)')
parser.add_argument('--train_dataset', required=True, type=str)
parser.add_argument('--val_dataset', type=str)
parser.add_argument('--save_freq', type=int, default=10)
parser.add_argument('--modelname', default='MedT', type=str, help='type of model')
parser.add_argument('--cuda', default="on", type=str, help='switch on/off cuda option (default: off)')
parser.add_argument('--aug', default='off', type=str, help='turn on img augmentation (default: False)')
parser.add_argument('--aug_jitter', default=None, type=str, help='with --aug on: colour jitter ranges "brightness,contrast,saturation,hue", e.g. "0.2,0.2,0.2,0.05"')
parser.add_argument('--aug_affine', default=None, type=float, help='with --aug on: probability of the random affine map (rotation, shear, scale 2, translation)')
parser.add_argument('--aug_elastic', default=None, type=float, help='with --aug on: probability of the elastic deformation (cubic B-spline over a coarse grid of random displacements)')
parser.add_argument('--aug_elastic_grid', default=None, type=int, help='with --aug_elastic: cells per side of the coarse grid, 1 .. 8 (default: 3)')
parser.add_argument('--aug_elastic_sigma', default=None, type=float, help='with --aug_elastic: standard deviation of the displacements in pixels (default: 4.0)')
parser.add_argument('--load', default='default', type=str, help='load a pretrained model')
parser.add_argument('--save', default='default', type=str, help='save the model')
parser.add_argument('--direc', default='./medt', type=str, help='directory to save')
parser.add_argument('--crop', type=int, default=None)
parser.add_argument('--imgsize', type=int, default=None)
parser.add_argument('--device', default='cuda', type=str)
parser.add_argument('--gray', default='no', type=str)
parser.add_argument('--synthetic', type=int, default=0, help='write this many synthetic PNG pairs into the dataset dirs first')
parser.add_argument('--eager', action='store_true', help='no hipGraph replay')
parser.add_argument('--loss', default='ce', choices=['ce', 'dice', 'ce+dice', 'ce+boundary', 'dice+boundary', 'ce+dice+boundary',
                                                      'ce+border', 'dice+border', 'ce+dice+border'],
                    help='cross entropy, soft Dice or their sum, +boundary: plus the boundary loss, +border: plus the border weight '
                         'for touching objects (default: ce)')
parser.add_argument('--class_weights', default=None, type=str, help='comma-separated class weights of the cross entropy, e.g. "1,3"')
parser.add_argument('--boundary_alpha', default=None, type=float, help='with a +boundary loss: weight of the boundary term in the first epoch (default: 0.01)')
parser.add_argument('--boundary_step', default=None, type=float, help='with a +boundary loss: added to the weight after every epoch (default: 0.01)')
parser.add_argument('--boundary_max', default=None, type=float, help='with a +boundary loss: the weight stops growing here (default: 1.0)')
parser.add_argument('--border_w0', default=None, type=float, help='with a +border loss: weight of the border term (default: 10)')
parser.add_argument('--border_sigma', default=None, type=float, help='with a +border loss: width of the border weight in pixels (default: 5)')
parser.add_argument('--border_connectivity', default=None, type=int, choices=[4, 8], help='with a +border loss: connectivity of the objects (default: 8)')

NUM_CLASSES = 2          # every network of lib.models ends in a 2-channel adjust convolution


def split_loss(loss):
    """--loss -> (region, extra): "ce", "dice" or "ce+dice", and None, "boundary" or "border"."""
    region, _, extra = loss.rpartition("+")
    return (region, extra) if extra in ("boundary", "border") else (loss, None)


def make_boundary(loss, alpha, step, vmax):
    """None without a +boundary loss, else the schedule of the boundary term's weight: alpha in the first epoch, + step after
    every epoch, at most max."""
    if split_loss(loss)[1] != "boundary":
        if alpha is not None or step is not None or vmax is not None:
            raise SystemExit("--boundary_alpha / --boundary_step / --boundary_max belong to the boundary loss: "
                             "use --loss ce+boundary, dice+boundary or ce+dice+boundary")
        return None
    sched = {"alpha": 0.01 if alpha is None else alpha, "step": 0.01 if step is None else step, "max": 1.0 if vmax is None else vmax}
    if not (sched["alpha"] >= 0.0 and sched["step"] >= 0.0 and sched["max"] >= sched["alpha"]):
        raise SystemExit("--boundary_alpha, --boundary_step >= 0 and --boundary_max >= --boundary_alpha expected, got %r" % (sched,))
    return sched


def boundary_alpha(sched, epoch):
    return min(sched["max"], sched["alpha"] + sched["step"] * epoch)


def make_border(loss, w0, sigma, connectivity):
    """None without a +border loss, else the settings of the border term: its weight, its width, the objects' connectivity."""
    if split_loss(loss)[1] != "border":
        if w0 is not None or sigma is not None or connectivity is not None:
            raise SystemExit("--border_w0 / --border_sigma / --border_connectivity belong to the border term: "
                             "use --loss ce+border, dice+border or ce+dice+border")
        return None
    border = {"w0": 10.0 if w0 is None else w0, "sigma": 5.0 if sigma is None else sigma,
              "connectivity": 8 if connectivity is None else connectivity}
    if not (border["w0"] >= 0.0 and 0.0 < border["sigma"] < float("inf")):
        raise SystemExit("--border_w0 >= 0 and --border_sigma > 0 expected, got %r" % (border,))
    return border


def make_criterion(loss, class_weights, boundary=None, border=None):
    weight = None
    region, extra = split_loss(loss)
    if class_weights is not None:
        try:
            weight = [float(w) for w in class_weights.split(",")]
        except ValueError:
            raise SystemExit("--class_weights: comma-separated numbers expected, got %r" % class_weights)
        if len(weight) != NUM_CLASSES:
            raise SystemExit("--class_weights: %d weights given, the networks have %d classes" % (len(weight), NUM_CLASSES))
        if region == "dice":
            raise SystemExit("--class_weights weigh the cross entropy: use --loss ce or ce+dice")
        weight = torch.tensor(weight, dtype=torch.float32)
    scales = {"weight": weight, "ce": 0.0 if region == "dice" else 1.0, "dice": 0.0 if region == "ce" else 1.0}
    if extra == "border":
        border = make_border(loss, None, None, None) if border is None else border
        return BorderLoss(w0=border["w0"], sigma=border["sigma"], connectivity=border["connectivity"], **scales)
    if extra == "boundary":
        return BoundaryLoss(alpha=0.01 if boundary is None else boundary["alpha"], **scales)
    if loss == "ce":
        return LogNLLLoss() if weight is None else LogNLLLoss(weight=weight)         # the defaults: reference train.py:110
    return DiceCELoss(**scales)


def make_augment(aug, aug_jitter, aug_affine, aug_elastic=None, aug_elastic_grid=None, aug_elastic_sigma=None):
    """None for --aug off (the host transform, as before), else the settings of the device-side transform: the defaults are
    the host transform's (crop from --crop, flip 0.5, no jitter, no affine map).  An "elastic" entry only with --aug_elastic > 0."""
    if aug != "on":                 # (any other value was parsed and ignored before the device path existed: still the host path)
        if aug_jitter is not None or aug_affine is not None:
            raise SystemExit("--aug_jitter / --aug_affine belong to the device-side augmentation: add --aug on")
        if aug_elastic is not None or aug_elastic_grid is not None or aug_elastic_sigma is not None:
            raise SystemExit("--aug_elastic / --aug_elastic_grid / --aug_elastic_sigma belong to the device-side augmentation: add --aug on")
        return None
    from medt_amd.augment import ELASTIC_MAX_GRID, parse_jitter
    jitter = None
    if aug_jitter is not None:
        try:
            jitter = parse_jitter(aug_jitter)
        except ValueError as e:
            raise SystemExit("--aug_jitter: %s" % e)
    p_affine = 0.0 if aug_affine is None else aug_affine
    if not 0.0 <= p_affine <= 1.0:
        raise SystemExit("--aug_affine: a probability in [0, 1] expected, got %r" % aug_affine)
    augment = {"jitter": jitter, "p_affine": p_affine}
    if aug_elastic is None:
        if aug_elastic_grid is not None or aug_elastic_sigma is not None:
            raise SystemExit("--aug_elastic_grid / --aug_elastic_sigma belong to the elastic deformation: add --aug_elastic P")
        return augment
    grid = 3 if aug_elastic_grid is None else aug_elastic_grid
    sigma = 4.0 if aug_elastic_sigma is None else aug_elastic_sigma
    if not 0.0 <= aug_elastic <= 1.0:
        raise SystemExit("--aug_elastic: a probability in [0, 1] expected, got %r" % aug_elastic)
    if not 1 <= grid <= ELASTIC_MAX_GRID:
        raise SystemExit("--aug_elastic_grid: 1 .. %d cells per side expected, got %r" % (ELASTIC_MAX_GRID, grid))
    if not 0.0 <= sigma < float("inf"):
        raise SystemExit("--aug_elastic_sigma: a finite standard deviation >= 0 in pixels expected, got %r" % sigma)
    if aug_elastic > 0.0:
        augment["elastic"] = {"p": aug_elastic, "grid": grid, "sigma": sigma}
    return augment


def main():
    args = parser.parse_args()
    boundary = make_boundary(args.loss, args.boundary_alpha, args.boundary_step, args.boundary_max)    # (so do --boundary_* alone)
    border = make_border(args.loss, args.border_w0, args.border_sigma, args.border_connectivity)        # (and --border_* alone)
    criterion = make_criterion(args.loss, args.class_weights, boundary, border)      # (a bad --class_weights ends the run before any work)
    augment = make_augment(args.aug, args.aug_jitter, args.aug_affine, args.aug_elastic, args.aug_elastic_grid,
                           args.aug_elastic_sigma)                                   # (so does a bad --aug_* combination)
    direc, modelname, imgsize = args.direc, args.modelname, args.imgsize
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    if args.gray == "yes":
        from utils_gray import JointTransform2D, ImageToImage2D, Image2D
        imgchant = 1
    else:
        from utils import JointTransform2D, ImageToImage2D, Image2D
        imgchant = 3
    device = torch.device(args.device)
    if device.type == "cuda":
        if device.index is None:
            device = torch.device("cuda", local_rank)
        torch.cuda.set_device(device)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl" if device.type == "cuda" else "gloo")
    if args.synthetic:
        # rank 0 writes the PNGs; nobody lists the directories before they are complete
        if rank == 0:
            make_synthetic_dataset(args.train_dataset, args.synthetic, imgsize or 128, 3000, args.gray == "yes")
            if args.val_dataset and args.val_dataset != args.train_dataset:
                make_synthetic_dataset(args.val_dataset, max(2, args.synthetic // 4), imgsize or 128, 3001,
                                       args.gray == "yes")
        if world > 1:
            dist.barrier()

    crop = (args.crop, args.crop) if args.crop is not None else None
    tf_train = JointTransform2D(crop=crop, p_flip=0.5, color_jitter_params=None, long_mask=True)
    tf_val = JointTransform2D(crop=crop, p_flip=0, color_jitter_params=None, long_mask=True)
    device_aug = elastic = None
    if augment is not None:        # the draws stay per item on the host; crop / flip / jitter / affine run on the device
        from medt_amd.augment import DeviceAugment, RawJointTransform2D
        elastic = augment.get("elastic")
        tf_train = RawJointTransform2D(crop=crop, p_flip=0.5, jitter=augment["jitter"], p_affine=augment["p_affine"],
                                       **({"elastic": elastic} if elastic else {}))
        device_aug = DeviceAugment(crop)
    train_dataset = ImageToImage2D(args.train_dataset, tf_train)
    val_dataset = ImageToImage2D(args.val_dataset or args.train_dataset, tf_val)
    Image2D(args.val_dataset or args.train_dataset)                    # predict_dataset: constructed, unused (:87)
    if args.batch_size % world:
        raise SystemExit("--batch_size (global) must be divisible by the number of ranks")
    sampler = torch.utils.data.distributed.DistributedSampler(train_dataset, world, rank, shuffle=True, seed=3000) if world > 1 else None
    dataloader = DataLoader(train_dataset, batch_size=args.batch_size // world, shuffle=sampler is None, sampler=sampler)
    valloader = DataLoader(val_dataset, 1, shuffle=True)

    factories = {"axialunet": lib.models.axialunet, "MedT": lib.models.axialnet.MedT,
                 "gatedaxialunet": lib.models.axialnet.gated, "logo": lib.models.axialnet.logo}
    model = factories[modelname](img_size=imgsize, imgchan=imgchant)
    if world > 1 and rank == 0:
        print("Let's use", world, "GPUs!")
    model.to(device)
    dp.broadcast_parameters(model)

    criterion.to(device)
    optimizer = FlatAdam(list(model.parameters()), lr=args.learning_rate, weight_decay=1e-5)
    train_step = TrainStep(model, optimizer, criterion, use_graph=not args.eager)
    infer_step = InferStep(model, use_graph=not args.eager)
    if rank == 0:
        print("Total_params: {}".format(sum(p.numel() for p in model.parameters() if p.requires_grad)))
    if rank == 0 and elastic is not None:
        print('elastic p {:.4f} grid {} sigma {:.4f}'.format(elastic["p"], elastic["grid"], elastic["sigma"]))
    if rank == 0 and border is not None:
        print('border w0 {:.4f} sigma {:.4f} connectivity {}'.format(border["w0"], border["sigma"], border["connectivity"]))

    seed = 3000
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)

    for epoch in range(args.epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        epoch_running_loss, batch_idx = 0.0, -1
        if boundary is not None:                  # filled in place: the captured step reads the weight from device memory
            criterion.set_alpha(boundary_alpha(boundary, epoch))
        # host decode + pinned staging + H2D run one step ahead on a copy stream (reference: blocking .to(), :134-135)
        stage = (4 if elastic else 3) if device_aug else 2          # + the record table, + the elastic control lattices
        for batch_idx, (X_batch, y_batch, *rest) in enumerate(DevicePrefetcher(dataloader, device, stage=stage)):
            X_batch = X_batch.to(device)
            y_batch = y_batch.to(device)
            if device_aug is not None:            # uint8 HWC batch + its record table -> float32 NCHW images, int64 masks
                if elastic:
                    X_batch, y_batch = device_aug(X_batch, y_batch, rest[0].to(device), field=rest[1].to(device))
                else:
                    X_batch, y_batch = device_aug(X_batch, y_batch, rest[0].to(device))
            loss = train_step(X_batch, y_batch)
            epoch_running_loss += loss.item()
            train_step.check_targets()            # mislabelled masks raise, as F.cross_entropy does in the reference
        if rank == 0 and boundary is not None:
            print('boundary alpha {:.4f}'.format(boundary_alpha(boundary, epoch)))
        if rank == 0:
            print('epoch [{}/{}], loss:{:.4f}'.format(epoch, args.epochs, epoch_running_loss / (batch_idx + 1)))

        if epoch == 10:
            for param in model.parameters():
                param.requires_grad = True
        if (epoch % args.save_freq) == 0 and rank == 0:
            fulldir = direc + "/{}/".format(epoch)
            os.makedirs(fulldir, exist_ok=True)
            for batch_idx, (X_batch, y_batch, *rest) in enumerate(valloader):
                image_filename = item_filename(rest, batch_idx)
                # the model stays in train mode here, as in the reference (:174-184): batch statistics, and every forward
                # updates the running statistics; replayed as one hipGraph per image shape (InferStep)
                y_out = infer_step(X_batch.to(device))
                yHaT = (y_out.detach().cpu().numpy() >= 0.5).astype(np.uint8) * 255
                imwrite(fulldir + image_filename, yHaT[0, 1, :, :])
            torch.save(model.state_dict(), fulldir + args.modelname + ".pth")
            torch.save(model.state_dict(), direc + "final_model.pth")
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
