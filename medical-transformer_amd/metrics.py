"""Drop-in for the reference's metrics.py.  LogNLLLoss.forward is plain mean cross entropy
(reference metrics.py:17-20; the log() line is commented out there) and runs as the HIP kernel pair
medt_ce_fwd / medt_ce_bwd; with class weights (F.cross_entropy(weight=...) in the reference) as medt_seg_loss_fwd / _bwd, which
also carry the soft Dice term of DiceCELoss (not in the reference).  The classwise helpers are imported by train.py:23 but
never called."""
import torch
from torch.nn.modules.loss import _WeightedLoss

import medt_amd

EPSILON = 1e-32


class LogNLLLoss(_WeightedLoss):
    __constants__ = ["weight", "reduction", "ignore_index"]

    def __init__(self, weight=None, size_average=None, reduce=None, reduction=None, ignore_index=-100):
        super().__init__(weight, size_average, reduce, reduction)
        self.ignore_index = ignore_index

    def forward(self, y_input, y_target):
        if self.weight is not None:
            return medt_amd.seg_loss(y_input, y_target, weight=self.weight, ignore_index=self.ignore_index)
        return medt_amd.cross_entropy(y_input, y_target, self.ignore_index)


class DiceCELoss(torch.nn.Module):
    """ce * (class-weighted) cross entropy + dice * soft Dice, one kernel pair (medt_amd.seg_loss has the formulas).

    The Dice term is per image and per class over the non-ignored pixels, 2 <= K <= 8 classes; `eps` keeps empty images and
    absent classes finite.  Under data parallel the Dice gradient of equal shards averages to the global batch's; the
    weighted cross entropy is a mean of per-rank weighted means, as with DistributedDataParallel."""

    def __init__(self, weight=None, ce=1.0, dice=1.0, eps=1.0, ignore_index=-100):
        super().__init__()
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).reshape(-1)
        self.register_buffer("weight", weight)
        self.ce, self.dice, self.eps, self.ignore_index = float(ce), float(dice), float(eps), ignore_index

    def forward(self, y_input, y_target):
        return medt_amd.seg_loss(y_input, y_target, weight=self.weight, ce=self.ce, dice=self.dice, eps=self.eps,
                                 ignore_index=self.ignore_index)


def classwise_iou(output, gt):
    dims = (0, *range(2, len(output.shape)))
    onehot = torch.zeros_like(output).scatter_(1, gt[:, None, :], 1)
    inter = output * onehot
    union = output + onehot - inter
    return (inter.sum(dim=dims).float() + EPSILON) / (union.sum(dim=dims) + EPSILON)


def classwise_f1(output, gt):
    eps = 1e-20
    n = output.shape[1]
    pred = torch.argmax(output, dim=1)
    tp = torch.tensor([((pred == i) * (gt == i)).sum() for i in range(n)]).float()
    sel = torch.tensor([(pred == i).sum() for i in range(n)]).float()
    rel = torch.tensor([(gt == i).sum() for i in range(n)]).float()
    precision, recall = (tp + eps) / (sel + eps), (tp + eps) / (rel + eps)
    return 2 * (precision * recall) / (precision + recall)


def make_weighted_metric(classwise_metric):
    def weighted_metric(output, gt, weights=None):
        if weights is not None and len(weights) != output.shape[1]:
            raise ValueError("The number of weights must match with the number of classes")
        return classwise_metric(output, gt).cpu()          # the reference computes weights and ignores them too
    return weighted_metric


jaccard_index = make_weighted_metric(classwise_iou)
f1_score = make_weighted_metric(classwise_f1)


# --------------------------------------------------------------------------- #
# Dataset scores without MATLAB
# --------------------------------------------------------------------------- #
def segmentation_scores(counts):
    """Per-image F1 / IoU / pixel accuracy from (N,4) {tp, fp, fn, tn} counts, with the conventions of the reference's
    scoring scripts (performancemetrics_monuseg.m:68-78): F = 2tp/(2tp+fp+fn), IoU = tp/(tp+fp+fn),
    PA = tp/(tp+fn) (their `tp/ttp`), and an image without a single true positive scores 1 on all three."""
    c = counts.detach().to("cpu").double()
    tp, fp, fn = c[:, 0], c[:, 1], c[:, 2]
    one = tp == 0
    f1 = 2 * tp / (2 * tp + fp + fn).clamp_min(1)
    iou = tp / (tp + fp + fn).clamp_min(1)
    pa = tp / (tp + fn).clamp_min(1)
    f1[one], iou[one], pa[one] = 1.0, 1.0, 1.0
    return f1, iou, pa


def surface_scores(pred_mask, target_mask):
    """Per-image surface-distance scores of two uint8 masks (N,H,W) or (H,W) on the device, foreground = mask != 0 (the
    {0,255} masks test.py writes; for a label map pass `(target > 0).to(torch.uint8)`):
      hd    Hausdorff distance: the largest distance from a border pixel of one mask to the border of the other
      hd95  the 95th percentile (linear interpolation, numpy.percentile) of those distances, both directions pooled
      assd  average symmetric surface distance, (mean A->B + mean B->A) / 2
    in pixels, with MedPy's surface (a foreground pixel with a 4-neighbour outside the foreground or the image).
    -> {"hd", "hd95", "assd": float64 (N,), "valid": bool (N,)} on the CPU.  An image whose prediction or target has no
    foreground has valid False and NaN scores (MedPy raises there; an evaluation loop must not).

    The distances are exact integers squared (medt_amd.ops.surface_d2, two calls); they are sorted on the device, the square
    roots are taken in float64 there, and hd is the float64 root of the largest integer."""
    import math
    from medt_amd import ops
    d_ab = ops.surface_d2(pred_mask, target_mask)
    d_ba = ops.surface_d2(target_mask, pred_mask)
    H, W = d_ab.shape[-2:]
    d_ab, d_ba = d_ab.reshape(-1, H * W), d_ba.reshape(-1, H * W)
    N = d_ab.shape[0]
    has = ((pred_mask.reshape(N, -1) != 0).any(dim=1) & (target_mask.reshape(N, -1) != 0).any(dim=1)).cpu()
    out = {k: torch.full((N,), float("nan"), dtype=torch.float64) for k in ("hd", "hd95", "assd")}
    out["valid"] = has.clone()
    for n in range(N):
        if not bool(has[n]):
            continue
        ab, ba = d_ab[n][d_ab[n] >= 0], d_ba[n][d_ba[n] >= 0]
        both, _ = torch.sort(torch.cat([ab, ba]))
        root = both.double().sqrt()
        k = both.numel()
        pos = 0.95 * (k - 1)
        lo = int(math.floor(pos))
        hi = min(lo + 1, k - 1)
        out["hd"][n] = math.sqrt(float(int(both[-1])))
        out["hd95"][n] = float(root[lo]) + (float(root[hi]) - float(root[lo])) * (pos - lo)
        out["assd"][n] = 0.5 * (float(ab.double().sqrt().mean()) + float(ba.double().sqrt().mean()))
    return out
