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


class _RegionCriterion(torch.nn.Module):
    """What the criteria around medt_amd.seg_loss and its relatives share: the class weights as the buffer `weight` (None without)
    and the region term's ce / dice / eps / ignore_index."""

    def __init__(self, weight, ce, dice, eps, ignore_index):
        super().__init__()
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).reshape(-1)
        self.register_buffer("weight", weight)
        self.ce, self.dice, self.eps, self.ignore_index = float(ce), float(dice), float(eps), ignore_index


class DiceCELoss(_RegionCriterion):
    """ce * (class-weighted) cross entropy + dice * soft Dice, one kernel pair (medt_amd.seg_loss has the formulas).

    The Dice term is per image and per class over the non-ignored pixels, 2 <= K <= 8 classes; `eps` keeps empty images and
    absent classes finite.  Under data parallel the Dice gradient of equal shards averages to the global batch's; the
    weighted cross entropy is a mean of per-rank weighted means, as with DistributedDataParallel."""

    def __init__(self, weight=None, ce=1.0, dice=1.0, eps=1.0, ignore_index=-100):
        super().__init__(weight, ce, dice, eps, ignore_index)

    def forward(self, y_input, y_target):
        return medt_amd.seg_loss(y_input, y_target, weight=self.weight, ce=self.ce, dice=self.dice, eps=self.eps,
                                 ignore_index=self.ignore_index)


class BoundaryLoss(_RegionCriterion):
    """ce * (class-weighted) cross entropy + dice * soft Dice + alpha * boundary loss (Kervadec et al., MIDL 2019) of the
    class `fg`: medt_amd.seg_boundary_loss has the formulas.  The signed distance map comes from the label map the step holds
    on the device (after the device-side augmentation, where there is one), not from the dataset.

    `alpha` is a registered float32 buffer of one element that the kernels read on the device: set_alpha() fills it in place,
    so a captured step follows the schedule without another capture."""

    def __init__(self, alpha=0.01, weight=None, ce=1.0, dice=0.0, eps=1.0, fg=1, ignore_index=-100):
        super().__init__(weight, ce, dice, eps, ignore_index)
        self.register_buffer("alpha", torch.full((1,), float(alpha), dtype=torch.float32))
        self.fg = int(fg)

    def set_alpha(self, v):
        self.alpha.fill_(float(v))

    def forward(self, y_input, y_target):
        return medt_amd.seg_boundary_loss(y_input, y_target, self.alpha, weight=self.weight, ce=self.ce, dice=self.dice,
                                          eps=self.eps, fg=self.fg, ignore_index=self.ignore_index)


class BorderLoss(_RegionCriterion):
    """ce * (class-weighted) cross entropy + dice * soft Dice + w0 * the border term for touching objects (the weight map of
    Ronneberger et al., U-Net, 2015, w0 exp(-(d1 + d2)^2 / (2 sigma^2)), applied to the cross entropy of the pixels between two
    objects of the class `fg`): medt_amd.seg_border_loss has the formulas.  The objects are the connected components of the label
    map the step holds on the device (after the device-side augmentation, where there is one), not of the dataset's masks.

    `w0` is a registered float32 buffer of one element that the kernels read on the device: set_w0() fills it in place, so a
    captured step follows a change without another capture."""

    def __init__(self, w0=10.0, sigma=5.0, weight=None, ce=1.0, dice=0.0, eps=1.0, fg=1, connectivity=8, ignore_index=-100):
        super().__init__(weight, ce, dice, eps, ignore_index)
        self.register_buffer("w0", torch.full((1,), float(w0), dtype=torch.float32))
        self.sigma, self.fg, self.connectivity = float(sigma), int(fg), int(connectivity)

    def set_w0(self, v):
        self.w0.fill_(float(v))

    def forward(self, y_input, y_target):
        return medt_amd.seg_border_loss(y_input, y_target, self.w0, sigma=self.sigma, weight=self.weight, ce=self.ce,
                                        dice=self.dice, eps=self.eps, fg=self.fg, connectivity=self.connectivity,
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


def _object_scores_image(ap, ag, rows):
    """The scores of one image from integer tables: ap / ag the pixel counts of the predicted / target objects (index 0 = object
    1), rows the (j, i, I) triples with I = |G_i ∩ P_j| > 0, sorted by (j, i), labels from 1."""
    kp, kg = len(ap), len(ag)
    nan = float("nan")
    if kp == 0 and kg == 0:
        return (nan,) * 6
    if kp == 0 or kg == 0:
        return (0.0,) * 6
    best_i = {}                        # j -> (I, i): the target object P_j overlaps most; ties to the lowest i
    best_j = {}                        # i -> (I, j): the predicted object G_i overlaps most; ties to the lowest j
    best_iou = {}                      # i -> (IoU, j, I)
    tp_pq, sum_iou = 0, 0.0
    for j, i, I in rows:               # (sorted by (j, i): a strict > keeps the lowest index on both sides)
        if j not in best_i or I > best_i[j][0]:
            best_i[j] = (I, i)
        if i not in best_j or I > best_j[i][0]:
            best_j[i] = (I, j)
        union = ag[i - 1] + ap[j - 1] - I
        iou = I / union
        if i not in best_iou or iou > best_iou[i][0]:
            best_iou[i] = (iou, j, I)
        if 2 * I > union:              # IoU > 0.5 in integers; an object is in at most one such pair
            tp_pq += 1
            sum_iou += iou
    # GlaS object F1
    tp, hit = 0, set()
    for j, (I, i) in best_i.items():
        if 2 * I >= ag[i - 1]:
            tp += 1
            hit.add(i)
    f1 = 2.0 * tp / (2 * tp + (kp - tp) + (kg - len(hit)))
    # GlaS object Dice
    tot_g, tot_p = sum(ag), sum(ap)
    sg = sum((ag[i - 1] / tot_g) * (2.0 * I / (ag[i - 1] + ap[j - 1])) for i, (I, j) in sorted(best_j.items()))
    sp = sum((ap[j - 1] / tot_p) * (2.0 * I / (ag[i - 1] + ap[j - 1])) for j, (I, i) in sorted(best_i.items()))
    dice = 0.5 * (sg + sp)
    # AJI
    C = U = 0
    used = set()
    for i in range(1, kg + 1):
        if i in best_iou:
            _, j, I = best_iou[i]
            C += I
            U += ag[i - 1] + ap[j - 1] - I
            used.add(j)
        else:
            U += ag[i - 1]
    U += sum(ap[j - 1] for j in range(1, kp + 1) if j not in used)
    aji = C / U
    # PQ
    dq = tp_pq / (tp_pq + (kp - tp_pq) / 2 + (kg - tp_pq) / 2)
    sq = sum_iou / tp_pq if tp_pq else 0.0
    return f1, dice, aji, dq * sq, dq, sq


def _object_tables(pred, target, connectivity, labelled):
    """What object_scores and object_hausdorff both start from -> (label maps (lp, lg), object counts on the device (cp, cg),
    the counts as lists, the area tables on the host, the overlap rows (n, j, i, |G_i ∩ P_j|) as a list).  Masks are labelled here
    at `connectivity`; with labelled=True the label maps are taken as given and the counts are their maxima.  labelled may also
    be a pair (pred_is_labelled, target_is_labelled): one side a label map, the other a mask."""
    from medt_amd import ops
    if isinstance(labelled, (bool, int)):
        labelled = (bool(labelled),) * 2
    if not isinstance(labelled, (tuple, list)) or len(labelled) != 2:
        raise ValueError(f"labelled: {labelled!r}: a bool, or a pair (pred_is_labelled, target_is_labelled)")

    def side(x, given):
        if not given:
            return ops.label(x, connectivity)
        N = x.reshape(-1, *x.shape[-2:]).shape[0]
        return x, x.reshape(N, -1).amax(dim=1).to(torch.int32)

    (lp, cp), (lg, cg) = side(pred, labelled[0]), side(target, labelled[1])
    area_p, _ = ops.label_tables(lp, cp)
    area_g, _ = ops.label_tables(lg, cg)
    rows = ops.label_overlaps(lp, cp, lg, cg).cpu().tolist()
    return (lp, lg), (cp, cg), (cp.cpu().tolist(), cg.cpu().tolist()), (area_p.cpu(), area_g.cpu()), rows


def object_scores(pred, target, connectivity=8, labelled=False):
    """Per-image object-level scores of a prediction against a target, on the device.  pred / target: uint8 masks (N,H,W) or
    (H,W), foreground = mask != 0, labelled here at `connectivity` (4 or 8; 8 is MATLAB's bwlabel); or with labelled=True int32
    label maps with consecutive labels 1..K per image, taken as given (instance annotations, medt_amd.ops.split_objects);
    labelled=(pred_is_labelled, target_is_labelled) says so per side.

    With P_j the predicted objects, G_i the target objects, I[i,j] = |G_i ∩ P_j|, ties to the lowest index:
      f1    GlaS object F1: P_j is a true positive when the G_i* it overlaps most has 2 I[i*,j] >= |G_i*|; FP = Kp - TP,
            FN = Kg - the distinct i* among the true positives; 2TP / (2TP + FP + FN)
      dice  GlaS object Dice: 0.5 (sum_i |G_i|/sum|G| D(G_i, P_j*(i)) + sum_j |P_j|/sum|P| D(G_i*(j), P_j)), D = 2|A∩B| / (|A|+|B|),
            0 without a partner
      aji   Aggregated Jaccard Index: every G_i in order takes the P_j of largest IoU among those it touches, C += I,
            U += |G_i ∪ P_j| (else U += |G_i|); then U += |P_j| of every P_j never taken; C / U
      pq    panoptic quality: matches are the pairs with IoU > 0.5; dq = TP / (TP + FP/2 + FN/2), sq = mean IoU of the matches
            (0 without one), pq = dq sq
    -> {"f1", "dice", "aji", "pq", "dq", "sq": float64 (N,), "n_pred", "n_gt": int64 (N,), "valid": bool (N,)} on the CPU.
    valid is False and the scores NaN only where BOTH images have no object; with exactly one side empty every score is 0.

    These follow the published descriptions of the GlaS and MoNuSeg challenges and of PQ; the challenges' own MATLAB / Python
    evaluation code was not available, so no bit-compatibility with it is claimed.

    Labelling, the area tables and the overlap table run on the device (medt_amd.ops.label / label_tables / label_overlaps);
    only those integer tables come to the host, where the scores are computed in float64 per image."""
    _, _, (cp, cg), (area_p, area_g), rows = _object_tables(pred, target, connectivity, labelled)
    area_p, area_g = area_p.tolist(), area_g.tolist()
    N = len(cp)
    per_image = [[] for _ in range(N)]
    for n, j, i, I in rows:
        per_image[n].append((j, i, I))
    keys = ("f1", "dice", "aji", "pq", "dq", "sq")
    out = {k: torch.empty(N, dtype=torch.float64) for k in keys}
    out["n_pred"], out["n_gt"] = torch.tensor(cp, dtype=torch.int64), torch.tensor(cg, dtype=torch.int64)
    out["valid"] = (out["n_pred"] > 0) | (out["n_gt"] > 0)
    for n in range(N):
        got = _object_scores_image(area_p[n][1:cp[n] + 1], area_g[n][1:cg[n] + 1], per_image[n])
        for k, v in zip(keys, got):
            out[k][n] = v
    return out


def hausdorff_box_bound_sq(box_a, boxes_b):
    """Squared lower bound of H(A, B) from the bounding boxes (y0, x0, y1, x1), A against every row of boxes_b (numpy int64):
    H(A,B) >= max(|ay0-by0|, |ay1-by1|, |ax0-bx0|, |ax1-bx1|).  Each object has a pixel in every extreme row and column of its
    box: if, say, ay0 < by0, the pixel of A in row ay0 is at least by0 - ay0 rows from every pixel of B, all of which lie in rows
    >= by0; if ay0 > by0 the pixel of B in row by0 is as far from all of A.  The same holds for the other three sides, and H is
    the larger of the two directed distances, so it is at least the largest of the four differences."""
    import numpy as np
    d = np.abs(boxes_b - box_a[None, :]).max(axis=1)
    return d * d


def _hausdorff_candidates(boxes_own, boxes_other, own, others, partner):
    """For the objects `own` (labels) without a partner: (label, sorted candidate labels of the other side, squared bounds)."""
    todo = []
    for l in own:
        if l not in partner:
            todo.append((l, others, hausdorff_box_bound_sq(boxes_own[l], boxes_other[others])))
    return todo


def object_hausdorff(pred, target, connectivity=8, labelled=False, prune=True):
    """Per-image object-level Hausdorff distance of GlaS (Sirinukunwattana et al.), on the device.  pred / target as in
    object_scores: uint8 masks labelled here at `connectivity`, or with labelled=True int32 label maps taken as given, or per
    side with labelled=(pred_is_labelled, target_is_labelled).

    With G_i the target objects and S_j the predicted ones,
      H(A,B) = max(max_{x in A} min_{y in B} |x-y|, max_{y in B} min_{x in A} |x-y|), Euclidean, in pixels, over ALL pixels of
               both objects (not only their borders),
      Hobj   = 1/2 [ sum_i |G_i|/sum|G| H(G_i, S*(G_i)) + sum_j |S_j|/sum|S| H(G*(S_j), S_j) ],
    S*(G_i) the predicted object that overlaps G_i most (ties to the lowest index, as in object_scores); a G_i that overlaps
    nothing takes the predicted object of smallest H(G_i, S_j), ties to the lowest j.  G*(S_j) likewise.
    -> {"hd": float64 (N,), "valid": bool (N,), "n_pred", "n_gt": int64 (N,), "pairs": int64 (N,) the jobs (pair x direction)
    evaluated per image, "partners_gt" / "partners_pred": per image the int64 partner label of every object 1..K} on the CPU.
    valid is False and hd NaN where EITHER side has no object: with both sides empty there is nothing to score, and with
    exactly one side empty the distance to an empty set is undefined and has no finite worst value, so the image is counted
    out -- what surface_scores does (object_scores, whose scores have a worst value, gives 0 there).  An object of a given
    label map without a pixel has weight 0 and is nobody's partner.

    Objects without overlap need min_j H.  prune=False evaluates every candidate.  prune=True (default) uses the bounding-box
    bound of hausdorff_box_bound_sq in two batched device calls: first the partners by overlap and, for every object without
    one, the candidate of smallest bound; then every remaining candidate whose squared bound is <= the best squared distance
    found (<=, not <: an equal distance at a lower index must still win the tie).  Both settings give identical scores and
    partners.  The distances are exact integers squared (medt_amd.ops.pair_hausdorff_sq); the roots are float64 roots of
    integers taken on the host and the weighted sums run per image in float64 in index order.

    This follows the published description of the GlaS challenge; no bit-compatibility with its MATLAB code is claimed."""
    import math
    import numpy as np
    from medt_amd import ops
    (lp, lg), (cp_dev, cg_dev), (cp, cg), (area_p, area_g), rows = _object_tables(pred, target, connectivity, labelled)
    box_p, box_g = ops.label_boxes(lp, cp_dev).cpu(), ops.label_boxes(lg, cg_dev).cpu()
    area_p, area_g = area_p.numpy().astype(np.int64), area_g.numpy().astype(np.int64)
    bp, bg = box_p.numpy().astype(np.int64), box_g.numpy().astype(np.int64)
    N = len(cp)
    out = {"hd": torch.full((N,), float("nan"), dtype=torch.float64), "pairs": torch.zeros(N, dtype=torch.int64),
           "n_pred": torch.tensor(cp, dtype=torch.int64), "n_gt": torch.tensor(cg, dtype=torch.int64)}
    objs_p = [[j for j in range(1, cp[n] + 1) if area_p[n][j] > 0] for n in range(N)]
    objs_g = [[i for i in range(1, cg[n] + 1) if area_g[n][i] > 0] for n in range(N)]
    valid = [bool(objs_p[n]) and bool(objs_g[n]) for n in range(N)]
    out["valid"] = torch.tensor(valid, dtype=torch.bool)
    part_g = [dict() for _ in range(N)]          # i -> (I, j): the predicted object G_i overlaps most; ties to the lowest j
    part_p = [dict() for _ in range(N)]          # j -> (I, i)
    for n, j, i, I in rows:                      # (sorted by (n, j, i): a strict > keeps the lowest index on both sides)
        if i not in part_g[n] or I > part_g[n][i][0]:
            part_g[n][i] = (I, j)
        if j not in part_p[n] or I > part_p[n][j][0]:
            part_p[n][j] = (I, i)
    part_g = [{i: j for i, (_, j) in d.items()} for d in part_g]
    part_p = [{j: i for j, (_, i) in d.items()} for d in part_p]

    dist = {}                                    # (n, j, i) -> squared H(S_j, G_i)

    def evaluate(keys):
        keys = sorted(k for k in set(keys) if k not in dist)
        if not keys:
            return
        d = ops.pair_hausdorff_sq(lp, cp_dev, lg, cg_dev, torch.tensor(keys, dtype=torch.int32).reshape(-1, 3),
                                  boxes=(box_p, box_g)).cpu().tolist()
        for k, (ab, ba) in zip(keys, d):
            dist[k] = max(ab, ba)
            out["pairs"][k[0]] += 2

    # objects without a partner by overlap: (n, side, label, candidates, squared bounds); side 0 = target object, 1 = predicted
    todo = []
    first = []
    for n in range(N):
        if not valid[n]:
            continue
        first += [(n, j, i) for i, j in part_g[n].items()] + [(n, j, i) for j, i in part_p[n].items()]
        cand_p, cand_g = np.asarray(objs_p[n]), np.asarray(objs_g[n])
        todo += [(n, 0, l, c, b) for l, c, b in _hausdorff_candidates(bg[n], bp[n], objs_g[n], cand_p, part_g[n])]
        todo += [(n, 1, l, c, b) for l, c, b in _hausdorff_candidates(bp[n], bg[n], objs_p[n], cand_g, part_p[n])]

    def key(n, side, l, c):
        return (n, int(c), l) if side == 0 else (n, l, int(c))

    if prune:
        start = [int(np.argmin(b)) for _, _, _, _, b in todo]            # (argmin: the first of equal bounds = the lowest index)
        evaluate(first + [key(n, side, l, c[k]) for (n, side, l, c, _), k in zip(todo, start)])
        seen = [c[b <= dist[key(n, side, l, c[k])]] for (n, side, l, c, b), k in zip(todo, start)]      # (holds c[k]: bound <= H)
    else:
        evaluate(first)
        seen = [c for _, _, _, c, _ in todo]
    evaluate([key(n, side, l, cc) for (n, side, l, _, _), ev in zip(todo, seen) for cc in ev])
    for (n, side, l, _, _), ev in zip(todo, seen):      # the evaluated candidate of smallest distance, ties to the lowest index
        d = [dist[key(n, side, l, cc)] for cc in ev]
        (part_g if side == 0 else part_p)[n][l] = int(ev[int(np.argmin(d))])
    out["partners_gt"] = [torch.tensor([part_g[n].get(i, 0) if valid[n] else 0 for i in range(1, cg[n] + 1)], dtype=torch.int64)
                          for n in range(N)]
    out["partners_pred"] = [torch.tensor([part_p[n].get(j, 0) if valid[n] else 0 for j in range(1, cp[n] + 1)], dtype=torch.int64)
                            for n in range(N)]
    for n in range(N):
        if not valid[n]:
            continue
        tot_g, tot_p = int(area_g[n][1:cg[n] + 1].sum()), int(area_p[n][1:cp[n] + 1].sum())
        sg = sp = 0.0
        for i in objs_g[n]:
            sg += (int(area_g[n][i]) / tot_g) * math.sqrt(float(dist[(n, part_g[n][i], i)]))
        for j in objs_p[n]:
            sp += (int(area_p[n][j]) / tot_p) * math.sqrt(float(dist[(n, j, part_p[n][j])]))
        out["hd"][n] = 0.5 * (sg + sp)
    return out
