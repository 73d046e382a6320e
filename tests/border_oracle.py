"""TEST INFRASTRUCTURE: numpy / float64 restatement of the border term for touching objects (medt_amd.ops.object_edt2_sq,
medt_amd.border_loss, medt_amd.seg_border_loss, metrics.BorderLoss): the squared distances to the nearest and the second-nearest
object by brute force (small maps) and from one SciPy distance transform per object, the weight e, the term R and the combined
loss in torch float64 under autograd.  tests/test_border_cpu.py holds the two maps to each other and to hand-computed cases."""
import numpy as np
import torch

import boundary_oracle as BO

IGNORE = BO.IGNORE
NONE = 2 ** 31 - 1                      # MEDT_EDT_NONE


def blob_labels(N, H, W, density, seed, connectivity=8):
    """int32 (N,H,W) label maps: the connected components (SciPy) of random blobs -- a coarse random grid upsampled 3x, thinned by
    single pixels so that objects touch, nearly touch and tie -- at about `density`.  density 0 gives no object."""
    from scipy import ndimage
    g = np.random.default_rng(seed)
    coarse = g.random((N, (H + 2) // 3, (W + 2) // 3)) < density
    m = np.repeat(np.repeat(coarse, 3, axis=1), 3, axis=2)[:, :H, :W] & (g.random((N, H, W)) < 0.9)
    st = np.ones((3, 3)) if connectivity == 8 else None
    return np.stack([ndimage.label(m[n], structure=st)[0] for n in range(N)]).astype(np.int32)


def label_targets(t, fg=1, ignore=IGNORE, connectivity=8):
    """int32 label maps of the components of {t == fg, t != ignore}, per image (SciPy)."""
    from scipy import ndimage
    t = np.asarray(t)
    f = (t == fg) & (t != ignore)
    st = np.ones((3, 3)) if connectivity == 8 else None
    return np.stack([ndimage.label(m, structure=st)[0] for m in f.reshape(-1, *t.shape[-2:])]).astype(np.int32).reshape(t.shape)


def _two_smallest(per_label):
    """(L,H,W) per-object minimum squared distances -> (d1sq, d2sq) int32, NONE where there are fewer than one / two objects."""
    H, W = per_label.shape[1:]
    pad = np.full((2, H, W), NONE, np.int64)
    s = np.sort(np.concatenate([per_label.astype(np.int64), pad]), axis=0)
    return s[0].astype(np.int32), s[1].astype(np.int32)


def edt2_brute(lab):
    """One (H,W) label map, every (pixel, labelled pixel) pair: per label the minimum squared distance, sorted."""
    lab = np.asarray(lab)
    H, W = lab.shape
    yy, xx = np.mgrid[0:H, 0:W]
    per = []
    for l in np.unique(lab[lab > 0]):
        ys, xs = np.nonzero(lab == l)
        per.append(((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(axis=-1))
    return _two_smallest(np.stack(per) if per else np.zeros((0, H, W), np.int64))


def edt2_scipy(lab):
    """The same from one scipy.ndimage.distance_transform_edt(lab != l) ** 2 per label, rounded to int."""
    from scipy import ndimage
    lab = np.asarray(lab)
    per = [np.rint(ndimage.distance_transform_edt(lab != l) ** 2) for l in np.unique(lab[lab > 0])]
    return _two_smallest(np.stack(per) if per else np.zeros((0,) + lab.shape, np.int64))


def edt2_batch(lab, how=edt2_scipy):
    lab = np.asarray(lab)
    pairs = [how(m) for m in lab.reshape(-1, *lab.shape[-2:])]
    return (np.stack([p[0] for p in pairs]).reshape(lab.shape), np.stack([p[1] for p in pairs]).reshape(lab.shape))


def weight_e(t, d1sq, d2sq, sigma, fg=1, ignore=IGNORE, dtype=torch.float64):
    """e = exp(-(sqrt(d1sq) + sqrt(d2sq))^2 / (2 sigma^2)) outside F = {t == fg} where d2sq is not NONE, 0 elsewhere."""
    t = torch.as_tensor(np.asarray(t))
    d1 = torch.as_tensor(np.asarray(d1sq)).to(dtype)
    d2 = torch.as_tensor(np.asarray(d2sq))
    on = ~((t == fg) & (t != ignore)) & (d2 != NONE)
    d2 = torch.where(on, d2, torch.zeros_like(d2)).to(dtype)
    d1 = torch.where(on, d1, torch.zeros_like(d1))
    return torch.where(on, torch.exp(-(d1.sqrt() + d2.sqrt()) ** 2 / (2.0 * sigma * sigma)), torch.zeros_like(d1))


def border_term(z, t, e, ignore=IGNORE):
    """R = mean over images of ( sum over valid pixels of e * nll / max(1, V_n) ), in z's dtype, differentiable."""
    N, K = z.shape[:2]
    valid = (t != ignore) & (t >= 0) & (t < K)
    nll = -torch.log_softmax(z, dim=1).gather(1, t.clamp(0, K - 1).unsqueeze(1)).squeeze(1)
    v = valid.to(z.dtype)
    num = (e.to(z.dtype) * nll * v).reshape(N, -1).sum(1)
    return (num / v.reshape(N, -1).sum(1).clamp(min=1.0)).mean()


def combined(z, t, e, w0, w=None, ce=0.0, dice=0.0, eps=1.0, ignore=IGNORE):
    """(loss, R): region term (tests/boundary_oracle.py; left out when ce == dice == 0) + w0 * R."""
    R = border_term(z, t, e, ignore)
    loss = w0 * R
    if ce or dice:
        loss = loss + BO.region_term(z, t, w, ce, dice, eps, ignore)
    return loss, R
