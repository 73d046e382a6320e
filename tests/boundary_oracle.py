"""TEST INFRASTRUCTURE: numpy / float64 restatement of the boundary loss (medt_amd.ops.signed_edt_sq, medt_amd.boundary_loss,
medt_amd.seg_boundary_loss, metrics.BoundaryLoss): the signed squared distance map by brute force (small maps) and from SciPy,
Kervadec's level-set value phi, the term B and the combined loss in torch float64 under autograd.  tests/test_boundary_cpu.py
holds the two distance maps to each other and to hand-computed cases."""
import numpy as np
import torch
import torch.nn.functional as F

IGNORE = -100


def blob_targets(N, H, W, K, density, seed, ignore=IGNORE):
    """int64 (N,H,W): random blobs (a coarse random grid, upsampled 3x) of class 1 ... K-1 at about `density`, class 0 elsewhere;
    ~10 % of the pixels ignored, a few (when the map has room) out of range."""
    g = np.random.default_rng(seed)
    coarse = g.random((N, (H + 2) // 3, (W + 2) // 3)) < density
    fg = np.repeat(np.repeat(coarse, 3, axis=1), 3, axis=2)[:, :H, :W]
    t = np.where(fg, g.integers(1, K, (N, H, W)), 0).astype(np.int64)
    t[g.random((N, H, W)) < 0.1] = ignore
    if H * W >= 35:
        t.reshape(N, -1)[:, 3] = K + 5
        t.reshape(N, -1)[:, 17] = -7
    return t


def _nearest_sq(f):
    """(H,W) int64: squared distance of every pixel to the nearest pixel of the boolean map f (which has one); brute force."""
    H, W = f.shape
    ys, xs = np.nonzero(f)
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(axis=-1)


def sd2_brute(t, fg=1, ignore=IGNORE):
    """int32 (H,W) from one (H,W) label map, every (pixel, pixel) pair; for small maps."""
    f = (np.asarray(t) == fg) & (np.asarray(t) != ignore)
    if not f.any():                                   # no F: 0 everywhere
        return np.zeros(f.shape, np.int32)
    if f.all():                                       # all F: 0 everywhere (SciPy's value without a zero is arbitrary)
        return np.zeros(f.shape, np.int32)
    return np.where(f, -_nearest_sq(~f), _nearest_sq(f)).astype(np.int32)


def sd2_scipy(t, fg=1, ignore=IGNORE):
    """The same from scipy.ndimage.distance_transform_edt(...) ** 2, rounded to int."""
    from scipy import ndimage
    f = (np.asarray(t) == fg) & (np.asarray(t) != ignore)
    if not f.any():
        return np.zeros(f.shape, np.int32)
    if f.all():
        return np.zeros(f.shape, np.int32)
    out = np.rint(ndimage.distance_transform_edt(~f) ** 2)             # at the pixels outside F: to the nearest pixel of F
    inn = np.rint(ndimage.distance_transform_edt(f) ** 2)              # at the pixels of F: to the nearest pixel outside
    return np.where(f, -inn, out).astype(np.int32)


def sd2_batch(t, fg=1, ignore=IGNORE, how=sd2_scipy):
    t = np.asarray(t)
    return np.stack([how(m, fg, ignore) for m in t.reshape(-1, *t.shape[-2:])]).reshape(t.shape)


def phi(sd2, dtype=torch.float64):
    """Kervadec's one_hot2dist, edt(neg) * neg - (edt(pos) - 1) * pos: sqrt outside F, -(sqrt - 1) inside, 0 where sd2 == 0."""
    s = torch.as_tensor(np.asarray(sd2)).to(dtype)
    return torch.where(s > 0, s.abs().sqrt(), torch.where(s < 0, -(s.abs().sqrt() - 1.0), torch.zeros_like(s)))


def boundary_term(z, t, sd2, fg=1, ignore=IGNORE):
    """B = mean over images of ( sum over valid pixels of phi * softmax(z)[fg] / max(1, V_n) ), in z's dtype, differentiable."""
    N, K = z.shape[:2]
    s = torch.softmax(z, dim=1)[:, fg]
    valid = ((t != ignore) & (t >= 0) & (t < K)).to(z.dtype)
    num = (phi(sd2, z.dtype) * s * valid).reshape(N, -1).sum(1)
    return (num / valid.reshape(N, -1).sum(1).clamp(min=1.0)).mean()


def region_term(z, t, w, ce, dice, eps=1.0, ignore=IGNORE):
    """ce * weighted cross entropy + dice * per-image soft Dice (tests/test_seg_loss_gpu.py::ref_loss) with targets out of
    range excluded like ignored ones."""
    N, K = z.shape[:2]
    t = torch.where((t < 0) | (t >= K), torch.full_like(t, ignore), t)
    total = z.new_zeros(())
    if ce:
        total = total + ce * F.cross_entropy(z, t, weight=w, ignore_index=ignore)
    if dice:
        p = torch.softmax(z, dim=1)
        valid = (t != ignore).unsqueeze(1).to(z.dtype)
        onehot = F.one_hot(t.clamp(0, K - 1), K).movedim(-1, 1).to(z.dtype) * valid
        dims = tuple(range(2, z.dim()))
        inter, psum, tsum = (p * onehot).sum(dims), (p * valid).sum(dims), onehot.sum(dims)
        total = total + dice * (1.0 - ((2 * inter + eps) / (psum + tsum + eps)).mean())
    return total


def combined(z, t, sd2, alpha, w=None, ce=0.0, dice=0.0, eps=1.0, fg=1, ignore=IGNORE):
    """(loss, B): region term (left out when ce == dice == 0) + alpha * B."""
    B = boundary_term(z, t, sd2, fg, ignore)
    loss = alpha * B
    if ce or dice:
        loss = loss + region_term(z, t, w, ce, dice, eps, ignore)
    return loss, B
