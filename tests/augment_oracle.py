"""TEST INFRASTRUCTURE: the joint augmentation (crop, flip, colour jitter, affine map) restated from its specification --
include/medt_abi.h's medt_augment_* comment / DESIGN.md 'Joint augmentation on the device' -- in array arithmetic, NOT from the
kernels.  `augment(...)` evaluates it in float64 numpy (the oracle) or, with backend=T32, in float32 torch on the CPU: the
deviation of the second from the first is the float32 noise of the formulas themselves, the yardstick of the GPU tests.

The geometry (which source pixel an output pixel takes) is always evaluated in float64 from the float32 record, and `near`
marks the output pixels whose source coordinate lies within NEAR_TOL of an integer, where a float32 evaluation (the kernel)
or PIL's fixed-point stepping may legitimately land on the neighbouring pixel.
"""
import numpy as np
import torch

P = 20
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 1, 2, 3, 4
NEAR_TOL = 1e-3


class NP64:
    dtype = np.float64
    asarray = staticmethod(lambda a: np.asarray(a, np.float64))
    where, floor, maximum, minimum, fmod, stack = np.where, np.floor, np.maximum, np.minimum, np.fmod, np.stack
    clamp01 = staticmethod(lambda a: np.clip(a, 0.0, 1.0))
    ones_like = np.ones_like
    mean = staticmethod(lambda a: a.mean())
    scalar = staticmethod(np.float64)
    numpy = staticmethod(lambda a: np.asarray(a))


class T32:
    dtype = torch.float32
    asarray = staticmethod(lambda a: torch.as_tensor(np.asarray(a)).to(torch.float32))
    where, floor, maximum, minimum, fmod = torch.where, torch.floor, torch.maximum, torch.minimum, torch.fmod
    stack = staticmethod(lambda seq, axis: torch.stack(list(seq), dim=axis))
    clamp01 = staticmethod(lambda a: a.clamp(0.0, 1.0))
    ones_like = torch.ones_like
    mean = staticmethod(lambda a: a.mean())
    scalar = staticmethod(lambda v: torch.tensor(float(np.float32(v)), dtype=torch.float32))
    numpy = staticmethod(lambda a: a.numpy())


def affine_source(m, th, tw):
    """(sx, sy, inside, near) of every output pixel of a th x tw image under the inverse map m = (m00 m01 m02 m10 m11 m12),
    in float64: fx = m00 (j+.5) + m01 (i+.5) + m02, fy likewise, sx = floor(fx), sy = floor(fy); inside tested on the floats."""
    m = [float(v) for v in m]
    j, i = np.meshgrid(np.arange(tw, dtype=np.float64) + 0.5, np.arange(th, dtype=np.float64) + 0.5)
    with np.errstate(all="ignore"):
        fx = m[0] * j + m[1] * i + m[2]
        fy = m[3] * j + m[4] * i + m[5]
        inside = (fx >= 0) & (fx < tw) & (fy >= 0) & (fy < th)          # False for NaN
        near = (np.abs(fx - np.round(fx)) < NEAR_TOL) | (np.abs(fy - np.round(fy)) < NEAR_TOL)
        near &= np.isfinite(fx) & np.isfinite(fy) & (fx > -1) & (fx < tw + 1) & (fy > -1) & (fy < th + 1)
        sx = np.where(inside, np.floor(fx), 0).astype(np.int64)
        sy = np.where(inside, np.floor(fy), 0).astype(np.int64)
    return sx, sy, inside, near


def gray(v, xp):
    """v: (..., C) -> (...): 0.299 c0 + 0.587 c1 + 0.114 c2 over the channels as stored; one channel: itself."""
    if v.shape[-1] == 1:
        return v[..., 0]
    return 0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2]


def hue(v, hf, xp):
    """RGB -> HSV, H = (H + hf) mod 1, HSV -> RGB, the hexcone model (torchvision.transforms.functional_tensor)."""
    if v.shape[-1] == 1:
        return v
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    maxc = xp.maximum(r, xp.maximum(g, b))
    minc = xp.minimum(r, xp.minimum(g, b))
    eqc = maxc == minc
    cr = maxc - minc
    ones = xp.ones_like(maxc)
    s = cr / xp.where(eqc, ones, maxc)
    crd = xp.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    h = xp.where(maxc == r, bc - gc, xp.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = xp.fmod(h / 6.0 + 1.0, ones)
    h = h + hf
    h = h - xp.floor(h)
    h6 = h * 6.0
    fi = xp.floor(h6)
    f = h6 - fi
    i = fi - 6.0 * xp.floor(fi / 6.0)
    p = xp.clamp01(maxc * (1.0 - s))
    q = xp.clamp01(maxc * (1.0 - s * f))
    t = xp.clamp01(maxc * (1.0 - s * (1.0 - f)))
    sel = lambda a: xp.where(i == 0, a[0], xp.where(i == 1, a[1], xp.where(i == 2, a[2], xp.where(i == 3, a[3], xp.where(i == 4, a[4], a[5])))))
    return xp.stack((sel((maxc, q, p, p, t, maxc)), sel((t, maxc, maxc, q, p, p)), sel((p, p, t, maxc, maxc, q))), -1)


def jitter(v, rec, xp):
    """The record's jitter slots, in order, on a (th, tw, C) image in [0,1]; returns (image, mean_g used by contrast or 0)."""
    mean_used = 0.0
    for k in range(4):
        op, fac = int(rec[10 + k]), xp.scalar(rec[14 + k])
        if op == OP_BRIGHTNESS:
            v = xp.clamp01(fac * v)
        elif op == OP_CONTRAST:
            mean_g = xp.mean(gray(v, xp))
            mean_used = float(mean_g)
            v = xp.clamp01(fac * v + (1.0 - fac) * mean_g)
        elif op == OP_SATURATION:
            if v.shape[-1] == 3:
                v = xp.clamp01(fac * v + (1.0 - fac) * gray(v, xp)[..., None])
        elif op == OP_HUE:
            v = hue(v, fac, xp)
    return v, mean_used


def augment(img_u8, mask_u8, params, size, backend=NP64):
    """img_u8 (N,H,W,C) uint8, mask_u8 (N,H,W) uint8, params (N,P) float32 (numpy) -> image (N,C,th,tw) in the backend's
    precision (numpy), mask (N,th,tw) int64, near (N,th,tw) bool, means (N,) float64."""
    xp = backend
    img_u8, mask_u8, params = np.asarray(img_u8), np.asarray(mask_u8), np.asarray(params, np.float32)
    N, H, W, C = img_u8.shape
    th, tw = size
    out_i, out_m, out_near, means = [], [], [], []
    for n in range(N):
        rec = params[n]
        cy, cx = int(rec[0]), int(rec[1])
        assert 0 <= cy and cy + th <= H and 0 <= cx and cx + tw <= W
        crop = img_u8[n, cy:cy + th, cx:cx + tw]
        cmask = mask_u8[n, cy:cy + th, cx:cx + tw]
        if rec[2] != 0:
            crop, cmask = crop[:, ::-1], cmask[:, ::-1]
        v = xp.asarray(np.ascontiguousarray(crop)) / 255.0
        v, mean_used = jitter(v, rec, xp)
        v = xp.numpy(v)
        means.append(mean_used)
        if rec[3] != 0:
            img, msk, near = v, cmask.astype(np.int64), np.zeros((th, tw), bool)
        else:
            sx, sy, inside, near = affine_source(rec[4:10], th, tw)
            img = np.where(inside[..., None], v[sy, sx], 0).astype(v.dtype)
            msk = np.where(inside, cmask[sy, sx], 0).astype(np.int64)
        out_i.append(np.transpose(img, (2, 0, 1)))
        out_m.append(msk)
        out_near.append(near)
    return np.stack(out_i), np.stack(out_m), np.stack(out_near), np.asarray(means, np.float64)
