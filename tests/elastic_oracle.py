"""TEST INFRASTRUCTURE: the elastic deformation of the joint augmentation restated from its specification -- include/medt_abi.h's
medt_augment_warp comment / DESIGN.md 3l -- in array arithmetic, NOT from the kernel.  `warp(...)` evaluates it in float64 numpy
(backend NP64, everything in float64 from the float32 record and lattice) or, with backend=T32, in float32 torch on the CPU:
the spline, the map, the floors, the weights and the blend in float32, operation for operation in the order the specification
states, so its deviation from NP64 is the float32 noise of the whole formula, geometry included -- the yardstick of the GPU tests.

Jitter and the records without the elastic flag go through tests/augment_oracle.py.  `near` marks the output pixels whose fx
or fy (float64) lies within NEAR_TOL of an integer: the mask tap floor(f) and the inside test 0 <= f < size are discontinuous
only there, so a float32 evaluation may legitimately land on the other side; the bilinear image sample is continuous everywhere
else (floor(fx - .5) jumps where the weight wraps from 1 to 0).  Coordinates further than one pixel outside the crop are not near."""
import numpy as np

import augment_oracle as AO
from augment_oracle import NP64, T32  # noqa: F401  (the two backends, handed on)

NEAR_TOL = AO.NEAR_TOL
ELASTIC_SLOT = 18


def bspline(u):
    """The four cubic B-spline weights at u in [0, 1] (non-negative, sum 1), in the precision of u."""
    om, u2 = 1.0 - u, u * u
    u3 = u2 * u
    return [om * om * om / 6.0, (3.0 * u3 - 6.0 * u2 + 4.0) / 6.0, (-3.0 * u3 + 3.0 * u2 + 3.0 * u + 1.0) / 6.0, u3 / 6.0]


def cells(extent, G, xp):
    """(cell index as int64 numpy, the four weights) of the output coordinates 0 .. extent-1 under G cells:
    t = (k + .5) G / extent, c = min(floor(t), G - 1), u = t - c."""
    k = xp.asarray(np.arange(extent)) + 0.5
    t = k * G / extent
    c = np.minimum(xp.numpy(xp.floor(t)).astype(np.int64), G - 1)
    return c, bspline(t - xp.asarray(c))


def displacement(lattice, th, tw, xp):
    """lattice (2, G+3, G+3) float32 -> (dx, dy), each (th, tw):  d = sum_a B_a(v) (sum_b B_b(u) lattice[.][cy+a][cx+b]), b ascending
    inside, a ascending outside; lattice indices clamped to [0, G+2]."""
    lattice = np.asarray(lattice, np.float32)
    G = lattice.shape[-1] - 3
    assert lattice.shape == (2, G + 3, G + 3) and 1 <= G <= 8
    cx, Bu = cells(tw, G, xp)
    cy, Bv = cells(th, G, xp)
    out = []
    with np.errstate(all="ignore"):
        for k in range(2):
            acc = 0.0
            for a in range(4):
                iy = np.clip(cy + a, 0, G + 2)[:, None]
                s = 0.0
                for b in range(4):
                    ix = np.clip(cx + b, 0, G + 2)[None, :]
                    s = s + Bu[b][None, :] * xp.asarray(lattice[k][iy, ix])
                acc = acc + Bv[a][:, None] * s
            out.append(acc)
    return out


def coordinates(rec, lattice, th, tw, xp):
    """(fx, fy) of every output pixel, (th, tw) each, in the backend's precision: p = (j+.5+dx, i+.5+dy), f = M p or p."""
    dx, dy = displacement(lattice, th, tw, xp)
    j = (xp.asarray(np.arange(tw)) + 0.5)[None, :]
    i = (xp.asarray(np.arange(th)) + 0.5)[:, None]
    with np.errstate(all="ignore"):
        px, py = j + dx, i + dy
        if rec[3] != 0:
            return px, py
        m = [float(v) for v in rec[4:10]]
        return m[0] * px + m[1] * py + m[2], m[3] * px + m[4] * py + m[5]


def near_of(rec, lattice, th, tw):
    """The pixels whose float64 coordinate lies within NEAR_TOL of an integer, inside the +-1 pixel window (as AO.affine_source)."""
    fx, fy = coordinates(rec, lattice, th, tw, NP64)
    with np.errstate(all="ignore"):
        near = (np.abs(fx - np.round(fx)) < NEAR_TOL) | (np.abs(fy - np.round(fy)) < NEAR_TOL)
        near &= np.isfinite(fx) & np.isfinite(fy) & (fx > -1) & (fx < tw + 1) & (fy > -1) & (fy < th + 1)
    return near


def warp_one(crop_v, cmask, rec, lattice, xp):
    """crop_v (th, tw, C): the cropped, flipped, jittered image as numpy in the backend's precision; cmask (th, tw) likewise
    cropped and flipped -> image (th, tw, C) numpy, mask (th, tw) int64."""
    th, tw = cmask.shape
    fx, fy = coordinates(rec, lattice, th, tw, xp)
    with np.errstate(all="ignore"):
        inside = xp.numpy((fx >= 0) & (fx < tw) & (fy >= 0) & (fy < th)).astype(bool)            # False for NaN
        sx = np.where(inside, xp.numpy(xp.floor(fx)), 0).astype(np.int64)
        sy = np.where(inside, xp.numpy(xp.floor(fy)), 0).astype(np.int64)
        msk = np.where(inside, cmask[sy, sx], 0).astype(np.int64)
        ux, uy = fx - 0.5, fy - 0.5
        fx0, fy0 = xp.floor(ux), xp.floor(uy)
        wx, wy = (ux - fx0)[..., None], (uy - fy0)[..., None]
        x0 = np.where(inside, xp.numpy(fx0), 0).astype(np.int64)
        y0 = np.where(inside, xp.numpy(fy0), 0).astype(np.int64)
        xa, xb = np.clip(x0, 0, tw - 1), np.clip(x0 + 1, 0, tw - 1)
        ya, yb = np.clip(y0, 0, th - 1), np.clip(y0 + 1, 0, th - 1)
        t00, t01, t10, t11 = (xp.asarray(crop_v[y, x]) for y, x in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
        img = xp.numpy((1.0 - wy) * ((1.0 - wx) * t00 + wx * t01) + wy * ((1.0 - wx) * t10 + wx * t11))
    img = np.where(inside[..., None], img, 0).astype(crop_v.dtype)
    return img, msk


def warp(img_u8, mask_u8, params, field, size, backend=NP64):
    """img_u8 (N,H,W,C) uint8, mask_u8 (N,H,W) uint8, params (N,20) float32, field (N,2,G+3,G+3) float32 -> image (N,C,th,tw) in
    the backend's precision (numpy), mask (N,th,tw) int64, near (N,th,tw) bool, means (N,) float64.  Records without the
    elastic flag are AO.augment's."""
    xp = backend
    img_u8, mask_u8, params = np.asarray(img_u8), np.asarray(mask_u8), np.asarray(params, np.float32)
    field = np.asarray(field, np.float32)
    N = len(img_u8)
    th, tw = size
    out_i, out_m, out_near, means = [], [], [], []
    for n in range(N):
        rec = params[n]
        if rec[ELASTIC_SLOT] == 0:
            i1, m1, n1, me1 = AO.augment(img_u8[n:n + 1], mask_u8[n:n + 1], params[n:n + 1], size, backend)
            out_i.append(i1[0]), out_m.append(m1[0]), out_near.append(n1[0]), means.append(me1[0])
            continue
        cy, cx = int(rec[0]), int(rec[1])
        assert 0 <= cy and cy + th <= img_u8.shape[1] and 0 <= cx and cx + tw <= img_u8.shape[2]
        crop = img_u8[n, cy:cy + th, cx:cx + tw]
        cmask = mask_u8[n, cy:cy + th, cx:cx + tw]
        if rec[2] != 0:
            crop, cmask = crop[:, ::-1], cmask[:, ::-1]
        v = xp.asarray(np.ascontiguousarray(crop)) / 255.0
        v, mean_used = AO.jitter(v, rec, xp)                   # every tap is jittered BEFORE the blend; the mean is the unwarped crop's
        img, msk = warp_one(xp.numpy(v), cmask, rec, field[n], xp)
        out_i.append(np.transpose(img, (2, 0, 1)))
        out_m.append(msk)
        out_near.append(near_of(rec, field[n], th, tw))
        means.append(mean_used)
    return np.stack(out_i), np.stack(out_m), np.stack(out_near), np.asarray(means, np.float64)
