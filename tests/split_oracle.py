"""TEST INFRASTRUCTURE: a numpy / SciPy restatement of DESIGN.md 'Splitting touching objects' (steps 1 to 8 of the definition):
scipy.ndimage.label, distance_transform_edt (its index output, so the squared depths are exact integers), maximum_filter and a
breadth-first growth, level by level, in which a pixel reached from several markers at once takes the smallest label.  Shares no
code with medt_amd.ops.split_* or csrc/split.hip."""
import numpy as np
from scipy import ndimage

EDT_NONE = 2 ** 31 - 1
BIG = np.int64(2 ** 62)


def structure(c):
    assert c in (4, 8)
    return None if c == 4 else np.ones((3, 3))


def depth2(mask):
    """(H,W) -> int64: squared distance to the nearest pixel of the image outside mask != 0; 0 outside; EDT_NONE without one."""
    F = mask != 0
    if F.all():
        return np.full(F.shape, EDT_NONE, np.int64)
    iy, ix = ndimage.distance_transform_edt(F, return_distances=False, return_indices=True)
    yy, xx = np.indices(F.shape)
    return ((iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2) * F


def near_top(M, d, t):
    """sqrt(M) - sqrt(d) <= t in integers (int64 arrays or Python ints)."""
    e = M - d - t * t
    return (e <= 0) | (e * e <= 4 * t * t * d)


def markers(mask, distance=7, tolerance=1, connectivity=8):
    """(H,W) mask -> uint8 {0,255} marker mask."""
    F = mask != 0
    comp, k = ndimage.label(F, structure(connectivity))
    d2 = depth2(mask)
    M = ndimage.maximum_filter(d2, size=2 * distance + 1, mode="constant", cval=0)
    cmax = np.zeros(k + 1, np.int64)
    if k:
        cmax[1:] = ndimage.maximum(d2, comp, np.arange(1, k + 1))
    return (F & (near_top(M, d2, np.int64(tolerance)) | (d2 == cmax[comp]))).astype(np.uint8) * np.uint8(255)


def _neighbours(a, connectivity, fill):
    """The shifted copies of a (H,W), `fill` shifted in at the frame."""
    p = np.pad(a, 1, constant_values=fill)
    H, W = a.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    return [p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in steps]


def grow(seeds, mask, connectivity=8):
    """(H,W) int seed map (> 0: a seed), mask -> (int32 labels, int32 step counts; -1 where no seed was reached)."""
    F = mask != 0
    lab = np.where(F & (seeds > 0), seeds, 0).astype(np.int64)
    dist = np.where(lab > 0, 0, -1).astype(np.int64)
    level = 0
    while True:
        front = np.where(dist == level, lab, BIG)
        cand = np.minimum.reduce(_neighbours(front, connectivity, BIG))
        new = F & (dist < 0) & (cand < BIG)
        if not new.any():
            break
        lab[new] = cand[new]
        dist[new] = level + 1
        level += 1
    return lab.astype(np.int32), dist.astype(np.int32)


def split(mask, distance=7, tolerance=1, connectivity=8):
    """(H,W) mask -> (int32 labels, K)."""
    seeds, k = ndimage.label(markers(mask, distance, tolerance, connectivity), structure(connectivity))
    return grow(seeds, mask, connectivity)[0], int(k)


def batched(fn, a, *more, **kw):
    """fn over the images of (N,H,W) arrays (or one (H,W) image) -> list of results, one per image."""
    a = np.asarray(a)
    if a.ndim == 2:
        return [fn(a, *more, **kw)]
    return [fn(a[n], *[m[n] if isinstance(m, np.ndarray) else m for m in more], **kw) for n in range(a.shape[0])]


def check_invariants(labels, k, mask, connectivity):
    """The consequences of the definition that hold for every input."""
    F = mask != 0
    assert np.array_equal(labels > 0, F)
    assert sorted(np.unique(labels[F]).tolist()) == list(range(1, k + 1))
    comp, _ = ndimage.label(F, structure(connectivity))
    for l in range(1, k + 1):
        cell = labels == l
        assert ndimage.label(cell, structure(connectivity))[1] == 1, ("label %d is not connected" % l)
        assert len(np.unique(comp[cell])) == 1, ("label %d spans components" % l)
