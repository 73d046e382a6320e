"""TEST INFRASTRUCTURE: plain-numpy restatement of the surface-distance scores (medt_amd.ops.edt_sq / surface_d2,
metrics.surface_scores) by brute force -- every (pixel, feature pixel) pair.  For small maps only.  tests/test_surface_cpu.py
holds it to SciPy and to hand-computed cases."""
import numpy as np

NONE = 2 ** 31 - 1                      # MEDT_EDT_NONE


def blobs(H, W, seed):
    """The seeded test mask: rng.random((H,W)) < 0.02, dilated twice by the 3x3 cross; uint8 {0,1}."""
    a = np.random.default_rng(seed).random((H, W)) < 0.02
    for _ in range(2):
        p = np.pad(a, 1)
        a = p[1:-1, 1:-1] | p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
    return a.astype(np.uint8)


def border(a):
    """Foreground pixels (a != 0) with a 4-neighbour outside the foreground; outside the image counts as outside."""
    a = np.asarray(a) != 0
    p = np.pad(a, 1)
    return a & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def edt_sq(f):
    """int32 (H,W): min over the pixels of f != 0 of the squared distance; NONE everywhere when f is empty."""
    f = np.asarray(f) != 0
    H, W = f.shape
    ys, xs = np.nonzero(f)
    if ys.size == 0:
        return np.full((H, W), NONE, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2
    return d.min(axis=-1).astype(np.int32)


def surface_d2(a, b):
    """int32 (H,W): at border pixels of a the squared distance to the border of b, -1 elsewhere."""
    return np.where(border(a), edt_sq(border(b)), -1).astype(np.int32)


def surface_scores(a, b):
    """(hd, hd95, assd, hd_sq) of two 2-D masks with foreground, float64; hd_sq is the integer under hd's root.  None when
    either mask has no foreground."""
    if not (np.asarray(a) != 0).any() or not (np.asarray(b) != 0).any():
        return None
    ab, ba = surface_d2(a, b), surface_d2(b, a)
    d_ab, d_ba = np.sqrt(ab[ab >= 0].astype(np.float64)), np.sqrt(ba[ba >= 0].astype(np.float64))
    hd_sq = int(max(ab.max(), ba.max()))
    return (float(np.sqrt(np.float64(hd_sq))), float(np.percentile(np.hstack((d_ab, d_ba)), 95)),
            float((d_ab.mean() + d_ba.mean()) / 2), hd_sq)
