"""TEST INFRASTRUCTURE: plain-numpy restatement of the bounding boxes (medt_amd.ops.label_boxes), of the directed squared
Hausdorff distances of object pairs (medt_amd.ops.pair_hausdorff_sq) by brute force over all pixel pairs, and of the object-level
Hausdorff distance of GlaS (metrics.object_hausdorff) with the matching written from the definition on a dense overlap matrix --
no pruning, no job tables.  For small objects only.  tests/test_object_hausdorff_cpu.py holds it to SciPy and to hand-computed
cases.  host_scipy() is the same score through one scipy.ndimage.distance_transform_edt per pair and direction: what a user
without the device path runs."""
import math

import numpy as np


def boxes(lab, k, stride=None):
    """int32 (stride, 4): (y0, x0, y1, x1), inclusive, of the labels 1..k; (H, W, -1, -1) for slot 0 and a label without a pixel."""
    stride = k + 1 if stride is None else stride
    H, W = lab.shape
    out = np.tile(np.asarray([H, W, -1, -1], np.int32), (stride, 1))
    for l in range(1, k + 1):
        ys, xs = np.nonzero(lab == l)
        if ys.size:
            out[l] = (ys.min(), xs.min(), ys.max(), xs.max())
    return out


def directed_sq(a, b):
    """max over the pixels of a (bool map) of the squared distance to the nearest pixel of b, an int; both non-empty."""
    ay, ax = np.nonzero(a)
    by, bx = np.nonzero(b)
    d = (ay[:, None] - by[None, :]).astype(np.int64) ** 2 + (ax[:, None] - bx[None, :]).astype(np.int64) ** 2
    return int(d.min(axis=1).max())


def pair_sq(la, a, lb, b):
    """(a -> b, b -> a) of object a of the label map la and object b of lb."""
    return directed_sq(la == a, lb == b), directed_sq(lb == b, la == a)


def hausdorff_sq(la, a, lb, b):
    return max(pair_sq(la, a, lb, b))


def bound(box_a, box_b):
    """The lower bound of H from two boxes (y0, x0, y1, x1): the largest of the four side differences."""
    return int(np.abs(np.asarray(box_a, np.int64) - np.asarray(box_b, np.int64)).max())


def _score(P, kp, G, kg, sq):
    """The score from a function sq(j, i) -> squared H(S_j, G_i): a dict hd (python float), valid, n_pred, n_gt, partners_gt
    (the predicted label matched to G_1..G_kg), partners_pred."""
    out = {"n_pred": kp, "n_gt": kg, "valid": bool(kp and kg), "hd": float("nan"), "partners_gt": [], "partners_pred": []}
    if not out["valid"]:
        return out
    I = np.zeros((kg, kp), np.int64)
    both = (G > 0) & (P > 0)
    np.add.at(I, (G[both] - 1, P[both] - 1), 1)
    ag = np.bincount(G.reshape(-1), minlength=kg + 1)[1:].astype(np.int64)
    ap = np.bincount(P.reshape(-1), minlength=kp + 1)[1:].astype(np.int64)
    assert ag.min() > 0 and ap.min() > 0, "every label 1..K has a pixel"
    cache = {}

    def h2(j, i):
        if (j, i) not in cache:
            cache[(j, i)] = sq(j, i)
        return cache[(j, i)]

    sg = sp = 0.0
    for i in range(1, kg + 1):
        if I[i - 1].max() > 0:
            j = int(np.argmax(I[i - 1])) + 1                # (argmax: the first of equal values = the lowest index)
        else:
            j = 1 + int(np.argmin([h2(jj, i) for jj in range(1, kp + 1)]))
        out["partners_gt"].append(j)
        sg += (int(ag[i - 1]) / int(ag.sum())) * math.sqrt(float(h2(j, i)))
    for j in range(1, kp + 1):
        if I[:, j - 1].max() > 0:
            i = int(np.argmax(I[:, j - 1])) + 1
        else:
            i = 1 + int(np.argmin([h2(j, ii) for ii in range(1, kg + 1)]))
        out["partners_pred"].append(i)
        sp += (int(ap[j - 1]) / int(ap.sum())) * math.sqrt(float(h2(j, i)))
    out["hd"] = 0.5 * (sg + sp)
    return out


def score_labelled(P, kp, G, kg):
    """Brute force: predicted label map P (labels 1..kp, each with a pixel) against the target label map G."""
    return _score(P, kp, G, kg, lambda j, i: hausdorff_sq(P, j, G, i))


def object_hausdorff(pred, target, conn=8):
    import label_oracle as LO
    P, kp = LO.label(pred, conn)
    G, kg = LO.label(target, conn)
    return score_labelled(P, kp, G, kg)


def host_scipy(P, kp, G, kg):
    """The same score with one whole-image scipy.ndimage.distance_transform_edt per object, cached, instead of brute force."""
    from scipy import ndimage
    edt = {}

    def to(side, lab, l):
        if (side, l) not in edt:
            edt[(side, l)] = ndimage.distance_transform_edt(lab != l)
        return edt[(side, l)]

    def sq(j, i):
        ab = to("g", G, i)[P == j].max()
        ba = to("p", P, j)[G == i].max()
        return int(round(float(max(ab, ba)) ** 2))

    return _score(P, kp, G, kg, sq)


def hausdorff_line(rows, total):
    """The line test.py --object_hausdorff on prints, from the per-image score dicts."""
    ok = [r["hd"] for r in rows if r["valid"]]
    mean = float(np.mean(np.asarray(ok, np.float64))) if ok else float("nan")
    return "object hausdorff images {}/{}  Hobj {:.4f}".format(len(ok), total, mean)


# ---- maps ----------------------------------------------------------------------------------------------------------------------
def blob_labels(H, W, seed, conn=8):
    """(int32 label map, K) of the seeded blob mask of the surface tests, labelled by the flood-fill oracle."""
    import label_oracle as LO
    import surface_oracle as SO
    return LO.label(SO.blobs(H, W, seed), conn)


def rect(H, W, *boxes_):
    """uint8 {0,1} map with the rectangles (y0, x0, y1, x1), inclusive, set."""
    m = np.zeros((H, W), np.uint8)
    for y0, x0, y1, x1 in boxes_:
        m[y0:y1 + 1, x0:x1 + 1] = 1
    return m
