"""TEST INFRASTRUCTURE: plain-numpy restatement of connected-component labelling (medt_amd.ops.label / label_tables /
remove_small_objects / fill_holes / label_overlaps) by flood fill, and of the object-level scores (metrics.object_scores) from
their formulas on a dense overlap matrix.  For small maps only.  tests/test_label_cpu.py holds it to SciPy and to hand-computed
cases."""
import numpy as np


# ---- labelling -------------------------------------------------------------------------------------------------------------
def label(mask, conn):
    """(int32 (H,W) labels, K): components of mask != 0 at connectivity 4 or 8, numbered from 1 in raster order of their first pixel."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if conn == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    else:
        assert conn == 4
    lab = np.zeros((H, W), np.int32)
    k = 0
    for y in range(H):
        for x in range(W):
            if not m[y, x] or lab[y, x]:
                continue
            k += 1
            lab[y, x] = k
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for dy, dx in steps:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and m[ny, nx] and not lab[ny, nx]:
                        lab[ny, nx] = k
                        stack.append((ny, nx))
    return lab, k


def tables(lab, k, stride=None):
    """(int32 area[stride], uint8 frame[stride]) of a label map with labels 0..k; stride defaults to k + 1."""
    stride = k + 1 if stride is None else stride
    area = np.zeros(stride, np.int32)
    frame = np.zeros(stride, np.uint8)
    H, W = lab.shape
    for y in range(H):
        for x in range(W):
            v = lab[y, x]
            area[v] += 1
            if v and (y in (0, H - 1) or x in (0, W - 1)):
                frame[v] = 1
    return area, frame


def remove_small(mask, min_area, conn):
    lab, k = label(mask, conn)
    area, _ = tables(lab, k)
    keep = area >= min_area
    keep[0] = False
    return (keep[lab] * 255).astype(np.uint8)


def fill_holes(mask):
    m = np.asarray(mask) != 0
    lab, k = label(~m, 4)
    _, frame = tables(lab, k)
    hole = frame == 0
    hole[0] = False
    return ((m | hole[lab]) * 255).astype(np.uint8)


def overlaps(la, lb, n=0):
    """int64 (M,4) rows (n, a, b, |a ∩ b|), a > 0 and b > 0, sorted by (a, b)."""
    pairs = {}
    for a, b in zip(la.reshape(-1).tolist(), lb.reshape(-1).tolist()):
        if a > 0 and b > 0:
            pairs[(a, b)] = pairs.get((a, b), 0) + 1
    return np.asarray([(n, a, b, c) for (a, b), c in sorted(pairs.items())], np.int64).reshape(-1, 4)


# ---- scores ----------------------------------------------------------------------------------------------------------------
KEYS = ("f1", "dice", "aji", "pq", "dq", "sq")


def scores_labelled(P, kp, G, kg):
    """The scores of a predicted label map P (labels 1..kp) against a target label map G (labels 1..kg): a dict of python floats
    f1, dice, aji, pq, dq, sq, ints n_pred, n_gt and bool valid.  I[i, j] = |G_i ∩ P_j| (0-based here)."""
    out = {"n_pred": kp, "n_gt": kg, "valid": bool(kp or kg)}
    if not kp and not kg:
        out.update({k: float("nan") for k in KEYS})
        return out
    if not kp or not kg:
        out.update({k: 0.0 for k in KEYS})
        return out
    I = np.zeros((kg, kp), np.int64)
    both = (G > 0) & (P > 0)
    np.add.at(I, (G[both] - 1, P[both] - 1), 1)
    ag = np.bincount(G.reshape(-1), minlength=kg + 1)[1:].astype(np.int64)
    ap = np.bincount(P.reshape(-1), minlength=kp + 1)[1:].astype(np.int64)
    # GlaS object F1
    tp, hit = 0, set()
    for j in range(kp):
        i = int(np.argmax(I[:, j]))                       # (argmax: the first of equal values = the lowest index)
        if I[i, j] > 0 and 2 * int(I[i, j]) >= int(ag[i]):
            tp += 1
            hit.add(i)
    fp, fn = kp - tp, kg - len(hit)
    out["f1"] = 2.0 * tp / (2 * tp + fp + fn)
    # GlaS object Dice
    sg = sp = 0.0
    for i in range(kg):
        j = int(np.argmax(I[i]))
        d = 2.0 * int(I[i, j]) / (int(ag[i]) + int(ap[j])) if I[i, j] > 0 else 0.0
        sg += (int(ag[i]) / int(ag.sum())) * d
    for j in range(kp):
        i = int(np.argmax(I[:, j]))
        d = 2.0 * int(I[i, j]) / (int(ag[i]) + int(ap[j])) if I[i, j] > 0 else 0.0
        sp += (int(ap[j]) / int(ap.sum())) * d
    out["dice"] = 0.5 * (sg + sp)
    # AJI
    C = U = 0
    used = set()
    for i in range(kg):
        best, bj = -1.0, -1
        for j in range(kp):
            if I[i, j] > 0:
                iou = int(I[i, j]) / (int(ag[i]) + int(ap[j]) - int(I[i, j]))
                if iou > best:
                    best, bj = iou, j
        if bj >= 0:
            C += int(I[i, bj])
            U += int(ag[i]) + int(ap[bj]) - int(I[i, bj])
            used.add(bj)
        else:
            U += int(ag[i])
    U += sum(int(ap[j]) for j in range(kp) if j not in used)
    out["aji"] = C / U
    # PQ
    tp, siou = 0, 0.0
    for i in range(kg):
        for j in range(kp):
            u = int(ag[i]) + int(ap[j]) - int(I[i, j])
            if 2 * int(I[i, j]) > u:
                tp += 1
                siou += int(I[i, j]) / u
    fp, fn = kp - tp, kg - tp
    out["dq"] = tp / (tp + fp / 2 + fn / 2)
    out["sq"] = siou / tp if tp else 0.0
    out["pq"] = out["dq"] * out["sq"]
    return out


def object_scores(pred, target, conn=8):
    """scores_labelled of two binary masks labelled at `conn`."""
    P, kp = label(pred, conn)
    G, kg = label(target, conn)
    return scores_labelled(P, kp, G, kg)


def objects_line(rows, total):
    """The line test.py --objects on prints, from the per-image score dicts."""
    ok = [r for r in rows if r["valid"]]
    mean = [float(np.mean(np.asarray([r[k] for r in ok], np.float64))) if ok else float("nan") for k in ("f1", "dice", "aji", "pq")]
    return "objects images {}/{}  F1obj {:.4f}  Diceobj {:.4f}  AJI {:.4f}  PQ {:.4f}".format(len(ok), total, *mean)


# ---- patterns (uint8 {0,1}) ---------------------------------------------------------------------------------------------------
def random_mask(H, W, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


def serpentine(H, W):
    """One 1-pixel path: every second row is set, joined alternately at the right and at the left end."""
    a = np.zeros((H, W), np.uint8)
    a[0::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        a[y, W - 1 if k % 2 == 0 else 0] = 1
    return a


def comb(H, W):
    """Vertical bars every second column, joined only by the last row."""
    a = np.zeros((H, W), np.uint8)
    a[:, 0::2] = 1
    a[H - 1] = 1
    return a


def checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def diagonal(H, W):
    a = np.zeros((H, W), np.uint8)
    k = np.arange(min(H, W))
    a[k, k] = 1
    return a


def corner_pair(H, W, y, x):
    """Two pixels that touch only diagonally across the point where the tiles above-left and below-right of (y, x) meet."""
    a = np.zeros((H, W), np.uint8)
    a[y - 1, x - 1] = a[y, x] = 1
    return a


def anti_corner_pair(H, W, y, x):
    a = np.zeros((H, W), np.uint8)
    a[y - 1, x] = a[y, x - 1] = 1
    return a


def ring(H, W, margin=1):
    a = np.zeros((H, W), np.uint8)
    if H > 2 * margin and W > 2 * margin:
        a[margin:H - margin, margin:W - margin] = 1
        if H > 2 * margin + 2 and W > 2 * margin + 2:
            a[margin + 1:H - margin - 1, margin + 1:W - margin - 1] = 0
    return a


def ring_in_ring(H, W):
    return ring(H, W, 1) | ring(H, W, 3)


def blobs_with_holes(H, W, seed):
    """Seeded blobs (a 3x3-dilated sprinkle) with single-pixel and 2-pixel holes punched in."""
    rng = np.random.default_rng(seed)
    a = rng.random((H, W)) < 0.04
    for _ in range(2):
        p = np.pad(a, 1)
        a = sum(p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) > 0
    holes = rng.random((H, W)) < 0.03
    holes[:, 1:] |= holes[:, :-1] & (rng.random((H, W - 1)) < 0.5) if W > 1 else False
    return (a & ~holes).astype(np.uint8)
