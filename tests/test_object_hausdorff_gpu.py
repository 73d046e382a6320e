"""Bounding boxes, per-pair directed Hausdorff distances and the object-level Hausdorff distance on the device (medt_label_boxes,
medt_pair_hausdorff; medt_amd.ops.label_boxes / pair_hausdorff_sq, metrics.object_hausdorff) against the brute-force numpy oracle
(tests/hausdorff_oracle.py) and the host SciPy path: every integer with torch.equal / array_equal, the float64 score exactly.
Written against the `device` fixture: `--emulate` runs everything on the CPU lane emulator."""
import functools
import math

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401
import hausdorff_oracle as HO
import label_oracle as LO
from test_label_gpu import _as_device, _dev, _host

pytestmark = pytest.mark.gpu


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


def _counts(ks, device):
    return _dev(np.asarray(ks, np.int32), device)


# ---- 1. boxes --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_case(h, w):
    """(label map, K, boxes) of a dense random mask at 4-connectivity: many small components, their labels in raster order."""
    lab, k = LO.label(LO.random_mask(h, w, 0.41, 7 * h + w), 4)
    want = HO.boxes(lab, k)
    for v in (lab, want):
        v.setflags(write=False)
    return lab, k, want


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (16, 64), (17, 65), (40, 132)], ids=lambda v: str(v))
def test_label_boxes_match_numpy(device, h, w):
    from medt_amd import ops
    lab, k, want = box_case(h, w)
    box = ops.label_boxes(_dev(lab, device), _counts([k], device))
    assert box.dtype == torch.int32 and tuple(box.shape) == (1, k + 1, 4)
    assert np.array_equal(_host(box)[0], want)
    assert _host(box)[0, 0].tolist() == [h, w, -1, -1]                                   # slot 0: never written
    one = ops.label_boxes(_dev(lab, device), _counts([k], device))                       # and again: the same bits
    assert torch.equal(one.cpu(), box.cpu())
    if (h, w) == (40, 132):
        # the same components under shuffled labels (a label map is taken as given): labels that are equal modulo the 256 slots
        # of a workgroup's LDS table now meet inside one 1024-pixel chunk, the claim of a slot is lost and the box goes to the
        # global table directly
        perm = np.concatenate([[0], 1 + np.random.default_rng(1).permutation(k)]).astype(np.int32)
        shuffled = perm[lab]
        lost = 0
        for c in range(0, shuffled.size, 1024):
            u = np.unique(shuffled.reshape(-1)[c:c + 1024])
            lost += len(u[u > 0]) - len(set((u[u > 0] % 256).tolist()))
        assert lost > 20
        want_shuffled = np.empty_like(want)
        want_shuffled[perm] = want
        assert np.array_equal(_host(ops.label_boxes(_dev(shuffled, device), _counts([k], device)))[0], want_shuffled)


def test_label_boxes_batch_with_an_empty_image_and_the_frame(device):
    from medt_amd import ops
    h, w = 17, 65
    a, ka = box_case(h, w)[:2]
    frame = np.zeros((h, w), np.int32)
    frame[0, :], frame[-1, :], frame[:, 0], frame[:, -1] = 1, 1, 1, 1                    # one label that touches all four sides
    frame[8, 30:33] = 2
    labs = np.stack([a, np.zeros((h, w), np.int32), frame])
    ks = [ka, 0, 2]
    stride = ka + 1
    box = _host(ops.label_boxes(_dev(labs, device), _counts(ks, device)))
    assert box.shape == (3, stride, 4)
    for n in range(3):
        assert np.array_equal(box[n], HO.boxes(labs[n], ks[n], stride)), n
    assert (box[1] == np.asarray([h, w, -1, -1])).all()
    assert box[2, 1].tolist() == [0, 0, h - 1, w - 1] and box[2, 2].tolist() == [8, 30, 8, 32]


def test_label_boxes_on_unaligned_and_non_contiguous_views(device):
    """A label map one element into its buffer (W % 4 == 0, so only the pointer sends it down the element-access body) and a
    column slice of a wider map."""
    from medt_amd import ops
    lab, k, want = box_case(16, 64)
    store = torch.zeros(lab.size + 8, dtype=torch.int32)
    store[1:1 + lab.size] = torch.from_numpy(lab.copy()).reshape(-1)
    view = _as_device(store, device)[1:1 + lab.size].view(16, 64)
    assert view.data_ptr() % 16 == 4
    assert np.array_equal(_host(ops.label_boxes(view, _counts([k], device)))[0], want)
    wide = np.zeros((16, 80), np.int32)
    wide[:, 5:69] = lab
    sliced = _dev(wide, device)[:, 5:69]
    assert not sliced.is_contiguous()
    assert np.array_equal(_host(ops.label_boxes(sliced, _counts([k], device)))[0], want)


# ---- 2. pairs ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blob_case(h, w, seed):
    """Two blob label maps and, from the oracle, the distances of every pair (a, b) of them and of every (a, a') of the first
    with itself (computed once, shared, never written to)."""
    la, ka = HO.blob_labels(h, w, seed)
    lb, kb = HO.blob_labels(h, w, seed + 100)
    ab = [(0, a, b) for a in range(1, ka + 1) for b in range(1, kb + 1)]
    aa = [(0, a, b) for a in range(1, ka + 1) for b in range(1, ka + 1)]
    ref = {"la": la, "ka": ka, "lb": lb, "kb": kb, "ab": ab, "aa": aa,
           "want_ab": np.asarray([HO.pair_sq(la, a, lb, b) for _, a, b in ab], np.int32),
           "want_aa": np.asarray([HO.pair_sq(la, a, la, b) for _, a, b in aa], np.int32)}
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@pytest.mark.parametrize("h,w,seed", [(33, 65, 4), (48, 80, 5)], ids=["33x65", "48x80"])
def test_every_pair_of_blob_maps(device, h, w, seed):
    from medt_amd import ops
    ref = blob_case(h, w, seed)
    assert ref["ka"] > 3 and ref["kb"] > 3
    A, B = _dev(ref["la"], device), _dev(ref["lb"], device)
    ca, cb = _counts([ref["ka"]], device), _counts([ref["kb"]], device)
    got = ops.pair_hausdorff_sq(A, ca, B, cb, _i32(ref["ab"]))
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(ref["want_ab"].copy()))
    own = ops.pair_hausdorff_sq(A, ca, A, ca, _i32(ref["aa"]))                         # every object against every object of its own map
    assert torch.equal(own.cpu(), torch.from_numpy(ref["want_aa"].copy()))
    diag = [k for k, (_, a, b) in enumerate(ref["aa"]) if a == b]
    assert (own.cpu()[diag] == 0).all() and (ref["want_aa"] > 0).any()
    # the two columns are the two directions: swapping the maps swaps them
    back = ops.pair_hausdorff_sq(B, cb, A, ca, _i32([(0, b, a) for _, a, b in ref["ab"]]))
    assert torch.equal(back.cpu(), got.cpu().flip(1))


def _check_pairs(device, la, ka, lb, kb, pairs=None, **kw):
    from medt_amd import ops
    pairs = pairs or [(0, a, b) for a in range(1, ka + 1) for b in range(1, kb + 1)]
    want = torch.tensor([HO.pair_sq(la, a, lb, b) for _, a, b in pairs], dtype=torch.int32)
    got = ops.pair_hausdorff_sq(_dev(la, device), _counts([ka], device), _dev(lb, device), _counts([kb], device), _i32(pairs), **kw)
    assert torch.equal(got.cpu(), want), (got.cpu().tolist(), want.tolist())
    return want


def test_single_pixels_the_frame_and_nested_objects(device):
    la = np.zeros((9, 11), np.int32)
    lb = la.copy()
    la[0, 0], la[8, 10], la[4, 5] = 1, 2, 3                                            # single pixels, two of them in corners
    lb[3, 4], lb[0, 10], lb[8, 0] = 1, 2, 3
    want = _check_pairs(device, la, 3, lb, 3)
    assert want[0].tolist() == [25, 25] and want[1].tolist() == [100, 100]            # (0,0)-(3,4): 3 and 4 apart; (0,0)-(0,10)
    one = np.zeros((1, 1), np.int32) + 1
    _check_pairs(device, one, 1, one, 1)                                               # a 1x1 map
    # objects that are the frame / lie on it
    fa = np.zeros((12, 14), np.int32)
    fa[0, :], fa[-1, :], fa[:, 0], fa[:, -1] = 1, 1, 1, 1
    fb = np.zeros((12, 14), np.int32)
    fb[0, 3:9], fb[5:9, 13], fb[11, 0] = 1, 2, 3
    _check_pairs(device, fa, 1, fb, 3)
    # a ring around a blob: the largest distance from the blob to the ring lies in the blob's interior
    ring = HO.rect(21, 23, (2, 2, 18, 20)).astype(np.int32)
    ring[3:18, 3:20] = 0
    blob = HO.rect(21, 23, (6, 7, 14, 15)).astype(np.int32)
    want = _check_pairs(device, ring, 1, blob, 1)
    border_only = max(HO.directed_sq(b, ring == 1) for b in [(blob == 1) & ~HO.rect(21, 23, (7, 8, 13, 14)).astype(bool)])
    assert int(want[0, 1]) > border_only                                               # (a border-only distance would be smaller)


def test_a_row_wider_than_a_workgroup(device):
    """8 x 600, two thin objects: one crop row is wider than a 256-wide workgroup, so a work-item's strided loop takes several
    pixels and the outward search both runs far (the ends of the long object) and exits early (above the short one)."""
    la = np.zeros((8, 600), np.int32)
    lb = la.copy()
    la[1, :] = 1
    lb[6, 100:401] = 1
    want = _check_pairs(device, la, 1, lb, 1)
    assert want[0].tolist() == [199 ** 2 + 25, 25]
    _check_pairs(device, lb, 1, la, 1)


def test_pairs_of_several_images_interleaved_and_chunked(device):
    from medt_amd import ops
    r4, r5 = blob_case(33, 65, 4), blob_case(33, 65, 14)
    la = np.stack([r4["la"], r5["la"], r4["lb"]])
    lb = np.stack([r4["lb"], r5["lb"], r4["la"]])
    ka, kb = [r4["ka"], r5["ka"], r4["kb"]], [r4["kb"], r5["kb"], r4["ka"]]
    per_image = [[(n, a, b) for a in range(1, ka[n] + 1) for b in range(1, kb[n] + 1)] for n in range(3)]
    pairs = [p[k] for k in range(max(map(len, per_image))) for p in per_image if k < len(p)]      # image 0, 1, 2, 0, 1, 2, ...
    assert [p[0] for p in pairs[:6]] == [0, 1, 2, 0, 1, 2]
    want = torch.tensor([HO.pair_sq(la[n], a, lb[n], b) for n, a, b in pairs], dtype=torch.int32)
    A, B, ca, cb = _dev(la, device), _dev(lb, device), _counts(ka, device), _counts(kb, device)
    got = ops.pair_hausdorff_sq(A, ca, B, cb, _i32(pairs))
    assert torch.equal(got.cpu(), want)
    alone = ops.pair_hausdorff_sq(A, ca, B, cb, _i32(pairs), max_scratch_elems=1)      # every job a chunk of its own
    some = ops.pair_hausdorff_sq(A, ca, B, cb, _i32(pairs), max_scratch_elems=300)     # a few jobs per chunk
    large = ops.pair_hausdorff_sq(A, ca, B, cb, _i32(pairs), max_scratch_elems=1 << 26)
    again = ops.pair_hausdorff_sq(A, ca, B, cb, _i32(pairs))
    for other in (alone, some, large, again):
        assert _host(other).tobytes() == _host(got).tobytes()


def test_pair_limits_are_refused_on_the_host(device):
    from medt_amd import MedtError, _lib as L, ops
    la = np.zeros((4, 4), np.int32)
    la[1, 1] = 1
    A, one, two = _dev(la, device), _counts([1], device), _counts([2], device)
    with pytest.raises(MedtError, match=r"\(-1\).*without a pixel"):                   # MEDT_EINVAL, from the boxes
        ops.pair_hausdorff_sq(A, two, A, one, _i32([(0, 2, 1)]))
    with pytest.raises(MedtError, match=r"\(-1\)"):
        ops.pair_hausdorff_sq(A, one, A, one, _i32([(1, 1, 1)]))
    with pytest.raises(MedtError):
        ops.pair_hausdorff_sq(A, one, A, one, _i32([(0, 1, 1)]), max_scratch_elems=0)
    if device.type == "cuda":
        with pytest.raises(MedtError):
            ops.label_boxes(torch.from_numpy(la), torch.tensor([1], dtype=torch.int32))   # no CPU path
    lib = L.lib()
    box = _as_device(torch.zeros(1, 2, 4, dtype=torch.int32), device)
    jobs = _as_device(torch.zeros(1, 16, dtype=torch.int32), device)
    out = _as_device(torch.full((2,), 7, dtype=torch.int32), device)
    assert lib.medt_label_boxes(A.data_ptr(), box.data_ptr(), 1, 4, 4, 1, 1, None) == -1          # stride cannot hold label 1
    assert lib.medt_label_boxes(None, box.data_ptr(), 1, 4, 4, 2, 1, None) == -1
    assert lib.medt_label_boxes(A.data_ptr(), box.data_ptr(), 1, 4097, 4, 2, 1, None) == -2
    args = (A.data_ptr(), A.data_ptr(), jobs.data_ptr(), box.data_ptr(), out.data_ptr())
    assert lib.medt_pair_hausdorff(*args, 0, 1, 1, 8, 2, 1, 1, 4, 4, None) == -1                  # no job
    assert lib.medt_pair_hausdorff(*args, 1, 1, 1, 0, 2, 1, 1, 4, 4, None) == -1                  # no scratch
    assert lib.medt_pair_hausdorff(A.data_ptr(), None, *args[2:], 1, 1, 1, 8, 2, 1, 1, 4, 4, None) == -1
    assert (_host(box) == 0).all() and (_host(out) == 7).all()                                    # nothing was launched


# ---- 3. the score ------------------------------------------------------------------------------------------------------------------
def sparse_blobs(h, w, seed, density=0.004, grow=3):
    a = np.random.default_rng(seed).random((h, w)) < density
    for _ in range(grow):
        p = np.pad(a, 1)
        a = p[1:-1, 1:-1] | p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
    return a.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def score_case():
    """(pred, target) uint8 (3,96,128) {0,255} and the host SciPy score of every image.  Image 0 and 1: the target shifted by
    (2, 3) without its left third, plus unrelated blobs -- objects with a partner by overlap and objects without one on both
    sides.  Image 2: an empty prediction."""
    h, w = 96, 128
    target = np.stack([sparse_blobs(h, w, s) for s in (11, 12, 13)])
    pred = np.roll(target, (2, 3), axis=(1, 2))
    pred[:, :, :w // 3] = 0
    pred |= np.stack([sparse_blobs(h, w, s, 0.001) for s in (21, 22, 23)])
    pred[2] = 0
    rows = []
    for n in range(3):
        P, kp = LO.label(pred[n], 8)
        G, kg = LO.label(target[n], 8)
        r = HO.host_scipy(P, kp, G, kg)
        r["lonely_gt"] = sum(1 for i in range(1, kg + 1) if not (P[G == i] > 0).any())
        r["lonely_pred"] = sum(1 for j in range(1, kp + 1) if not (G[P == j] > 0).any())
        r["P"], r["G"] = P, G
        rows.append(r)
    pred, target = pred * np.uint8(255), target * np.uint8(255)
    for v in (pred, target):
        v.setflags(write=False)
    return pred, target, rows


def test_object_hausdorff_equals_the_host_scipy_path(device):
    """hd against one scipy.ndimage.distance_transform_edt per object on the host.  Both sides take float64 roots of the same
    integers and add the same products in the same order, so the bound is 0: exact equality (measured largest difference: 0)."""
    import metrics
    pred, target, rows = score_case()
    for n in (0, 1):                                                                   # the construction produced the cases
        assert rows[n]["valid"] and rows[n]["lonely_gt"] > 0 and rows[n]["lonely_pred"] > 0, (n, rows[n]["lonely_gt"], rows[n]["lonely_pred"])
        assert rows[n]["lonely_gt"] < rows[n]["n_gt"] and rows[n]["lonely_pred"] < rows[n]["n_pred"]
    assert rows[2]["n_pred"] == 0 and rows[2]["n_gt"] > 0 and not rows[2]["valid"]
    got = metrics.object_hausdorff(_dev(pred, device), _dev(target, device))
    off = metrics.object_hausdorff(_dev(pred, device), _dev(target, device), prune=False)
    assert got["hd"].dtype == torch.float64 and got["valid"].tolist() == [True, True, False]
    worst = 0.0
    for n in range(3):
        assert (int(got["n_pred"][n]), int(got["n_gt"][n])) == (rows[n]["n_pred"], rows[n]["n_gt"])
        if not rows[n]["valid"]:
            assert math.isnan(float(got["hd"][n])) and int(got["pairs"][n]) == 0
            continue
        for g in (got, off):
            assert g["partners_gt"][n].tolist() == rows[n]["partners_gt"] and g["partners_pred"][n].tolist() == rows[n]["partners_pred"]
        print(f"image {n}: hd {float(got['hd'][n])!r} host {rows[n]['hd']!r} jobs {int(got['pairs'][n])} / unpruned {int(off['pairs'][n])}")
        worst = max(worst, abs(float(got["hd"][n]) - rows[n]["hd"]))
    print("largest difference to the host path:", worst)
    assert worst == 0.0
    assert got["hd"][:2].tolist() == off["hd"][:2].tolist() and int(got["pairs"].sum()) < int(off["pairs"].sum())
    alone = metrics.object_hausdorff(_dev(pred[1], device), _dev(target[1], device))
    assert float(alone["hd"][0]).hex() == float(got["hd"][1]).hex()                   # an image scores the same alone


def test_object_hausdorff_of_given_instance_maps(device):
    import metrics
    _, _, rows = score_case()
    P, G = rows[0]["P"], rows[0]["G"]
    given = metrics.object_hausdorff(_dev(P, device), _dev(G, device), labelled=True)
    assert bool(given["valid"][0]) and float(given["hd"][0]) == rows[0]["hd"]
    # touching instances that a binary labelling would merge: two halves of one rectangle against the whole
    halves = np.zeros((20, 30), np.int32)
    halves[5:15, 4:14], halves[5:15, 14:24] = 1, 2
    whole = (halves > 0).astype(np.int32)
    got = metrics.object_hausdorff(_dev(halves, device), _dev(whole, device), labelled=True)
    want = HO.score_labelled(halves, 2, whole, 1)
    assert want["partners_pred"] == [1, 1] and want["partners_gt"] == [1]             # (equal overlaps: the lowest index)
    assert float(got["hd"][0]) == want["hd"] == 0.5 * (10.0 + 10.0)
    assert got["partners_gt"][0].tolist() == [1] and int(got["pairs"][0]) == 4
