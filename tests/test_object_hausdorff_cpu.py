"""No GPU: the numpy oracle of the object-level Hausdorff distance (tests/hausdorff_oracle.py) against SciPy and hand-computed
cases, the bounding-box bound on random pairs, and the product's boxes, per-pair distances and metrics.object_hausdorff on the
CPU lane emulator against the oracle -- the kernels' index arithmetic, the job tables and the host code, and that the work-item
order does not change a bit of the result."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401
import hausdorff_oracle as HO
import label_oracle as LO
import surface_oracle as SO


@pytest.fixture(scope="module")
def emu():
    import test_lane_emu as T
    from medt_amd import _lib as L
    lib = C.CDLL(T.build_emulator())
    lib.emu_set_order.argtypes = [C.c_int, C.c_ulonglong]
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


@pytest.fixture()
def emulated(emu):
    from emu_device import emulated_device
    with emulated_device(emu):
        yield emu


def dev(a):
    from emu_device import DeviceTensor
    return torch.from_numpy(np.ascontiguousarray(a)).as_subclass(DeviceTensor)


def all_pairs(ka, kb, n=0):
    return [(n, a, b) for a in range(1, ka + 1) for b in range(1, kb + 1)]


def ring7():
    """A 7x7 ring (label 1 of the first map) around a 3x3 square (label 1 of the second), both centred at (5, 5) of an 11x11 map."""
    ring = HO.rect(11, 11, (2, 2, 8, 8))
    ring[3:8, 3:8] = 0
    return ring.astype(np.int32), HO.rect(11, 11, (4, 4, 6, 6)).astype(np.int32)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_oracle_equals_scipy():
    from scipy import ndimage
    la, ka = HO.blob_labels(33, 65, 4)
    lb, kb = HO.blob_labels(33, 65, 104)
    assert ka > 2 and kb > 2
    for _, a, b in all_pairs(ka, kb):
        A, B = la == a, lb == b
        want = (int(round(ndimage.distance_transform_edt(~B)[A].max() ** 2)), int(round(ndimage.distance_transform_edt(~A)[B].max() ** 2)))
        assert HO.pair_sq(la, a, lb, b) == want, (a, b)


def test_oracle_on_hand_computed_cases():
    one = np.zeros((6, 6), np.int32)
    other = one.copy()
    one[0, 0], other[3, 4] = 1, 1                                   # two 1-pixel objects, 3 and 4 apart
    assert HO.pair_sq(one, 1, other, 1) == (25, 25)
    ring, square = ring7()
    # from the ring: its corner (2,2) to the square's corner (4,4): 2^2 + 2^2; from the square: its centre (5,5) is 3 from the ring
    assert HO.pair_sq(ring, 1, square, 1) == (8, 9) and HO.hausdorff_sq(ring, 1, square, 1) == 9
    la, ka = HO.blob_labels(33, 65, 4)
    for a in range(1, ka + 1):
        assert HO.pair_sq(la, a, la, a) == (0, 0)                   # identical objects
    # the score: one target object of 2 pixels matched by overlap, one predicted object without overlap
    G = np.zeros((4, 12), np.int32)
    P = G.copy()
    G[0, 0:2] = 1
    P[0, 1:3] = 1                                                   # overlaps G_1: H = 1
    P[0, 6:8] = 2                                                   # overlaps nothing: its partner is G_1, H = 6 (pixel 7 to pixel 1)
    s = HO.score_labelled(P, 2, G, 1)
    assert s["valid"] and s["partners_gt"] == [1] and s["partners_pred"] == [1, 1]
    assert s["hd"] == 0.5 * (1.0 * 1.0 + (0.5 * 1.0 + 0.5 * 6.0))


def test_box_bound_holds_on_random_pairs():
    import metrics
    pairs = equal = 0
    for seed in range(12):
        la, ka = HO.blob_labels(40, 56, seed)
        lb, kb = HO.blob_labels(40, 56, seed + 50)
        ba, bb = HO.boxes(la, ka), HO.boxes(lb, kb)
        for a in range(1, ka + 1):
            prod = metrics.hausdorff_box_bound_sq(ba[a].astype(np.int64), bb[1:].astype(np.int64))
            for b in range(1, kb + 1):
                lo, h2 = HO.bound(ba[a], bb[b]), HO.hausdorff_sq(la, a, lb, b)
                assert prod[b - 1] == lo * lo and lo * lo <= h2, (seed, a, b, lo, h2)
                pairs += 1
                equal += lo * lo == h2
    assert pairs > 500 and equal > 10


# ---- the emulated kernels ----------------------------------------------------------------------------------------------------------
def test_emulated_boxes_and_pairs_match_oracle_under_every_order(emu):
    from emu_device import emulated_device
    from medt_amd import ops
    la, ka = HO.blob_labels(33, 65, 4)
    lb, kb = HO.blob_labels(33, 65, 104)
    pairs = all_pairs(ka, kb)
    want = np.asarray([HO.pair_sq(la, a, lb, b) for _, a, b in pairs], np.int32)
    runs = []
    for mode, seed in ((0, 0), (1, 0), (2, 1), (2, 2)):
        emu.emu_set_order(mode, seed)
        try:
            with emulated_device(emu):
                A, B = dev(la), dev(lb)
                ca, cb = dev(np.asarray([ka], np.int32)), dev(np.asarray([kb], np.int32))
                box = ops.label_boxes(A, ca)
                got = ops.pair_hausdorff_sq(A, ca, B, cb, torch.tensor(pairs, dtype=torch.int32))
                small = ops.pair_hausdorff_sq(A, ca, B, cb, torch.tensor(pairs, dtype=torch.int32), max_scratch_elems=1)
        finally:
            emu.emu_set_order(0, 0)
        assert box.dtype == torch.int32 and got.dtype == torch.int32 and tuple(got.shape) == (len(pairs), 2)
        runs.append((box.numpy().tobytes(), got.numpy().tobytes(), small.numpy().tobytes()))
    assert all(r == runs[0] for r in runs)
    assert runs[0][0] == HO.boxes(la, ka)[None].tobytes()
    assert runs[0][1] == want.tobytes() and runs[0][2] == want.tobytes()


def test_emulated_hand_cases_and_refusals(emulated):
    from medt_amd import MedtError, ops
    ring, square = ring7()
    one = dev(np.asarray([1], np.int32))
    got = ops.pair_hausdorff_sq(dev(ring), one, dev(square), one, torch.tensor([[0, 1, 1]], dtype=torch.int32))
    assert got.tolist() == [[8, 9]]
    got = ops.pair_hausdorff_sq(dev(ring), one, dev(ring), one, torch.tensor([[0, 1, 1]], dtype=torch.int32))
    assert got.tolist() == [[0, 0]]
    none = ops.pair_hausdorff_sq(dev(ring), one, dev(square), one, torch.zeros(0, 3, dtype=torch.int32))
    assert tuple(none.shape) == (0, 2)
    two = dev(np.asarray([2], np.int32))                             # label 2 is counted but has no pixel
    assert ops.label_boxes(dev(ring), two)[0].tolist() == [[11, 11, -1, -1], [2, 2, 8, 8], [11, 11, -1, -1]]
    with pytest.raises(MedtError, match=r"\(-1\).*without a pixel"):
        ops.pair_hausdorff_sq(dev(ring), two, dev(square), one, torch.tensor([[0, 2, 1]], dtype=torch.int32))
    with pytest.raises(MedtError, match=r"\(-1\)"):
        ops.pair_hausdorff_sq(dev(ring), one, dev(square), one, torch.tensor([[0, 1, 2]], dtype=torch.int32))
    with pytest.raises(MedtError):
        ops.pair_hausdorff_sq(dev(ring), one, dev(square), one, torch.tensor([[0, 1, 1]], dtype=torch.int64))


def score_maps():
    """(pred, target) uint8 (3,40,56): blob maps of different seeds, so that objects without overlap exist on both sides."""
    pred = np.stack([SO.blobs(40, 56, s) for s in (1, 2, 3)])
    target = np.stack([SO.blobs(40, 56, s) for s in (31, 32, 33)])
    return pred * np.uint8(255), target * np.uint8(255)


def test_emulated_object_hausdorff_prune_on_and_off(emulated):
    import metrics
    pred, target = score_maps()
    on = metrics.object_hausdorff(dev(pred), dev(target))
    off = metrics.object_hausdorff(dev(pred), dev(target), prune=False)
    unmatched = 0
    for n in range(3):
        want = HO.object_hausdorff(pred[n], target[n])
        P, G = LO.label(pred[n], 8)[0], LO.label(target[n], 8)[0]
        unmatched += sum(1 for i in range(1, want["n_gt"] + 1) if not (P[G == i] > 0).any())
        unmatched += sum(1 for j in range(1, want["n_pred"] + 1) if not (G[P == j] > 0).any())
        for got in (on, off):
            assert bool(got["valid"][n]) and (int(got["n_pred"][n]), int(got["n_gt"][n])) == (want["n_pred"], want["n_gt"])
            assert got["partners_gt"][n].tolist() == want["partners_gt"] and got["partners_pred"][n].tolist() == want["partners_pred"]
            assert float(got["hd"][n]) == want["hd"], (n, float(got["hd"][n]), want["hd"])
    assert unmatched > 4, "no object without overlap: the case checks nothing"
    assert on["hd"].dtype == torch.float64 and on["pairs"].dtype == torch.int64 and on["valid"].dtype == torch.bool
    assert torch.equal(on["hd"], off["hd"]) and int(on["pairs"].sum()) < int(off["pairs"].sum())      # pruning saved jobs


def test_emulated_object_hausdorff_empty_sides_and_given_labels(emulated):
    import metrics
    pred, target = score_maps()
    zero = np.zeros_like(pred[0])
    got = metrics.object_hausdorff(dev(np.stack([zero, pred[0], zero, pred[1]])), dev(np.stack([zero, zero, target[0], target[1]])))
    assert got["valid"].tolist() == [False, False, False, True] and got["pairs"][:3].tolist() == [0, 0, 0]
    assert all(math.isnan(float(got["hd"][n])) for n in range(3))
    assert float(got["hd"][3]) == HO.object_hausdorff(pred[1], target[1])["hd"]
    assert got["n_pred"][:3].tolist() == [0, LO.label(pred[0], 8)[1], 0]
    P, kp = LO.label(pred[2], 4)
    G, kg = LO.label(target[2], 4)
    given = metrics.object_hausdorff(dev(P), dev(G), labelled=True)
    want = HO.score_labelled(P, kp, G, kg)
    assert float(given["hd"][0]) == want["hd"] and given["partners_gt"][0].tolist() == want["partners_gt"]
    assert float(metrics.object_hausdorff(dev(pred[2]), dev(target[2]), connectivity=4)["hd"][0]) == want["hd"]
