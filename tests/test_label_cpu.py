"""No GPU: the numpy oracle of the labelling tests (tests/label_oracle.py) against SciPy and against hand-computed scores, and the
product's labelling (medt_amd.ops.label and what builds on it, metrics.object_scores) on the CPU lane emulator against both --
the kernels' index arithmetic and the host code, and that the work-item order does not change a bit of the result."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401
import label_oracle as LO


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


def patterns():
    """(name, mask): random maps near both percolation thresholds and the structured patterns, 1x1 to about 140 per side."""
    out = [("one", np.ones((1, 1), np.uint8)), ("none", np.zeros((1, 1), np.uint8))]
    for k, (h, w) in enumerate([(1, 9), (9, 1), (5, 7), (33, 65), (70, 45), (17, 130), (64, 64), (140, 37), (90, 141)]):
        out += [(f"rand41_{h}x{w}", LO.random_mask(h, w, 0.41, 10 + k)), (f"rand59_{h}x{w}", LO.random_mask(h, w, 0.59, 30 + k))]
    for h, w in [(17, 65), (33, 129), (8, 8), (2, 2)]:
        out += [(f"serpentine_{h}x{w}", LO.serpentine(h, w)), (f"comb_{h}x{w}", LO.comb(h, w)),
                (f"checker_{h}x{w}", LO.checkerboard(h, w)), (f"diag_{h}x{w}", LO.diagonal(h, w)),
                (f"ring_{h}x{w}", LO.ring(h, w)), (f"rings_{h}x{w}", LO.ring_in_ring(h, w)),
                (f"full_{h}x{w}", np.ones((h, w), np.uint8)), (f"empty_{h}x{w}", np.zeros((h, w), np.uint8))]
    out += [("corner", LO.corner_pair(32, 128, 16, 64)), ("anticorner", LO.anti_corner_pair(32, 128, 16, 64)),
            ("holes", LO.blobs_with_holes(70, 45, 3)), ("holes2", LO.blobs_with_holes(40, 131, 4))]
    return out


def test_oracle_and_emulated_labels_equal_scipy(emulated):
    from scipy import ndimage
    from medt_amd import ops
    for name, m in patterns():
        for conn, structure in ((4, None), (8, np.ones((3, 3)))):
            want, k = ndimage.label(m, structure)
            lab, ko = LO.label(m, conn)
            assert ko == k and np.array_equal(lab, want), (name, conn)
            got, cnt = ops.label(dev(m * np.uint8(255)), conn)
            assert got.dtype == torch.int32 and cnt.tolist() == [k] and np.array_equal(got.numpy(), want), (name, conn)


def test_pattern_component_counts(emulated):
    """The counts the patterns are built for, from the oracle and from the emulated kernels."""
    from medt_amd import ops

    def counts(m):
        got = tuple(int(ops.label(dev(m), conn)[1][0]) for conn in (4, 8))
        assert got == (LO.label(m, 4)[1], LO.label(m, 8)[1])
        return got

    assert counts(LO.checkerboard(7, 9)) == (math.ceil(63 / 2), 1)
    assert counts(LO.diagonal(6, 9)) == (6, 1)
    assert counts(LO.serpentine(9, 6)) == (1, 1) and counts(LO.comb(9, 6)) == (1, 1)
    assert counts(LO.corner_pair(4, 4, 2, 2)) == (2, 1) and counts(LO.anti_corner_pair(32, 128, 16, 64)) == (2, 1)


def test_oracle_and_emulated_fill_holes_equal_scipy(emulated):
    from scipy import ndimage
    from medt_amd import ops
    for name, m in patterns():
        want = ndimage.binary_fill_holes(m != 0)
        assert np.array_equal(LO.fill_holes(m) == 255, want) and set(np.unique(LO.fill_holes(m))) <= {0, 255}, name
        got = ops.fill_holes(dev(m)).numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want * np.uint8(255)), name
    m = LO.random_mask(70, 45, 0.6, 1)                                              # the issue's own check
    assert np.array_equal(ops.fill_holes(dev(m)).numpy() == 255, ndimage.binary_fill_holes(m))
    inner = LO.fill_holes(LO.ring_in_ring(12, 14))
    assert (inner[1:-1, 1:-1] == 255).all() and inner[0].max() == 0                 # everything inside the outer ring is filled


def test_oracle_and_emulated_tables_and_small_objects(emulated):
    from scipy import ndimage
    from medt_amd import ops
    m = LO.blobs_with_holes(70, 45, 3)
    lab, k = LO.label(m, 8)
    area, frame = LO.tables(lab, k)
    assert np.array_equal(area[1:], ndimage.sum_labels(m, lab, np.arange(1, k + 1)).astype(np.int32)) and area[0] == (m == 0).sum()
    edge = np.zeros_like(m, bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    assert np.array_equal(frame[1:] != 0, np.isin(np.arange(1, k + 1), np.unique(lab[edge])))
    dl, dc = ops.label(dev(m), 8)
    ga, gf = ops.label_tables(dl, dc)
    assert np.array_equal(ga.numpy(), area[None]) and np.array_equal(gf.numpy(), frame[None])
    for a in (1, 2, int(np.median(area[1:])), int(area[1:].max()) + 1):
        want = np.isin(lab, 1 + np.nonzero(area[1:] >= a)[0]) * np.uint8(255)
        assert np.array_equal(LO.remove_small(m, a, 8), want)
        assert np.array_equal(ops.remove_small_objects(dev(m), a, 8).numpy(), want)
    assert LO.remove_small(m, int(area[1:].max()) + 1, 8).max() == 0


def row(width, *spans, rows=1, at=0):
    """A (rows + 2, width) map with the pixels [a, b) of row `at` set for every span."""
    m = np.zeros((rows + 2, width), np.uint8)
    for a, b in spans:
        m[at, a:b] = 1
    return m


# (name, pred, target, expected f1, dice, aji, pq, dq, sq) -- worked out by hand from the formulas in metrics.object_scores
HAND = [
    ("identical", row(9, (0, 3), (5, 8)), row(9, (0, 3), (5, 8)), 1.0, 1.0, 1.0, 1.0, 1.0, 1.0),
    # one gland of 8 pixels predicted as a 3-pixel and a 4-pixel piece: I = [3, 4]; only the second piece covers half of it
    # (2*4 >= 8, the >= edge), and its IoU is exactly 4/8 (the strict edge of PQ: no match)
    ("split", row(9, (0, 3), (4, 8)), row(9, (0, 8)), 2 / 3, 148 / 231, 4 / 11, 0.0, 0.0, 0.0),
    # two glands of 3 pixels predicted as one object of 7: I = [[3],[3]], the tie goes to the first gland
    ("merged", row(9, (0, 7)), row(9, (0, 3), (4, 7)), 2 / 3, 0.6, 3 / 7, 0.0, 0.0, 0.0),
    ("missed_and_spurious", row(9, (0, 3)) | row(9, (5, 8), at=2), row(9, (0, 3), (5, 8)), 0.5, 0.5, 1 / 3, 0.5, 0.5, 1.0),
    ("half_overlap", row(9, (2, 6)), row(9, (0, 4)), 1.0, 0.5, 1 / 3, 0.0, 0.0, 0.0),           # 2*2 >= 4: a true positive
    ("below_half_overlap", row(9, (3, 7)), row(9, (0, 5)), 0.0, 4 / 9, 2 / 7, 0.0, 0.0, 0.0),    # 2*2 < 5: not one
    ("iou_half", row(9, (0, 2)), row(9, (0, 4)), 1.0, 2 / 3, 0.5, 0.0, 0.0, 0.0),                # IoU 2/4 is not > 0.5
    ("iou_three_quarters", row(9, (0, 3)), row(9, (0, 4)), 1.0, 6 / 7, 0.75, 0.75, 1.0, 0.75),
]


def check_hand(got, name, want):
    for k, w in zip(("f1", "dice", "aji", "pq", "dq", "sq"), want):
        g = float(got[k])
        assert abs(g - w) <= 1e-15 + 1e-12 * abs(w), (name, k, g, w)


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_scores_on_hand_computed_cases(emulated, case):
    import metrics
    name, pred, target, *want = case
    o = LO.object_scores(pred, target, 8)
    assert o["valid"]
    check_hand(o, name, want)
    got = metrics.object_scores(dev(pred), dev(target))
    assert bool(got["valid"][0]) and got["f1"].dtype == torch.float64
    assert (int(got["n_pred"][0]), int(got["n_gt"][0])) == (o["n_pred"], o["n_gt"])
    check_hand({k: got[k][0] for k in LO.KEYS}, name, want)


def test_scores_with_empty_sides(emulated):
    import metrics
    empty, some = np.zeros((3, 9), np.uint8), row(9, (0, 3))
    o = LO.object_scores(empty, empty)
    assert not o["valid"] and all(math.isnan(o[k]) for k in LO.KEYS)
    for p, t in ((empty, some), (some, empty)):
        o = LO.object_scores(p, t)
        assert o["valid"] and all(o[k] == 0.0 for k in LO.KEYS)
    got = metrics.object_scores(dev(np.stack([empty, empty, some])), dev(np.stack([empty, some, empty])))
    assert got["valid"].tolist() == [False, True, True]
    for k in LO.KEYS:
        assert math.isnan(float(got[k][0])) and got[k][1:].tolist() == [0.0, 0.0], k
    assert got["n_pred"].tolist() == [0, 0, 1] and got["n_gt"].tolist() == [0, 1, 0]


def test_label_is_independent_of_work_item_order(emu):
    """ascending, descending and shuffled work-item orders of the emulator: identical bytes (labels and counts)."""
    from emu_device import emulated_device
    from medt_amd import ops
    masks = {"serpentine": LO.serpentine(35, 131), "random": LO.random_mask(35, 131, 0.59, 7)}
    for name, m in masks.items():
        want = LO.label(m, 4)
        runs = []
        for mode, seed in ((0, 0), (1, 0), (2, 1), (2, 2)):
            emu.emu_set_order(mode, seed)
            try:
                with emulated_device(emu):
                    lab, cnt = ops.label(dev(m), 4)
                    area, frame = ops.label_tables(lab, cnt)
            finally:
                emu.emu_set_order(0, 0)
            runs.append((lab.numpy().tobytes(), cnt.numpy().tobytes(), area.numpy().tobytes(), frame.numpy().tobytes()))
        assert all(r == runs[0] for r in runs), name
        assert runs[0][0] == want[0].tobytes() and np.frombuffer(runs[0][1], np.int32).tolist() == [want[1]], name


def test_label_tile_mirrors_the_header():
    import os
    import re
    from medt_amd import ops
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "medt_abi.h")).read()
    tile = tuple(int(re.search(r"#define\s+MEDT_LABEL_TILE_%s\s+(\d+)" % k, src).group(1)) for k in "HW")
    assert ops.LABEL_TILE == tile
