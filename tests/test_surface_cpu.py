"""The surface-distance oracle (tests/surface_oracle.py) against SciPy and hand-computed cases, and the host-side surface of
the feature: binding table, header version, import without a device.  No GPU."""
import os
import re

import numpy as np
import pytest

import helpers as H  # noqa: F401
import surface_oracle as SO

SHAPES = [(1, 9, 1), (9, 1, 2), (5, 7, 3), (33, 65, 4), (70, 45, 5), (64, 64, 6), (17, 130, 7)]


@pytest.mark.parametrize("Hh,Ww,seed", SHAPES)
def test_oracle_matches_scipy(Hh, Ww, seed):
    nd = pytest.importorskip("scipy.ndimage")
    cross = nd.generate_binary_structure(2, 1)
    for s in (seed, seed + 100):
        a = SO.blobs(Hh, Ww, s)
        a[0, 0] = 1                                        # (never empty, whatever the seed draws on the small maps)
        A = a != 0
        assert np.array_equal(A & ~nd.binary_erosion(A, cross), SO.border(a))
        for F in (A, SO.border(a)):
            assert np.array_equal(np.rint(nd.distance_transform_edt(~F) ** 2).astype(np.int64), SO.edt_sq(F).astype(np.int64))


def test_oracle_blobs_are_the_dilated_draw():
    nd = pytest.importorskip("scipy.ndimage")
    raw = np.random.default_rng(4).random((33, 65)) < 0.02
    want = nd.binary_dilation(raw, nd.generate_binary_structure(2, 1), iterations=2)
    assert np.array_equal(SO.blobs(33, 65, 4) != 0, want)


def test_oracle_hand_cases():
    # two single pixels in opposite corners of a 1 x 9 map: every distance is 8
    a, b = np.zeros((1, 9), np.uint8), np.zeros((1, 9), np.uint8)
    a[0, 0], b[0, 8] = 1, 1
    hd, hd95, assd, hd_sq = SO.surface_scores(a, b)
    assert (hd, hd95, assd, hd_sq) == (8.0, 8.0, 8.0, 64)
    assert SO.surface_d2(a, b).tolist() == [[64, -1, -1, -1, -1, -1, -1, -1, -1]]
    # a full 5 x 5 map: the frame is the border; the centre is 2 from it
    full = np.ones((5, 5), np.uint8)
    bd = SO.border(full)
    assert bd.sum() == 16 and not bd[1:4, 1:4].any()
    assert SO.edt_sq(bd)[2, 2] == 4 and SO.edt_sq(full).max() == 0
    # a plus sign: its four arms are border, its centre is not; the diagonal neighbour of the centre is 1 away
    plus = np.zeros((5, 5), np.uint8)
    plus[2, 1:4] = plus[1:4, 2] = 1
    arms = plus != 0
    arms[2, 2] = False
    assert np.array_equal(SO.border(plus), arms)
    assert SO.edt_sq(plus)[1, 1] == 1 and SO.edt_sq(plus)[0, 0] == 5
    # identical masks: all distances 0;  empty: no scores, sentinel everywhere
    assert SO.surface_scores(plus, plus)[:3] == (0.0, 0.0, 0.0)
    assert SO.surface_scores(plus, np.zeros((5, 5), np.uint8)) is None
    assert (SO.edt_sq(np.zeros((3, 4), np.uint8)) == SO.NONE).all()
    # a 3 x 3 square against its centre pixel: A->B distances 1 (x4) and sqrt 2 (x4), B->A 1
    sq, c = np.zeros((7, 7), np.uint8), np.zeros((7, 7), np.uint8)
    sq[2:5, 2:5], c[3, 3] = 1, 1
    hd, hd95, assd, hd_sq = SO.surface_scores(sq, c)
    assert hd_sq == 2 and hd == np.sqrt(2.0)
    assert abs(assd - ((4 + 4 * np.sqrt(2.0)) / 8 + 1.0) / 2) < 1e-15
    assert hd95 == np.sqrt(2.0)                           # 9 values, 0.95 * 8 = 7.6: between two sqrt(2)


def test_binding_table_and_header():
    from medt_amd import _lib
    for name in ("medt_edt_cols", "medt_edt_rows"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["medt_edt_cols"][1]) == 7 and len(_lib.SIGNATURES["medt_edt_rows"][1]) == 7
    src = open(os.path.join(H.ROOT, "include", "medt_abi.h")).read()
    assert re.search(r"#define\s+MEDT_ABI_VERSION\s+11\b", src) and _lib.ABI_VERSION == 11
    assert re.search(r"#define\s+MEDT_EDT_NONE\s+2147483647\b", src)
    for name in ("medt_edt_cols", "medt_edt_rows"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src)


def test_surface_scores_importable_without_a_device():
    import torch
    import metrics
    from medt_amd import MedtError, ops
    assert callable(metrics.surface_scores) and callable(ops.edt_sq) and callable(ops.surface_d2)
    assert ops.EDT_NONE == SO.NONE
    with pytest.raises(MedtError):                        # no CPU path: a CPU tensor is refused
        ops.edt_sq(torch.zeros(4, 4, dtype=torch.uint8))
