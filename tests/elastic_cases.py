"""TEST INFRASTRUCTURE: the named cases of the elastic deformation (shapes, seeds, records, lattices) that tests/test_elastic_cpu.py
(the oracle alone: the cap on what a comparison may leave out) and tests/test_elastic_gpu.py (the kernel) share.

A case is a dict: img (N,H,W,C) uint8, mask (N,H,W) uint8 with classes 1 and 2 (the fill class 0 stands out), recs (N,20)
float32, field (N,2,G+3,G+3) float32, size (th, tw).  The lattice is normal with a standard deviation of a sixteenth of the
crop (at least half a pixel), clipped to three of them: displacements of a few pixels at 32 x 32, a dozen at 128 x 128.

SEEDS: the seed of a case is chosen so that the cap holds -- at most 1 % of the pixels within NEAR_TOL of an integer coordinate,
for the tiny crops (one pixel is 2 - 3 % there) at most one such pixel per image.  test_elastic_cpu.py asserts it for every case;
a case whose seed is not listed here takes seed 0."""
import itertools

import numpy as np

import augment_oracle as AO
from medt_amd.augment import inverse_affine_matrix, make_record

SHAPES = [(9, 11, 5, 6), (9, 11, 7, 8), (35, 40, 32, 32), (150, 140, 128, 128)]     # element tail, 16-byte stores, rows, blocks
GRIDS = [1, 3, 8]
SEEDS = {}


def data(seed, N, Hh, W, C):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (N, Hh, W, C)).astype(np.uint8)
    return img, (1 + rng.randint(0, 2, (N, Hh, W))).astype(np.uint8)


def lattice(rng, N, G, th, tw, scale=1.0):
    sigma = scale * max(0.5, min(th, tw) / 16.0)
    return np.clip(rng.normal(0.0, sigma, (N, 2, G + 3, G + 3)), -3 * sigma, 3 * sigma).astype(np.float32)


def affine_records(rng, N, th, tw, Hh, W):
    """The distributions of tests/test_augment_gpu.py::_affine_records, from the case's own generator."""
    recs = []
    for n in range(N):
        m = inverse_affine_matrix((tw * 0.5, th * 0.5), rng.uniform(-90, 90), (int(rng.randint(-tw // 2, tw // 2 + 1)),
                                  int(rng.randint(-th // 2, th // 2 + 1))), rng.uniform(0.7, 2.0), (rng.uniform(-45, 45), 0.0))
        recs.append(make_record(int(rng.randint(0, Hh - th + 1)), int(rng.randint(0, W - tw + 1)), bool(n & 1), m, elastic=True))
    return recs


def jitter_records():
    """One record per permutation of the four operations, the factors at the edges of (0.4, 0.4, 0.4, 0.1) and inside
    (tests/test_augment_gpu.py::_jitter_records, "all")."""
    rng = np.random.RandomState(7)
    edges = {AO.OP_BRIGHTNESS: (0.6, 1.4), AO.OP_CONTRAST: (0.6, 1.4), AO.OP_SATURATION: (0.6, 1.4), AO.OP_HUE: (-0.1, 0.1)}
    recs = []
    for k, perm in enumerate(itertools.permutations((AO.OP_BRIGHTNESS, AO.OP_CONTRAST, AO.OP_SATURATION, AO.OP_HUE))):
        ops = [(op, (edges[op][0], edges[op][1], rng.uniform(*edges[op]))[(k + op) % 3]) for op in perm]
        recs.append(make_record(0, 0, bool(k & 1), None, ops, elastic=True))
    return recs


def _store(name, seed):
    _, Hh, W, th, tw, C, G = name
    rng = np.random.RandomState(1000 + seed)
    img, mask = data(seed, 3, Hh, W, C)
    m = inverse_affine_matrix((tw * 0.5, th * 0.5), rng.uniform(-40, 40), (int(rng.randint(-1, 2)), int(rng.randint(-1, 2))),
                              rng.uniform(1.0, 1.5), (rng.uniform(-15, 15), 0.0))
    recs = [make_record(Hh - th, W - tw, True, elastic=True), make_record(1, 2, False, elastic=True),
            make_record(0, W - tw, True, m, elastic=True)]
    return dict(img=img, mask=mask, recs=np.stack(recs), field=lattice(rng, 3, G, th, tw), size=(th, tw))


def _composition(name, seed):
    what = name[1]
    rng = np.random.RandomState(2000 + seed)
    if what == "jitter":                                                   # 24 records, 16 x 16, the contrast mean from stats
        N, Hh, W, th, tw, G = 24, 16, 16, 16, 16, 3
        img, mask = data(seed, N, Hh, W, 3)
        img[0], img[1], img[2] = 77, 0, 255
        img[3, :, :8], img[3, :, 8:] = (255, 0, 0), (0, 0, 255)
        img[4, :8], img[4, 8:] = (0, 255, 0), (255, 255, 0)
        return dict(img=img, mask=mask, recs=np.stack(jitter_records()), field=lattice(rng, N, G, th, tw), size=(th, tw))
    N, Hh, W, th, tw, G = 4, 40, 45, 32, 32, 3
    img, mask = data(seed, N, Hh, W, 3)
    if what == "alone":
        recs = [make_record(int(rng.randint(0, Hh - th + 1)), int(rng.randint(0, W - tw + 1)), False, elastic=True) for _ in range(N)]
    elif what == "flip_far_corner":
        recs = [make_record(Hh - th, W - tw, True, elastic=True) for _ in range(N)]
    elif what == "affine":
        recs = affine_records(rng, N, th, tw, Hh, W)
    else:                                                                  # everything at once; one image without the affine map
        assert what == "everything"
        recs = affine_records(rng, N, th, tw, Hh, W)
        jit = [jitter_records()[k] for k in (0, 7, 13, 22)]
        for n in range(N):
            recs[n][10:18] = jit[n][10:18]
        recs[3][3], recs[3][4:10] = 1.0, (1, 0, 0, 0, 1, 0)
    return dict(img=img, mask=mask, recs=np.stack(recs), field=lattice(rng, N, G, th, tw), size=(th, tw))


def _mixed(name, seed):
    """Flags [1, 0, 1, 0]; every record with crop, two with flip, two with an affine map, all with jitter (one contrast)."""
    rng = np.random.RandomState(3000 + seed)
    N, Hh, W, th, tw, G = 4, 40, 45, 32, 32, 3
    img, mask = data(seed, N, Hh, W, 3)
    recs = affine_records(rng, N, th, tw, Hh, W)
    jit = [jitter_records()[k] for k in (0, 7, 13, 22)]
    for n in range(N):
        recs[n][10:18] = jit[n][10:18]
        recs[n][18] = 1.0 if n % 2 == 0 else 0.0
    for n in (2, 3):
        recs[n][3], recs[n][4:10] = 1.0, (1, 0, 0, 0, 1, 0)
    return dict(img=img, mask=mask, recs=np.stack(recs), field=lattice(rng, N, G, th, tw), size=(th, tw))


STORE = [("store", Hh, W, th, tw, C, G) for (Hh, W, th, tw) in SHAPES for C in (3, 1) for G in GRIDS]
COMPOSITIONS = [("composition", w) for w in ("alone", "flip_far_corner", "affine", "jitter", "everything")]
MIXED = ("mixed",)
NAMES = STORE + COMPOSITIONS + [MIXED]
_BUILD = {"store": _store, "composition": _composition, "mixed": _mixed}


def case(name):
    return _BUILD[name[0]](name, SEEDS.get(name, 0))


def case_id(name):
    return "-".join(str(v) for v in name)


def cap_holds(near, size):
    """The cap on what a comparison may leave out: 1 % of the batch's pixels; for the tiny crops, where one pixel is already
    more than 1 % (5 x 6, 7 x 8), at most one pixel per image."""
    if size[0] * size[1] >= 100:
        return bool(near.mean() <= 0.01)
    return bool((near.reshape(len(near), -1).sum(1) <= 1).all())
