"""TEST INFRASTRUCTURE: the masks the splitting tests share (tests/test_split_cpu.py on the lane emulator, tests/test_split_gpu.py
on the device), built from integers and seeded generators only.  The tile of the kernels is 16 x 64."""
import numpy as np


def discs(h, w, *items):
    """uint8 {0,1} map of the union of the discs (cy, cx, radius): (y - cy)^2 + (x - cx)^2 <= radius^2."""
    yy, xx = np.indices((h, w))
    m = np.zeros((h, w), bool)
    for cy, cx, r in items:
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m.astype(np.uint8)


def disc_pair(gap, r1=10, r2=10, h=40, w=64):
    """Two discs on one row whose centres are `gap` apart."""
    return discs(h, w, (h // 2, 16, r1), (h // 2, 16 + gap, r2))


# (mask, marker count at distance 7, tolerance 1, connectivity 8): the counts of the numpy prototype of the definition
DISC_PAIRS = [("r10_r10_gap16", disc_pair(16), 2), ("r10_r7_gap13", disc_pair(13, 10, 7), 2), ("r10_r10_gap10", disc_pair(10), 2),
              ("r12_r6_gap18", disc_pair(18, 12, 6), 2), ("r10_r10_gap6", disc_pair(6), 1), ("single", discs(40, 64, (20, 30, 10)), 1),
              ("rectangle_20x55", np.pad(np.ones((20, 55), np.uint8), 5), 1),
              ("triangle", discs(60, 64, (18, 20, 10), (18, 36, 10), (32, 28, 10)), 4)]


def serpentine(h=40, w=136):
    """A corridor one pixel wide: the even rows in full, joined at alternating ends by one pixel of the odd row between them.
    40 x 136 winds through all 3 x 3 tiles.  -> (mask, first end (y, x), far end (y, x))."""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    rows = (h + 1) // 2
    last = 2 * (rows - 1)
    return m, (0, 0), (last, w - 1 if rows % 2 == 1 else 0)


def random_discs(h, w, count, seed, rmin=4, rmax=11):
    g = np.random.default_rng(seed)
    return discs(h, w, *[(int(g.integers(0, h)), int(g.integers(0, w)), int(g.integers(rmin, rmax + 1))) for _ in range(count)])


def single_seed(mask, at, label=1):
    s = np.zeros(mask.shape, np.int32)
    s[at] = label
    return s


def cases():
    """(name, mask (H,W) or (N,H,W) uint8, distance, tolerance, connectivity)."""
    corridor = serpentine()[0]
    out = [("one", np.ones((1, 1), np.uint8), 7, 1, 8), ("none", np.zeros((1, 1), np.uint8), 7, 1, 8),
           ("row_1x70", np.pad(np.ones((1, 60), np.uint8), ((0, 0), (3, 7))), 7, 1, 8),
           ("col_70x1", np.pad(np.ones((60, 1), np.uint8), ((7, 3), (0, 0))), 7, 1, 4),
           ("past_tile_17x65", random_discs(17, 65, 6, 1, 3, 6), 7, 1, 8),
           ("tile_16x64", random_discs(16, 64, 6, 2, 3, 6), 7, 1, 8),
           ("corridor_40x136", corridor, 7, 1, 8), ("corridor_40x136_c4", corridor, 3, 0, 4),
           ("window_over_frame_20x20", discs(20, 20, (6, 6, 5), (13, 13, 5)), 32, 1, 8),
           ("full_33x70", np.ones((33, 70), np.uint8), 7, 1, 8), ("empty_33x70", np.zeros((33, 70), np.uint8), 7, 1, 8),
           ("pixel_20x70", single_seed(np.zeros((20, 70)), (17, 65)).astype(np.uint8), 7, 1, 8),
           ("pair_c4", disc_pair(16), 7, 1, 4), ("pair_c8", disc_pair(16), 7, 1, 8),
           ("diagonal_contact", np.kron(np.eye(4, dtype=np.uint8), np.ones((6, 6), np.uint8)), 2, 1, 4),
           ("diagonal_contact_c8", np.kron(np.eye(4, dtype=np.uint8), np.ones((6, 6), np.uint8)), 2, 1, 8),
           ("tolerance_0", discs(40, 70, (20, 22, 12), (20, 44, 12)), 7, 0, 8),
           ("tolerance_2_r3", random_discs(50, 90, 14, 5), 3, 2, 8),
           ("batch_2", np.stack([random_discs(40, 70, 8, 3), disc_pair(16, h=40, w=70)]), 7, 1, 8),
           ("discs_128", random_discs(128, 128, 40, 4), 7, 1, 8)]
    out += [("pair_" + name, m, 7, 1, 8) for name, m, _ in DISC_PAIRS]
    return out
