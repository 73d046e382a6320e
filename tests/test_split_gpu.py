"""Splitting touching objects on the device (medt_split_*, medt_grow_*, medt_amd.ops.split_markers / grow_labels / split_objects,
metrics.object_scores with a labelled side) against the numpy / SciPy oracle (tests/split_oracle.py): marker masks, label maps,
counts, step counts bit for bit.  No tolerance anywhere: everything compared is an integer, or derived on the host from equal
integers.  Written against the `device` fixture: `--emulate` runs everything on the CPU lane emulator."""
import functools

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401
import split_cases as SC
import split_oracle as SO

pytestmark = pytest.mark.gpu

CASES = SC.cases()


def _as_device(t, device):
    """On the emulated device (pytest --emulate) CPU tensors stand in for device tensors."""
    if device.type == "cpu":
        from emu_device import DeviceTensor
        return t.as_subclass(DeviceTensor)
    return t.to(device)


def _dev(a, device):
    return _as_device(torch.from_numpy(np.array(a)), device)


@functools.lru_cache(maxsize=None)
def reference(k):
    """What the oracle says about case k (computed once, shared, never written to): markers, labels, counts."""
    _, m, r, t, c = CASES[k]
    imgs = m if m.ndim == 3 else m[None]
    mk = np.stack([SO.markers(i, r, t, c) for i in imgs]).reshape(m.shape)
    sp = [SO.split(i, r, t, c) for i in imgs]
    return mk, np.stack([s[0] for s in sp]).reshape(m.shape), [s[1] for s in sp]


@functools.lru_cache(maxsize=None)
def corridor():
    """The 40 x 136 corridor, one pixel wide, through all 3 x 3 tiles, with the oracle's growth from one end and from both."""
    from medt_amd import ops
    assert ops.LABEL_TILE == (16, 64)
    m, a, b = SC.serpentine()
    out = {"mask": m, "a": a, "b": b}
    for c in (4, 8):
        one = SC.single_seed(m, a, 5)
        two = one.copy()
        two[b] = 3
        out[c] = (one, SO.grow(one, m, c), two, SO.grow(two, m, c))
    return out


def test_the_shared_shapes_cover_the_tile():
    from medt_amd import ops
    assert ops.LABEL_TILE == (16, 64)
    shapes = {tuple(m.shape[-2:]) for _, m, *_ in CASES}
    assert {(1, 1), (1, 70), (70, 1), (17, 65), (16, 64), (40, 136), (20, 20), (128, 128)} <= shapes
    assert any(m.ndim == 3 and m.shape[0] == 2 and not np.array_equal(m[0], m[1]) for _, m, *_ in CASES)
    assert any(r == 32 and max(m.shape) <= 32 for _, m, r, _, _ in CASES)
    assert {c for *_, c in CASES} == {4, 8}


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_markers_and_objects_equal_the_oracle(device, k):
    from medt_amd import ops
    _, m, r, t, c = CASES[k]
    mk, lab, cnt = reference(k)
    x = _dev(m * np.uint8(255), device)
    got_mk = ops.split_markers(x, r, t, c)
    assert got_mk.dtype == torch.uint8 and got_mk.shape == x.shape
    assert torch.equal(got_mk.cpu(), torch.from_numpy(mk))
    got, got_cnt = ops.split_objects(x, r, t, c)
    assert got.dtype == torch.int32 and got_cnt.dtype == torch.int32
    assert got_cnt.cpu().tolist() == cnt and torch.equal(got.cpu(), torch.from_numpy(lab))
    again, again_cnt = ops.split_objects(x, r, t, c)            # two runs: equal bytes
    assert torch.equal(again, got) and torch.equal(again_cnt, got_cnt) and torch.equal(ops.split_markers(x, r, t, c), got_mk)
    # growth alone from the oracle's markers, labelled on the host
    from scipy import ndimage
    if m.ndim == 2:
        seeds = ndimage.label(mk, SO.structure(c))[0].astype(np.int32)
        grown = ops.grow_labels(_dev(seeds, device), x, c)
        assert torch.equal(grown.cpu(), torch.from_numpy(lab))


def test_connectivity_changes_the_result(device):
    """Squares that touch at their corners only: four objects at connectivity 4, one component at 8 (whose markers still make
    four); and a seed that reaches across a corner at 8 only."""
    from medt_amd import ops
    m = np.kron(np.eye(4, dtype=np.uint8), np.ones((6, 6), np.uint8))
    seeds = SC.single_seed(m, (0, 0), 1)
    g4 = ops.grow_labels(_dev(seeds, device), _dev(m, device), 4).cpu().numpy()
    g8 = ops.grow_labels(_dev(seeds, device), _dev(m, device), 8).cpu().numpy()
    assert np.array_equal(g4, SO.grow(seeds, m, 4)[0]) and np.array_equal(g8, SO.grow(seeds, m, 8)[0])
    assert g4.sum() == 36 and g8.sum() == 4 * 36


@pytest.mark.parametrize("c", [4, 8])
def test_growth_through_the_corridor(device, c):
    """One seed at one end: the labels need more than one pass (the corridor crosses every tile edge) and the far end carries
    the geodesic distance.  A seed at either end: the tie falls where the oracle puts it."""
    from medt_amd import ops
    ref = corridor()
    one, (want, wd), two, (want2, wd2) = ref[c]
    x = _dev(ref["mask"], device)
    got, passes, dist = ops.grow_labels(_dev(one, device), x, c, return_passes=True, return_distance=True)
    assert passes > 1
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and torch.equal(dist.cpu(), torch.from_numpy(wd))
    assert int(dist[ref["b"]]) == int(wd[ref["b"]]) and int(wd[ref["b"]]) >= 2 * 136
    got2, dist2 = ops.grow_labels(_dev(two, device), x, c, return_distance=True)
    assert torch.equal(got2.cpu(), torch.from_numpy(want2)) and torch.equal(dist2.cpu(), torch.from_numpy(wd2))
    assert sorted(np.unique(want2).tolist()) == [0, 3, 5]
    again = ops.grow_labels(_dev(two, device), x, c)
    assert torch.equal(again, got2)


def test_tie_across_a_tile_edge(device):
    from medt_amd import ops
    bar = np.ones((1, 128), np.uint8)
    seeds = np.zeros((1, 128), np.int32)
    seeds[0, 0], seeds[0, 127] = 2, 1
    got = ops.grow_labels(_dev(seeds, device), _dev(bar, device), 4).cpu().numpy()
    assert np.array_equal(got, SO.grow(seeds, bar, 4)[0]) and got[0, 63] == 2 and got[0, 64] == 1
    odd = np.ones((1, 129), np.uint8)                           # the middle pixel, x = 64, is 64 steps from both: the smaller label
    seeds = np.zeros((1, 129), np.int32)
    seeds[0, 0], seeds[0, 128] = 2, 1
    got = ops.grow_labels(_dev(seeds, device), _dev(odd, device), 8).cpu().numpy()
    assert np.array_equal(got, SO.grow(seeds, odd, 8)[0]) and got[0, 63] == 2 and got[0, 64] == 1


def test_unseeded_component_and_misaligned_out(device):
    from medt_amd import ops
    m = SC.discs(17, 65, (5, 8, 4), (10, 50, 5))
    seeds = SC.single_seed(m, (5, 8), 9)
    want = SO.grow(seeds, m, 8)[0]
    assert want[10, 50] == 0 and want[5, 8] == 9
    store = _as_device(torch.full((17 * 65 + 1,), -7, dtype=torch.int32), device)
    out = store[1:].reshape(17, 65)                             # 4 bytes past a 16-byte boundary
    assert out.data_ptr() % 16 == 4
    got = ops.grow_labels(_dev(seeds, device), _dev(m, device), 8, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out.cpu(), torch.from_numpy(want)) and int(store[0]) == -7
    lab, k = SO.split(m, 7, 1, 8)
    store.fill_(-7)
    got, cnt = ops.split_objects(_dev(m, device), out=out)
    assert got.data_ptr() == out.data_ptr() and cnt.cpu().tolist() == [k] and torch.equal(out.cpu(), torch.from_numpy(lab))
    assert int(store[0]) == -7


def test_images_of_a_batch_do_not_interact(device):
    from medt_amd import ops
    a, b = SC.random_discs(40, 70, 8, 3), SC.disc_pair(16, h=40, w=70)
    both, cnt = ops.split_objects(_dev(np.stack([a, b]), device))
    swapped, cnt_s = ops.split_objects(_dev(np.stack([b, a]), device))
    assert torch.equal(both[0], swapped[1]) and torch.equal(both[1], swapped[0]) and cnt.cpu().tolist() == cnt_s.cpu().tolist()[::-1]
    alone, cnt_a = ops.split_objects(_dev(b, device))
    assert torch.equal(alone, both[1]) and cnt_a.cpu().tolist() == [2]


def test_object_scores_of_a_labelled_prediction(device):
    """object_scores(labelled=(True, False)) on the device's split labels equals the scores computed on the host from the
    oracle's labels."""
    import label_oracle as LO
    import metrics
    pred = np.stack([SC.disc_pair(16, h=40, w=70), SC.random_discs(40, 70, 8, 3)])
    target = np.stack([SC.discs(40, 70, (20, 16, 10)), SC.random_discs(40, 70, 6, 11)])
    labels, cnt = __import__("medt_amd.ops", fromlist=["ops"]).split_objects(_dev(pred, device))
    got = metrics.object_scores(labels, _dev(target, device), 8, labelled=(True, False))
    for n in range(2):
        lab, k = SO.split(pred[n], 7, 1, 8)
        tl, tk = LO.label(target[n], 8)
        ap = [int((lab == j).sum()) for j in range(1, k + 1)]
        ag = [int((tl == i).sum()) for i in range(1, tk + 1)]
        rows = sorted((j, i, int(((lab == j) & (tl == i)).sum())) for j in range(1, k + 1) for i in range(1, tk + 1)
                      if ((lab == j) & (tl == i)).any())
        want = metrics._object_scores_image(ap, ag, rows)
        assert (int(got["n_pred"][n]), int(got["n_gt"][n])) == (k, tk)
        for key, w in zip(("f1", "dice", "aji", "pq", "dq", "sq"), want):
            assert float(got[key][n]) == w, (n, key)
    assert int(got["n_pred"][0]) == 2 and int(got["n_gt"][0]) == 1
