"""No GPU: the numpy / SciPy oracle of the splitting tests (tests/split_oracle.py) against hand-written cases and the consequences
of the definition, the integer marker predicate against its float64 statement, and the product's splitting (medt_amd.ops.split_markers
/ grow_labels / split_objects, csrc/split.hip) on the CPU lane emulator against the oracle -- under three work-item orders and on
guard-paged memory -- and the refusals of the ops, the C ABI and test.py's new flags."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401
import split_cases as SC
import split_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "medical-transformer_amd")


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


# ---- the oracle against hand-written cases ----------------------------------------------------------------------------------------
def test_oracle_bars_tie_to_the_smaller_label():
    for w, want in ((9, [1, 1, 1, 1, 1, 2, 2, 2, 2]), (10, [1, 1, 1, 1, 1, 2, 2, 2, 2, 2])):
        mask = np.ones((1, w), np.uint8)
        seeds = np.zeros((1, w), np.int32)
        seeds[0, 0], seeds[0, -1] = 1, 2
        for c in (4, 8):
            lab, dist = SO.grow(seeds, mask, c)
            assert lab[0].tolist() == want and dist[0].tolist() == [min(x, w - 1 - x) for x in range(w)], (w, c)
    # the odd bar with the labels the other way round: the middle pixel, equally far from both, takes the smaller label
    seeds = np.zeros((1, 9), np.int32)
    seeds[0, 0], seeds[0, -1] = 2, 1
    assert SO.grow(seeds, np.ones((1, 9), np.uint8), 8)[0][0].tolist() == [2, 2, 2, 2, 1, 1, 1, 1, 1]


def test_oracle_small_maps_at_both_connectivities():
    # 3 x 3, two squares that touch at a corner only: one component at 8, two at 4
    m = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]], np.uint8)
    s = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 0]], np.int32)
    assert SO.grow(s, m, 8)[0].tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 1]] and SO.grow(s, m, 8)[1][2, 2] == 2
    assert SO.grow(s, m, 4)[0].tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 0]] and SO.grow(s, m, 4)[1][2, 2] == -1
    # 5 x 7: a wall with one gap; the seeds sit left (2) and right (1) of it
    m = np.ones((5, 7), np.uint8)
    m[:, 3] = 0
    m[4, 3] = 1
    s = np.zeros((5, 7), np.int32)
    s[0, 0], s[0, 6] = 2, 1
    lab4, d4 = SO.grow(s, m, 4)
    assert lab4[:, :3].min() == 2 and lab4[:, :3].max() == 2 and lab4[:, 4:].min() == 1 and lab4[:, 4:].max() == 1
    assert lab4[4, 3] == 1 and d4[4, 3] == 7 and d4[4, 0] == 4           # the gap is 7 steps from either seed: label 1 wins
    lab8, d8 = SO.grow(s, m, 8)
    assert d8[4, 3] == 4 and lab8[4, 3] == 1 and d8[4, 6] == 4 and d8[2, 2] == 2
    # splitting them: every pixel of the 3 x 3 squares has depth 1 or 2; all are within one pixel of the top
    lab, k = SO.split(np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]], np.uint8), 1, 1, 4)
    assert k == 2 and lab.tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 2]]
    lab, k = SO.split(np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]], np.uint8), 1, 1, 8)
    assert k == 1 and lab.tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 1]]


@pytest.mark.parametrize("case", SC.DISC_PAIRS, ids=[c[0] for c in SC.DISC_PAIRS])
def test_oracle_marker_counts_of_the_disc_pairs(case):
    from scipy import ndimage
    _, m, want = case
    assert ndimage.label(SO.markers(m, 7, 1, 8), np.ones((3, 3)))[1] == want
    lab, k = SO.split(m, 7, 1, 8)
    assert k == want
    SO.check_invariants(lab, k, m, 8)


def test_oracle_depth_and_full_image():
    from scipy import ndimage
    m = SC.random_discs(40, 70, 8, 3)
    assert np.array_equal(SO.depth2(m), np.rint(ndimage.distance_transform_edt(m) ** 2).astype(np.int64))
    assert (SO.depth2(np.ones((3, 4), np.uint8)) == SO.EDT_NONE).all()
    assert (SO.markers(np.ones((3, 4), np.uint8)) == 255).all()


def test_integer_predicate_equals_its_float64_statement():
    """e <= 0 or e^2 <= 4 t^2 d with e = M - d - t^2  against  sqrt(M) - sqrt(d) <= t  on every depth2 <= M <= 4096, t in 0..2.
    The float64 statement is only decisive away from equality; where the two roots differ from t by less than 1e-9 the pair is
    an exact case (M = (sqrt(d) + t)^2 with an integer root), which the integers get right by construction."""
    M, d = np.meshgrid(np.arange(4097, dtype=np.int64), np.arange(4097, dtype=np.int64), indexing="ij")
    keep = d <= M
    for t in (0, 1, 2):
        got = SO.near_top(M, d, np.int64(t))
        gap = np.sqrt(M.astype(np.float64)) - np.sqrt(d.astype(np.float64)) - t
        sure = keep & (np.abs(gap) > 1e-9)
        assert np.array_equal(got[sure], (gap <= 0)[sure]), t
        edge = keep & ~sure                                    # exact equality: sqrt(M) = sqrt(d) + t, a marker
        r = np.rint(np.sqrt(d[edge].astype(np.float64))).astype(np.int64)
        assert got[edge].all() and (edge.sum() > 0) and (t == 0 or np.array_equal(r * r, d[edge]))


@pytest.mark.parametrize("case", SC.cases(), ids=[c[0] for c in SC.cases()])
def test_oracle_invariants_on_the_shared_cases(case):
    _, m, r, t, c = case
    for img in (m if m.ndim == 3 else m[None]):
        lab, k = SO.split(img, r, t, c)
        SO.check_invariants(lab, k, img, c)
        comp, kc = __import__("scipy.ndimage").ndimage.label(img, SO.structure(c))
        seeds = __import__("scipy.ndimage").ndimage.label(SO.markers(img, r, t, c), SO.structure(c))[0]
        for l in range(1, kc + 1):                             # a component with a single marker comes back whole
            inside = np.unique(seeds[(comp == l) & (seeds > 0)])
            if len(inside) == 1:
                assert (lab[comp == l] == inside[0]).all()


# ---- the kernels on the lane emulator ---------------------------------------------------------------------------------------------
def want_of(m, r, t, c):
    imgs = m if m.ndim == 3 else m[None]
    mk = np.stack([SO.markers(i, r, t, c) for i in imgs]).reshape(m.shape)
    sp = [SO.split(i, r, t, c) for i in imgs]
    return mk, np.stack([s[0] for s in sp]).reshape(m.shape), [s[1] for s in sp]


@pytest.mark.parametrize("case", SC.cases(), ids=[c[0] for c in SC.cases()])
def test_emulated_kernels_equal_the_oracle(emulated, case):
    from medt_amd import ops
    _, m, r, t, c = case
    mk, lab, k = want_of(m, r, t, c)
    x = dev(m * np.uint8(255))
    got_mk = ops.split_markers(x, r, t, c)
    assert got_mk.dtype == torch.uint8 and np.array_equal(got_mk.numpy(), mk)
    got, cnt = ops.split_objects(x, r, t, c)
    assert got.dtype == torch.int32 and cnt.dtype == torch.int32 and cnt.tolist() == k and np.array_equal(got.numpy(), lab)


def test_emulated_growth_through_the_corridor(emulated):
    from medt_amd import ops
    m, a, b = SC.serpentine()
    for c in (4, 8):
        seeds = SC.single_seed(m, a, 5)
        want, wd = SO.grow(seeds, m, c)
        got, passes, dist = ops.grow_labels(dev(seeds), dev(m), c, return_passes=True, return_distance=True)
        assert np.array_equal(got.numpy(), want) and np.array_equal(dist.numpy(), wd) and passes > 1
        assert int(dist[b]) == int(wd[b]) > 2000
        seeds[b] = 3                                            # a second seed at the far end: the tie falls on a tile edge or not
        want, wd = SO.grow(seeds, m, c)
        got, dist = ops.grow_labels(dev(seeds), dev(m), c, return_distance=True)
        assert np.array_equal(got.numpy(), want) and np.array_equal(dist.numpy(), wd)
    bar = np.ones((1, 128), np.uint8)                           # the tie of an even bar exactly across the tile edge at x = 64
    seeds = np.zeros((1, 128), np.int32)
    seeds[0, 0], seeds[0, 127] = 2, 1
    got = ops.grow_labels(dev(seeds), dev(bar), 4).numpy()
    assert np.array_equal(got, SO.grow(seeds, bar, 4)[0]) and got[0, 63] == 2 and got[0, 64] == 1
    # a component without a seed stays 0; out: a view that is not 16-byte aligned
    two = np.zeros((5, 9), np.uint8)
    two[1, 1:4], two[3, 5:8] = 1, 1
    seeds = np.zeros((5, 9), np.int32)
    seeds[1, 2] = 7
    store = torch.zeros(5 * 9 + 1, dtype=torch.int32)
    out = dev(store.numpy())[1:].reshape(5, 9)
    got = ops.grow_labels(dev(seeds), dev(two), 8, out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.numpy(), np.where(np.arange(5)[:, None] == 1, two * 7, 0))


def test_emulated_kernels_are_independent_of_work_item_order(emu):
    """ascending, descending and shuffled work-item orders of the emulator: identical bytes, those of the oracle."""
    from emu_device import emulated_device
    from medt_amd import ops
    for m, r, t, c in ((SC.random_discs(40, 136, 16, 9), 7, 1, 8), (SC.serpentine()[0], 3, 0, 4)):
        mk, lab, k = want_of(m, r, t, c)
        runs = []
        for mode, seed in ((0, 0), (1, 0), (2, 1), (2, 2)):
            emu.emu_set_order(mode, seed)
            try:
                with emulated_device(emu):
                    g_mk = ops.split_markers(dev(m), r, t, c)
                    g_lab, g_cnt = ops.split_objects(dev(m), r, t, c)
            finally:
                emu.emu_set_order(0, 0)
            runs.append((g_mk.numpy().tobytes(), g_lab.numpy().tobytes(), g_cnt.numpy().tobytes()))
        assert all(run == runs[0] for run in runs)
        assert runs[0][0] == mk.tobytes() and runs[0][1] == lab.tobytes() and np.frombuffer(runs[0][2], np.int32).tolist() == k


@pytest.mark.parametrize("placement", ["tail", "head"])
def test_on_guarded_memory(placement):
    """The marker and growth kernels with every buffer flush against a guard page: -11 would mean a read or write outside a
    buffer -- the halo reads of both kernels are what could."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "split_guard_driver.py"), placement], capture_output=True,
                         text=True, timeout=900, cwd=ROOT)
    lines = run.stdout.strip().splitlines()
    last = next((ln for ln in reversed(lines) if ln.startswith("CALL ")), "(no library call announced)")
    assert run.returncode == 0, "return code %d%s\nlast announced: %s\n%s" % (
        run.returncode, " (SIGSEGV: the kernel left a buffer it was given)" if run.returncode == -11 else "", last, run.stderr[-3000:])
    s = json.loads(lines[-1])
    print(json.dumps(s))
    e = s["entries"]
    assert s["cases"] >= 8 and e.get("medt_split_markers", 0) >= 2 * s["cases"] and e.get("medt_grow_passes", 0) >= s["cases"]
    assert e.get("medt_split_cmax") == e.get("medt_split_markers") and e.get("medt_grow_init") == e.get("medt_grow_labels")
    assert s["unguarded"] == 0 and s["allowed"] == 0 and s["in_arena"] + s["stood_in"] == s["pointers"]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_ops_refusals(emulated):
    from medt_amd import MedtError, ops
    m = dev(np.ones((4, 6), np.uint8))
    s = dev(np.zeros((4, 6), np.int32))
    for bad in (dict(distance=0), dict(distance=33), dict(distance=2.0), dict(distance=True), dict(tolerance=-1), dict(tolerance=9),
                dict(tolerance=1.0), dict(connectivity=6)):
        for fn in (ops.split_markers, ops.split_objects):
            with pytest.raises(MedtError):
                fn(m, **bad)
    for fn in (ops.split_markers, ops.split_objects):
        with pytest.raises(MedtError):
            fn(dev(np.ones((4, 6), np.int32)))                  # dtype
        with pytest.raises(MedtError):
            fn(dev(np.ones((6,), np.uint8)))                    # shape
        with pytest.raises(MedtError):
            fn(dev(np.ones((0, 6), np.uint8)))                  # empty
    with pytest.raises(MedtError):
        ops.split_objects(m, out=dev(np.zeros((4, 6), np.int64)))
    with pytest.raises(MedtError):
        ops.split_objects(m, out=dev(np.zeros((4, 7), np.int32)))
    with pytest.raises(MedtError):
        ops.grow_labels(dev(np.zeros((4, 6), np.int64)), m)
    with pytest.raises(MedtError):
        ops.grow_labels(dev(np.zeros((4, 5), np.int32)), m)
    with pytest.raises(MedtError):
        ops.grow_labels(s, m, connectivity=5)
    with pytest.raises(MedtError):
        ops.grow_labels(s, dev(np.ones((0, 6), np.uint8)))
    outside = np.zeros((4, 6), np.int32)
    outside[0, 0] = 1
    hole = np.ones((4, 6), np.uint8)
    hole[0, 0] = 0
    with pytest.raises(MedtError, match="outside the mask"):
        ops.grow_labels(dev(outside), dev(hole))
    with pytest.raises(MedtError, match="negative"):
        ops.grow_labels(dev(-outside), m)


def test_ops_refuse_host_tensors():
    from medt_amd import MedtError, ops
    with pytest.raises(MedtError):
        ops.split_objects(torch.ones(4, 6, dtype=torch.uint8))
    with pytest.raises(MedtError):
        ops.grow_labels(torch.zeros(4, 6, dtype=torch.int32), torch.ones(4, 6, dtype=torch.uint8))


def test_abi_refusals():
    from medt_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.lib()
    one = C.create_string_buffer(64)                            # a non-null, 16-byte aligned stand-in: refused before any use
    p = (C.addressof(one) + 15) // 16 * 16
    assert lib.medt_grow_workspace_bytes(1, 16, 64) == 16 * 64 * 8 + 16              # two flags, rounded up to 16 bytes
    assert lib.medt_grow_workspace_bytes(2, 17, 65) == (2 * 17 * 65 * 8 + 255) // 256 * 256 + 2 * 2 * 4 * 4     # keys padded to 256 bytes, 4 tiles
    assert lib.medt_grow_workspace_bytes(1, 4097, 4) == 0 and lib.medt_grow_workspace_bytes(0, 4, 4) == 0
    big = 1 << 40
    assert lib.medt_split_cmax(None, p, p, 1, 4, 4, 2, 1, None) == -1 and b"null" in lib.medt_last_error()
    assert lib.medt_split_cmax(p, p, p, 1, 4, 4, 2, 2, None) == -1 and b"stride" in lib.medt_last_error()
    assert lib.medt_split_cmax(p, p, p, 1, 4, 4097, 2, 1, None) == -2
    assert lib.medt_split_markers(p, p, p, None, 1, 4, 4, 2, 7, 1, None) == -1 and b"null" in lib.medt_last_error()
    for r, t, word in ((0, 1, b"distance"), (33, 1, b"distance"), (7, -1, b"tolerance"), (7, 9, b"tolerance")):
        assert lib.medt_split_markers(p, p, p, p, 1, 4, 4, 2, r, t, None) == -1 and word in lib.medt_last_error()
    assert lib.medt_split_markers(p, p, p, p, 1, 4, 4, 0, 7, 1, None) == -1 and b"stride" in lib.medt_last_error()
    assert lib.medt_split_markers(p, p, p, p, 1, 5000, 4, 2, 7, 1, None) == -2
    assert lib.medt_grow_init(p, p, None, big, 1, 4, 4, None) == -1 and lib.medt_grow_init(None, p, p, big, 1, 4, 4, None) == -1
    assert lib.medt_grow_init(p, p, p + 8, big, 1, 4, 4, None) == -1 and b"aligned" in lib.medt_last_error()
    assert lib.medt_grow_init(p, p, p, 4 * 4 * 8, 1, 4, 4, None) == -4 and b"workspace" in lib.medt_last_error()
    assert lib.medt_grow_init(p, p, p, big, 1, 4, 4097, None) == -2
    assert lib.medt_grow_passes(p, big, None, 1, 0, 1, 4, 4, 8, None) == -1
    assert lib.medt_grow_passes(p, big, p, 1, 0, 1, 4, 4, 6, None) == -1 and b"connectivity" in lib.medt_last_error()
    for n, first in ((0, 0), (65, 0), (1, -1)):
        assert lib.medt_grow_passes(p, big, p, n, first, 1, 4, 4, 8, None) == -1 and b"passes" in lib.medt_last_error()
    assert lib.medt_grow_passes(p, 8, p, 1, 0, 1, 4, 4, 8, None) == -4
    assert lib.medt_grow_labels(p, big, None, None, 1, 4, 4, None) == -1 and lib.medt_grow_labels(p, big, p, p, 1, 4, 4, None) == -1
    assert lib.medt_grow_labels(None, big, p, None, 1, 4, 4, None) == -1 and lib.medt_grow_labels(p, 8, p, None, 1, 4, 4, None) == -4
    assert lib.medt_abi_version() == _lib.ABI_VERSION == 11


def test_limits_mirror_the_header():
    import re
    from medt_amd import ops
    src = open(os.path.join(ROOT, "include", "medt_abi.h")).read()

    def macro(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))
    assert (ops.SPLIT_MAX_DISTANCE, ops.SPLIT_MAX_TOLERANCE, ops.GROW_MAX_PASSES) == (
        macro("MEDT_SPLIT_MAX_DISTANCE"), macro("MEDT_SPLIT_MAX_TOLERANCE"), macro("MEDT_GROW_MAX_PASSES"))
    assert max(ops.GROW_BATCHES) <= ops.GROW_MAX_PASSES


# ---- metrics and test.py ------------------------------------------------------------------------------------------------------------
def test_scores_take_a_labelled_side(emulated):
    """labelled=(True, False): the prediction is a label map taken as given, the target a mask labelled here -- equal to the
    scores of the two label maps, and different from the scores of the merged prediction."""
    import metrics
    pred = SC.disc_pair(16)
    tgt_lab = np.where(SC.discs(40, 64, (20, 16, 10)) > 0, 1, 0) + np.where((SC.discs(40, 64, (20, 32, 10)) > 0) & (SC.discs(40, 64, (20, 16, 10)) == 0), 2, 0)
    lab, k = SO.split(pred, 7, 1, 8)
    assert k == 2
    both = metrics.object_scores(dev(lab), dev(tgt_lab.astype(np.int32)), 8, labelled=True)
    mixed = metrics.object_scores(dev(lab), dev((tgt_lab > 0).astype(np.uint8)), 8, labelled=(True, False))
    other = metrics.object_scores(dev(pred), dev(tgt_lab.astype(np.int32)), 8, labelled=(False, True))
    plain = metrics.object_scores(dev(pred), dev((tgt_lab > 0).astype(np.uint8)), 8)
    assert both["n_pred"].tolist() == [2] and both["n_gt"].tolist() == [2]
    assert mixed["n_pred"].tolist() == [2] and mixed["n_gt"].tolist() == [1]
    assert other["n_pred"].tolist() == [1] and other["n_gt"].tolist() == [2]
    assert plain["n_pred"].tolist() == [1] and plain["n_gt"].tolist() == [1] and float(plain["aji"][0]) == 1.0
    assert float(both["pq"][0]) > float(other["pq"][0]) and float(both["aji"][0]) > float(other["aji"][0])
    h = metrics.object_hausdorff(dev(lab), dev((tgt_lab > 0).astype(np.uint8)), 8, labelled=(True, False))
    assert h["n_pred"].tolist() == [2] and h["n_gt"].tolist() == [1] and bool(h["valid"][0])
    for bad in ((True,), (True, False, True), "yes"):
        with pytest.raises(ValueError):
            metrics.object_scores(dev(lab), dev(lab), 8, labelled=bad)


def _test_py(*argv, cwd):
    env = dict(os.environ, PYTHONPATH=PKG)
    return subprocess.run([sys.executable, os.path.join(PKG, "test.py"), *argv], env=env, capture_output=True, text=True,
                          timeout=300, cwd=cwd)


def test_cli_refusals(tmp_path):
    """Before any work: no dataset exists, no GPU is touched."""
    none = str(tmp_path / "none")
    for extra, word in ((["--split_distance", "3"], "add --split on"), (["--split_tolerance", "0"], "add --split on"),
                        (["--split", "on", "--split_distance", "0"], "--split_distance"),
                        (["--split", "on", "--split_distance", "33"], "--split_distance"),
                        (["--split", "on", "--split_tolerance", "9"], "--split_tolerance"),
                        (["--split", "on", "--split_tolerance=-1"], "--split_tolerance"),
                        (["--instance_labels", none, "--crop", "32"], "--crop"),
                        (["--instance_labels", none], "not a directory"),
                        (["--write_instances", "on"], "add --split on")):
        r = _test_py("--val_dataset", none, *extra, cwd=str(tmp_path))
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr[-1000:])
    assert not (tmp_path / "none").exists()


def test_instance_files_are_renumbered_in_raster_order(tmp_path):
    sys.path.insert(0, PKG)
    from medt_amd import instances as I
    from PIL import Image
    ids = np.array([[0, 700, 700, 0], [9, 0, 700, 3], [9, 9, 0, 3]], np.uint16)
    Image.fromarray(ids).save(str(tmp_path / "a.png"))
    np.save(str(tmp_path / "b.npy"), ids.astype(np.int64))
    want = [[0, 1, 1, 0], [2, 0, 1, 3], [2, 2, 0, 3]]
    for stem in ("a", "b"):
        lab, k = I.read_instances(str(tmp_path), stem + ".png", (3, 4))
        assert lab.dtype == np.int32 and k == 3 and lab.tolist() == want
    with pytest.raises(SystemExit):
        I.read_instances(str(tmp_path), "a.png", (3, 5))         # not the image's size
    with pytest.raises(SystemExit):
        I.read_instances(str(tmp_path), "missing.png", (3, 4))
    I.write_instances(str(tmp_path / "c_inst.png"), np.asarray(want, np.int32))
    with Image.open(str(tmp_path / "c_inst.png")) as im:
        assert np.array_equal(np.array(im), np.asarray(want)) and im.mode in ("I;16", "I")
    with pytest.raises(SystemExit):
        I.write_instances(str(tmp_path / "d_inst.png"), np.full((2, 2), 65536, np.int32))
