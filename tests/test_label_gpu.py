"""Connected-component labelling on the device (medt_label_*, medt_amd.ops.label / label_tables / remove_small_objects /
fill_holes / label_overlaps, metrics.object_scores) against the flood-fill numpy oracle (tests/label_oracle.py): label maps,
counts, tables, cleaned masks and overlap tables bit for bit, the float64 scores to the summation order.  Written against the
`device` fixture: `--emulate` runs everything on the CPU lane emulator."""
import functools
import math

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401
import label_oracle as LO
import surface_oracle as SO

pytestmark = pytest.mark.gpu

TH, TW = 16, 64                     # asserted against ops.LABEL_TILE below: the shapes are derived from it


def _shapes():
    fixed = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 65), (70, 45), (64, 64), (17, 130)]
    hs, ws = (TH - 1, TH, TH + 1, 2 * TH + 1), (TW - 1, TW, TW + 1, 2 * TW + 1)
    tiled = [(h, w) for h in hs for w in ws if h % TH or w % TW] + [(2 * TH, 2 * TW)]
    return fixed + [s for s in tiled if s not in fixed]


SHAPES = _shapes()
IDS = ["%dx%d" % s for s in SHAPES]


def test_shapes_follow_the_tile():
    from medt_amd import ops
    assert ops.LABEL_TILE == (TH, TW)
    assert len(SHAPES) == len(set(SHAPES)) == 8 + 15 + 1 - 1                         # ((2 TH + 1, TW + 1) is one of the listed shapes)


def _as_device(t, device):
    """On the emulated device (pytest --emulate) CPU tensors stand in for device tensors."""
    if device.type == "cpu":
        from emu_device import DeviceTensor
        return t.as_subclass(DeviceTensor)
    return t.to(device)


def _dev(a, device):
    return _as_device(torch.from_numpy(np.array(a)), device)


def _host(t):
    return torch.as_tensor(t).cpu().numpy()


def masks_of(h, w):
    """(names, uint8 (M,h,w) {0,255}): every mask family of a shape."""
    k = h * 131 + w
    ms = [("rand41", LO.random_mask(h, w, 0.41, k)), ("rand59", LO.random_mask(h, w, 0.59, k + 1)), ("blobs", SO.blobs(h, w, k + 2)),
          ("serpentine", LO.serpentine(h, w)), ("comb", LO.comb(h, w)), ("checker", LO.checkerboard(h, w)),
          ("diagonal", LO.diagonal(h, w)), ("full", np.ones((h, w), np.uint8)), ("empty", np.zeros((h, w), np.uint8)),
          ("ring", LO.ring(h, w)), ("rings", LO.ring_in_ring(h, w)), ("holes", LO.blobs_with_holes(h, w, k + 3))]
    if h > TH and w > TW:               # two pixels that touch only diagonally, exactly where four tiles meet: both diagonals
        ms += [("corner", LO.corner_pair(h, w, TH, TW)), ("anticorner", LO.anti_corner_pair(h, w, TH, TW))]
    return [n for n, _ in ms], np.stack([m for _, m in ms]) * np.uint8(255)


@functools.lru_cache(maxsize=None)
def case(h, w):
    """Everything the oracle says about the masks of a shape (computed once, shared, never written to)."""
    names, ms = masks_of(h, w)
    ref = {"names": names, "masks": ms}
    for conn in (4, 8):
        labs = [LO.label(m, conn) for m in ms]
        counts = np.asarray([k for _, k in labs], np.int32)
        stride = int(counts.max()) + 1
        tabs = [LO.tables(lab, k, stride) for lab, k in labs]
        ref[conn] = {"labels": np.stack([lab for lab, _ in labs]), "counts": counts,
                     "area": np.stack([a for a, _ in tabs]), "frame": np.stack([f for _, f in tabs])}
    bg = [LO.label(m == 0, 4) for m in ms]
    ref["background"] = (np.stack([lab for lab, _ in bg]), np.asarray([k for _, k in bg], np.int32))
    ref["filled"] = np.stack([LO.fill_holes(m) for m in ms])
    for v in list(ref.values()) + [x for c in (4, 8) for x in ref[c].values()]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ---- 1. labels, counts, tables, clean-ups on every shape ------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES, ids=IDS)
def test_label_and_tables_match_oracle(device, h, w):
    from medt_amd import ops
    ref = case(h, w)
    m = _dev(ref["masks"], device)
    for conn in (4, 8):
        want = ref[conn]
        labels, counts = ops.label(m, conn)
        assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(labels.shape) == ref["masks"].shape
        assert _host(counts).tolist() == want["counts"].tolist(), (conn, ref["names"])
        bad = [n for k, n in enumerate(ref["names"]) if not np.array_equal(_host(labels[k]), want["labels"][k])]
        assert not bad, (conn, bad)
        area, frame = ops.label_tables(labels, counts)
        assert area.dtype == torch.int32 and frame.dtype == torch.uint8
        assert np.array_equal(_host(area), want["area"]) and np.array_equal(_host(frame), want["frame"]), conn
    names = ref["names"]
    full, checker, diag = names.index("full"), names.index("checker"), names.index("diagonal")
    flat = min(h, w) == 1                                                           # (a 1-pixel-wide map has no diagonal neighbours)
    assert ref[4]["counts"][checker] == math.ceil(h * w / 2) and ref[8]["counts"][checker] == (math.ceil(h * w / 2) if flat else 1)
    assert ref[4]["counts"][diag] == min(h, w) and ref[8]["counts"][diag] == 1 and ref[4]["counts"][full] == 1
    assert ref[4]["counts"][names.index("serpentine")] == 1 and ref[4]["counts"][names.index("comb")] == 1
    if "corner" in names:
        for n in ("corner", "anticorner"):
            assert (ref[4]["counts"][names.index(n)], ref[8]["counts"][names.index(n)]) == (2, 1)
    one, cnt = ops.label(m[1], 4)                                                   # (H,W) in, (H,W) out
    assert tuple(one.shape) == (h, w) and np.array_equal(_host(one), ref[4]["labels"][1]) and _host(cnt).tolist() == [ref[4]["counts"][1]]


@pytest.mark.parametrize("h,w", SHAPES, ids=IDS)
def test_background_and_fill_holes_match_oracle(device, h, w):
    from medt_amd import ops
    ref = case(h, w)
    m = _dev(ref["masks"], device)
    labels, counts = ops.label(m, 4, background=True)
    assert np.array_equal(_host(labels), ref["background"][0]) and _host(counts).tolist() == ref["background"][1].tolist()
    filled = ops.fill_holes(m)
    assert filled.dtype == torch.uint8 and np.array_equal(_host(filled), ref["filled"])
    names = ref["names"]
    if h >= 3 and w >= 3:                                                            # everything inside the outer ring is filled
        for n in ("ring", "rings"):
            got = _host(filled[names.index(n)])
            assert (got[1:-1, 1:-1] == 255).all() and got[0].max() == 0 and got[:, 0].max() == 0


# ---- 2. batches ----------------------------------------------------------------------------------------------------------------
def test_components_do_not_cross_images(device):
    from medt_amd import ops
    h, w = TH + 1, TW + 1
    b = np.zeros((3, h, w), np.uint8)
    b[0, -1], b[1, 0] = 255, 255                                                     # last row of image 0, first row of image 1
    for conn in (4, 8):
        labels, counts = ops.label(_dev(b, device), conn)
        assert _host(counts).tolist() == [1, 1, 0]
        assert np.array_equal(_host(labels), (b != 0).astype(np.int32))
        for n in range(3):
            alone, c1 = ops.label(_dev(b[n], device), conn)
            assert np.array_equal(_host(alone), _host(labels[n])) and _host(c1).tolist() == [_host(counts)[n]]
    area, frame = ops.label_tables(labels, counts)
    assert _host(area).tolist() == [[h * w - w, w], [h * w - w, w], [h * w, 0]] and _host(frame).tolist() == [[0, 1], [0, 1], [0, 0]]


def test_misaligned_views(device):
    """The element-access bodies: the mask one byte into its buffer, `out` one element into an int32 buffer whose canaries
    in front and behind survive."""
    from medt_amd import ops
    for h, w in ((33, 65), (17, 128)):
        ref = case(h, w) if (h, w) in SHAPES else None
        m = ref["masks"][0] if ref else LO.random_mask(h, w, 0.5, 3) * np.uint8(255)
        want4, k4 = LO.label(m, 4)
        want8, k8 = LO.label(m, 8)
        store = torch.zeros(m.size + 8, dtype=torch.uint8)
        store[1:1 + m.size] = torch.from_numpy(m.copy()).reshape(-1)
        view = _as_device(store, device)[1:1 + m.size].view(h, w)
        canary = _as_device(torch.full((m.size + 8,), -7, dtype=torch.int32), device)
        out = canary[1:1 + m.size].view(h, w)
        labels, counts = ops.label(view, 8, out=out)
        assert np.array_equal(_host(out), want8) and _host(counts).tolist() == [k8]
        assert (_host(canary)[:1] == -7).all() and (_host(canary)[1 + m.size:] == -7).all()
        labels, counts = ops.label(view, 4)                                          # misaligned mask alone
        assert np.array_equal(_host(labels), want4) and _host(counts).tolist() == [k4]
        labels, counts = ops.label(_dev(m, device), 4, out=out)                      # misaligned out alone
        assert np.array_equal(_host(out), want4)
        assert (_host(canary)[:1] == -7).all() and (_host(canary)[1 + m.size:] == -7).all()
        area, frame = ops.label_tables(out, counts)                                  # ... and as the tables' input
        wa, wf = LO.tables(want4, k4)
        assert np.array_equal(_host(area)[0], wa) and np.array_equal(_host(frame)[0], wf)
        assert np.array_equal(_host(ops.fill_holes(view)), LO.fill_holes(m))
        assert np.array_equal(_host(ops.remove_small_objects(view, 3, 4)), LO.remove_small(m, 3, 4))


# ---- 3. clean-ups --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
def test_remove_small_objects(device, conn):
    from medt_amd import ops
    m = np.stack([SO.blobs(70, 45, 5), LO.blobs_with_holes(70, 45, 6)]) * np.uint8(255)
    areas = np.concatenate([LO.tables(*LO.label(x, conn))[0][1:] for x in m])
    mid = int(np.sort(areas)[len(areas) // 2])
    assert 2 < mid < areas.max()
    for a in (1, 2, mid, int(areas.max()) + 1):
        got = ops.remove_small_objects(_dev(m, device), a, conn)
        want = np.stack([LO.remove_small(x, a, conn) for x in m])
        assert got.dtype == torch.uint8 and np.array_equal(_host(got), want), a
    assert want.max() == 0                                                           # at max + 1 nothing is left
    assert np.array_equal(_host(ops.remove_small_objects(_dev(m, device), 1, conn)), m)


def test_fill_holes_on_blobs_with_holes(device):
    from medt_amd import ops
    m = np.stack([LO.blobs_with_holes(70, 45, s) for s in (3, 4)] + [LO.random_mask(70, 45, 0.6, 1)])
    want = np.stack([LO.fill_holes(x) for x in m])
    assert ((want != 0) != (m != 0)).sum() > 20                                      # (there are holes to fill)
    assert np.array_equal(_host(ops.fill_holes(_dev(m, device))), want)


# ---- 4. overlaps and scores ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair(h, w, seed):
    a, b = SO.blobs(h, w, seed) * np.uint8(255), SO.blobs(h, w, seed + 100) * np.uint8(255)
    ref = {"a": a, "b": b}
    for conn in (4, 8):
        ref[conn] = LO.object_scores(a, b, conn)
    for v in (a, b):
        v.setflags(write=False)
    return ref


def _check_scores(got, n, want):
    assert bool(got["valid"][n]) == want["valid"]
    assert (int(got["n_pred"][n]), int(got["n_gt"][n])) == (want["n_pred"], want["n_gt"])
    for k in LO.KEYS:
        g, w = float(got[k][n]), want[k]
        print(f"{k}: got {g!r} want {w!r}")
        if math.isnan(w):
            assert math.isnan(g), k
        else:
            assert abs(g - w) <= 1e-12 * abs(w), (k, g, w)


@pytest.mark.parametrize("h,w,seed", [(33, 65, 4), (70, 45, 5)], ids=["33x65", "70x45"])
def test_overlaps_and_object_scores_match_oracle(device, h, w, seed):
    import metrics
    from medt_amd import ops
    ref = pair(h, w, seed)
    a, b = _dev(ref["a"], device), _dev(ref["b"], device)
    for conn in (4, 8):
        la, ca = ops.label(a, conn)
        lb, cb = ops.label(b, conn)
        rows = ops.label_overlaps(la, ca, lb, cb)
        want = LO.overlaps(LO.label(ref["a"], conn)[0], LO.label(ref["b"], conn)[0])
        assert rows.dtype == torch.int64 and len(want) > 0 and np.array_equal(_host(rows), want), conn
        got = metrics.object_scores(a, b, conn)
        for k in LO.KEYS:
            assert got[k].dtype == torch.float64 and tuple(got[k].shape) == (1,)
        assert got["valid"].dtype == torch.bool and got["n_pred"].dtype == torch.int64
        assert ref[conn]["n_pred"] > 1 and ref[conn]["n_gt"] > 1 and ref[conn]["aji"] > 0
        _check_scores(got, 0, ref[conn])
        given = metrics.object_scores(_dev(LO.label(ref["a"], conn)[0], device), _dev(LO.label(ref["b"], conn)[0], device),
                                      labelled=True)                                # the oracle's label maps, taken as given
        _check_scores(given, 0, ref[conn])


def test_object_scores_batches_with_empty_images(device):
    import metrics
    r4, r5 = pair(33, 65, 4), pair(33, 65, 14)
    zero = np.zeros((33, 65), np.uint8)
    pred = np.stack([r4["a"], zero, r5["a"], zero, r4["a"]])
    target = np.stack([r4["b"], zero, r5["b"], r4["b"], zero])
    got = metrics.object_scores(_dev(pred, device), _dev(target, device))
    assert got["valid"].tolist() == [True, False, True, True, True]
    assert got["valid"][:3].tolist() == [True, False, True] and all(math.isnan(float(got[k][1])) for k in LO.KEYS)
    _check_scores(got, 0, r4[8])
    _check_scores(got, 2, r5[8])
    for n in (3, 4):                                                                 # one side empty: missed everything
        assert all(float(got[k][n]) == 0.0 for k in LO.KEYS)
        _check_scores(got, n, LO.object_scores(pred[n], target[n]))
    alone = metrics.object_scores(_dev(pred[2], device), _dev(target[2], device))
    for k in LO.KEYS:
        assert float(alone[k][0]).hex() == float(got[k][2]).hex()


# ---- 5. determinism --------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits(device):
    import metrics
    from medt_amd import ops
    m = _dev(np.stack([LO.random_mask(2 * TH + 1, 2 * TW + 1, d, 9) for d in (0.41, 0.59)] + [LO.serpentine(2 * TH + 1, 2 * TW + 1)]), device)
    t = _dev(np.stack([SO.blobs(2 * TH + 1, 2 * TW + 1, s) for s in (1, 2, 3)]), device)
    runs = []
    for _ in range(2):
        one = []
        for conn in (4, 8):
            labels, counts = ops.label(m, conn)
            area, frame = ops.label_tables(labels, counts)
            s = metrics.object_scores(m, t, conn)
            one += [_host(x).tobytes() for x in (labels, counts, area, frame, ops.remove_small_objects(m, 5, conn))]
            one += [s[k].numpy().tobytes() for k in LO.KEYS]
        one.append(_host(ops.fill_holes(m)).tobytes())
        runs.append(one)
    assert runs[0] == runs[1]


# ---- 6. limits -------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_on_the_host(device):
    from medt_amd import MedtError, _lib as L, ops
    for shape in ((4097, 1), (1, 4097)):
        with pytest.raises(MedtError, match=r"\(-2\).*4096"):                      # MEDT_EUNSUPPORTED, before any launch
            ops.label(_as_device(torch.ones(shape, dtype=torch.uint8), device))
    m = _as_device(torch.ones(2, 4, 4, dtype=torch.uint8), device)
    with pytest.raises(MedtError, match="connectivity"):
        ops.label(m, 6)
    with pytest.raises(MedtError):
        ops.label(m.int())                                                         # uint8 only
    with pytest.raises(MedtError):
        ops.label(m, out=_as_device(torch.zeros(2, 4, 4), device))                 # int32 out only
    if device.type == "cuda":
        with pytest.raises(MedtError):
            ops.label(torch.ones(4, 4, dtype=torch.uint8))                         # no CPU path
    # the raw ABI: an undersized workspace, a connectivity of 6, null pointers, a stride that cannot hold the counts
    lib = L.lib()
    need = lib.medt_label_workspace_bytes(2, 4, 4)
    assert need >= 2 * 4 * 4 * 4 and lib.medt_label_workspace_bytes(1, 4097, 1) == 0
    labels = _as_device(torch.zeros(2, 4, 4, dtype=torch.int32), device)
    counts = _as_device(torch.zeros(2, dtype=torch.int32), device)
    ws = _as_device(torch.zeros(need // 4 + 4, dtype=torch.int32), device)
    args = (m.data_ptr(), labels.data_ptr(), counts.data_ptr(), ws.data_ptr())
    assert lib.medt_label_components(*args, need - 1, 2, 4, 4, 8, 0, None) == -4   # MEDT_EWORKSPACE
    assert b"workspace too small" in lib.medt_last_error()
    assert lib.medt_label_components(*args, need, 2, 4, 4, 6, 0, None) == -1       # MEDT_EINVAL
    assert lib.medt_label_components(None, *args[1:], need, 2, 4, 4, 8, 0, None) == -1
    area = _as_device(torch.zeros(2, 4, dtype=torch.int32), device)
    frame = _as_device(torch.zeros(2, 4, dtype=torch.uint8), device)
    assert lib.medt_label_tables(labels.data_ptr(), area.data_ptr(), frame.data_ptr(), 2, 4, 4, 4, 4, None) == -1
    assert lib.medt_label_tables(labels.data_ptr(), None, frame.data_ptr(), 2, 4, 4, 4, 3, None) == -1
    assert lib.medt_label_select(labels.data_ptr(), None, None, frame.data_ptr(), 2, 4, 4, 4, None) == -1
    assert (_host(labels) == 0).all() and (_host(counts) == 0).all()               # nothing was launched
