"""No GPU: the oracle of the border term for touching objects (tests/border_oracle.py) -- brute force against one SciPy transform
per object, hand-computed cases -- the kernels on the CPU lane emulator against it under three work-item orders (the two-deep
column sweep, the row search over both entries of every column, the host code, and that the order changes no bit), their
refusals, and train.py's handling of the new flags."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import border_oracle as RO
import helpers as H
from test_boundary_cpu import ORDERS

PKG = os.path.join(H.ROOT, "medical-transformer_amd")
NONE = RO.NONE
EDT_SHAPES = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 5, 7), (3, 17, 19), (2, 64, 64), (1, 33, 130), (1, 130, 33)]
# 0 objects | sparse (0, 1 or 2 in the small maps) | many | many that touch
DENSITIES = (0.0, 0.12, 0.4, 0.8)


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
    a = a.numpy() if torch.is_tensor(a) else a
    return torch.from_numpy(np.ascontiguousarray(a)).as_subclass(DeviceTensor)


def edt_cases():
    """(labels int32 (N,H,W)) for every shape and density, + three tall maps, + maps with exactly one and exactly two objects per
    image (the last two)."""
    cases = [RO.blob_labels(*s, d, 100 + 10 * i + j) for i, s in enumerate(EDT_SHAPES) for j, d in enumerate(DENSITIES)]
    one = np.zeros((2, 17, 19), np.int32)
    one[0, 3:6, 4:9] = 1
    one[1, 16, 18] = 1
    two = np.zeros((2, 33, 40), np.int32)
    two[0, 2:5, 2:5], two[0, 20:30, 35:40] = 1, 2
    two[1, :, 0], two[1, :, 39] = 2, 1
    # the column pass's other paths: more segments than a workgroup has slots (above 256 rows), 8 columns per workgroup (above 2048)
    tall = [RO.blob_labels(1, 300, 20, 0.4, 7), RO.blob_labels(1, 2100, 9, 0.12, 8), RO.blob_labels(1, 2100, 9, 0.5, 9)]
    return cases + tall + [one, two]


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_brute_force_equals_scipy(connectivity):
    counts = set()
    for i, s in enumerate(EDT_SHAPES):
        for j, d in enumerate(DENSITIES):
            lab = RO.blob_labels(*s, d, 100 + 10 * i + j, connectivity)
            counts.update(int(m.max()) for m in lab)
            b, sc = RO.edt2_batch(lab, RO.edt2_brute), RO.edt2_batch(lab, RO.edt2_scipy)
            assert np.array_equal(b[0], sc[0]) and np.array_equal(b[1], sc[1]), (s, d)
    assert {0, 1, 2} <= counts and max(counts) > 20                   # no, one, two and many objects all occur


HAND_THIRD = np.array([[3, 3, 0],
                       [0, 3, 0],
                       [0, 3, 0],
                       [1, 0, 0],
                       [0, 0, 0],
                       [2, 0, 0],
                       [0, 0, 0]], np.int32)


def hand_cases():
    """[(labels, {(y, x): (d1sq, d2sq)}, whole-map expectation or None)]"""
    yy, xx = np.mgrid[0:5, 0:5]
    one = np.zeros((5, 5), np.int32)
    one[2, 2] = 7
    none = np.zeros((3, 4), np.int32)
    row = np.array([[0, 1, 0, 0, 0, 2, 0]], np.int32)
    corner4 = np.zeros((4, 4), np.int32)
    corner4[0:2, 0:2], corner4[2:4, 2:4] = 1, 2
    corner8 = (corner4 > 0).astype(np.int32)
    return [
        (one, {}, ((yy - 2) ** 2 + (xx - 2) ** 2, np.full((5, 5), NONE))),                   # one object: no second anywhere
        (none, {}, (np.full((3, 4), NONE), np.full((3, 4), NONE))),                          # no object
        (row, {}, (np.array([[1, 0, 1, 4, 1, 0, 1]]), np.array([[25, 16, 9, 4, 9, 16, 25]]))),   # x = 3: the tie d1sq == d2sq
        (row.T.copy(), {}, (np.array([[1, 0, 1, 4, 1, 0, 1]]).T, np.array([[25, 16, 9, 4, 9, 16, 25]]).T)),
        # two blocks that touch at a corner: two objects at connectivity 4 ...
        (corner4, {(0, 2): (1, 4), (1, 1): (0, 2), (1, 2): (1, 1), (2, 1): (1, 1), (3, 3): (0, 8), (0, 3): (4, 4), (3, 0): (4, 4)}, None),
        # ... and one at 8
        (corner8, {(1, 2): (1, NONE), (0, 3): (4, NONE), (1, 1): (0, NONE)}, None),
        # column 0 holds labels 1, 2, 3; at (3, 0), inside object 1, the second-nearest object is 3 -- third along column 0
        # (9 against 4 for label 2), but 1 + 1 away through column 1
        (HAND_THIRD, {(3, 0): (0, 2), (3, 1): (1, 1), (4, 0): (1, 1), (6, 2): (5, 13), (0, 2): (1, 13), (5, 0): (0, 4)}, None),
    ]


def test_oracle_on_hand_computed_cases():
    for lab, points, whole in hand_cases():
        for f in (RO.edt2_brute, RO.edt2_scipy):
            d1, d2 = f(lab)
            for (y, x), (w1, w2) in points.items():
                assert (d1[y, x], d2[y, x]) == (w1, w2), (lab, y, x)
            if whole is not None:
                assert np.array_equal(d1, whole[0]) and np.array_equal(d2, whole[1])
    # e and R by hand: one row, targets 1 0 1 -> two objects, the middle pixel one away from each; sigma 1 -> e = exp(-2);
    # z = 0 -> nll = ln 2 at every pixel; V = 3
    t = np.array([[[1, 0, 1]]], np.int64)
    lab = RO.label_targets(t)
    assert lab.tolist() == [[[1, 0, 2]]]
    d1, d2 = RO.edt2_batch(lab)
    e = RO.weight_e(t, d1, d2, 1.0)
    assert e[0, 0, 0] == 0 and e[0, 0, 2] == 0 and abs(e[0, 0, 1].item() - math.exp(-2.0)) < 1e-15
    z = torch.zeros(1, 2, 1, 3, dtype=torch.float64)
    assert abs(RO.border_term(z, torch.from_numpy(t), e).item() - math.exp(-2.0) * math.log(2.0) / 3) < 1e-15
    # fewer than two objects: e is 0 everywhere; an ignored pixel is not in F, so it separates 1 1 from 1
    for row in ([1, 1, 0], [0, 0, 0]):
        tt = np.array([[row]], np.int64)
        dd = RO.edt2_batch(RO.label_targets(tt))
        assert not RO.weight_e(tt, *dd, 1.0).any()
    tt = np.array([[[1, 1, RO.IGNORE, 1, 0]]], np.int64)
    assert RO.label_targets(tt).tolist() == [[[1, 1, 0, 2, 0]]]
    assert abs(RO.weight_e(tt, *RO.edt2_batch(RO.label_targets(tt)), 1.0)[0, 0, 4].item() - math.exp(-(1 + 3) ** 2 / 2.0)) < 1e-18


# ---- the emulated kernels ----------------------------------------------------------------------------------------------------------
def test_emulated_object_edt2_matches_oracle_under_every_order(emu):
    from emu_device import emulated_device
    from medt_amd import ops
    cases = edt_cases() + [lab[None] for lab, _, _ in hand_cases()]
    runs = []
    for mode, seed in ORDERS:
        emu.emu_set_order(mode, seed)
        try:
            with emulated_device(emu):
                runs.append([tuple(d.numpy().copy() for d in ops.object_edt2_sq(dev(lab))) for lab in cases])
        finally:
            emu.emu_set_order(0, 0)
    want = [RO.edt2_batch(lab) for lab in cases]
    for r in runs:
        for got, w, lab in zip(r, want, cases):
            assert got[0].dtype == np.int32 and got[0].shape == lab.shape
            assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]), lab.shape


def test_emulated_corner_blocks_through_label(emulated):
    """The node's own chain label() -> object_edt2_sq(): two objects at connectivity 4, one at 8."""
    from medt_amd import ops
    m = np.zeros((1, 4, 4), np.uint8)
    m[0, 0:2, 0:2] = m[0, 2:4, 2:4] = 1
    lab4, c4 = ops.label(dev(m), 4)
    lab8, c8 = ops.label(dev(m), 8)
    assert (c4.item(), c8.item()) == (2, 1)
    d1, d2 = ops.object_edt2_sq(lab4)
    assert (d1[0, 0, 2].item(), d2[0, 0, 2].item()) == (1, 4) and (d1[0, 1, 1].item(), d2[0, 1, 1].item()) == (0, 2)
    d1, d2 = ops.object_edt2_sq(lab8)
    assert d1[0, 1, 2].item() == 1 and (d2 == NONE).all()


def test_emulated_loss_and_gradient_under_every_order(emu):
    """The GPU test's bounds (tests/test_border_gpu.py): 1e-5 relative on the loss, 1e-5 on the gradient."""
    import medt_amd
    from emu_device import emulated_device
    from medt_amd import ops
    import boundary_oracle as BO
    g = torch.Generator().manual_seed(5)
    N, K, Hh, Ww = 2, 3, 33, 35
    logits = torch.randn(N, K, Hh, Ww, generator=g) * 3
    t = BO.blob_targets(N, Hh, Ww, K, 0.3, 9)
    tt = torch.from_numpy(t)
    for conn in (4, 8):
        e = RO.weight_e(t, *RO.edt2_batch(RO.label_targets(t, 2, connectivity=conn)), 3.0, fg=2)
        assert (e > 1e-3).sum() > 20
        w = torch.tensor([0.5, 1.0, 2.0])
        z64 = logits.double().requires_grad_(True)
        want, R = RO.combined(z64, tt, e, 0.8, w.double(), 0.7, 1.3)
        (want * 1.7).backward()
        z64b = logits.double().requires_grad_(True)
        alone = 0.8 * RO.border_term(z64b, tt, e)
        (alone * 1.7).backward()
        runs = []
        old, ops.CHECK_TARGETS = ops.CHECK_TARGETS, False
        try:
            for mode, seed in ORDERS:
                emu.emu_set_order(mode, seed)
                with emulated_device(emu):
                    a = torch.full((1,), 0.8)
                    ld = logits.clone().requires_grad_(True)
                    loss = medt_amd.seg_border_loss(ld, tt, a, sigma=3.0, weight=w, ce=0.7, dice=1.3, fg=2, connectivity=conn)
                    (loss * 1.7).backward()
                    lb = logits.clone().requires_grad_(True)
                    only = medt_amd.border_loss(lb, tt, a, sigma=3.0, fg=2, connectivity=conn)
                    (only * 1.7).backward()
                runs.append((loss.detach().clone(), ld.grad.clone(), loss._medt_border_out.clone(), only.detach().clone(), lb.grad.clone()))
        finally:
            ops.CHECK_TARGETS = old
            emu.emu_set_order(0, 0)
        for r in runs[1:]:
            assert all(torch.equal(x, y) for x, y in zip(runs[0], r))
        loss, grad, out, only, gonly = runs[0]
        assert abs(loss.item() - want.item()) < 1e-5 * max(1.0, abs(want.item())) and H.rel_err(grad, z64.grad) < 1e-5
        assert abs(only.item() - alone.item()) < 1e-5 * max(1.0, abs(alone.item())) and H.rel_err(gonly, z64b.grad) < 1e-5
        assert abs(out[1].item() - R.item()) < 1e-5 * max(1.0, abs(R.item())) and out[2].item() == np.float32(0.8)
        invalid = ((tt < 0) | (tt >= K)).unsqueeze(1).expand_as(logits)
        assert invalid.any() and (grad[invalid] == 0).all() and (gonly[invalid] == 0).all()
        assert (gonly[(e == 0).unsqueeze(1).expand_as(logits)] == 0).all() and (gonly != 0).any()


def test_emulated_refusals(emulated):
    import medt_amd
    from medt_amd import _lib as L, ops
    E = medt_amd.MedtError
    for shape in ((1, 1, 4097), (1, 4097, 1)):                      # above MEDT_EDT_MAX_DIM: refused on the host, before any launch
        with pytest.raises(E, match=r"\(-2\).*at most 4096"):
            ops.object_edt2_sq(dev(np.zeros(shape, np.int32)))
    with pytest.raises(E):
        ops.object_edt2_sq(dev(np.zeros((1, 4, 4), np.int64)))
    with pytest.raises(E):
        ops.object_edt2_sq(dev(np.zeros((1, 4, 4), np.int32)), out=dev(np.zeros((1, 4, 4), np.int32)))
    z, t, a = dev(torch.zeros(1, 3, 4, 4)), dev(np.zeros((1, 4, 4), np.int64)), dev(torch.zeros(1))
    for fg in (-1, 3):
        with pytest.raises(E):
            medt_amd.border_loss(z, t, a, fg=fg)
    for sigma in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(E, match="sigma"):
            medt_amd.border_loss(z, t, a, sigma=sigma)
    with pytest.raises(E, match="connectivity"):
        medt_amd.border_loss(z, t, a, connectivity=6)
    with pytest.raises(E):
        medt_amd.seg_border_loss(z, t, a, ce=0.0, dice=0.0)
    # the C ABI's own checks (the Python wrappers refuse these earlier)
    lab, d1, d2 = (dev(np.zeros((1, 4, 4), np.int32)) for _ in range(3))
    scratch, part, out = dev(np.zeros((4, 4, 4), np.int32)), dev(torch.zeros(8)), dev(torch.zeros(4))
    fwd = lambda fg, sigma: emulated.medt_border_fwd(z.data_ptr(), t.data_ptr(), d1.data_ptr(), d2.data_ptr(), sigma, a.data_ptr(), None,
                                                     part.data_ptr(), out.data_ptr(), 1, 3, 16, fg, -100, None)
    bwd = lambda fg, sigma: emulated.medt_border_bwd(z.data_ptr(), t.data_ptr(), d1.data_ptr(), d2.data_ptr(), sigma, out.data_ptr(), None,
                                                     z.data_ptr(), 1, 3, 16, fg, -100, 0, None)
    for fg in (-1, 3):
        assert fwd(fg, 5.0) == -1 and b"foreground class" in emulated.medt_last_error()
        assert bwd(fg, 5.0) == -1
    for sigma in (0.0, -2.0, float("inf"), float("nan")):
        assert fwd(1, sigma) == -1 and b"sigma" in emulated.medt_last_error()
        assert bwd(1, sigma) == -1
    assert fwd(1, 5.0) == 0 and bwd(1, 5.0) == 0
    edt2 = lambda s, o1, o2, Hh=4, Ww=4: emulated.medt_object_edt2(lab.data_ptr(), s.data_ptr(), o1.data_ptr(), o2.data_ptr(), 1, Hh, Ww, None)
    assert edt2(scratch, d1, d1) == -1 and edt2(d1, d1, d2) == -1 and edt2(d2, d1, d2) == -1          # outputs that are one buffer
    assert emulated.medt_object_edt2(None, scratch.data_ptr(), d1.data_ptr(), d2.data_ptr(), 1, 4, 4, None) == -1
    assert edt2(scratch, d1, d2, 4, 4097) == -2 and edt2(scratch, d1, d2, 4097, 4) == -2 and edt2(scratch, d1, d2, 0, 4) == -1
    assert emulated.medt_object_edt2(lab.data_ptr(), scratch.data_ptr(), d1.data_ptr(), d2.data_ptr(), 2 ** 9, 2048, 2048, None) == -2
    assert edt2(scratch, d1, d2) == 0
    assert emulated.medt_border_workspace(2, 300) == 2 * 2 * 2 and emulated.medt_border_out_floats(5) == 8
    assert emulated.medt_border_workspace(0, 300) == 0 and emulated.medt_border_out_floats(0) == 0
    for name in ("medt_object_edt2", "medt_border_workspace", "medt_border_out_floats", "medt_border_fwd", "medt_border_bwd"):
        assert name in L.SIGNATURES
    assert medt_amd.border_loss is ops.border_loss and medt_amd.seg_border_loss is ops.seg_border_loss


# ---- train.py ----------------------------------------------------------------------------------------------------------------------
def load_train():
    spec = importlib.util.spec_from_file_location("cli_train_border", os.path.join(PKG, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_border_flags_need_a_border_loss():
    mod = load_train()
    for flag, v in (("--border_w0", "3"), ("--border_sigma", "2"), ("--border_connectivity", "4")):
        for loss in ("ce", "dice", "ce+dice", "ce+boundary"):
            a = mod.parser.parse_args(["--train_dataset", "x", "--loss", loss, flag, v])
            with pytest.raises(SystemExit, match="border"):
                mod.make_border(a.loss, a.border_w0, a.border_sigma, a.border_connectivity)
    a = mod.parser.parse_args(["--train_dataset", "x"])
    assert (a.border_w0, a.border_sigma, a.border_connectivity) == (None, None, None)
    assert mod.make_border(a.loss, a.border_w0, a.border_sigma, a.border_connectivity) is None
    a = mod.parser.parse_args(["--train_dataset", "x", "--loss", "ce+border"])
    assert mod.make_border(a.loss, a.border_w0, a.border_sigma, a.border_connectivity) == {"w0": 10.0, "sigma": 5.0, "connectivity": 8}
    a = mod.parser.parse_args(["--train_dataset", "x", "--loss", "ce+dice+border", "--border_w0", "3", "--border_sigma", "2.5",
                               "--border_connectivity", "4"])
    assert mod.make_border(a.loss, a.border_w0, a.border_sigma, a.border_connectivity) == {"w0": 3.0, "sigma": 2.5, "connectivity": 4}
    for w0, sigma in ((-1.0, None), (None, 0.0), (None, -3.0)):
        with pytest.raises(SystemExit):
            mod.make_border("ce+border", w0, sigma, None)
    for bad in (["--loss", "border"], ["--loss", "ce+border+boundary"], ["--loss", "ce+boundary+border"],
                ["--loss", "ce+border", "--border_connectivity", "6"]):
        with pytest.raises(SystemExit):
            mod.parser.parse_args(["--train_dataset", "x"] + bad)
    # the boundary flags still belong to the boundary loss alone
    a = mod.parser.parse_args(["--train_dataset", "x", "--loss", "ce+border", "--boundary_alpha", "0.1"])
    with pytest.raises(SystemExit, match="boundary"):
        mod.make_boundary(a.loss, a.boundary_alpha, a.boundary_step, a.boundary_max)


def test_make_criterion_today_and_with_border():
    from metrics import BorderLoss, BoundaryLoss, DiceCELoss, LogNLLLoss
    mod = load_train()
    c = mod.make_criterion("ce", None)
    assert type(c) is LogNLLLoss and c.weight is None
    c = mod.make_criterion("ce+dice", "1,3")
    assert type(c) is DiceCELoss and (c.ce, c.dice) == (1.0, 1.0) and c.weight.tolist() == [1.0, 3.0]
    c = mod.make_criterion("ce+dice+boundary", "1,3", mod.make_boundary("ce+dice+boundary", 0.05, 0.1, 0.5))
    assert type(c) is BoundaryLoss and c.alpha.tolist() == [np.float32(0.05)]
    c = mod.make_criterion("ce+dice+border", "1,3", None, mod.make_border("ce+dice+border", 3.0, 2.5, 4))
    assert type(c) is BorderLoss and (c.ce, c.dice, c.fg, c.sigma, c.connectivity) == (1.0, 1.0, 1, 2.5, 4)
    assert c.weight.tolist() == [1.0, 3.0]
    assert c.w0.dtype == torch.float32 and c.w0.tolist() == [3.0] and "w0" in dict(c.named_buffers())
    ptr = c.w0.data_ptr()
    c.set_w0(0.25)
    assert c.w0.data_ptr() == ptr and c.w0.item() == 0.25
    c = mod.make_criterion("ce+border", None, None, mod.make_border("ce+border", None, None, None))
    assert (c.ce, c.dice, c.sigma, c.connectivity) == (1.0, 0.0, 5.0, 8) and c.w0.item() == 10.0
    c = mod.make_criterion("dice+border", None, None, mod.make_border("dice+border", None, None, None))
    assert (c.ce, c.dice) == (0.0, 1.0)
    with pytest.raises(SystemExit):
        mod.make_criterion("dice+border", "1,3", None, None)             # class weights weigh the cross entropy
    d = BorderLoss()
    assert (d.w0.item(), d.sigma, d.ce, d.dice, d.eps, d.fg, d.connectivity, d.ignore_index) == (10.0, 5.0, 1.0, 0.0, 1.0, 1, 8, -100)
