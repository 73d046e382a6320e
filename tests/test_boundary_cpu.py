"""No GPU: the oracle of the boundary loss (tests/boundary_oracle.py) -- brute force against SciPy, hand-computed cases -- the
kernels on the CPU lane emulator against it under three work-item orders (the index arithmetic, the LDS hand-over of the column
pass, the host code, and that the order changes no bit), their refusals, and train.py's handling of the new flags."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import boundary_oracle as BO
import helpers as H

PKG = os.path.join(H.ROOT, "medical-transformer_amd")
EDT_SHAPES = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 5, 7), (3, 17, 19), (2, 64, 64), (1, 33, 130), (1, 130, 33)]


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


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EDT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_brute_force_equals_scipy(shape):
    for density in (0.3, 0.7):
        t = BO.blob_targets(*shape, 3, density, 11 + EDT_SHAPES.index(shape))
        for fg in (1, 2):
            assert np.array_equal(BO.sd2_batch(t, fg, how=BO.sd2_brute), BO.sd2_batch(t, fg, how=BO.sd2_scipy)), (density, fg)


def test_oracle_on_hand_computed_cases():
    one = np.zeros((5, 5), np.int64)
    one[2, 2] = 1
    yy, xx = np.mgrid[0:5, 0:5]
    want = (yy - 2) ** 2 + (xx - 2) ** 2
    want[2, 2] = -1                                                 # the F pixel: its nearest pixel outside F is one away
    for f in (BO.sd2_brute, BO.sd2_scipy):
        assert np.array_equal(f(one), want)
    block = np.zeros((7, 7), np.int64)
    block[2:5, 2:5] = 1
    for f in (BO.sd2_brute, BO.sd2_scipy):
        got = f(block)
        assert got[3, 3] == -4 and (got[2:5, 2:5][np.arange(9).reshape(3, 3) != 4] == -1).all()
        assert got[0, 0] == 8 and got[3, 0] == 4 and got[1, 3] == 1
        p = BO.phi(got)
        assert p[3, 3] == -1.0 and (p[2:5, 2:5].reshape(-1)[[0, 1, 2, 3, 5, 6, 7, 8]] == 0).all()      # the ring: phi = 0
        assert p[3, 0] == 2.0 and abs(p[0, 0].item() - 8 ** 0.5) < 1e-15
    row = np.array([[0, 0, 1, 1, 1, 0, BO.IGNORE]], np.int64)       # one row; the ignored pixel is outside F
    col = row.T.copy()
    for f in (BO.sd2_brute, BO.sd2_scipy):
        assert f(row).tolist() == [[4, 1, -1, -4, -1, 1, 4]]
        assert f(col).tolist() == [[4], [1], [-1], [-4], [-1], [1], [4]]
        # the two empty cases: no F, all F
        assert not f(np.zeros((3, 4), np.int64)).any() and not f(np.ones((3, 4), np.int64)).any()
        assert not f(np.full((3, 4), BO.IGNORE, np.int64)).any() and not f(np.ones((3, 4), np.int64), fg=1, ignore=1).any()
    # B by hand: two pixels, one of F; z = 0 -> s = 1/2; phi = (1, 0) -> B = 1/2 * 1 / 2
    z = torch.zeros(1, 2, 1, 2, dtype=torch.float64)
    t = torch.tensor([[[0, 1]]])
    assert BO.boundary_term(z, t, BO.sd2_batch(t.numpy())).item() == 0.25


# ---- the emulated kernels ----------------------------------------------------------------------------------------------------------
ORDERS = ((0, 0), (1, 0), (2, 1))


def test_emulated_signed_edt_matches_oracle_under_every_order(emu):
    from emu_device import emulated_device
    from medt_amd import ops
    cases = [(s, d, BO.blob_targets(*s, 3, d, 11 + i)) for i, s in enumerate(EDT_SHAPES) for d in (0.3, 0.7)]
    extra = BO.blob_targets(3, 40, 50, 3, 0.5, 77)
    extra[1][extra[1] == 1] = 0                                      # no F
    extra[2] = 1                                                      # all F
    cases.append(((3, 40, 50), 0.5, extra))
    runs = []
    for mode, seed in ORDERS:
        emu.emu_set_order(mode, seed)
        try:
            with emulated_device(emu):
                runs.append([ops.signed_edt_sq(dev(t), fg=fg).numpy().copy() for _, _, t in cases for fg in (1, 2)])
        finally:
            emu.emu_set_order(0, 0)
    want = [BO.sd2_batch(t, fg) for _, _, t in cases for fg in (1, 2)]
    for r in runs:
        assert all(np.array_equal(a, b) for a, b in zip(r, want))
    assert not runs[0][-2][1].any() and not runs[0][-2][2].any() and runs[0][-2][0].all()


def test_emulated_loss_and_gradient_under_every_order(emu):
    """The GPU test's bounds (tests/test_boundary_gpu.py): 1e-5 relative on the loss, 1e-5 on the gradient."""
    import medt_amd
    from emu_device import emulated_device
    from medt_amd import ops
    g = torch.Generator().manual_seed(5)
    N, K, Hh, Ww = 2, 3, 33, 35
    logits = torch.randn(N, K, Hh, Ww, generator=g) * 3
    t = BO.blob_targets(N, Hh, Ww, K, 0.3, 9)
    sd2 = BO.sd2_batch(t, fg=2)
    w = torch.tensor([0.5, 1.0, 2.0])
    z64 = logits.double().requires_grad_(True)
    want, B = BO.combined(z64, torch.from_numpy(t), sd2, 0.3, w.double(), 0.7, 1.3, fg=2)
    (want * 1.7).backward()
    z64b = logits.double().requires_grad_(True)
    alone = 0.3 * BO.boundary_term(z64b, torch.from_numpy(t), sd2, fg=2)
    (alone * 1.7).backward()
    runs = []
    old, ops.CHECK_TARGETS = ops.CHECK_TARGETS, False
    try:
        for mode, seed in ORDERS:
            emu.emu_set_order(mode, seed)
            with emulated_device(emu):
                a = torch.full((1,), 0.3)
                ld = logits.clone().requires_grad_(True)
                loss = medt_amd.seg_boundary_loss(ld, torch.from_numpy(t), a, weight=w, ce=0.7, dice=1.3, fg=2)
                (loss * 1.7).backward()
                lb = logits.clone().requires_grad_(True)
                only = medt_amd.boundary_loss(lb, torch.from_numpy(t), a, fg=2)
                (only * 1.7).backward()
            runs.append((loss.detach().clone(), ld.grad.clone(), loss._medt_boundary_out.clone(), only.detach().clone(), lb.grad.clone()))
    finally:
        ops.CHECK_TARGETS = old
        emu.emu_set_order(0, 0)
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))
    loss, grad, out, only, gonly = runs[0]
    assert abs(loss.item() - want.item()) < 1e-5 * max(1.0, abs(want.item())) and H.rel_err(grad, z64.grad) < 1e-5
    assert abs(only.item() - alone.item()) < 1e-5 * max(1.0, abs(alone.item())) and H.rel_err(gonly, z64b.grad) < 1e-5
    assert abs(out[1].item() - B.item()) < 1e-5 * max(1.0, abs(B.item())) and out[2].item() == np.float32(0.3)
    tt = torch.from_numpy(t)
    invalid = ((tt < 0) | (tt >= K)).unsqueeze(1).expand_as(logits)
    assert invalid.any() and (grad[invalid] == 0).all() and (gonly[invalid] == 0).all()


def test_emulated_refusals(emulated):
    import medt_amd
    from medt_amd import _lib as L, ops
    E = medt_amd.MedtError
    for shape in ((1, 1, 4097), (1, 4097, 1)):                      # above MEDT_EDT_MAX_DIM: refused on the host, before any launch
        with pytest.raises(E, match=r"\(-2\).*at most 4096"):
            ops.signed_edt_sq(dev(np.zeros(shape, np.int64)))
    z, t, a = dev(torch.zeros(1, 3, 4, 4)), dev(np.zeros((1, 4, 4), np.int64)), dev(torch.zeros(1))
    for fg in (-1, 3):
        with pytest.raises(E):
            medt_amd.boundary_loss(z, t, a, fg=fg)
    # the C ABI's own checks (the Python wrappers refuse these earlier)
    sd2, part, out = dev(np.zeros((1, 4, 4), np.int32)), dev(torch.zeros(8)), dev(torch.zeros(4))
    for fg in (-1, 3):
        rc = emulated.medt_boundary_fwd(z.data_ptr(), t.data_ptr(), sd2.data_ptr(), a.data_ptr(), None, part.data_ptr(), out.data_ptr(),
                                        1, 3, 16, fg, -100, None)
        assert rc == -1 and b"foreground class" in emulated.medt_last_error()
        rc = emulated.medt_boundary_bwd(z.data_ptr(), t.data_ptr(), sd2.data_ptr(), out.data_ptr(), None, z.data_ptr(), 1, 3, 16, fg,
                                        -100, 0, None)
        assert rc == -1
    assert emulated.medt_signed_edt(t.data_ptr(), sd2.data_ptr(), sd2.data_ptr(), 1, 4, 4, 1, -100, None) == -1      # sd2 is g2
    assert emulated.medt_signed_edt(t.data_ptr(), sd2.data_ptr(), out.data_ptr(), 1, 4, 4097, 1, -100, None) == -2
    assert emulated.medt_boundary_workspace(2, 300) == 2 * 2 * 2 and emulated.medt_boundary_out_floats(5) == 8
    assert "medt_signed_edt" in L.SIGNATURES and "medt_boundary_bwd" in L.SIGNATURES


# ---- train.py ----------------------------------------------------------------------------------------------------------------------
def load_train():
    spec = importlib.util.spec_from_file_location("cli_train_boundary", os.path.join(PKG, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_boundary_flags_need_a_boundary_loss():
    mod = load_train()
    for flag in ("--boundary_alpha", "--boundary_step", "--boundary_max"):
        for loss in ("ce", "dice", "ce+dice"):
            a = mod.parser.parse_args(["--train_dataset", "x", "--loss", loss, flag, "0.1"])
            with pytest.raises(SystemExit, match="boundary"):
                mod.make_boundary(a.loss, a.boundary_alpha, a.boundary_step, a.boundary_max)
    a = mod.parser.parse_args(["--train_dataset", "x"])
    assert (a.boundary_alpha, a.boundary_step, a.boundary_max) == (None, None, None)
    assert mod.make_boundary(a.loss, a.boundary_alpha, a.boundary_step, a.boundary_max) is None
    a = mod.parser.parse_args(["--train_dataset", "x", "--loss", "ce+boundary"])
    sched = mod.make_boundary(a.loss, a.boundary_alpha, a.boundary_step, a.boundary_max)
    assert sched == {"alpha": 0.01, "step": 0.01, "max": 1.0}
    assert [round(mod.boundary_alpha(sched, e), 6) for e in (0, 1, 98, 99, 100, 400)] == [0.01, 0.02, 0.99, 1.0, 1.0, 1.0]
    with pytest.raises(SystemExit):
        mod.make_boundary("ce+boundary", 0.5, None, 0.1)           # the ceiling below the start
    with pytest.raises(SystemExit):
        mod.parser.parse_args(["--train_dataset", "x", "--loss", "boundary"])


def test_make_criterion_today_and_with_boundary():
    from metrics import BoundaryLoss, DiceCELoss, LogNLLLoss
    mod = load_train()
    c = mod.make_criterion("ce", None)
    assert type(c) is LogNLLLoss and c.weight is None
    c = mod.make_criterion("ce", "1,3")
    assert type(c) is LogNLLLoss and c.weight.tolist() == [1.0, 3.0]
    c = mod.make_criterion("ce+dice", "1,3")
    assert type(c) is DiceCELoss and (c.ce, c.dice) == (1.0, 1.0) and c.weight.tolist() == [1.0, 3.0]
    c = mod.make_criterion("dice", None)
    assert type(c) is DiceCELoss and (c.ce, c.dice) == (0.0, 1.0) and c.weight is None
    sched = mod.make_boundary("ce+dice+boundary", 0.05, 0.1, 0.5)
    c = mod.make_criterion("ce+dice+boundary", "1,3", sched)
    assert type(c) is BoundaryLoss and (c.ce, c.dice, c.fg) == (1.0, 1.0, 1) and c.weight.tolist() == [1.0, 3.0]
    assert c.alpha.dtype == torch.float32 and c.alpha.tolist() == [np.float32(0.05)] and "alpha" in dict(c.named_buffers())
    ptr = c.alpha.data_ptr()
    c.set_alpha(0.25)
    assert c.alpha.data_ptr() == ptr and c.alpha.item() == 0.25
    c = mod.make_criterion("ce+boundary", None, mod.make_boundary("ce+boundary", None, None, None))
    assert (c.ce, c.dice) == (1.0, 0.0) and c.alpha.item() == np.float32(0.01)
    c = mod.make_criterion("dice+boundary", None, mod.make_boundary("dice+boundary", None, None, None))
    assert (c.ce, c.dice) == (0.0, 1.0)
    with pytest.raises(SystemExit):
        mod.make_criterion("dice+boundary", "1,3", None)             # class weights weigh the cross entropy
