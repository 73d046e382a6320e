"""The boundary loss on the device -- medt_amd.ops.signed_edt_sq (medt_signed_edt), medt_amd.boundary_loss and
medt_amd.seg_boundary_loss (medt_boundary_fwd / _bwd behind the unchanged medt_seg_loss_*), metrics.BoundaryLoss in TrainStep --
against tests/boundary_oracle.py: the distance map torch.equal SciPy's (held to brute force in tests/test_boundary_cpu.py), loss
and gradient against float64 autograd.

Bounds: |loss - loss64| < 1e-5 * max(1, |loss64|) and rel_err(dlogits) < 1e-5 for every shape, configuration and alpha: the
bound tests/test_seg_loss_gpu.py holds, relative because phi reaches tens of pixels.  Worst case measured on the MI355X:
loss 1.2e-7 relative ((2,2,130,130), ce+dice+boundary, alpha 0.01), dlogits 4.9e-7 ((2,3,5,7), boundary alone, alpha 0.01); no
case needed a bound of its own.  The same file runs on the CPU lane emulator: `-m gpu --emulate`."""
import numpy as np
import pytest
import torch

import boundary_oracle as BO
import helpers as H

pytestmark = pytest.mark.gpu

IGNORE = BO.IGNORE
# N, H, W: one pixel | one row | one column | small | W % 4 != 0 | aligned | more columns than one workgroup of the column pass
# (16) and more rows than one 32-row word, ragged in both | the transpose
EDT_SHAPES = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 5, 7), (3, 17, 19), (2, 64, 64), (1, 33, 130), (1, 130, 33)]
LOSS_SHAPES = [(3, 2, 17, 19), (2, 3, 5, 7), (1, 5, 16, 16), (2, 2, 130, 130)]
# name -> (class weights?, ce, dice)
CONFIGS = {"boundary": (False, 0.0, 0.0), "wce+boundary": (True, 1.0, 0.0), "dice+boundary": (False, 0.0, 1.0),
           "ce+dice+boundary": (False, 0.7, 1.3)}
ALPHAS = [0.01, 0.7]


def ids(s):
    return "x".join(map(str, s))


# ---- the signed distance map -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.3, 0.7])
@pytest.mark.parametrize("shape", EDT_SHAPES, ids=ids)
def test_signed_edt_equals_oracle(shape, density, device):
    from medt_amd import ops
    N, Hh, Ww = shape
    t = BO.blob_targets(N, Hh, Ww, 2, density, 11 + EDT_SHAPES.index(shape))
    got = ops.signed_edt_sq(torch.from_numpy(t).to(device))
    want = torch.from_numpy(BO.sd2_batch(t))
    assert got.dtype == torch.int32 and tuple(got.shape) == shape
    assert torch.equal(got.cpu(), want)
    f = torch.from_numpy((t == 1))
    if f.any() and not f.all() and N == 1:
        assert (got.cpu()[f] <= -1).all() and (got.cpu()[~f] >= 1).all()


def test_signed_edt_empty_and_full_images_other_class_and_unaligned_out(device):
    from medt_amd import ops
    t = BO.blob_targets(3, 17, 19, 3, 0.3, 5)
    t[1][t[1] == 2] = 0                                               # image 1: no pixel of class 2
    t[2] = 2                                                          # image 2: nothing but class 2
    td = torch.from_numpy(t).to(device)
    got = ops.signed_edt_sq(td, fg=2)
    assert torch.equal(got.cpu(), torch.from_numpy(BO.sd2_batch(t, fg=2)))
    assert (got[0] != 0).all() and (got[1] == 0).all() and (got[2] == 0).all()
    assert torch.equal(ops.signed_edt_sq(td, fg=1).cpu(), torch.from_numpy(BO.sd2_batch(t, fg=1)))
    # ignored pixels are outside F whatever their value: ignore_index == fg leaves no foreground
    assert (ops.signed_edt_sq(td, fg=2, ignore_index=2) == 0).all()
    # (H,W) input; an out= view one int32 past a 16-byte boundary
    one = ops.signed_edt_sq(td[0], fg=2)
    assert tuple(one.shape) == (17, 19) and torch.equal(one, got[0])
    buf = torch.empty(3 * 17 * 19 + 4, dtype=torch.int32, device=device)
    view = buf[1:1 + 3 * 17 * 19].view(3, 17, 19)
    assert view.data_ptr() % 16 == 4
    assert ops.signed_edt_sq(td, fg=2, out=view) is view and torch.equal(view, got)
    t64 = BO.blob_targets(2, 64, 64, 2, 0.3, 6)
    buf = torch.empty(2 * 64 * 64 + 4, dtype=torch.int32, device=device)
    view = buf[3:3 + 2 * 64 * 64].view(2, 64, 64)
    ops.signed_edt_sq(torch.from_numpy(t64).to(device), out=view)
    assert torch.equal(view.cpu(), torch.from_numpy(BO.sd2_batch(t64)))


def test_signed_edt_argument_errors(device):
    import medt_amd
    from medt_amd import ops
    E = medt_amd.MedtError
    t = torch.zeros(2, 4, 4, dtype=torch.int64, device=device)
    with pytest.raises(E):
        ops.signed_edt_sq(t.int())
    with pytest.raises(E):
        ops.signed_edt_sq(t, fg=-1)
    with pytest.raises(E):
        ops.signed_edt_sq(t, out=torch.empty(2, 4, 4, dtype=torch.int64, device=device))
    with pytest.raises(E):
        ops.signed_edt_sq(t.reshape(2, 2, 2, 4))
    with pytest.raises(E, match="at most 4096"):
        ops.signed_edt_sq(torch.zeros(1, 1, 4097, dtype=torch.int64, device=device))


# ---- loss and gradient ---------------------------------------------------------------------------------------------------------------
_REF = {}


def case(shape):
    """(logits, target): randn * 3 logits; blobs of the classes 1 .. K-1, ~10 % ignored, two pixels per image out of range; the
    last image (of two or more) has no pixel of class 1."""
    key = ("case", shape)
    if key not in _REF:
        N, K, Hh, Ww = shape
        g = torch.Generator().manual_seed(21 + LOSS_SHAPES.index(shape))
        logits = torch.randn(N, K, Hh, Ww, generator=g) * 3
        t = BO.blob_targets(N, Hh, Ww, K, 0.3, 31 + LOSS_SHAPES.index(shape))
        if N > 1:
            t[N - 1][t[N - 1] == 1] = 0
        _REF[key] = (logits, torch.from_numpy(t), BO.sd2_batch(t))
    return _REF[key]


def class_weights(K):
    return torch.rand(K, generator=torch.Generator().manual_seed(11)) * 2 + 0.25


def reference(shape, name, alpha):
    """(loss64, B64, dlogits64 of loss * 1.7), once per case."""
    key = (shape, name, alpha)
    if key not in _REF:
        weighted, ce, dice = CONFIGS[name]
        logits, target, sd2 = case(shape)
        w = class_weights(shape[1]).double() if weighted else None
        z64 = logits.double().requires_grad_(True)
        loss64, B = BO.combined(z64, target, sd2, alpha, w, ce, dice)
        (loss64 * 1.7).backward()
        _REF[key] = (loss64.item(), B.item(), z64.grad)
    return _REF[key]


def run_product(shape, name, alpha, device):
    import medt_amd
    weighted, ce, dice = CONFIGS[name]
    logits, target, _ = case(shape)
    ld = logits.to(device).clone().requires_grad_(True)
    td = target.to(device)
    a = torch.full((1,), alpha, dtype=torch.float32, device=device)
    if name == "boundary":
        loss = medt_amd.boundary_loss(ld, td, a)
    else:
        w = class_weights(shape[1]).to(device) if weighted else None
        loss = medt_amd.seg_boundary_loss(ld, td, a, weight=w, ce=ce, dice=dice)
    (loss * 1.7).backward()
    return loss, ld.grad


@pytest.fixture()
def unchecked_targets():
    """What a captured step sees: out-of-range targets are counted and excluded, not raised on."""
    from medt_amd import ops
    old, ops.CHECK_TARGETS = ops.CHECK_TARGETS, False
    yield
    ops.CHECK_TARGETS = old


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=ids)
def test_boundary_loss_matches_float64(shape, name, alpha, device, unchecked_targets):
    loss64, B64, g64 = reference(shape, name, alpha)
    logits, target, _ = case(shape)
    loss, grad = run_product(shape, name, alpha, device)
    err_l, err_g = abs(loss.item() - loss64) / max(1.0, abs(loss64)), H.rel_err(grad, g64)
    print(f"boundary {shape} {name} alpha {alpha}: loss {loss.item():.7f} ref {loss64:.7f} rel {err_l:.2e}  dlogits rel_err {err_g:.2e}")
    assert err_l < 1e-5
    assert err_g < 1e-5
    K = shape[1]
    invalid = ((target == IGNORE) | (target < 0) | (target >= K)).unsqueeze(1).expand_as(logits)
    assert invalid.any() and (grad.cpu()[invalid] == 0).all()
    out = loss._medt_boundary_out.cpu()
    assert out[0].item() == loss.item() and out[2].item() == np.float32(alpha)
    assert abs(out[1].item() - B64) < 1e-5 * max(1.0, abs(B64))
    if name != "boundary":
        bad = int(((target != IGNORE) & ((target < 0) | (target >= K))).sum())
        assert loss._medt_ce_out[2].item() == bad


def test_out_of_range_targets_raise_outside_capture(device):
    import medt_amd
    logits, target, _ = case(LOSS_SHAPES[0])
    a = torch.full((1,), 0.01, device=device)
    with pytest.raises(medt_amd.MedtError, match="target value"):
        medt_amd.seg_boundary_loss(logits.to(device), target.to(device), a)


# ---- composition, determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wce+boundary", "ce+dice+boundary"])
def test_alpha_zero_is_seg_loss_bit_for_bit(name, device, unchecked_targets):
    """The accumulate path leaves the region term's bits alone: adding +-0 changes nothing."""
    import medt_amd
    shape = LOSS_SHAPES[3]
    weighted, ce, dice = CONFIGS[name]
    logits, target, _ = case(shape)
    w = class_weights(shape[1]).to(device) if weighted else None
    td = target.to(device)
    a = logits.to(device).clone().requires_grad_(True)
    b = logits.to(device).clone().requires_grad_(True)
    la = medt_amd.seg_boundary_loss(a, td, torch.zeros(1, device=device), weight=w, ce=ce, dice=dice)
    lb = medt_amd.seg_loss(b, td, weight=w, ce=ce, dice=dice)
    (la * 1.7).backward()
    (lb * 1.7).backward()
    assert torch.equal(la.detach(), lb.detach()) and torch.equal(a.grad, b.grad)
    assert la._medt_boundary_out[1].item() != 0 and la._medt_boundary_out[2].item() == 0      # B was computed, alpha read as 0
    assert torch.equal(la._medt_ce_out[:5], lb._medt_ce_out[:5])         # (the Dice coefficients behind them exist with Dice on)


def test_determinism(device, unchecked_targets):
    runs = [run_product(LOSS_SHAPES[3], "ce+dice+boundary", 0.7, device) for _ in range(2)]
    assert torch.equal(runs[0][0].detach(), runs[1][0].detach()) and torch.equal(runs[0][1], runs[1][1])
    from medt_amd import ops
    t = torch.from_numpy(BO.blob_targets(1, 33, 130, 2, 0.3, 3)).to(device)
    assert torch.equal(ops.signed_edt_sq(t), ops.signed_edt_sq(t))


def test_argument_errors(device):
    import medt_amd
    E = medt_amd.MedtError
    z = torch.zeros(2, 3, 4, 4, device=device)
    t = torch.zeros(2, 4, 4, dtype=torch.int64, device=device)
    a = torch.zeros(1, device=device)
    for fg in (-1, 3):
        with pytest.raises(E):
            medt_amd.boundary_loss(z, t, a, fg=fg)
    with pytest.raises(E):
        medt_amd.boundary_loss(z, t, torch.zeros(2, device=device))
    with pytest.raises(E):
        medt_amd.boundary_loss(z, t, a.double())
    with pytest.raises(E):
        medt_amd.boundary_loss(z, t.int(), a)
    with pytest.raises(E):
        medt_amd.boundary_loss(z.reshape(2, 3, 16), t.reshape(2, 16), a)
    with pytest.raises(E):
        medt_amd.seg_boundary_loss(z, t, a, ce=0.0, dice=0.0)
    with pytest.raises(E):
        medt_amd.seg_boundary_loss(z, t, a, weight=torch.ones(2, device=device))
    with pytest.raises(E):
        medt_amd.seg_boundary_loss(torch.zeros(2, 9, 4, 4, device=device), t, a, dice=1.0)
    medt_amd.seg_boundary_loss(z, t, 0.25, fg=2, dice=1.0)                                  # a number for alpha; the valid call


# ---- metrics.BoundaryLoss in the training step -----------------------------------------------------------------------------------------
def _as_device(t, device):
    """On the emulated device (pytest --emulate) CPU tensors stand in for device tensors."""
    if device.type == "cpu":
        from emu_device import DeviceTensor
        return t.as_subclass(DeviceTensor)
    return t.to(device)


def _schedule(device, use_graph, alphas):
    """TrainStep with BoundaryLoss(ce=1, dice=1) on gatedaxialunet at 64 px, 2 images: one step per entry of `alphas`, set_alpha()
    wherever the value changes (the eager run spends its FlatAdam adoption step in a rolled-back warm-up, as the captured run
    does: tests/test_seg_loss_gpu.py::_train_steps).  -> (losses, final state_dict, graphs captured)."""
    from metrics import BoundaryLoss
    from medt_amd.optim import FlatAdam
    from medt_amd.trainer import TrainStep
    from test_model_gpu import build
    st = H.seeded_state("gatedaxialunet", 64, 33)
    x, y = H.seeded_input(34, 2, 3, 64)
    y[:, 20:44, 16:40] = 1                                     # a blob among the noise: distances of more than one pixel
    xd, yd = _as_device(x, device), _as_device(y, device)
    model = build("gatedaxialunet", 64, device)
    model.load_state_dict(st)
    model.train()
    crit = BoundaryLoss(alpha=alphas[0], ce=1.0, dice=1.0).to(device)
    ptr = crit.alpha.data_ptr()
    opt = FlatAdam(list(model.parameters()), lr=1e-3, weight_decay=1e-5)
    step = TrainStep(model, opt, crit, use_graph=use_graph, warmup=2)
    if not use_graph:
        snap = step._snapshot()
        step._eager(xd, yd)
        step._restore(snap)
    losses, current = [], alphas[0]
    for a in alphas:
        if a != current:
            crit.set_alpha(a)
            current = a
        losses.append(step(xd, yd).item())
        step.check_targets()
    assert crit.alpha.data_ptr() == ptr and crit.alpha.item() == np.float32(alphas[-1])
    return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, len(step._graphs)


def test_train_step_follows_alpha_without_recapture(device):
    """Two steps at alpha 0.01, set_alpha(0.5), two more: the replayed run equals the eager one in all four losses and in the
    final state, over ONE captured graph; and the third loss is not what alpha 0.01 would have given (a third, eager run).
    (The emulated device has no graphs: the eager runs alone.)"""
    alphas = [0.01, 0.01, 0.5, 0.5]
    l0, s0, _ = _schedule(device, False, alphas)
    lc, _, _ = _schedule(device, False, [0.01, 0.01, 0.01])
    print(f"BoundaryLoss schedule, eager: {l0}; alpha held at 0.01: {lc}")
    assert all(v == v and abs(v) < 1e3 for v in l0)
    assert l0[:2] == lc[:2] and l0[2] != lc[2]
    if device.type != "cuda":
        return                                                 # no graphs to compare with, none to count
    l1, s1, graphs = _schedule(device, True, alphas)
    print(f"BoundaryLoss schedule, replayed: {l1}; graphs captured: {graphs}")
    assert l0 == l1, (l0, l1)
    diff = [k for k in s0 if not torch.equal(s0[k], s1[k])]
    assert not diff, diff[:5]
    assert graphs == 1
