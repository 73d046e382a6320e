"""The border term for touching objects on the device -- medt_amd.ops.object_edt2_sq (medt_object_edt2), medt_amd.border_loss and
medt_amd.seg_border_loss (medt_border_fwd / _bwd behind the unchanged medt_seg_loss_*, with ops.label in between),
metrics.BorderLoss in TrainStep -- against tests/border_oracle.py: the two distance maps torch.equal the oracle's (one SciPy
transform per object, held to brute force in tests/test_border_cpu.py), loss and gradient against float64 autograd over the
oracle's weight map.

Bounds: |loss - loss64| < 1e-5 * max(1, |loss64|) and rel_err(dlogits) < 1e-5 for every shape, configuration and w0: the bound
tests/test_boundary_gpu.py holds.  Worst case measured on the MI355X: loss 8.8e-8 relative ((1,3,16,16), dice+border, w0 10), dlogits
4.1e-7 ((4,2,16,16), dice+border, w0 0.5); no case needed a bound of its own.  The same file runs on the CPU lane emulator: `-m gpu --emulate` (without the replayed halves
of the TrainStep tests: the emulated device has no graphs)."""
import numpy as np
import pytest
import torch

import border_oracle as RO
import boundary_oracle as BO
import helpers as H
from test_border_cpu import EDT_SHAPES, DENSITIES, edt_cases, hand_cases

pytestmark = pytest.mark.gpu

IGNORE = RO.IGNORE
NONE = RO.NONE
# N, K, H, W: K = 2 and 3; N = 1, 3, 4; 16^2, 64^2 and 33 x 130 (ragged against the 256-pixel workgroups and the row tile)
LOSS_SHAPES = [(1, 3, 16, 16), (3, 2, 64, 64), (4, 3, 33, 130), (4, 2, 16, 16)]
# name -> (class weights?, ce, dice, connectivity)
CONFIGS = {"border": (False, 0.0, 0.0, 8), "wce+border": (True, 1.0, 0.0, 8), "dice+border": (False, 0.0, 1.0, 4),
           "ce+dice+border": (False, 0.7, 1.3, 8)}
W0S = [10.0, 0.5]
SIGMA = 3.0


def ids(s):
    return "x".join(map(str, s))


# ---- the two distance maps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EDT_SHAPES, ids=ids)
def test_object_edt2_equals_oracle(shape, device):
    """0, 1, 2 and many objects at every shape; the same bits on a second run."""
    from medt_amd import ops
    i = EDT_SHAPES.index(shape)
    for j, d in enumerate(DENSITIES):
        lab = RO.blob_labels(*shape, d, 100 + 10 * i + j)
        ld = torch.from_numpy(lab).to(device)
        d1, d2 = ops.object_edt2_sq(ld)
        w1, w2 = RO.edt2_batch(lab)
        assert d1.dtype == d2.dtype == torch.int32 and tuple(d1.shape) == tuple(d2.shape) == shape
        assert torch.equal(d1.cpu(), torch.from_numpy(w1)) and torch.equal(d2.cpu(), torch.from_numpy(w2)), d
        assert ((d1 == 0) == (ld > 0)).all() and (d2 >= d1).all()
        again = ops.object_edt2_sq(ld)
        assert torch.equal(again[0], d1) and torch.equal(again[1], d2)


def test_object_edt2_hand_cases_few_objects_and_unaligned_out(device):
    from medt_amd import ops
    for lab, points, whole in hand_cases():
        d1, d2 = (d.cpu().numpy() for d in ops.object_edt2_sq(torch.from_numpy(lab).to(device)))     # (H,W) input
        assert d1.shape == lab.shape
        for (y, x), (w1, w2) in points.items():
            assert (d1[y, x], d2[y, x]) == (w1, w2), (lab, y, x)
        if whole is not None:
            assert np.array_equal(d1, whole[0]) and np.array_equal(d2, whole[1])
    for i, lab in enumerate(edt_cases()[-5:]):                        # the tall maps; exactly one / exactly two objects per image
        d1, d2 = ops.object_edt2_sq(torch.from_numpy(lab).to(device))
        w1, w2 = RO.edt2_batch(lab)
        assert torch.equal(d1.cpu(), torch.from_numpy(w1)) and torch.equal(d2.cpu(), torch.from_numpy(w2)), lab.shape
        assert i < 3 or bool((d2 == NONE).all()) == bool(lab.max() < 2)
    # out= views one and three int32 past a 16-byte boundary
    for shape, seed in (((3, 17, 19), 5), ((2, 64, 64), 6)):
        lab = RO.blob_labels(*shape, 0.4, seed)
        n = lab.size
        b1, b2 = (torch.empty(n + 4, dtype=torch.int32, device=device) for _ in range(2))
        v1, v2 = b1[1:1 + n].view(shape), b2[3:3 + n].view(shape)
        assert v1.data_ptr() % 16 == 4 and v2.data_ptr() % 16 == 12
        got = ops.object_edt2_sq(torch.from_numpy(lab).to(device), out=(v1, v2))
        assert got[0] is v1 and got[1] is v2
        w1, w2 = RO.edt2_batch(lab)
        assert torch.equal(v1.cpu(), torch.from_numpy(w1)) and torch.equal(v2.cpu(), torch.from_numpy(w2))


def test_object_edt2_after_label_at_both_connectivities(device):
    """The chain the loss node runs: {target == fg} -> ops.label -> ops.object_edt2_sq, against SciPy's labels and transforms."""
    from medt_amd import ops
    t = BO.blob_targets(2, 33, 130, 3, 0.3, 41)
    mask = torch.from_numpy(((t == 1) & (t != IGNORE)).astype(np.uint8)).to(device)
    for conn in (4, 8):
        lab, _ = ops.label(mask, conn)
        d1, d2 = ops.object_edt2_sq(lab)
        w1, w2 = RO.edt2_batch(RO.label_targets(t, 1, connectivity=conn))
        assert torch.equal(d1.cpu(), torch.from_numpy(w1)) and torch.equal(d2.cpu(), torch.from_numpy(w2))


def test_object_edt2_argument_errors(device):
    import medt_amd
    from medt_amd import ops
    E = medt_amd.MedtError
    lab = torch.zeros(2, 4, 4, dtype=torch.int32, device=device)
    with pytest.raises(E):
        ops.object_edt2_sq(lab.long())
    with pytest.raises(E):
        ops.object_edt2_sq(lab, out=torch.empty(2, 4, 4, dtype=torch.int32, device=device))
    with pytest.raises(E):
        ops.object_edt2_sq(lab, out=(torch.empty(2, 4, 4, dtype=torch.int64, device=device),) * 2)
    with pytest.raises(E):
        ops.object_edt2_sq(lab.reshape(2, 2, 2, 4))
    with pytest.raises(E, match="at most 4096"):
        ops.object_edt2_sq(torch.zeros(1, 1, 4097, dtype=torch.int32, device=device))


# ---- loss and gradient ---------------------------------------------------------------------------------------------------------------
_REF = {}


def case(shape):
    """(logits, target): randn * 3 logits; blobs of the classes 1 .. K-1, ~10 % ignored, two pixels per image out of range; the
    last image (of two or more) holds one block of class 1 and nothing else: fewer than two objects, e = 0 everywhere."""
    key = ("case", shape)
    if key not in _REF:
        N, K, Hh, Ww = shape
        g = torch.Generator().manual_seed(21 + LOSS_SHAPES.index(shape))
        logits = torch.randn(N, K, Hh, Ww, generator=g) * 3
        t = BO.blob_targets(N, Hh, Ww, K, 0.3, 31 + LOSS_SHAPES.index(shape))
        if N > 1:
            t[N - 1] = 0
            t[N - 1, 2:7, 3:9] = 1
        _REF[key] = (logits, torch.from_numpy(t))
    return _REF[key]


def weight_map(shape, conn):
    key = ("e", shape, conn)
    if key not in _REF:
        t = case(shape)[1].numpy()
        _REF[key] = RO.weight_e(t, *RO.edt2_batch(RO.label_targets(t, 1, connectivity=conn)), SIGMA)
    return _REF[key]


def class_weights(K):
    return torch.rand(K, generator=torch.Generator().manual_seed(11)) * 2 + 0.25


def reference(shape, name, w0):
    """(loss64, R64, dlogits64 of loss * 1.7), once per case."""
    key = (shape, name, w0)
    if key not in _REF:
        weighted, ce, dice, conn = CONFIGS[name]
        logits, target = case(shape)
        w = class_weights(shape[1]).double() if weighted else None
        z64 = logits.double().requires_grad_(True)
        loss64, R = RO.combined(z64, target, weight_map(shape, conn), w0, w, ce, dice)
        (loss64 * 1.7).backward()
        _REF[key] = (loss64.item(), R.item(), z64.grad)
    return _REF[key]


def run_product(shape, name, w0, device):
    import medt_amd
    weighted, ce, dice, conn = CONFIGS[name]
    logits, target = case(shape)
    ld = logits.to(device).clone().requires_grad_(True)
    td = target.to(device)
    a = torch.full((1,), w0, dtype=torch.float32, device=device)
    if name == "border":
        loss = medt_amd.border_loss(ld, td, a, sigma=SIGMA, connectivity=conn)
    else:
        w = class_weights(shape[1]).to(device) if weighted else None
        loss = medt_amd.seg_border_loss(ld, td, a, sigma=SIGMA, weight=w, ce=ce, dice=dice, connectivity=conn)
    (loss * 1.7).backward()
    return loss, ld.grad


@pytest.fixture()
def unchecked_targets():
    """What a captured step sees: out-of-range targets are counted and excluded, not raised on."""
    from medt_amd import ops
    old, ops.CHECK_TARGETS = ops.CHECK_TARGETS, False
    yield
    ops.CHECK_TARGETS = old


@pytest.mark.parametrize("w0", W0S)
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=ids)
def test_border_loss_matches_float64(shape, name, w0, device, unchecked_targets):
    loss64, R64, g64 = reference(shape, name, w0)
    logits, target = case(shape)
    e = weight_map(shape, CONFIGS[name][3])
    assert (e > 1e-3).sum() >= 5 and R64 > 1e-4                       # the term is there: pixels between two objects
    loss, grad = run_product(shape, name, w0, device)
    err_l, err_g = abs(loss.item() - loss64) / max(1.0, abs(loss64)), H.rel_err(grad, g64)
    print(f"border {shape} {name} w0 {w0}: loss {loss.item():.7f} ref {loss64:.7f} rel {err_l:.2e}  dlogits rel_err {err_g:.2e}")
    assert err_l < 1e-5
    assert err_g < 1e-5
    K = shape[1]
    invalid = ((target == IGNORE) | (target < 0) | (target >= K)).unsqueeze(1).expand_as(logits)
    assert invalid.any() and (grad.cpu()[invalid] == 0).all()
    out = loss._medt_border_out.cpu()
    assert out[0].item() == loss.item() and out[2].item() == np.float32(w0)
    assert abs(out[1].item() - R64) < 1e-5 * max(1.0, abs(R64))
    if name == "border":                                              # the term alone: no gradient where e is 0
        assert (grad.cpu()[(e == 0).unsqueeze(1).expand_as(logits)] == 0).all()
        if shape[0] > 1:
            assert (grad[-1] == 0).all()                              # the image with one object
    else:
        bad = int(((target != IGNORE) & ((target < 0) | (target >= K))).sum())
        assert loss._medt_ce_out[2].item() == bad


def test_fewer_than_two_objects_contribute_exactly_nothing(device):
    """One object, no object, everything one object: R == 0 and the gradient is 0 everywhere, bit for bit; with a region term
    loss and gradient are seg_loss's."""
    import medt_amd
    g = torch.Generator().manual_seed(8)
    logits = torch.randn(3, 2, 16, 16, generator=g) * 3
    t = torch.zeros(3, 16, 16, dtype=torch.int64)
    t[0, 2:7, 3:9] = 1
    t[2] = 1
    td = t.to(device)
    a = torch.full((1,), 10.0, device=device)
    ld = logits.to(device).clone().requires_grad_(True)
    loss = medt_amd.border_loss(ld, td, a)
    loss.backward()
    assert loss.item() == 0.0 and loss._medt_border_out[1].item() == 0.0 and (ld.grad == 0).all()
    t2 = torch.zeros(1, 16, 16, dtype=torch.int64)
    t2[0, 2:7, 3:6] = t2[0, 2:7, 8:12] = 1                     # two objects ... that ignore_index == fg takes out of F
    assert medt_amd.border_loss(logits[:1].to(device), t2.to(device), a).item() > 0.0
    assert medt_amd.border_loss(logits[:1].to(device), t2.to(device), a, ignore_index=1).item() == 0.0
    x = logits.to(device).clone().requires_grad_(True)
    y = logits.to(device).clone().requires_grad_(True)
    lx = medt_amd.seg_border_loss(x, td, a, dice=1.0)
    ly = medt_amd.seg_loss(y, td, dice=1.0)
    lx.backward()
    ly.backward()
    assert torch.equal(lx.detach(), ly.detach()) and torch.equal(x.grad, y.grad)


def test_out_of_range_targets_raise_outside_capture(device):
    import medt_amd
    logits, target = case(LOSS_SHAPES[1])
    a = torch.full((1,), 10.0, device=device)
    with pytest.raises(medt_amd.MedtError, match="target value"):
        medt_amd.seg_border_loss(logits.to(device), target.to(device), a)


# ---- composition, determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wce+border", "ce+dice+border"])
def test_w0_zero_is_seg_loss_bit_for_bit(name, device, unchecked_targets):
    """The accumulate path leaves the region term's bits alone: adding +-0 changes nothing."""
    import medt_amd
    shape = LOSS_SHAPES[2]
    weighted, ce, dice, conn = CONFIGS[name]
    logits, target = case(shape)
    w = class_weights(shape[1]).to(device) if weighted else None
    td = target.to(device)
    a = logits.to(device).clone().requires_grad_(True)
    b = logits.to(device).clone().requires_grad_(True)
    la = medt_amd.seg_border_loss(a, td, torch.zeros(1, device=device), sigma=SIGMA, weight=w, ce=ce, dice=dice, connectivity=conn)
    lb = medt_amd.seg_loss(b, td, weight=w, ce=ce, dice=dice)
    (la * 1.7).backward()
    (lb * 1.7).backward()
    assert torch.equal(la.detach(), lb.detach()) and torch.equal(a.grad, b.grad)
    assert la._medt_border_out[1].item() > 0 and la._medt_border_out[2].item() == 0          # R was computed, w0 read as 0
    assert torch.equal(la._medt_ce_out[:5], lb._medt_ce_out[:5])


def test_determinism(device, unchecked_targets):
    runs = [run_product(LOSS_SHAPES[2], "ce+dice+border", 10.0, device) for _ in range(2)]
    assert torch.equal(runs[0][0].detach(), runs[1][0].detach()) and torch.equal(runs[0][1], runs[1][1])


def test_argument_errors(device):
    import medt_amd
    E = medt_amd.MedtError
    z = torch.zeros(2, 3, 4, 4, device=device)
    t = torch.zeros(2, 4, 4, dtype=torch.int64, device=device)
    a = torch.zeros(1, device=device)
    for fg in (-1, 3):
        with pytest.raises(E):
            medt_amd.border_loss(z, t, a, fg=fg)
    for sigma in (0.0, -1.0, float("inf")):
        with pytest.raises(E, match="sigma"):
            medt_amd.border_loss(z, t, a, sigma=sigma)
        with pytest.raises(E, match="sigma"):
            medt_amd.seg_border_loss(z, t, a, sigma=sigma)
    with pytest.raises(E, match="connectivity"):
        medt_amd.seg_border_loss(z, t, a, connectivity=6)
    with pytest.raises(E):
        medt_amd.border_loss(z, t, torch.zeros(2, device=device))
    with pytest.raises(E):
        medt_amd.border_loss(z, t, a.double())
    with pytest.raises(E):
        medt_amd.border_loss(z, t.int(), a)
    with pytest.raises(E):
        medt_amd.border_loss(z.reshape(2, 3, 16), t.reshape(2, 16), a)
    with pytest.raises(E):
        medt_amd.seg_border_loss(z, t, a, ce=0.0, dice=0.0)
    with pytest.raises(E):
        medt_amd.seg_border_loss(z, t, a, weight=torch.ones(2, device=device))
    with pytest.raises(E):
        medt_amd.seg_border_loss(torch.zeros(2, 9, 4, 4, device=device), t, a, dice=1.0)
    medt_amd.seg_border_loss(z, t, 0.25, fg=2, dice=1.0, connectivity=4)                    # a number for w0; the valid call


# ---- metrics.BorderLoss in the training step -------------------------------------------------------------------------------------------
def _as_device(t, device):
    """On the emulated device (pytest --emulate) CPU tensors stand in for device tensors."""
    if device.type == "cpu":
        from emu_device import DeviceTensor
        return t.as_subclass(DeviceTensor)
    return t.to(device)


def _schedule(device, model_name, S, use_graph, w0s):
    """TrainStep with BorderLoss(ce=1, dice=1) on 2 images: one step per entry of `w0s`, set_w0() wherever the value changes (the
    eager run spends its FlatAdam adoption step in a rolled-back warm-up, as the captured run does:
    tests/test_seg_loss_gpu.py::_train_steps).  -> (losses, final state_dict, graphs captured)."""
    from metrics import BorderLoss
    from medt_amd.optim import FlatAdam
    from medt_amd.trainer import TrainStep
    from test_model_gpu import build
    st = H.seeded_state(model_name, S, 33)
    x, y = H.seeded_input(34, 2, 3, S)
    y[:] = 0                                                   # three glands a few pixels apart, one of them touching the frame
    q = S // 8
    y[:, q:3 * q, q:3 * q - 1] = 1
    y[:, q:3 * q, 3 * q + 1:5 * q] = 1
    y[:, 3 * q + 2:S, 2 * q:6 * q] = 1
    xd, yd = _as_device(x, device), _as_device(y, device)
    model = build(model_name, S, device)
    model.load_state_dict(st)
    model.train()
    crit = BorderLoss(w0=w0s[0], ce=1.0, dice=1.0).to(device)
    ptr = crit.w0.data_ptr()
    opt = FlatAdam(list(model.parameters()), lr=1e-3, weight_decay=1e-5)
    step = TrainStep(model, opt, crit, use_graph=use_graph, warmup=2)
    if not use_graph:
        snap = step._snapshot()
        step._eager(xd, yd)
        step._restore(snap)
    losses, current = [], w0s[0]
    for a in w0s:
        if a != current:
            crit.set_w0(a)
            current = a
        losses.append(step(xd, yd).item())
        step.check_targets()
    assert crit.w0.data_ptr() == ptr and crit.w0.item() == np.float32(w0s[-1])
    return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, len(step._graphs)


@pytest.mark.parametrize("model_name,S", [("gatedaxialunet", 64), ("MedT", 128)])
def test_train_step_replayed_equals_eager_and_follows_w0(model_name, S, device):
    """Two steps at w0 10, set_w0(2), two more: the replayed run equals the eager one in all four losses and in the final state,
    over ONE captured graph; and the third loss is not what w0 10 would have given (a third, eager run).
    (The emulated device has no graphs: the eager runs alone.)"""
    w0s = [10.0, 10.0, 2.0, 2.0]
    l0, s0, _ = _schedule(device, model_name, S, False, w0s)
    lc, _, _ = _schedule(device, model_name, S, False, [10.0, 10.0, 10.0])
    print(f"BorderLoss {model_name} {S}, eager: {l0}; w0 held at 10: {lc}")
    assert all(v == v and abs(v) < 1e3 for v in l0)
    assert l0[:2] == lc[:2] and l0[2] != lc[2]
    if device.type != "cuda":
        return                                                 # no graphs to compare with, none to count
    l1, s1, graphs = _schedule(device, model_name, S, True, w0s)
    print(f"BorderLoss {model_name} {S}, replayed: {l1}; graphs captured: {graphs}")
    assert l0 == l1, (l0, l1)
    diff = [k for k in s0 if not torch.equal(s0[k], s1[k])]
    assert not diff, diff[:5]
    assert graphs == 1
