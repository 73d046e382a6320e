"""medt_amd.seg_loss -- class-weighted cross entropy + per-image soft Dice as one HIP kernel pair (medt_seg_loss_fwd / _bwd) --
against a float64 CPU restatement: F.cross_entropy(z64, t, weight=w64, ignore_index=...) is literally what the reference's
LogNLLLoss calls (metrics.py:19), the Dice term is written out from its definition and differentiated by autograd.

Bounds: |loss - loss64| < 1e-5 and rel_err(dlogits) < 1e-5, the bounds tests/test_ops_gpu.py::test_cross_entropy holds, for every
shape (the 130 x 130 case needed no bound of its own).  The same file runs on the CPU lane emulator: `-m gpu --emulate`."""
import pytest
import torch
import torch.nn.functional as F

import helpers as H

pytestmark = pytest.mark.gpu

IGNORE = -100
# HW = 323: two workgroups per image, the second ragged (test_cross_entropy's shape) | an image smaller than one workgroup, K = 3 |
# exactly one full workgroup, K = 5 | K = 8, the Dice limit | 67 workgroups per image: more than the 64 lanes of a finalize wave
SHAPES = [(3, 2, 17, 19), (2, 3, 5, 7), (1, 5, 16, 16), (2, 8, 9, 9), (2, 2, 130, 130)]
# name -> (class weights?, ce, dice); "wzero": one class weighs 0
CONFIGS = {"wce": (True, 1.0, 0.0), "dice": (False, 0.0, 1.0), "both": (True, 0.7, 1.3), "wzero": (True, 1.0, 0.5)}


def ref_loss(z64, t, w64, ce, dice, eps=1.0, ignore=IGNORE):
    """The issue's formulas in float64 (targets in range or `ignore`)."""
    N, K = z64.shape[:2]
    total = z64.new_zeros(())
    if ce:
        total = total + ce * F.cross_entropy(z64, t, weight=w64, ignore_index=ignore)
    if dice:
        p = torch.softmax(z64, dim=1)
        valid = (t != ignore).unsqueeze(1).to(z64.dtype)                                     # (N,1,H,W)
        onehot = F.one_hot(t.clamp(0, K - 1), K).movedim(-1, 1).to(z64.dtype) * valid       # (N,K,H,W)
        dims = tuple(range(2, z64.dim()))
        inter, psum, tsum = (p * onehot).sum(dims), (p * valid).sum(dims), onehot.sum(dims)
        total = total + dice * (1.0 - ((2 * inter + eps) / (psum + tsum + eps)).mean())
    return total


def make_case(shape, seed):
    """logits randn * 3; targets: random, ~10 % ignored, class K-1 absent from image 0, the last image (of two or more) entirely
    ignored -- its Dice terms come from eps alone and its gradients are exactly 0."""
    N, K, Hh, Ww = shape
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, K, Hh, Ww, generator=g) * 3
    target = torch.randint(0, K, (N, Hh, Ww), generator=g)
    target[torch.rand(N, Hh, Ww, generator=g) < 0.1] = IGNORE
    target[0][target[0] == K - 1] = 0
    if N > 1:
        target[N - 1] = IGNORE
    return logits, target


def class_weights(K, name, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(K, generator=g) * 2 + 0.25
    if name == "wzero":
        w[K - 1] = 0.0               # (class K-1: image 0 holds none of it, the other classes keep the denominator positive)
    return w


_REF = {}


def reference(shape, name):
    """(logits, target, weight, loss64, dlogits64 of loss * 1.7), computed once per case."""
    key = (shape, name)
    if key not in _REF:
        weighted, ce, dice = CONFIGS[name]
        logits, target = make_case(shape, 7 + SHAPES.index(shape))
        w = class_weights(shape[1], name, 11) if weighted else None
        z64 = logits.double().requires_grad_(True)
        loss64 = ref_loss(z64, target, None if w is None else w.double(), ce, dice)
        (loss64 * 1.7).backward()
        _REF[key] = (logits, target, w, loss64.item(), z64.grad)
    return _REF[key]


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seg_loss_matches_float64(shape, name, device):
    import medt_amd
    _, ce, dice = CONFIGS[name]
    logits, target, w, loss64, g64 = reference(shape, name)
    ld = logits.to(device).clone().requires_grad_(True)
    td = target.to(device)
    loss = medt_amd.seg_loss(ld, td, weight=None if w is None else w.to(device), ce=ce, dice=dice)
    (loss * 1.7).backward()
    err_l, err_g = abs(loss.item() - loss64), H.rel_err(ld.grad, g64)
    print(f"seg_loss {shape} {name}: loss {loss.item():.7f} ref {loss64:.7f} |diff| {err_l:.2e}  dlogits rel_err {err_g:.2e}")
    assert err_l < 1e-5
    assert err_g < 1e-5
    # pixels that are not valid: exactly 0 in every class (the whole last image where it is ignored)
    invalid = (target == IGNORE).unsqueeze(1).expand_as(logits)
    assert invalid.any() and (ld.grad.cpu()[invalid] == 0).all()
    out = loss._medt_ce_out.cpu()
    assert out[2].item() == 0 and abs(out[0].item() - loss.item()) == 0
    if w is None:
        assert out[1].item() == float((target != IGNORE).sum())              # without weights: the pixel count
    else:
        assert abs(out[1].item() - w[target[target != IGNORE]].double().sum().item()) < 1e-5 * out[1].item()


def test_plain_random_targets_and_eps(device):
    """No ignored pixel, every class in every image, eps away from its default."""
    import medt_amd
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(3, 4, 17, 19, generator=g) * 3
    target = torch.randint(0, 4, (3, 17, 19), generator=g)
    w = class_weights(4, "wce", 5)
    z64 = logits.double().requires_grad_(True)
    loss64 = ref_loss(z64, target, w.double(), 0.5, 2.0, eps=0.25)
    (loss64 * 1.7).backward()
    ld = logits.to(device).clone().requires_grad_(True)
    loss = medt_amd.seg_loss(ld, target.to(device), weight=w.to(device), ce=0.5, dice=2.0, eps=0.25)
    (loss * 1.7).backward()
    assert abs(loss.item() - loss64.item()) < 1e-5
    assert H.rel_err(ld.grad, z64.grad) < 1e-5
    out = loss._medt_ce_out.cpu().double()
    ce64 = F.cross_entropy(logits.double(), target, weight=w.double()).item()
    assert abs(out[3].item() - ce64) < 1e-5 and abs(0.5 * out[3].item() + 2.0 * out[4].item() - loss64.item()) < 1e-5


def test_out_of_range_targets_are_counted_and_raise(device):
    import medt_amd
    from medt_amd import ops
    logits, target, w, _, _ = reference(SHAPES[0], "both")
    bad = target.clone()
    bad[1, 3, :4] = 255
    bad[1, 5, 2] = -7
    ld = logits.to(device).clone().requires_grad_(True)
    with pytest.raises(medt_amd.MedtError, match="5 target value"):
        medt_amd.seg_loss(ld, bad.to(device), weight=w.to(device), ce=0.7, dice=1.3)
    old, ops.CHECK_TARGETS = ops.CHECK_TARGETS, False              # what a captured step sees: counted, excluded, not raised
    try:
        loss = medt_amd.seg_loss(ld, bad.to(device), weight=w.to(device), ce=0.7, dice=1.3)
    finally:
        ops.CHECK_TARGETS = old
    assert loss._medt_ce_out[2].item() == 5
    (loss * 1.7).backward()
    masked = bad.clone()
    masked[(bad == 255) | (bad == -7)] = IGNORE                    # excluded like ignored pixels
    z64 = logits.double().requires_grad_(True)
    loss64 = ref_loss(z64, masked, w.double(), 0.7, 1.3)
    (loss64 * 1.7).backward()
    assert abs(loss.item() - loss64.item()) < 1e-5 and H.rel_err(ld.grad, z64.grad) < 1e-5
    assert (ld.grad.cpu()[(masked == IGNORE).unsqueeze(1).expand_as(logits)] == 0).all()


def test_unit_weights_reduce_to_cross_entropy(device):
    import medt_amd
    logits, target, _, _, _ = reference(SHAPES[0], "wce")
    td = target.to(device)
    a = logits.to(device).clone().requires_grad_(True)
    b = logits.to(device).clone().requires_grad_(True)
    la = medt_amd.seg_loss(a, td, weight=torch.ones(2, device=device), dice=0.0)
    lb = medt_amd.cross_entropy(b, td)
    (la * 1.7).backward()
    (lb * 1.7).backward()
    assert abs(la.item() - lb.item()) < 1e-6
    assert H.rel_err(a.grad, b.grad) < 1e-6
    c = logits.to(device).clone().requires_grad_(True)
    lc = medt_amd.seg_loss(c, td)                                   # no weight at all: the same number
    assert abs(lc.item() - lb.item()) < 1e-6


def test_weighted_ce_alone_takes_any_class_count(device):
    import medt_amd
    g = torch.Generator().manual_seed(9)
    for K in (1, 11):
        logits = torch.randn(2, K, 6, 7, generator=g) * 3
        target = torch.randint(0, K, (2, 6, 7), generator=g)
        w = torch.rand(K, generator=g) + 0.5
        z64 = logits.double().requires_grad_(True)
        loss64 = F.cross_entropy(z64, target, weight=w.double())
        (loss64 * 1.7).backward()
        ld = logits.to(device).clone().requires_grad_(True)
        loss = medt_amd.seg_loss(ld, target.to(device), weight=w.to(device))
        (loss * 1.7).backward()
        assert abs(loss.item() - loss64.item()) < 1e-5
        assert H.rel_err(ld.grad, z64.grad) < 1e-5


def test_lognllloss_with_class_weights(device):
    """The module surface: LogNLLLoss(weight=w) is F.cross_entropy(weight=w), as in the reference (metrics.py:19)."""
    from metrics import DiceCELoss, LogNLLLoss
    logits, target, w, _, _ = reference(SHAPES[0], "wce")
    z64 = logits.double().requires_grad_(True)
    loss64 = F.cross_entropy(z64, target, weight=w.double(), ignore_index=IGNORE)
    (loss64 * 1.7).backward()
    crit = LogNLLLoss(weight=w).to(device)
    ld = logits.to(device).clone().requires_grad_(True)
    loss = crit(ld, target.to(device))
    (loss * 1.7).backward()
    assert abs(loss.item() - loss64.item()) < 1e-5
    assert H.rel_err(ld.grad, z64.grad) < 1e-5
    both = DiceCELoss(weight=w.tolist(), ce=0.7, dice=1.3).to(device)
    assert "weight" in dict(both.named_buffers())
    assert abs(both(logits.to(device), target.to(device)).item() - reference(SHAPES[0], "both")[3]) < 1e-5


def test_determinism(device):
    import medt_amd
    logits, target, w, _, _ = reference(SHAPES[4], "both")
    runs = []
    for _ in range(2):
        ld = logits.to(device).clone().requires_grad_(True)
        loss = medt_amd.seg_loss(ld, target.to(device), weight=w.to(device), ce=0.7, dice=1.3)
        (loss * 1.7).backward()
        runs.append((loss.detach().clone(), ld.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_argument_errors(device):
    import medt_amd
    E = medt_amd.MedtError
    t1 = torch.zeros(2, 4, 4, dtype=torch.int64, device=device)
    for K in (1, 9):                                                # Dice: 2 <= K <= 8
        with pytest.raises(E):
            medt_amd.seg_loss(torch.zeros(2, K, 4, 4, device=device), t1, dice=1.0)
    z = torch.zeros(2, 3, 4, 4, device=device)
    with pytest.raises(E):
        medt_amd.seg_loss(z, t1, weight=torch.ones(2, device=device))                         # wrong length
    with pytest.raises(E):
        medt_amd.seg_loss(z, t1, weight=torch.ones(3, dtype=torch.float64, device=device))    # wrong dtype
    other = torch.device("cpu") if device.type == "cuda" else torch.device("meta")
    with pytest.raises(E):
        medt_amd.seg_loss(z, t1, weight=torch.ones(3, device=other))                          # wrong device
    with pytest.raises(E):
        medt_amd.seg_loss(z, t1, eps=-1.0)
    with pytest.raises(E):
        medt_amd.seg_loss(z, t1.int())
    medt_amd.seg_loss(z, t1, weight=torch.ones(3, device=device), dice=1.0)                   # and the valid call goes through


def _as_device(t, device):
    """On the emulated device (pytest --emulate) CPU tensors stand in for device tensors."""
    if device.type == "cpu":
        from emu_device import DeviceTensor
        return t.as_subclass(DeviceTensor)
    return t.to(device)


_STEPS = {}


def _train_steps(name, S, device, use_graph):
    """Three steps of TrainStep with DiceCELoss(weight=[1, 3]) on N = 2 seeded images, after
    tests/test_model_gpu.py::test_graphed_train_step_equals_eager (the eager run spends its FlatAdam adoption step in a
    rolled-back warm-up, as the captured run does); then one step on a mask that holds a 255.  check_targets() is silent on the
    good targets and raises after the bad step -- a replay cannot raise, the count is read afterwards; the eager step raises
    itself.  -> (losses, state after the first step, state after the third, float64 loss of the initial forward's logits);
    computed once per (model, mode)."""
    key = (name, S, use_graph)
    if key in _STEPS:
        return _STEPS[key]
    import medt_amd
    from metrics import DiceCELoss
    from medt_amd.optim import FlatAdam
    from medt_amd.trainer import TrainStep
    from test_model_gpu import build
    st = H.seeded_state(name, S, 33)
    x, y = H.seeded_input(34, 2, 3, S)
    ybad = y.clone()
    ybad[1, 2, 3] = 255
    xd, yd, ybd = _as_device(x, device), _as_device(y, device), _as_device(ybad, device)
    model = build(name, S, device)
    model.load_state_dict(st)
    model.train()
    with torch.no_grad():
        z64 = model(xd).double().cpu()
    want = ref_loss(z64, y, torch.tensor([1.0, 3.0], dtype=torch.float64), 1.0, 1.0).item()
    model = build(name, S, device)
    model.load_state_dict(st)
    model.train()
    crit = DiceCELoss(weight=[1.0, 3.0]).to(device)
    opt = FlatAdam(list(model.parameters()), lr=1e-3, weight_decay=1e-5)
    step = TrainStep(model, opt, crit, use_graph=use_graph, warmup=2)
    if not use_graph:
        snap = step._snapshot()
        step._eager(xd, yd)
        step._restore(snap)
    losses = [step(xd, yd).item()]
    step.check_targets()                                       # good targets: silent
    first = {k: v.detach().clone() for k, v in model.state_dict().items()}
    losses += [step(xd, yd).item() for _ in range(2)]
    step.check_targets()
    final = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if use_graph:
        step(xd, ybd)
        with pytest.raises(medt_amd.MedtError):
            step.check_targets()
    else:
        with pytest.raises(medt_amd.MedtError):
            step(xd, ybd)
    assert any((first[k].cpu() != st[k]).any() for k in first if first[k].is_floating_point() and k in st)     # it did train
    _STEPS[key] = (losses, first, final, want)
    return _STEPS[key]


def test_dice_ce_in_the_train_step_loss_and_check_targets(device):
    """gatedaxialunet at 64 px, N = 2: the first step's loss is the float64 value of the eager forward's logits, eager and
    replayed; check_targets() is silent on good targets and reports a mask left at 255 (see _train_steps).  (The emulated device
    has no graphs: the eager run alone.)"""
    for use_graph in ((False, True) if device.type == "cuda" else (False,)):
        losses, _, _, want = _train_steps("gatedaxialunet", 64, device, use_graph)
        print(f"DiceCELoss step, use_graph={use_graph}: losses {losses}, float64 of the first {want:.7f}")
        assert abs(losses[0] - want) < 1e-5, (use_graph, losses[0], want)
        assert all(v == v and abs(v) < 1e3 for v in losses)


@pytest.mark.parametrize("name,S", [("gatedaxialunet", 64), ("MedT", 128)])
def test_dice_ce_graphed_train_step_equals_eager(name, S, device):
    """The replayed step with DiceCELoss IS the eager step: losses and the state after one and after three steps are
    torch.equal between use_graph=False and True.

    MedT 128 is the model of test_graphed_train_step_equals_eager: every reduction of its step has a fixed order.
    gatedaxialunet 64 is the smallest gated network the fixtures support.  Its 16-px and shorter layers take the generic two-pass attention
    backward, whose wrapped-diagonal pass used to end in LDS float atomics on the relative-table gradients (~1e-7 run to run,
    amplified by Adam and training-mode BatchNorm).  Measured on the MI355X with those atomics: 7 of 502 state tensors differed
    after the first step, 340 after the third; losses eager [3.347581386566162, 1.4833853244781494, 1.1750959157943726],
    replayed [3.347581386566162, 1.4833852052688599, 1.1750916242599487].  That pass now hands its sums over in a fixed order
    (attn_bwd_kernel in axial_core.hip); the loss kernels themselves never had atomics (test_determinism)."""
    if device.type != "cuda":
        pytest.skip("emulated device: no graphs to compare with")
    l0, f0, s0, _ = _train_steps(name, S, device, False)
    l1, f1, s1, _ = _train_steps(name, S, device, True)
    diff1 = [k for k in f0 if not torch.equal(f0[k], f1[k])]
    diff3 = [k for k in s0 if not torch.equal(s0[k], s1[k])]
    print(f"{name} {S}: losses eager {l0} replayed {l1}; tensors that differ after step 1: {len(diff1)}, after step 3: {len(diff3)} "
          f"of {len(f0)}")
    assert l0 == l1, (l0, l1)
    assert not diff1, ("after the first step", diff1[:5])
    assert not diff3, ("after three steps", diff3[:5])
