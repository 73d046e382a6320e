"""Parity of the HIP axial-attention layer (through the C ABI) against the CPU oracle and the
reference-generated golden fixtures.  Tolerance: north_star's 1e-3 relative (fp32 vs fp64 oracle);
the kernels are in practice ~1e-5."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import helpers as H
from oracle import medt_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-3
LAYER_FILES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(H.GOLDEN, "layer_*.npz")))


def make_layer(kind, C, L, width, stride, device):
    import lib as droplib
    ax = droplib.models.axialnet
    if kind in ("gatedsig", "gateddata"):
        from lib.models import model_codes
        cls = model_codes.AxialAttention_gated_sig if kind == "gatedsig" else model_codes.AxialAttention_gated_data
    else:
        cls = {"dynamic": ax.AxialAttention_dynamic, "plain": ax.AxialAttention, "wopos": ax.AxialAttention_wopos}[kind]
    return cls(C, C, groups=8, kernel_size=L, stride=stride, width=width).to(device)


def run_case(layer, st, x, dout, kind, width, stride, device, training=True, bn_groups=1):
    """Returns dicts (got, want) of named tensors."""
    layer.load_state_dict(st)
    for p in layer.parameters():
        p.requires_grad_(True)
        p.grad = None
    layer.train(training)
    layer.bn_groups = bn_groups
    xg = x.to(device).float().clone().requires_grad_(True)   # (clone: under --emulate the device is the CPU and .to() is the identity)
    y = layer(xg)
    (y * dout.to(device).float()).sum().backward()
    torch.cuda.synchronize()
    got = {"y": y.detach(), "dx": xg.grad}
    for k, p in layer.named_parameters():
        got["grad/" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    for k, b in layer.state_dict().items():
        if "running" in k or "num_batches" in k:
            got["buf/" + k] = b.clone()
    # oracle in fp64
    ost = O.clone_state({("m." + k): v for k, v in st.items()}, torch.float64, requires_grad=True)
    xo = x.double().requires_grad_(True)
    yo = O.axial_attention(xo, ost, "m", width, stride, training, bn_groups,
                           gate_mode={"gatedsig": "sigmoid", "gateddata": "data"}.get(kind, "raw"))
    (yo * dout.double()).sum().backward()
    want = {"y": yo.detach(), "dx": xo.grad}
    for k, _ in layer.named_parameters():
        g = ost["m." + k].grad
        want["grad/" + k] = g if g is not None else torch.zeros_like(ost["m." + k])
    for k in got:
        if k.startswith("buf/"):
            want[k] = ost["m." + k[4:]]
    return got, want


def compare(got, want, tol=TOL, grad_floor=1e-3, grad_tol=None):
    gscale = max(want[k].abs().max().item() for k in want if k.startswith("grad/"))
    bad = []
    for k in want:
        a, b = got[k].detach().double().cpu(), want[k].detach().double().cpu()
        if k.startswith("grad/"):
            # gradients that are mathematically zero (bn_similarity.bias, ...) are compared on the layer's scale
            scale = max(b.abs().max().item(), grad_floor * gscale)
        else:
            scale = max(b.abs().max().item(), 1e-30)
        err = (a - b).abs().max().item() / scale
        if not err < (grad_tol if (grad_tol is not None and k.startswith("grad/")) else tol):
            bad.append((k, err))
    assert not bad, bad


CASES = [
    # kind, C, L, width, stride, N, other
    ("dynamic", 16, 64, False, 1, 2, 8),
    ("dynamic", 16, 64, True, 1, 2, 8),
    ("dynamic", 32, 32, True, 2, 2, 32),
    ("dynamic", 64, 16, False, 1, 3, 16),
    ("dynamic", 128, 16, True, 2, 2, 16),
    ("dynamic", 32, 128, True, 1, 1, 4),
    ("plain", 32, 32, False, 1, 2, 6),
    ("wopos", 16, 16, False, 1, 4, 16),
    ("wopos", 32, 8, True, 2, 4, 8),
    ("wopos", 64, 4, False, 1, 4, 4),
    ("wopos", 128, 2, True, 2, 4, 2),
    ("gatedsig", 16, 64, True, 1, 2, 8),        # model_codes.AxialAttention_gated_sig: sigmoid(f) gates
    ("gatedsig", 64, 16, False, 2, 2, 16),
    ("gateddata", 16, 64, True, 1, 2, 8),       # model_codes.AxialAttention_gated_data: per-sequence gates from an MLP
    ("gateddata", 32, 32, False, 2, 2, 32),
    ("gateddata", 128, 8, True, 1, 2, 8),
    ("dynamic", 16, 24, True, 1, 2, 5),         # non power-of-two length, ragged tile
    # the single-sweep backward (csrc/axial_bwd.hip: gp <= 4, L in {32, 64, 128}) on both axes, ragged tiles, stride 2,
    # with (dynamic: GATES variant) and without (plain) gate gradients
    ("dynamic", 32, 64, False, 1, 2, 20),
    ("dynamic", 32, 64, True, 2, 2, 64),
    ("dynamic", 16, 32, True, 1, 3, 5),
    ("dynamic", 16, 32, False, 2, 2, 32),
    ("dynamic", 16, 128, False, 1, 1, 6),
    # round 5: gp = 4 at L = 128 on the sweep (<4, 128, 32>: 32 lanes per sequence) -- layer2.0 of the 256-px networks
    ("dynamic", 32, 128, False, 1, 2, 6),
    ("dynamic", 32, 128, True, 2, 1, 8),
    ("plain", 32, 128, False, 1, 1, 5),
    ("plain", 16, 64, True, 2, 2, 64),
    ("plain", 16, 64, False, 1, 3, 7),
    ("plain", 32, 64, False, 1, 1, 64),
    ("wopos", 16, 12, False, 1, 3, 7),
    # attention lengths that are no power of two (the networks at 96 / 160 / 192 / 384 px: L = 48, 24, 12, 6 / 80, 40 / 96 / 192), so the
    # thresholds of axial_geom and wopos_small_ok are met between the lengths they were tuned at; rectangular maps (other != L) throughout
    ("dynamic", 16, 48, True, 1, 2, 5),
    ("dynamic", 16, 48, False, 2, 1, 48),
    ("dynamic", 32, 24, True, 2, 2, 24),
    ("dynamic", 64, 12, False, 1, 3, 12),
    ("dynamic", 128, 6, True, 2, 2, 6),
    ("dynamic", 16, 96, False, 1, 1, 4),
    ("dynamic", 32, 80, True, 1, 1, 3),
    ("plain", 16, 40, False, 1, 2, 7),
    ("dynamic", 16, 192, True, 1, 1, 2),        # between the 128 the sweeps stop at and the longest length the layer takes (256)
    ("gatedsig", 16, 48, True, 1, 2, 6),
    ("wopos", 32, 12, True, 2, 4, 12),
    ("wopos", 64, 6, False, 1, 4, 6),
    ("wopos", 16, 24, True, 1, 4, 24),
    ("wopos", 32, 8, True, 1, 3, 5),
    ("wopos", 64, 4, False, 1, 5, 7),
    ("wopos", 16, 16, True, 1, 3, 5),           # wopos_small_ok's third length (4, 8, 16) on a rectangular map: P = 240
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_layer_vs_oracle(case, training, device):
    kind, C, L, width, stride, N, other = case
    layer = make_layer(kind, C, L, width, stride, device)
    st = O.randomize_state({k: v.cpu() for k, v in layer.state_dict().items()}, 100 + C + L)
    g = torch.Generator().manual_seed(7 + L)
    shape = (N, C, other, L) if width else (N, C, L, other)
    x = torch.randn(shape, generator=g)
    oshape = (N, C, shape[2] // stride, shape[3] // stride)
    dout = torch.randn(oshape, generator=g)
    got, want = run_case(layer, st, x, dout, kind, width, stride, device, training)
    if not training:
        got = {k: v for k, v in got.items() if not k.startswith("buf/")}
        want = {k: v for k, v in want.items() if not k.startswith("buf/")}
    compare(got, want)


@pytest.mark.parametrize("case", [("dynamic", 16, 64, True, 1, 2, 8), ("dynamic", 32, 64, False, 2, 2, 64), ("dynamic", 32, 32, True, 1, 3, 5),
                                  ("plain", 32, 128, False, 1, 1, 6), ("dynamic", 64, 16, False, 1, 3, 16), ("wopos", 16, 16, False, 1, 4, 16)],
                         ids=lambda c: "-".join(str(v) for v in c))
def test_layer_fused_output_relu_vs_oracle(case, device):
    """The width layer of an AxialBlock runs with its ReLU fused (out_relu): round 6 applies the ReLU's backward inside the single
    sweep and the statistics kernel in front of it (mask on load, no relu_mask launch); the generic kernels (gp = 8 here) and the
    small position-free layers keep their own handling.  Oracle: relu(axial_attention(x)) in float64."""
    kind, C, L, width, stride, N, other = case
    layer = make_layer(kind, C, L, width, stride, device)
    st = O.randomize_state({k: v.cpu() for k, v in layer.state_dict().items()}, 300 + C + L)
    g = torch.Generator().manual_seed(11 + L)
    shape = (N, C, other, L) if width else (N, C, L, other)
    x = torch.randn(shape, generator=g)
    dout = torch.randn((N, C, shape[2] // stride, shape[3] // stride), generator=g)
    layer.load_state_dict(st)
    for p in layer.parameters():
        p.requires_grad_(True)
        p.grad = None
    layer.train(True)
    xg = x.to(device).float().clone().requires_grad_(True)
    y = layer.run(xg, 1, True)
    (y * dout.to(device).float()).sum().backward()
    torch.cuda.synchronize()
    got = {"y": y.detach(), "dx": xg.grad}
    for k, p in layer.named_parameters():
        got["grad/" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    ost = O.clone_state({("m." + k): v for k, v in st.items()}, torch.float64, requires_grad=True)
    xo = x.double().requires_grad_(True)
    yo = torch.relu(O.axial_attention(xo, ost, "m", width, stride, True, 1, gate_mode="raw"))
    (yo * dout.double()).sum().backward()
    want = {"y": yo.detach(), "dx": xo.grad}
    for k, _ in layer.named_parameters():
        gr = ost["m." + k].grad
        want["grad/" + k] = gr if gr is not None else torch.zeros_like(ost["m." + k])
    assert (want["y"] == 0).float().mean().item() > 0.2          # (the mask matters on this input)
    compare(got, want)


@pytest.mark.parametrize("kind,C,L,width,stride", [("wopos", 16, 16, False, 1), ("wopos", 32, 8, True, 2),
                                                   ("dynamic", 16, 16, True, 1), ("dynamic", 16, 32, True, 1),
                                                   ("plain", 32, 32, False, 2)])
def test_layer_bn_groups(kind, C, L, width, stride, device):
    """Batched LoGo patches: 4 BN groups on the batch dim == 4 sequential calls."""
    layer = make_layer(kind, C, L, width, stride, device)
    st = O.randomize_state({k: v.cpu() for k, v in layer.state_dict().items()}, 55)
    g = torch.Generator().manual_seed(3)
    x = torch.randn((8, C, L, L), generator=g)
    dout = torch.randn((8, C, L // stride, L // stride), generator=g)
    got, want = run_case(layer, st, x, dout, kind, width, stride, device, True, bn_groups=4)
    compare(got, want)


@pytest.mark.parametrize("fn", LAYER_FILES)
def test_layer_vs_reference_fixture(fn, device):
    fx = H.load_golden(fn)
    C, L, width, stride, N, seed = [int(v) for v in fx["meta"]]
    kind = fn.split("_")[1]
    layer = make_layer(kind, C, L, bool(width), stride, device)
    layout = json.loads(str(fx["state_layout"]))
    assert [k for k, _, _ in layout] == list(layer.state_dict().keys())
    st = O.randomize_state({k: v.cpu() for k, v in layer.state_dict().items()}, seed)
    layer.load_state_dict(st)
    for p in layer.parameters():
        p.requires_grad_(True)
    x = torch.from_numpy(fx["x"]).float().to(device)
    layer.eval()
    with torch.no_grad():
        assert H.rel_err(layer(x), fx["out_eval"]) < TOL
    layer.train()
    xg = x.clone().requires_grad_(True)
    y = layer(xg)
    assert H.rel_err(y, fx["out_train"]) < TOL
    (y * torch.from_numpy(fx["dout"]).float().to(device)).sum().backward()
    assert H.rel_err(xg.grad, fx["dx"]) < TOL
    gscale = max(np.abs(fx[k]).max() for k in fx if k.startswith("grad/"))
    for k in fx:
        if k.startswith("grad/"):
            p = dict(layer.named_parameters())[k[5:]]
            want = torch.from_numpy(fx[k])
            scale = max(want.abs().max().item(), 1e-3 * gscale)
            err = (p.grad.double().cpu() - want).abs().max().item() / scale
            assert err < TOL, (k, err)
        if k.startswith("buf/"):
            assert H.rel_err(layer.state_dict()[k[4:]].double(), fx[k]) < TOL, k


BF16_TOL = 3e-2      # bf16 storage of qkv_raw / stacked: 2^-9 relative rounding per stored element (fp32 arithmetic)


@pytest.mark.parametrize("case", [("dynamic", 16, 64, True, 1, 2, 8), ("dynamic", 32, 32, False, 2, 2, 32),
                                  ("dynamic", 64, 16, True, 1, 3, 16), ("dynamic", 128, 8, False, 2, 2, 8),
                                  ("plain", 32, 128, True, 1, 1, 4), ("gatedsig", 16, 24, True, 1, 2, 5)],
                         ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_layer_bf16_storage_vs_oracle(case, training, device):
    """BASELINE.json configs[1]: qkv_transform output and sv|sve kept as bfloat16 between the kernels and for backward,
    fp32 arithmetic and statistics.  Against the fp64 oracle (which rounds nothing) within BF16_TOL."""
    import medt_amd
    kind, C, L, width, stride, N, other = case
    medt_amd.set_activation_dtype(torch.bfloat16)
    try:
        layer = make_layer(kind, C, L, width, stride, device)
        st = O.randomize_state({k: v.cpu() for k, v in layer.state_dict().items()}, 300 + C + L)
        g = torch.Generator().manual_seed(17 + L)
        shape = (N, C, other, L) if width else (N, C, L, other)
        x = torch.randn(shape, generator=g)
        dout = torch.randn((N, C, shape[2] // stride, shape[3] // stride), generator=g)
        got, want = run_case(layer, st, x, dout, kind, width, stride, device, training)
    finally:
        medt_amd.set_activation_dtype(torch.float32)
    if not training:
        got = {k: v for k, v in got.items() if not k.startswith("buf/")}
        want = {k: v for k, v in want.items() if not k.startswith("buf/")}
    # parameter gradients that are sums with heavy cancellation (the gates, bn_similarity.bias == 0 analytically) carry
    # the rounding noise of the stored activations: they are judged on 10 % of the layer's largest gradient, at 2x the
    # activation tolerance (observed worst: gate gradients, 3.3e-2)
    compare(got, want, BF16_TOL, grad_floor=0.1, grad_tol=2 * BF16_TOL)
    # and it is not silently the fp32 path: the result differs from the fp32-storage run beyond fp32 noise
    got32, _ = run_case(layer, st, x, dout, kind, width, stride, device, training)
    assert H.rel_err(got["y"], got32["y"]) > 1e-5


def test_large_batch_property(device):
    """At bench scale (B* = 4096 rows of L=64) the oracle is too slow; check size-independent properties:
    softmax rows reproduce (lse) and the layer is invariant to a per-head constant added to the logits
    (bn_similarity.bias), and outputs for replicated images are identical."""
    layer = make_layer("dynamic", 16, 64, True, 1, device)
    st = O.randomize_state({k: v.cpu() for k, v in layer.state_dict().items()}, 9)
    layer.load_state_dict(st)
    layer.eval()
    g = torch.Generator().manual_seed(1)
    x1 = torch.randn((1, 16, 64, 64), generator=g).to(device)
    x = x1.repeat(64, 1, 1, 1)
    with torch.no_grad():
        y = layer(x)
        assert torch.equal(y[0], y[63])
        layer.bn_similarity.bias.add_(3.0)
        y2 = layer(x)
    assert H.rel_err(y2, y) < 1e-5


@pytest.mark.parametrize("width", [True, False], ids=["w", "h"])
def test_dispatch_scale_variants_vs_oracle(width, device):
    """The kernels that only dispatch on big problems -- attn_fwd4r (four rows per lane), the bound-referenced softmax with its
    repair pass behind, the persistent multi-tile loops of the forward and of the backward sweep, the 4-wave workgroups --
    UNFORCED at their own dispatch scale: N = 64 images of (16, 64, 64), i.e. 4096 sequences, 134M logits per launch.
    The batch is 16 replicas of a 4-image batch, so its BatchNorm batch statistics equal the 4-image batch's exactly:
      * train mode: output, dx and every parameter gradient against the fp64 oracle ON THE 4-IMAGE BATCH (parameter gradients
        of the big batch are 16x the small batch's, running statistics and dx per image are the same);
      * every replica's output / dx must equal replica 0's bit for bit (tile- and workgroup-independent arithmetic)."""
    C, L, R = 16, 64, 16
    layer = make_layer("dynamic", C, L, width, 1, device)
    st = O.randomize_state({k: v.cpu() for k, v in layer.state_dict().items()}, 77)
    g = torch.Generator().manual_seed(5)
    x4 = torch.randn((4, C, L, L), generator=g)
    d4 = torch.randn((4, C, L, L), generator=g)
    x, dout = x4.repeat(R, 1, 1, 1), d4.repeat(R, 1, 1, 1)
    layer.load_state_dict(st)
    for p in layer.parameters():
        p.requires_grad_(True)
        p.grad = None
    layer.train()
    xg = x.to(device).clone().requires_grad_(True)
    y = layer(xg)
    (y * dout.to(device)).sum().backward()
    torch.cuda.synchronize()
    for r in range(1, R):
        assert torch.equal(y[4 * r:4 * r + 4], y[:4]), r
        assert torch.equal(xg.grad[4 * r:4 * r + 4], xg.grad[:4]), r
    ost = O.clone_state({("m." + k): v for k, v in st.items()}, torch.float64, requires_grad=True)
    xo = x4.double().requires_grad_(True)
    yo = O.axial_attention(xo, ost, "m", width, 1, True)
    (yo * d4.double()).sum().backward()
    got = {"y": y[:4].detach(), "dx": xg.grad[:4]}
    want = {"y": yo.detach(), "dx": xo.grad}
    for k, p in layer.named_parameters():
        got["grad/" + k] = p.grad / R
        want["grad/" + k] = ost["m." + k].grad
    for k, b in layer.state_dict().items():
        if "running" in k:
            got["buf/" + k] = b.clone()
            want["buf/" + k] = ost["m." + k]
    # (the unbiased running variance divides by count - 1: 16x the population moves it by < 1e-5 relative)
    compare(got, want)


def _run_layer_subprocess(env_extra, emulate=False):
    import subprocess
    import sys
    code = r'''
import os, sys, torch
sys.path[:0] = [os.path.join(os.environ["MEDT_ROOT"], "medical-transformer_amd"), os.environ["MEDT_ROOT"], os.path.join(os.environ["MEDT_ROOT"], "tests")]
import lib as droplib
from oracle import medt_oracle as O
dev = torch.device("cuda:0")
if os.environ.get("MEDT_TEST_EMULATE") == "1":          # pytest --emulate: the CPU lane emulator as the device (tests/emu_device.py)
    import ctypes
    import test_lane_emu as T
    from emu_device import emulated_device
    from medt_amd import _lib as L
    emu = ctypes.CDLL(T.build_emulator())
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(emu, name)
        fn.restype, fn.argtypes = res, args
    _emulated = emulated_device(emu)                      # (kept alive: leaving the context restores the product's device checks)
    _emulated.__enter__()
    dev = torch.device("cpu")
tol = 1e-3
if os.environ.get("MEDT_TEST_BF16") == "1":              # bfloat16 storage of qkv_raw / stacked (BF16_TOL of this file)
    import medt_amd
    medt_amd.set_activation_dtype(torch.bfloat16)
    tol = 3e-2
for C, L, width in ((16, 64, True), (32, 32, False), (32, 128, True), (16, 16, False), (16, 64, False), (16, 32, True),
                    (16, 128, False), (16, 128, True), (16, 16, True), (16, 32, False)):
    layer = droplib.models.axialnet.AxialAttention_dynamic(C, C, groups=8, kernel_size=L, stride=1, width=width).to(dev)
    st = O.randomize_state({k: v.cpu() for k, v in layer.state_dict().items()}, 5)
    layer.load_state_dict(st)
    layer.train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn((3, C, 7, L) if width else (3, C, L, 7), generator=g)
    y = layer(x.to(dev))
    ost = O.clone_state({("m." + k): v for k, v in st.items()}, torch.float64)
    yo = O.axial_attention(x.double(), ost, "m", width, 1, True)
    err = (y.double().cpu() - yo).abs().max().item() / yo.abs().max().item()
    assert err < tol, (C, L, err)
print("layers ok")
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MEDT_ROOT=root, MEDT_TEST_EMULATE="1" if emulate else "0", **env_extra)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=3000 if emulate else 600)
    assert r.returncode == 0 and "layers ok" in r.stdout, r.stderr[-1500:]


def test_softmax_bound_path(device, emulating):
    """Large problems take the bound-referenced softmax kernel (softmax shifted by a cheap per-row upper bound of
    the logits instead of a running maximum).  MEDT_BOUND_PATH=1 forces it on small shapes: same results."""
    _run_layer_subprocess({"MEDT_BOUND_PATH": "1"}, emulating)


def test_softmax_bound_repair_pass(device, emulating):
    """When the bound is so loose that a row's sum underflows the kernel raises a flag and the exact kernel queued
    behind it redoes the launch.  MEDT_DEBUG_BOUND_SHIFT=400 pushes every bound 400 octaves up, so every launch
    is repaired: results must not change."""
    _run_layer_subprocess({"MEDT_BOUND_PATH": "1", "MEDT_DEBUG_BOUND_SHIFT": "400"}, emulating)


@pytest.mark.parametrize("bound,shift", [("0", "0"), ("1", "0"), ("1", "400")], ids=["exact", "bound", "repair"])
def test_four_rows_per_lane_kernel(bound, shift, device, emulating):
    """gp = 2 layers of large problems run the four-rows-per-lane forward kernel (MEDT_ROWS4=1 forces it on the
    small test shapes, ragged tiles included): exact, bound-referenced and repaired variants, both axes, L = 16..128."""
    _run_layer_subprocess({"MEDT_ROWS4": "1", "MEDT_BOUND_PATH": bound, "MEDT_DEBUG_BOUND_SHIFT": shift}, emulating)


@pytest.mark.parametrize("env", [{"MEDT_TEST_BF16": "1"}, {"MEDT_F4R_VEC": "0"}, {"MEDT_F4R_VEC": "0", "MEDT_TEST_BF16": "1"}],
                         ids=["bf16", "scalar-movers", "scalar-movers-bf16"])
def test_four_rows_per_lane_kernel_movers(env, device, emulating):
    """Round 5: on the width axis the four-rows-per-lane kernel moves a sequence with the lanes that sweep it, 16 bytes of
    float32 / 8 of bfloat16 per access and no workgroup barrier in the tile loop.  bfloat16 storage through those movers, and
    the 4-byte movers (MEDT_F4R_VEC=0: what misaligned tensors get) with both storage types."""
    _run_layer_subprocess({"MEDT_ROWS4": "1", "MEDT_BOUND_PATH": "1", "MEDT_DEBUG_BOUND_SHIFT": "0", **env}, emulating)


def test_layer_by_layer_fallback_of_small_layers(device, emulating):
    """Position-free layers / 1x1 conv blocks whose BatchNorm group fits one workgroup normally run the fused
    small-layer kernels (axial_small.hip, conv_small.hip).  MEDT_DISABLE_SMALL=1 forces the layer-by-layer path those
    shapes used before, which stays the path of larger groups: same parity tests, in a subprocess."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MEDT_DISABLE_SMALL="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(root, "tests", "test_axial_layer_gpu.py"), os.path.join(root, "tests", "test_ops_gpu.py"),
                        "-k", "wopos or test_conv_block"] + (["--emulate"] if emulating else []), env=env, capture_output=True,
                       text=True, timeout=7000 if emulating else 900, cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-1500:] + r.stderr[-500:]


def test_narrow_sweep_instances_on_the_test_shapes(device, emulating):
    """Round 5: launches of fewer than 1024 waves take the sweep with twice the lanes per sequence (<2,64,32>, <4,64,32>,
    <2,32,16>, <4,32,16>, <2,128,32>) -- which is every test shape.  MEDT_BWD_WIDE=0 forces the lane counts of the bandwidth
    shapes (<2,64,16>, <4,64,16>, <2,32,8>, <4,32,8>, <2,128,16>) onto the same parity and bit-reproducibility tests."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MEDT_BWD_WIDE="0")
    sel = "(test_layer_vs_oracle and (dynamic or plain) and train) or test_layer_backward_is_bit_reproducible"
    if emulating:
        sel = "test_layer_vs_oracle and train and (dynamic-16-32-True or dynamic-32-64-False or plain-16-64-False)"
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(root, "tests", "test_axial_layer_gpu.py"), "-k", sel] + (["--emulate"] if emulating else []),
                       env=env, capture_output=True, text=True, timeout=7000 if emulating else 900, cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-1500:] + r.stderr[-500:]


@pytest.mark.parametrize("case", [("dynamic", 16, 64, True, 1, 4, 64), ("dynamic", 32, 32, False, 2, 4, 32),
                                  ("dynamic", 64, 16, True, 1, 2, 16), ("dynamic", 64, 32, False, 2, 2, 32),
                                  ("dynamic", 128, 16, True, 1, 2, 16), ("dynamic", 32, 128, True, 2, 2, 128)],
                         ids=lambda c: "-".join(str(v) for v in c))
def test_layer_backward_is_bit_reproducible(case, device):
    """Two runs of the same layer backward give bit-identical gradients -- every one, the relative tables included (the
    reference's index_select backward is deterministic on the CPU; the table gradients are accumulated along lane-private
    diagonals / per-wave LDS rows and reduced in a fixed order, no float atomics).  Since round 4 the gp = 8 layers (third
    and fourth case) and gp = 16 at L = 16 (fifth) run the single sweep too: exact as well."""
    kind, C, L, width, stride, N, other = case
    layer = make_layer(kind, C, L, width, stride, device)
    st = O.randomize_state({k: v.cpu() for k, v in layer.state_dict().items()}, 300 + C)
    g = torch.Generator().manual_seed(11)
    shape = (N, C, other, L) if width else (N, C, L, other)
    x = torch.randn(shape, generator=g)
    dout = torch.randn((N, C, shape[2] // stride, shape[3] // stride), generator=g)
    runs = []
    for _ in range(2):
        layer.load_state_dict(st)
        for p in layer.parameters():
            p.requires_grad_(True)
            p.grad = None
        layer.train(True)
        xg = x.to(device).clone().requires_grad_(True)
        (layer(xg) * dout.to(device)).sum().backward()
        torch.cuda.synchronize()
        runs.append({"dx": xg.grad.clone(), **{k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None}})
    exact = True
    for k in runs[0]:
        if exact:
            assert torch.equal(runs[0][k], runs[1][k]), k
        else:
            assert H.rel_err(runs[1][k], runs[0][k]) < 1e-6, k


@pytest.mark.parametrize("zero", ["f_qr", "f_kr", "both"])
@pytest.mark.parametrize("C,L,width", [(16, 64, True), (32, 32, False), (64, 16, True)], ids=["sweep-gp2", "sweep-gp4", "generic-gp8"])
def test_layer_zero_gate_gradients(zero, C, L, width, device):
    """a gate that is exactly 0.  The single-sweep backward forms the gate gradient as e T + (u S2 + w S1) / f
    from the saved statistics of the GATED logits and skips the second term at f == 0; that term is exactly 0 there (the
    gated logits are constant, so bn_similarity's backward means vanish), and every gradient -- the zeroed gate's own
    included -- must still match the oracle, which differentiates through the gate like the reference's autograd."""
    layer = make_layer("dynamic", C, L, width, 1, device)
    st = O.randomize_state({k: v.cpu() for k, v in layer.state_dict().items()}, 41 + C)
    for k in (("f_qr", "f_kr") if zero == "both" else (zero,)):
        st[k] = torch.zeros_like(st[k])
    g = torch.Generator().manual_seed(23)
    shape = (2, C, 6, L) if width else (2, C, L, 6)
    x = torch.randn(shape, generator=g)
    dout = torch.randn(shape, generator=g)
    got, want = run_case(layer, st, x, dout, "dynamic", width, 1, device, True)
    compare(got, want)
