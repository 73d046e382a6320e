"""Side-by-side launches for conv_down and the downsample path of a layer's first block (medt_conv_block_pair_fwd, net.PAIR).

The pair kernels are the single kernels' bodies with the block coordinates handed in, so the check is exact equality
(torch.equal), not a tolerance: the pair entry point against two calls of the single entry point on clones of the same inputs
(z, y, saved statistics; running statistics and num_batches_tracked after the queue flush), and two whole training steps of
MedT 128 with net.PAIR on and off."""
import ctypes as C

import pytest
import torch

import helpers as H
from test_model_gpu import build

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1

# (name, N, bn_groups, H, W, Cin, (Cout, stride) of conv_down, (Cout, stride) of the downsample path)
CASES = [
    ("both-fused-small", 8, 2, 8, 8, 32, (16, 1), (32, 2)),
    ("both-generic-tiles-s1", 2, 1, 32, 32, 8, (16, 1), (32, 1)),
    ("both-generic-tiles-s2", 2, 1, 32, 32, 8, (16, 1), (32, 2)),
    ("mixed-families", 8, 2, 16, 16, 64, (16, 1), (32, 2)),
    ("ragged", 3, 1, 10, 10, 8, (16, 1), (32, 1)),
    # rectangular maps: the pair kernels decode (row, column) from the handed-in block coordinates with H and W of their own member
    ("both-fused-small-8x12", 4, 2, 8, 12, 32, (16, 1), (32, 2)),       # 192 / 48 positions per group: both the 256-thread instantiation
    ("both-generic-tiles-24x32", 2, 1, 24, 32, 8, (16, 1), (32, 2)),    # 1536 / 384 positions: six / one and a half 256-position blocks
]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Member:
    """Device arguments of one 1x1 conv + BatchNorm block."""

    def __init__(self, L, lib, gen, x, groups, Cout, stride, relu, training, dev):
        N, Cin, Hh, Ww = x.shape
        self.desc = L.ConvDesc(N, Cin, Hh, Ww, Cout, 1, stride, 0, 0, 1, 0, int(relu), int(training), groups, EPS, MOM, 0)
        Ho, Wo = (Hh - 1) // stride + 1, (Ww - 1) // stride + 1
        r = lambda *s: torch.randn(*s, generator=gen)
        self.x = x
        self.w = (r(Cout, Cin, 1, 1) * 0.3).to(dev)
        self.weight, self.bias = (r(Cout) * 0.2 + 1).to(dev), (r(Cout) * 0.2).to(dev)
        self.rm, self.rv = (r(Cout) * 0.1).to(dev), (torch.rand(Cout, generator=gen) + 0.5).to(dev)
        self.nbt = torch.zeros((), dtype=torch.int64, device=dev)
        self.bn = L.BnPtrs(self.weight.data_ptr(), self.bias.data_ptr(), self.rm.data_ptr(), self.rv.data_ptr(),
                           self.nbt.data_ptr() if training else None)
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        self.z, self.y = nan(N, Cout, Ho, Wo), nan(N, Cout, Ho, Wo)
        self.stats = nan(max(int(lib.medt_conv_stats_floats(C.byref(self.desc))), 1))
        self.ws_bytes = int(lib.medt_conv_workspace_bytes(C.byref(self.desc)))
        assert self.ws_bytes > 0
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)

    def args(self):
        return [C.byref(self.desc), self.x.data_ptr(), self.w.data_ptr(), None, C.byref(self.bn), None, self.z.data_ptr(),
                self.y.data_ptr(), self.stats.data_ptr(), self.ws.data_ptr(), self.ws_bytes]

    def results(self):
        return dict(z=self.z, y=self.y, stats=self.stats, running_mean=self.rm, running_var=self.rv, nbt=self.nbt)


def _members(L, lib, case, training, dev):
    _, N, groups, Hh, Ww, Cin, (ca, sa), (cb, sb) = case
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(N, Cin, Hh, Ww, generator=gen).to(dev)
    return (Member(L, lib, gen, x, groups, ca, sa, True, training, dev),
            Member(L, lib, gen, x, groups, cb, sb, False, training, dev))


@pytest.mark.parametrize("queued", [False, True], ids=["immediate", "recorded+flush"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pair_fwd_equals_two_single_calls(case, training, queued, device):
    from medt_amd import _lib as L
    lib = L.lib()
    out = {}
    for mode in ("single", "pair"):
        a, b = _members(L, lib, case, training, device)
        s = _stream()
        q = None
        try:
            if queued:
                q = lib.medt_queue_create()
                assert lib.medt_queue_bind(q, s) == 0
            if mode == "single":
                L.check(lib.medt_conv_block_fwd(*a.args(), s), "single A")
                L.check(lib.medt_conv_block_fwd(*b.args(), s), "single B")
            else:
                L.check(lib.medt_conv_block_pair_fwd(*a.args(), *b.args(), s), "pair")
            if queued:
                out[mode + "/pending"] = int(lib.medt_queue_pending(q))
                assert lib.medt_queue_flush(q, s) == 0
        finally:
            if q:
                lib.medt_queue_bind(None, s)
                lib.medt_queue_destroy(q)
        torch.cuda.synchronize()
        out[mode] = ({k: v.cpu() for k, v in a.results().items()}, {k: v.cpu() for k, v in b.results().items()})
    if queued:
        assert out["pair/pending"] == out["single/pending"]
    for m in range(2):
        for k, want in out["single"][m].items():
            assert not torch.isnan(want.double()).any(), (m, k)
            assert torch.equal(out["pair"][m][k], want), (case[0], "AB"[m], k)
    if training:
        assert int(out["pair"][0]["nbt"]) == case[2]               # one running-statistics update per BatchNorm group


# --------------------------------------------------------------------------------------------------------------------- #
# whole model: two training steps of MedT 128 at batch 2, net.PAIR on against off
# --------------------------------------------------------------------------------------------------------------------- #
_RUNS = {}


def _train(device, pair, use_graph, monkeypatch):
    import medt_amd
    from medt_amd import net, ops
    from medt_amd.optim import FlatAdam
    from medt_amd.trainer import TrainStep
    monkeypatch.setattr(net, "PAIR", pair)
    torch.manual_seed(170)
    model = build("MedT", 128, device)
    model.train()
    x, y = H.seeded_input(171, 2, 3, 128)
    xd, yd = x.to(device), y.to(device)
    opt = FlatAdam(list(model.parameters()), lr=1e-3, weight_decay=1e-5)
    step = TrainStep(model, opt, medt_amd.cross_entropy, use_graph=use_graph, warmup=1)
    calls = ops.PAIR_CALLS
    losses = [step(xd, yd).item() for _ in range(2)]
    torch.cuda.synchronize()
    return dict(losses=losses, calls=ops.PAIR_CALLS - calls,
                state={k: v.detach().cpu().clone() for k, v in model.state_dict().items()})


def _run(device, pair, use_graph, monkeypatch):
    key = (pair, use_graph)
    if key not in _RUNS:
        _RUNS[key] = _train(device, pair, use_graph, monkeypatch)
    return _RUNS[key]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "replayed"])
def test_medt_training_steps_pair_on_equals_off(use_graph, device, monkeypatch):
    on, off = _run(device, True, use_graph, monkeypatch), _run(device, False, use_graph, monkeypatch)
    assert off["calls"] == 0
    assert on["calls"] > 0, "net.PAIR is on but medt_conv_block_pair_fwd was never reached"
    assert on["losses"] == off["losses"]
    assert sorted(on["state"]) == sorted(off["state"])
    for k, want in off["state"].items():                                # parameters and buffers
        assert torch.equal(on["state"][k], want), k


def test_medt_eval_forward_pair_on_equals_off(device, monkeypatch):
    from medt_amd import net, ops
    torch.manual_seed(170)
    model = build("MedT", 128, device)
    model.eval()
    x, _ = H.seeded_input(172, 2, 3, 128)
    outs = {}
    with torch.no_grad():
        for pair in (True, False):
            monkeypatch.setattr(net, "PAIR", pair)
            calls = ops.PAIR_CALLS
            outs[pair] = model(x.to(device)).cpu()
            assert (ops.PAIR_CALLS - calls > 0) == pair
    assert torch.equal(outs[True], outs[False])
