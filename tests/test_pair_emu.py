"""medt_conv_block_pair_fwd on the CPU lane emulator (tests/lane_emu): the pair entry point against two calls of
medt_conv_block_fwd on copies of the same inputs -- exact equality of z, y, the saved statistics, the running statistics and
num_batches_tracked (after the queue flush where a queue is bound).  The pair kernels are the single kernels' bodies with the
block coordinates handed in, so every bit must agree; the emulator also checks that the new device code compiles under its shims
and stays inside the LDS it asked for."""
import ctypes as C

import numpy as np
import pytest

import helpers as H  # noqa: F401
from test_lane_emu import build_emulator, emu, f32, ptr  # noqa: F401  (emu: the module-scoped fixture)

EPS, MOM = 1e-5, 0.1

# (name, N, bn_groups, H, W, Cin, (Cout, stride) of conv_down, (Cout, stride) of the downsample path)
CASES = [
    ("both-fused-small", 8, 2, 8, 8, 32, (16, 1), (32, 2)),
    ("both-generic-tiles-s1", 2, 1, 32, 32, 8, (16, 1), (32, 1)),
    ("both-generic-tiles-s2", 2, 1, 32, 32, 8, (16, 1), (32, 2)),
    ("mixed-families", 8, 2, 16, 16, 64, (16, 1), (32, 2)),
    ("ragged", 3, 1, 10, 10, 8, (16, 1), (32, 1)),
]


class Member:
    """Host-memory arguments of one conv + BatchNorm block."""

    def __init__(self, L, rng, x, N, groups, Hh, Ww, Cin, Cout, stride, relu, training):
        self.desc = L.ConvDesc(N, Cin, Hh, Ww, Cout, 1, stride, 0, 0, 1, 0, int(relu), int(training), groups, EPS, MOM, 0)
        Ho, Wo = (Hh - 1) // stride + 1, (Ww - 1) // stride + 1
        self.x = x
        self.w = f32(rng.standard_normal((Cout, Cin, 1, 1)) * 0.3)
        self.p = dict(weight=f32(rng.uniform(0.5, 1.5, Cout)), bias=f32(rng.standard_normal(Cout) * 0.2),
                      running_mean=f32(rng.standard_normal(Cout) * 0.1), running_var=f32(rng.uniform(0.5, 1.5, Cout)))
        self.nbt = np.zeros(1, dtype=np.int64)
        self.bn = L.BnPtrs(ptr(self.p["weight"]), ptr(self.p["bias"]), ptr(self.p["running_mean"]), ptr(self.p["running_var"]),
                           ptr(self.nbt) if training else None)
        self.z = np.full((N, Cout, Ho, Wo), np.nan, dtype=np.float32)
        self.y = np.full((N, Cout, Ho, Wo), np.nan, dtype=np.float32)

    def alloc(self, lib):
        self.stats = np.full(max(int(lib.medt_conv_stats_floats(C.byref(self.desc))), 1), np.nan, dtype=np.float32)
        self.ws_bytes = int(lib.medt_conv_workspace_bytes(C.byref(self.desc)))
        assert self.ws_bytes > 0, lib.medt_last_error()
        self.ws = np.zeros(self.ws_bytes, dtype=np.uint8)

    def args(self):
        return [C.byref(self.desc), ptr(self.x), ptr(self.w), None, C.byref(self.bn), None, ptr(self.z), ptr(self.y),
                ptr(self.stats), ptr(self.ws), self.ws_bytes]

    def results(self):
        return dict(z=self.z, y=self.y, stats=self.stats, rm=self.p["running_mean"], rv=self.p["running_var"], nbt=self.nbt)


def members(L, lib, case, training):
    _, N, groups, Hh, Ww, Cin, (ca, sa), (cb, sb) = case
    rng = np.random.default_rng(7)
    x = f32(rng.standard_normal((N, Cin, Hh, Ww)))
    a = Member(L, rng, x, N, groups, Hh, Ww, Cin, ca, sa, True, training)
    b = Member(L, rng, x, N, groups, Hh, Ww, Cin, cb, sb, False, training)
    a.alloc(lib)
    b.alloc(lib)
    return a, b


@pytest.mark.parametrize("queued", [False, True], ids=["immediate", "recorded+flush"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pair_fwd_equals_two_single_calls(emu, case, training, queued):
    from medt_amd import _lib as L
    out = {}
    for mode in ("single", "pair"):
        a, b = members(L, emu, case, training)
        stream = C.c_void_p(0x5151) if queued else None
        q = None
        try:
            if queued:
                q = emu.medt_queue_create()
                assert emu.medt_queue_bind(q, stream) == 0
            if mode == "single":
                assert emu.medt_conv_block_fwd(*a.args(), stream) == 0, emu.medt_last_error()
                assert emu.medt_conv_block_fwd(*b.args(), stream) == 0, emu.medt_last_error()
            else:
                assert emu.medt_conv_block_pair_fwd(*a.args(), *b.args(), stream) == 0, emu.medt_last_error()
            if queued:
                out[mode + "/pending"] = int(emu.medt_queue_pending(q))
                assert emu.medt_queue_flush(q, stream) == 0
        finally:
            if q:
                emu.medt_queue_bind(None, stream)
                emu.medt_queue_destroy(q)
        out[mode] = (a.results(), b.results())
    if queued:
        assert out["pair/pending"] == out["single/pending"]
    for m in range(2):
        for k, want in out["single"][m].items():
            got = out["pair"][m][k]
            assert not np.isnan(want.astype(np.float64)).any(), (m, k)
            assert np.array_equal(got, want), (case[0], "AB"[m], k)
    if training:
        assert int(out["pair"][0]["nbt"][0]) == case[2]            # one running-statistics update per BatchNorm group


def test_pair_fwd_shares_the_argument_checks(emu):
    """A null pointer or a short workspace in EITHER member is refused like the single entry point refuses it."""
    from medt_amd import _lib as L
    a, b = members(L, emu, CASES[0], True)
    bad = b.args()
    bad[6] = None                                                  # z of member B
    assert emu.medt_conv_block_pair_fwd(*a.args(), *bad, None) == emu.medt_conv_block_fwd(*bad, None) != 0
    short = a.args()
    short[10] = 16
    assert emu.medt_conv_block_pair_fwd(*short, *b.args(), None) == emu.medt_conv_block_fwd(*short, None) != 0
