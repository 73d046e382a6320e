"""One family of guarded-memory cases in one process: run by tests/test_guarded_memory.py as
`python tests/guard_driver.py FAMILY PLACEMENT`, or by hand (tests/lane_emu/README.md, "Guarded memory").

The product's own Python path (medt_amd.ops / axial / block / net / optim / defer / window) runs on the CPU lane emulator with
every buffer that reaches the C ABI in a guard-page arena at its logical size (tests/guarded_mem.py).  A kernel that reads or
writes outside a buffer it was given ends this process with SIGSEGV (return code -11); the last "CALL" line on stdout then names
the entry point and the case, and faulthandler's dump on stderr the Python frames.  Every case also asserts the parity of the
emulator test it comes from, at that test's tolerance: the arena fills "uninitialised" allocations with NaNs, so a read of
workspace or output nobody wrote shows up as a NaN in a compared tensor (every comparison used here fails on NaN).
The last line printed is a JSON summary."""
import ctypes as C
import faulthandler
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "medical-transformer_amd"), ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

FULL = os.environ.get("MEDT_GUARD_FULL") == "1"          # the largest shapes of each family (README.md, test section)

# Pointers that may reach the kernels outside the arena: (entry point, argument path) -> reason.  Empty: every pointer of every
# family is either an arena buffer or a torch-made tensor the proxy stands in the arena at the tensor's exact size.  No
# workspace, output, saved-tensor or gradient-destination argument may ever be listed here.
ALLOW = {}

# environment a family needs before the library reads its switches (once per process)
FAMILY_ENV = {"attention_repair": {"MEDT_ROWS4": "1", "MEDT_BOUND_PATH": "1", "MEDT_DEBUG_BOUND_SHIFT": "400"},
              "offset_pointers": {"MEDT_ROWS4": "1", "MEDT_BOUND_PATH": "1", "MEDT_DEBUG_BOUND_SHIFT": "0"}}


def emu_lib():
    import test_lane_emu as T
    from medt_amd import _lib as L
    lib = C.CDLL(T.build_emulator())
    lib.emu_set_order.argtypes = [C.c_int, C.c_ulonglong]
    lib.emu_last_error.restype = C.c_char_p
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.medt_abi_version() == L.ABI_VERSION
    return lib


class Run:
    def __init__(self, family, placement):
        self.family, self.placement = family, placement
        self.cases, self.t0 = [], time.time()
        self.arena = self.proxy = None

    def case(self, name):
        self.proxy.end_case()                              # results of the previous case are home; its stand-ins are dropped
        self.proxy.case = name
        self.cases.append(name)
        print("CASE %s" % name, flush=True)

    @staticmethod
    def announce(entry, case):
        print("CALL %s case=%s" % (entry, case), flush=True)


def finite(*tensors):
    for t in tensors:
        if t is not None:
            assert torch.isfinite(torch.as_tensor(t).float()).all(), "non-finite output: a read of memory nobody wrote?"


# ------------------------------------------------------------------------------------------------------------------------ #
# Attention layers: lib.models.axialnet / model_codes layers through medt_amd.axial against float64 autograd through the oracle
# (test_axial_layer_gpu.run_case / compare at the emulator tests' 3e-4), parameters re-pointed at arena copies.
# ------------------------------------------------------------------------------------------------------------------------ #
def layer_case(run, kind, Cc, Lq, width, stride, training, bn_groups=1, N=2, other=None, seed=0, bf16=False):
    import medt_amd
    import test_axial_layer_gpu as TG
    from oracle import medt_oracle as O
    other = Lq if other is None else other
    run.case("layer %s C%d L%d o%d %s s%d N%d g%d %s%s" % (kind, Cc, Lq, other, "w" if width else "h", stride, N, bn_groups,
                                                           "train" if training else "eval", " bf16" if bf16 else ""))
    layer = TG.make_layer(kind, Cc, Lq, width, stride, "cpu")
    for p in list(layer.parameters()) + list(layer.buffers()):
        p.data = run.arena.copy_of(p.data)                 # (load_state_dict copies in place: the arena storage stays)
    st = O.randomize_state({k: v.clone() for k, v in layer.state_dict().items()}, 40 + seed)
    g = torch.Generator().manual_seed(seed)
    shape = (N, Cc, other, Lq) if width else (N, Cc, Lq, other)
    x = torch.randn(shape, generator=g).double()
    dout = torch.randn((N, Cc, shape[2] // stride, shape[3] // stride), generator=g).double()
    if bf16:
        medt_amd.set_activation_dtype(torch.bfloat16)
    try:
        got, want = TG.run_case(layer, st, x, dout, kind, width, stride, "cpu", training, bn_groups)
    finally:
        if bf16:
            medt_amd.set_activation_dtype(torch.float32)
    finite(*got.values())
    if not training:
        got = {k: v for k, v in got.items() if not k.startswith("buf/")}
        want = {k: v for k, v in want.items() if not k.startswith("buf/")}
    if bf16:
        TG.compare(got, want, TG.BF16_TOL, grad_floor=0.1, grad_tol=2 * TG.BF16_TOL)
    else:
        TG.compare(got, want, tol=3e-4)


def family_attention(run):
    for training in (True, False):
        layer_case(run, "dynamic", 16, 24, True, 1, training, N=2, other=5, seed=1)         # non power-of-two length, ragged tile
    # the single sweep with ragged other-axis extents 5, 6, 7 and 20
    layer_case(run, "dynamic", 16, 32, True, 1, True, N=3, other=5, seed=2)
    layer_case(run, "dynamic", 16, 128, False, 1, True, N=1, other=6, seed=3)
    layer_case(run, "plain", 16, 64, False, 1, True, N=3, other=7, seed=4)
    layer_case(run, "wopos", 16, 12, False, 1, True, N=3, other=7, seed=5)
    layer_case(run, "dynamic", 32, 64, False, 1, True, N=2, other=20, seed=6)
    layer_case(run, "plain", 32, 128, False, 1, False, N=1, other=5, seed=7)
    # stride 2 on both axes
    layer_case(run, "dynamic", 16, 16, True, 2, True, seed=8)
    layer_case(run, "dynamic", 16, 32, False, 2, True, N=2, other=6, seed=9)
    layer_case(run, "wopos", 32, 8, True, 2, True, N=4, seed=10)
    # several BatchNorm groups
    layer_case(run, "wopos", 16, 16, False, 1, True, bn_groups=4, N=8, seed=11)
    layer_case(run, "dynamic", 16, 16, True, 1, True, bn_groups=2, N=4, other=6, seed=12)
    layer_case(run, "plain", 32, 32, False, 2, True, bn_groups=2, N=2, other=6, seed=13)
    # attn_bwd_sweep_kernel<4, 128, 32> at N = 1, other = 6
    layer_case(run, "dynamic", 32, 128, False, 1, True, N=1, other=6, seed=9)
    layer_case(run, "dynamic", 32, 128, True, 2, True, N=1, other=6, seed=9)
    # the gated kinds (gateddata: with the gate MLP in front)
    layer_case(run, "gatedsig", 16, 16, False, 1, True, seed=14)
    layer_case(run, "gateddata", 16, 16, True, 1, True, seed=15)
    layer_case(run, "gateddata", 16, 24, True, 1, False, N=2, other=5, seed=16)
    # bfloat16 storage of qkv_raw / stacked
    layer_case(run, "gatedsig", 16, 24, True, 1, True, N=2, other=5, seed=17, bf16=True)
    layer_case(run, "dynamic", 32, 32, False, 2, True, N=2, other=6, seed=18, bf16=True)
    if FULL:
        layer_case(run, "dynamic", 32, 128, False, 1, True, N=2, other=6, seed=19)
        layer_case(run, "dynamic", 64, 16, False, 1, True, N=3, other=16, seed=20)
        layer_case(run, "gateddata", 32, 32, False, 2, True, N=2, other=32, seed=21)


def family_attention_random(run):
    import test_lane_emu as T
    for cfg in T._random_layer_configs(24, 2024):
        kind, Cc, Lq, other, width, stride, N, groups, training = cfg
        layer_case(run, kind, Cc, Lq, width, stride, training, groups, N, other, seed=sum(map(int, cfg[1:4])))


def family_attention_repair(run):
    """MEDT_ROWS4=1 MEDT_BOUND_PATH=1 MEDT_DEBUG_BOUND_SHIFT=400 (set by the parent: read once per process): the four-rows
    forward kernel whose every row underflows and is redone inside the kernel, on ragged tiles of both axes."""
    assert os.environ.get("MEDT_DEBUG_BOUND_SHIFT") == "400"
    for Cc, Lq, width in ((16, 64, True), (32, 32, False), (16, 16, False), (16, 32, True), (16, 16, True)):
        layer_case(run, "dynamic", Cc, Lq, width, 1, True, N=3, other=7, seed=30 + Lq)
    layer_case(run, "dynamic", 16, 32, False, 1, False, N=1, other=5, seed=31)


# ------------------------------------------------------------------------------------------------------------------------ #
# ops.conv_block and the recorded weight gradients: tests/test_ops_gpu.py's own cases and references (2e-4), on the guarded device
# ------------------------------------------------------------------------------------------------------------------------ #
def _rows(table, wanted):
    rows = [c for c in table if "-".join(str(int(v)) for v in c) in wanted]
    assert len(rows) == len(set(wanted)), (wanted, rows)
    return rows


CONV_ROWS = ["3-40-7-2-3-1-0-0-1-3-64-1",        # the 7x7 stem with a partial channel tile
             "20-24-3-1-1-0-1-0-1-3-9-1",        # odd sizes
             "72-24-3-2-1-0-1-1-1-6-18-3",       # ragged: stride 2, 81-position maps, grouped statistics
             "8-40-3-1-1-0-1-0-1-2-64-1",        # 8-channel chunks, a half-empty last workgroup
             "32-64-1-2-0-0-1-0-0-2-16-1",       # the stride-2 1x1 downsample
             "256-256-3-2-1-1-0-0-0-8-2-1",      # 256 -> 256 on 2x2 maps
             "16-32-1-1-0-0-1-1-1-4-8-2",        # conv_up + identity + relu
             "16-2-1-1-0-1-0-0-0-2-16-1"]        # adjust
CONV_ROWS_SMALL1X1 = ["128-64-1-1-0-0-1-0-1-64-4-16", "64-128-1-1-0-0-1-1-1-64-4-16", "128-256-1-1-0-0-1-1-1-64-2-16"]   # bn_dgrad1x1_small
CONV_ROWS_FULL = ["40-72-3-1-1-0-1-1-1-36-15-2", "64-32-1-1-0-0-1-0-1-64-8-16", "32-64-1-1-0-0-1-1-1-64-8-16",
                  "64-64-1-1-0-0-1-0-1-64-8-16", "128-128-1-1-0-0-1-0-1-64-4-16"]


def family_conv(run):
    import test_ops_gpu as TO
    dev = torch.device("cpu")
    rows = _rows(TO.CONV_CASES, CONV_ROWS + CONV_ROWS_SMALL1X1 + (CONV_ROWS_FULL if FULL else []))
    for case in rows:
        for training in (True, False):
            run.case("conv_block %s %s" % ("-".join(str(int(v)) for v in case), "train" if training else "eval"))
            TO.test_conv_block(case, training, dev)
    run.case("conv_block single image, 1x1 map, eval")
    TO.test_conv_block((3, 4, 1, 1, 0, False, True, False, True, 1, 1, 1), False, dev)


# rectangular maps (H != W, neither a power of two): the planners test H and W separately, so an index that mixes them up leaves a
# buffer only off the square diagonal.  The many-image MFMA cases (N >= 16) take minutes each on the emulator: MEDT_GUARD_FULL=1
def family_conv_rect(run):
    import test_ops_gpu as TO
    dev = torch.device("cpu")
    for case in TO.RECT_CONV_CASES:
        if case[9] >= 16 and not FULL:
            continue
        for training in (True, False):
            run.case("conv_block %s %s" % ("-".join(str(int(v)) for v in case), "train" if training else "eval"))
            TO.test_conv_block(case, training, dev)
    for case in TO.RECORDED_CASES:
        if len(case) == 10:                                  # ..., N, H, W, groups
            run.case("recorded wgrad %s" % "-".join(str(int(v)) for v in case))
            TO.test_recorded_weight_gradient(case, dev)


RECORDED_ROWS = ["20-24-1-1-0-1-3-6-3", "8-8-1-1-0-1-2-3-1", "16-16-3-1-1-1-2-6-1", "72-40-1-1-0-0-2-10-1", "32-64-1-2-0-1-2-16-1",
                 "16-16-3-2-1-1-2-8-1", "32-16-3-1-1-1-3-12-3"]


def family_recorded(run):
    import test_ops_gpu as TO
    for case in _rows(TO.RECORDED_CASES, RECORDED_ROWS):
        run.case("recorded wgrad %s" % "-".join(str(int(v)) for v in case))
        TO.test_recorded_weight_gradient(case, torch.device("cpu"))


# ------------------------------------------------------------------------------------------------------------------------ #
def flat_adam_case(run):
    """FlatAdam over groups of 1, 5, 67 and 4k+3 elements (parameters that join one step after the other form one group each),
    then steps whose gradients are written straight into the slots, against torch.optim.Adam in float64 (1e-5, as
    test_ops_gpu.test_flat_adam_matches_torch_adam)."""
    import test_ops_gpu as TO
    from medt_amd import optim as OPT
    run.case("FlatAdam groups 1, 5, 67, 103; slots written directly")
    g = torch.Generator().manual_seed(3)
    shapes = [(), (5,), (67,), (103,)]
    init = [torch.randn(s, generator=g) for s in shapes]
    ref = [torch.nn.Parameter(p.clone().double()) for p in init]
    mine = [torch.nn.Parameter(run.arena.copy_of(p)) for p in init]
    o_ref = torch.optim.Adam(ref, lr=1e-2, weight_decay=1e-2)
    o_mine = OPT.FlatAdam(mine, lr=1e-2, weight_decay=1e-2)
    for step in range(6):
        o_ref.zero_grad()
        o_mine.zero_grad()
        for k, (a, b) in enumerate(zip(ref, mine)):
            if k > step:
                continue                                    # joins later: a group of its own
            gr = torch.randn(a.shape, generator=g)
            a.grad = gr.double()
            slot = OPT.live(OPT.grad_slot(b)) if k < step else None
            if slot is not None:                            # an adopted parameter: the gradient goes straight into its slot
                dst, direct = OPT.claim(slot)
                assert direct
                dst.copy_(gr)
            else:
                b.grad = gr.clone()
        o_ref.step()
        o_mine.step()
    assert [grp.numel for grp in o_mine.groups] == [1, 5, 67, 103]
    for a, b in zip(ref, mine):
        finite(b)
        TO._cmp(b, a, 1e-5)


WINDOW_GATHER = [(1, 70, 45, 32, 16), (3, 20, 50, 32, 16), (1, 50, 21, 32, 8), (3, 10, 11, 16, 8), (1, 9, 10, 4, 1), (3, 7, 6, 3, 1)]
WINDOW_BLEND = [(2, 70, 45, 32, 16), (3, 20, 50, 32, 16), (2, 50, 21, 32, 8), (2, 9, 10, 4, 1), (2, 40, 36, 16, 5)]


def family_small_ops(run):
    import test_ops_gpu as TO
    import test_window_gpu as TW
    dev = torch.device("cpu")
    for shape in ((2, 3, 1, 1), (1, 5, 7, 3)):
        for skip in (True, False):
            run.case("up2x_relu_add %s skip=%s" % (shape, skip))
            TO.test_up2x_relu_add(shape, skip, dev)
    run.case("patch_gather / logo_merge 128")
    TO.test_patch_gather_and_merge(128, dev)
    run.case("cross_entropy 3x2x17x19 with ignored pixels")
    TO.test_cross_entropy(dev)
    run.case("seg_counts 5x2x37x41")
    TO.test_seg_counts_and_scores(dev)
    layer_case(run, "gateddata", 16, 8, False, 1, True, N=3, other=5, seed=50)               # the gate MLP, forward and backward
    flat_adam_case(run)
    for c in WINDOW_GATHER:
        run.case("window_gather %s" % (c,))
        TW.test_window_gather_equals_indexing(*c, dev)
    for c in WINDOW_BLEND:
        run.case("window_blend %s" % (c,))
        TW.test_window_blend_against_float64(*c, dev)


# ------------------------------------------------------------------------------------------------------------------------ #
# The scalar bodies behind the kernels' 16-byte alignment guards.  Each guard ANDs a shape condition with a pointer test:
#   axial_fast.hip  attn_fwd (four rows per lane): axis == 1, W % 4 == 0, HW % 4 == 0     and qkv_raw | stacked | lse
#   conv_mfma.hip   conv_wgrad_v4_ok: stride 1, K == 1 with HW % 4 == 0 or K == 3 with W % 4 == 0   and dy | raw | x
#   elementwise.hip bn_fin_apply: HW % 4 == 0 and z | y | res;   up2x_relu_add_fwd: W even and y | skip
#   medt_api.hip    conv_block_bwd: dy | y | z | dres | dz
# When the shape condition holds the tensors' byte counts are multiples of 16, so the exact placements ("tail", "head") always
# satisfy the pointer test; only shapes that fail the shape condition reach the scalar bodies there.  This family runs shapes
# that PASS the shape condition in the arena's "offset" placement (every such tensor at 12 mod 16, one canary element behind
# it), so that the pointer test is what sends them to the scalar bodies; GUARD_POINTERS names the arguments the guards look at,
# and the test asserts each was seen misaligned.
# ------------------------------------------------------------------------------------------------------------------------ #
GUARD_POINTERS = {
    "axial_fast.hip attn_fwd rows4": ["medt_axial_layer_fwd:arg4.qkv_raw", "medt_axial_layer_fwd:arg4.stacked", "medt_axial_layer_fwd:arg4.lse"],
    "conv_mfma.hip conv_wgrad_v4_ok": ["medt_conv_block_bwd:arg7", "medt_conv_block_bwd:arg4", "medt_conv_block_bwd:arg1"],     # dy, raw (z), x
    "elementwise.hip bn_fin_apply": ["medt_conv_block_fwd:arg6", "medt_conv_block_fwd:arg7", "medt_conv_block_fwd:arg5"],         # z, y, res
    "elementwise.hip up2x_relu_add_fwd": ["medt_up2x_relu_add_fwd:arg2", "medt_up2x_relu_add_fwd:arg1"],                         # y, skip
    "medt_api.hip conv_block_bwd": ["medt_conv_block_bwd:arg7", "medt_conv_block_bwd:arg5", "medt_conv_block_bwd:arg13"],        # dy, y, dres
}


def family_offset_pointers(run):
    import test_ops_gpu as TO
    assert run.placement == "offset", "this family is about misaligned pointers: placement 'offset' only"
    dev = torch.device("cpu")
    for shape in ((2, 4, 2, 2), (2, 16, 16, 16)):                      # W even: the float4 kernel but for the pointers
        for skip in (True, False):
            run.case("up2x_relu_add %s skip=%s" % (shape, skip))
            TO.test_up2x_relu_add(shape, skip, dev)
    for case in _rows(TO.CONV_CASES, ["32-16-1-1-0-0-1-0-1-2-16-1", "16-32-1-1-0-0-1-1-1-4-8-2", "20-24-3-1-1-0-1-0-1-3-9-1"]):
        for training in (True, False):                                  # HW = 256 / 64 (% 4 == 0), with and without the residual
            run.case("conv_block %s %s" % ("-".join(str(int(v)) for v in case), "train" if training else "eval"))
            TO.test_conv_block(case, training, dev)
    for case in _rows(TO.RECORDED_CASES, ["32-16-1-1-0-1-2-16-1", "16-32-1-1-0-1-4-8-2", "16-16-3-1-1-1-2-8-1", "32-16-3-1-1-1-3-12-3"]):
        run.case("recorded wgrad %s" % "-".join(str(int(v)) for v in case))   # the 16-byte body's shapes (K = 1 and K = 3)
        TO.test_recorded_weight_gradient(case, dev)
    # MEDT_ROWS4=1 MEDT_BOUND_PATH=1: the four-rows forward on the width axis, W % 4 == 0 and HW % 4 == 0 (its 4-byte movers)
    for Cc, Lq, other in ((16, 64, 8), (16, 32, 7), (16, 16, 4), (32, 32, 6)):
        layer_case(run, "dynamic", Cc, Lq, True, 1, True, N=3, other=other, seed=60 + Lq)
    layer_case(run, "dynamic", 16, 32, False, 1, True, N=2, other=8, seed=61)


# ------------------------------------------------------------------------------------------------------------------------ #
def family_blocks(run):
    """The one-launch blocks through the real medt_wopos_block_* entry points (medt_amd.block), from the committed fixtures."""
    import test_block_gpu as TB
    import test_lane_emu as T
    from medt_amd import block
    dev, emu = torch.device("cpu"), run.proxy
    old = block.BWD_ENABLED
    try:
        emu.emu_set_block_bwd(1)
        block.BWD_ENABLED = True
        run.case("block 4x4 fwd + bwd, immediate (fixture)")
        TB.test_block_vs_reference_fixture(True, dev)
        assert emu.stats["entries"].get("medt_wopos_block_fwd") and emu.stats["entries"].get("medt_wopos_block_bwd")
        block.BWD_ENABLED = old
        run.case("block 4x4 fwd + bwd, recorded + flush, gradient slots (fixture)")
        T.test_block_node_with_gradient_slots_and_recorded_jobs(emu)
        run.case("block stride-2 first block fwd (fixture)")
        emu.emu_set_block_bwd(0)
        TB.test_stride2_block_vs_reference_fixture(True, dev)
        assert emu.stats["entries"].get("medt_wopos_block_s2_fwd")
        for training in (True, False):
            run.case("block 8x8 fwd %s" % ("train" if training else "eval"))
            T.test_block8_forward_kernel_on_the_emulator(emu, training, 0)
            run.case("block 8x8 bwd %s" % ("train" if training else "eval"))
            T.test_block8_backward_kernel_on_the_emulator(emu, training)
    finally:
        block.BWD_ENABLED = old
        emu.emu_set_block_bwd(0)


# ------------------------------------------------------------------------------------------------------------------------ #
def _train_steps(model_fn, batch_fn, steps, flip_at, arena=None):
    import medt_amd
    from medt_amd.optim import FlatAdam
    from medt_amd.trainer import TrainStep
    model = model_fn()
    if arena is not None:
        for p in list(model.parameters()) + list(model.buffers()):
            p.data = arena.copy_of(p.data)
    opt = FlatAdam(list(model.parameters()), lr=1e-3, weight_decay=1e-5)
    step = TrainStep(model, opt, medt_amd.cross_entropy, use_graph=False)
    trace = []
    for s in range(steps):
        if s == flip_at:
            for p in model.parameters():
                p.requires_grad = True                      # train.py:169-171: the gates join as a second group
        x, y = batch_fn(s)
        if arena is not None:
            from emu_device import DeviceTensor
            x, y = arena.copy_of(x).as_subclass(DeviceTensor), arena.copy_of(y).as_subclass(DeviceTensor)
        loss = float(step(x, y).detach())
        trace.append((loss, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}))
    return trace, {k: v.detach().clone() for k, v in model.state_dict().items()}, [g.numel for g in opt.groups]


def _train_reference(lib, model_fn, batch_fn, steps=2):
    from emu_device import emulated_device
    with emulated_device(lib):
        return _train_steps(model_fn, batch_fn, steps, 1)


def _train_family(run, model_fn, batch_fn, name, steps=2):
    """TrainStep(use_graph=False) + FlatAdam + the recorded jobs, two steps, every parameter trainable from the second (the
    gates' group and the GATES kernel instances).  Reference (run.ref, computed before the guarded device is entered): the same
    steps on the plain emulated device -- the same kernels on ordinary memory; tests/test_dp_cpu.py and test_lane_emu.py hold
    those to the reference -- losses to 1e-5, every gradient to 1e-4 of the tensor scale (test_dp_cpu's bound for another
    summation order: alignment picks other load widths), weights after the steps to 2e-3 of one lr step."""
    run.case(name)
    got, sd, groups = _train_steps(model_fn, batch_fn, steps, 1, run.arena)
    run.proxy.end_case()
    want, sd0, groups0 = run.ref
    assert groups == groups0 and len(groups) == min(steps, 2), (groups, groups0)
    for s, ((l1, g1), (l0, g0)) in enumerate(zip(got, want)):
        assert abs(l1 - l0) < 1e-5 * abs(l0), (s, l1, l0)
        assert set(g1) == set(g0)
        gmax = max(v.abs().max().item() for v in g0.values())
        for k in g0:
            finite(g1[k])
            err = (g1[k] - g0[k]).abs().max().item() / max(g0[k].abs().max().item(), 1e-3 * gmax)
            assert err < 1e-4, (s, k, err)
    for k in sd0:
        if sd0[k].is_floating_point():
            finite(sd[k])
            assert (sd[k] - sd0[k]).abs().max().item() < 2e-3 * 1e-3 + 1e-5 * sd0[k].abs().max().item(), k


def _gated32():
    import lib as droplib
    torch.manual_seed(100)
    return droplib.models.axialnet.gated(img_size=32, imgchan=3).train()


def _medt128():
    import lib as droplib
    torch.manual_seed(100)
    return droplib.models.axialnet.MedT(img_size=128, imgchan=3).train()


def _batches(N, S, seed):
    def batch_fn(s):
        from emu_device import DeviceTensor
        g = torch.Generator().manual_seed(seed + 10 * s)
        return (torch.rand(N, 3, S, S, generator=g).as_subclass(DeviceTensor),
                torch.randint(0, 2, (N, S, S), generator=g).as_subclass(DeviceTensor))
    return batch_fn


def family_train(run):
    _train_family(run, _gated32, _batches(2, 32, 8000), "TrainStep axialnet.gated 32 px N=2, two steps")


family_train.reference = lambda lib: _train_reference(lib, _gated32, _batches(2, 32, 8000))


def family_train_medt128(run):
    """MedT at 128 px (bench.py's network: both branches, the 16 patches of the local one), one image, one step: opt-in
    (MEDT_GUARD_FULL=1), minutes per placement on the emulator."""
    _train_family(run, _medt128, _batches(1, 128, 8100), "TrainStep MedT 128 px N=1, one step", steps=1)


family_train_medt128.reference = lambda lib: _train_reference(lib, _medt128, _batches(1, 128, 8100), steps=1)


FAMILIES = {"attention": family_attention, "attention_random": family_attention_random, "attention_repair": family_attention_repair,
            "conv": family_conv, "conv_rect": family_conv_rect, "recorded": family_recorded, "small_ops": family_small_ops, "blocks": family_blocks,
            "train": family_train, "train_medt128": family_train_medt128, "offset_pointers": family_offset_pointers}


def main(family, placement):
    faulthandler.enable()
    torch.set_num_threads(1)
    from guarded_mem import guarded_device
    os.environ.update(FAMILY_ENV.get(family, {}))             # (the library reads its switches once per process)
    run = Run(family, placement)
    lib = emu_lib()
    ref = getattr(FAMILIES[family], "reference", None)
    if ref is not None:
        run.ref = ref(lib)
    with guarded_device(lib, placement, allow=ALLOW, announce=Run.announce) as (arena, proxy):
        run.arena, run.proxy = arena, proxy
        FAMILIES[family](run)
        proxy.end_case()
    st = proxy.stats
    assert st["unguarded"] == 0, st
    canaries = arena.check_canaries()                       # ("offset" placement: nothing wrote the element behind a buffer)
    print(json.dumps({"family": family, "placement": placement, "cases": len(run.cases), "calls": st["calls"],
                      "pointers": st["pointers"], "in_arena": st["in_arena"], "stood_in": st["shadowed"], "allowed": st["allowed"],
                      "unguarded": st["unguarded"], "misaligned_calls": sum(st["misaligned_calls"].values()),
                      "misaligned_entries": sorted(st["misaligned_calls"]), "misaligned_pointers": st["misaligned_pointers"],
                      "canaries": canaries, "allocations": arena.allocations,
                      "arena_bytes": arena.bytes, "seconds": round(time.time() - run.t0, 1)}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
