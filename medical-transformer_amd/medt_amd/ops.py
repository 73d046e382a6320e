"""autograd.Functions over the C ABI for everything around the attention layers:
convolution blocks (conv + BatchNorm + residual + ReLU), bilinear-x2 + ReLU + skip,
the LoGo patch gather / merge and the cross-entropy loss.

Reference lines: lib/models/axialnet.py:285-300, 450-454, 475-502, 623-705; metrics.py:17-20.
PyTorch supplies device memory, the stream and the autograd graph only.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, NamedTuple

import torch

from . import _lib as L
from . import optim as OPT
from . import defer as DEFER
from .axial import _bn_ptrs, _momentum, _require_device


def _stream():
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------------------------- #
# y = act( BN( conv(x) + bias ) + res )
# --------------------------------------------------------------------------- #
class GradSink:
    """Gradient fan-in without add kernels.  A block input x feeds conv_down AND the residual / downsample path, the layer
    outputs x1..x3 also feed a decoder skip: the reference's autograd sums those gradients with one add kernel per extra
    consumer.  Consumers that share a sink hand their contribution over instead: whoever finishes its backward first
    deposits its gradient tensor here and returns nothing to autograd; the next one adds the deposit in the epilogue of
    its own dgrad kernel (medt_conv_block_bwd's dx_add) and either re-deposits the sum (role "deposit") or -- the
    consumer autograd runs last, conv_down: the earliest-created node -- returns it (role "final").  If the order ever
    differs (final already ran) a depositor simply returns its gradient the ordinary way."""
    __slots__ = ("pending", "closed")

    def __init__(self):
        self.pending, self.closed = None, False

    def deposit(self, t) -> bool:
        """True: taken (the caller returns None to autograd).  False: return the gradient normally."""
        if self.closed or self.pending is not None:
            return False
        self.pending = t
        return True

    def take(self):
        t, self.pending = self.pending, None
        return t


def sink_of(x):
    """The sink shared by the consumers of tensor x (created on first use)."""
    s = getattr(x, "_medt_sink", None)
    if s is None:
        s = x._medt_sink = GradSink()
    return s


# Scheduling hint (net.medt_forward sets it per call): True when the OTHER branch's stream runs CU-filling persistent kernels
# (MedT's global branch beyond 128 px): the local branch then keeps to kernels with small LDS footprints (medt_conv_desc.lean)
# Per THREAD (nn.DataParallel's thread-per-replica model, a validation thread next to a training thread): a forward of one thread
# must not change the kernels another thread's forward picks.
import threading
_hint = threading.local()


def set_lean(v: bool):
    _hint.lean = bool(v)


def lean() -> bool:
    return getattr(_hint, "lean", False)



class ConvBlockCfg:
    __slots__ = ("stride", "pad", "bn", "relu", "bn_groups", "x_sink", "x_role", "res_sink", "last_of_branch", "pre", "lean")

    def __init__(self, stride, pad, bn, relu, bn_groups=1, x_sink=None, x_role=None, res_sink=None, last_of_branch=False,
                 pre=None):
        self.stride, self.pad, self.bn, self.relu, self.bn_groups = stride, pad, bn, relu, bn_groups
        self.x_sink, self.x_role, self.res_sink = x_sink, x_role, res_sink
        self.last_of_branch = last_of_branch       # this block's backward is the last work of its stream's backward pass
        self.pre = pre                             # (z, y, stats) already computed by the one-launch block forward (block.py)
        self.lean = lean()


def _conv_desc(x, w, cfg: ConvBlockCfg, has_bias, has_res, training) -> L.ConvDesc:
    N, Cin, H, W = x.shape
    bn = cfg.bn
    return L.ConvDesc(N, Cin, H, W, w.shape[0], w.shape[2], cfg.stride, cfg.pad, int(has_bias), int(bn is not None),
                      int(has_res), int(cfg.relu), int(training), cfg.bn_groups,
                      bn.eps if bn is not None else 1e-5,
                      _momentum(bn) if bn is not None else 0.1, int(cfg.lean))


class ConvBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, bn_w, bn_b, res, cfg: ConvBlockCfg, training: bool):
        _require_device(x)
        lib = L.lib()
        x = x.contiguous()
        if res is not None:
            res = res.contiguous()
        desc = _conv_desc(x, w, cfg, bias is not None, res is not None, training)
        K, s, p = w.shape[2], cfg.stride, cfg.pad
        N, _, H, W = x.shape
        Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        has_bn = cfg.bn is not None
        if cfg.pre is not None:                    # adopt mode: the one-launch block forward already produced these
            z, y, stats = cfg.pre
            cfg.pre = None
        else:
            y = torch.empty((N, w.shape[0], Ho, Wo), device=x.device, dtype=torch.float32)
            z = torch.empty_like(y) if has_bn else y
            stats = torch.empty((max(lib.medt_conv_stats_floats(C.byref(desc)), 1),), device=x.device, dtype=torch.float32)
            ws_bytes = lib.medt_conv_workspace_bytes(C.byref(desc))
            if ws_bytes == 0:
                raise L.MedtError("conv block: " + lib.medt_last_error().decode())
            ws = torch.empty((ws_bytes,), device=x.device, dtype=torch.uint8)
            bnp = _bn_ptrs(cfg.bn, training) if has_bn else None
            # (recorded jobs write into stats at the flush: the BatchNorm finalisation, and the weight flip of a training-mode
            #  3x3 layer with or without BatchNorm -- the queue keeps both buffers alive until then)
            q = DEFER.recording() if (has_bn or stats.numel() > 1) else None
            L.check(lib.medt_conv_block_fwd(C.byref(desc), x.data_ptr(), w.data_ptr(), L.ptr(bias),
                                            C.byref(bnp) if has_bn else None, L.ptr(res), z.data_ptr(), y.data_ptr(),
                                            stats.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "medt_conv_block_fwd")
            if q is not None:
                q.hold(ws, stats)
        ctx.cfg, ctx.training, ctx.has_bias, ctx.has_res = cfg, training, bias is not None, res is not None
        # gradient slots of (w, bias, bn.weight, bn.bias) in FlatAdam's flat bucket: backward writes them directly
        ctx.slots = tuple(OPT.grad_slot(t) if t is not None else None for t in (w, bias, bn_w, bn_b))
        # (stats: the BatchNorm statistics and, behind them, the flipped weights a training-mode forward leaves for the MFMA
        #  backward-data kernel -- medt_conv_stats_floats says how much; layers without either bring a one-float dummy)
        ctx.save_for_backward(x, w, z if has_bn else None, y if (cfg.relu or has_bn) else None,
                              stats if (has_bn or stats.numel() > 1) else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.lib()
        x, w, z, y, stats = ctx.saved_tensors
        cfg, training = ctx.cfg, ctx.training
        dy = dy.contiguous()
        desc = _conv_desc(x, w, cfg, ctx.has_bias, ctx.has_res, training)
        has_bn = cfg.bn is not None
        dev = x.device
        Cout = w.shape[0]
        need_dx = ctx.needs_input_grad[0]
        dx = torch.empty_like(x) if need_dx else None
        # fan-in of the input's gradient (GradSink): add what the other consumers deposited in this dgrad's epilogue
        xs = cfg.x_sink if need_dx else None
        dep = xs.take() if xs is not None else None
        dx_add = dep if (dep is not None and w.shape[2] == 1) else None       # the dgrad epilogue add exists for 1x1 only
        present = (True, ctx.has_bias, has_bn, has_bn)
        shapes = (w.shape, (Cout,), (Cout,), (Cout,))
        dst, ret, pend = [None] * 4, [None] * 4, []
        for k in range(4):
            if not present[k]:
                continue
            slot = OPT.live(ctx.slots[k])
            if slot is not None and ctx.needs_input_grad[k + 1]:
                dst[k], direct = OPT.claim(slot)
                if not direct:
                    pend.append((slot, dst[k]))
            else:
                dst[k] = torch.empty(shapes[k], device=dev, dtype=torch.float32)
                if ctx.needs_input_grad[k + 1]:
                    ret[k] = dst[k]
        dres = torch.empty_like(dy) if ctx.has_res else None
        ws_bytes = lib.medt_conv_workspace_bytes(C.byref(desc))
        ws = torch.empty((ws_bytes,), device=dev, dtype=torch.uint8)
        bnp = _bn_ptrs(cfg.bn, False) if has_bn else None
        # parameter gradients may only be recorded for the grouped flush when they all land in persistent slots
        q = DEFER.recording(allow=not pend and all(r is None for r in ret))
        L.check(lib.medt_conv_block_bwd(C.byref(desc), x.data_ptr(), w.data_ptr(), C.byref(bnp) if has_bn else None,
                                        L.ptr(z), L.ptr(y), L.ptr(stats), dy.data_ptr(), L.ptr(dx), dst[0].data_ptr(),
                                        L.ptr(dst[1]), L.ptr(dst[2]), L.ptr(dst[3]), L.ptr(dres), L.ptr(dx_add), ws.data_ptr(),
                                        ws_bytes, _stream()), "medt_conv_block_bwd")
        if q is not None:                      # recorded weight / bias gradient jobs read these at the flush
            q.hold(ws, x, dy, stats, dres, *dst)
        for slot, tmp in pend:
            OPT.accumulate(slot, tmp)
        if dep is not None and dx_add is None:         # a wider consumer: the deposit is added explicitly, never dropped
            dx.add_(dep)
        if xs is not None:
            if cfg.x_role == "final":
                xs.closed = True
            elif xs.deposit(dx):                       # role "deposit": hand dx to the consumer that runs after this one
                dx = None
        if dres is not None and cfg.res_sink is not None and cfg.res_sink.deposit(dres):
            dres = None
        if cfg.last_of_branch:                         # nothing else of this branch follows: its recorded jobs go out now
            if DEFER.flush_current_stream():
                OPT.branch_done(0)                     # ... and (data parallel) its gradient bucket goes on the wire
        return (dx, ret[0], ret[1], ret[2], ret[3], dres, None, None)


def conv_block(x, conv, bn=None, res=None, relu=False, training=False, bn_groups=1, x_sink=None, x_role=None,
               res_sink=None, last_of_branch=False, pre=None):
    """conv: nn.Conv2d holder, bn: nn.BatchNorm2d holder or None.  x_sink / x_role / res_sink: see GradSink.
    pre: (z, y, stats) computed by the one-launch block forward (medt_amd.block) -- nothing is launched then."""
    cfg = ConvBlockCfg(conv.stride[0], conv.padding[0], bn, relu, bn_groups if bn is not None else 1, x_sink, x_role,
                       res_sink, last_of_branch, pre)
    if bn is None:
        # without BatchNorm the descriptor's `training` flag only says "a backward pass follows": the forward then leaves the
        # flipped weights of the MFMA backward-data kernel behind (medt_conv_stats_floats), off the backward chain
        training = torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad)
    return ConvBlockFn.apply(x, conv.weight, conv.bias, bn.weight if bn is not None else None,
                             bn.bias if bn is not None else None, res, cfg, training)


PAIR_CALLS = 0      # medt_conv_block_pair_fwd calls issued by this process (tests assert that the pair path is reached)


def conv_block_pair_pre(x, conv_a, bn_a, relu_a, conv_b, bn_b, relu_b, bn_groups=1):
    """The forwards of two 1x1 conv + BatchNorm blocks that read the same x (a first block's conv_down and its downsample
    path) in side-by-side launches (medt_conv_block_pair_fwd).  Returns ((z, y, stats) of a, (z, y, stats) of b): the two
    conv_block calls adopt them through `pre`, so the autograd graph and everything saved are those of two single calls.
    None when the pair does not apply (not both 1x1 with BatchNorm, or a residual input)."""
    global PAIR_CALLS
    if bn_a is None or bn_b is None or conv_a.bias is not None or conv_b.bias is not None:
        return None
    if conv_a.weight.shape[2] != 1 or conv_b.weight.shape[2] != 1:
        return None
    _require_device(x)
    lib = L.lib()
    x = x.contiguous()
    N, _, H, W = x.shape
    dev = x.device
    args, outs, held = [], [], []
    for conv, bn, relu in ((conv_a, bn_a, relu_a), (conv_b, bn_b, relu_b)):
        cfg = ConvBlockCfg(conv.stride[0], conv.padding[0], bn, relu, bn_groups)
        w = conv.weight
        desc = _conv_desc(x, w, cfg, False, False, bn.training)
        s, p = cfg.stride, cfg.pad
        y = torch.empty((N, w.shape[0], (H + 2 * p - 1) // s + 1, (W + 2 * p - 1) // s + 1), device=dev, dtype=torch.float32)
        z = torch.empty_like(y)
        stats = torch.empty((max(lib.medt_conv_stats_floats(C.byref(desc)), 1),), device=dev, dtype=torch.float32)
        ws_bytes = lib.medt_conv_workspace_bytes(C.byref(desc))
        if ws_bytes == 0:
            raise L.MedtError("conv block pair: " + lib.medt_last_error().decode())
        ws = torch.empty((ws_bytes,), device=dev, dtype=torch.uint8)
        bnp = _bn_ptrs(bn, bn.training)
        held += [desc, bnp, ws, stats]
        args += [C.byref(desc), x.data_ptr(), w.data_ptr(), None, C.byref(bnp), None, z.data_ptr(), y.data_ptr(),
                 stats.data_ptr(), ws.data_ptr(), ws_bytes]
        outs.append((z, y, stats))
    q = DEFER.recording()          # (the recorded BatchNorm finalisations write into stats at the flush)
    L.check(lib.medt_conv_block_pair_fwd(*args, _stream()), "medt_conv_block_pair_fwd")
    PAIR_CALLS += 1
    if q is not None:
        q.hold(*(t for t in held if isinstance(t, torch.Tensor)))
    return outs[0], outs[1]


# --------------------------------------------------------------------------- #
# y = relu(bilinear_x2(x)) + skip
# --------------------------------------------------------------------------- #
class UpReluAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip, skip_sink=None):
        ctx.skip_sink = skip_sink
        _require_device(x)
        lib = L.lib()
        x = x.contiguous()
        N, Cc, H, W = x.shape
        y = torch.empty((N, Cc, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
        if skip is not None:
            skip = skip.contiguous()
        L.check(lib.medt_up2x_relu_add_fwd(x.data_ptr(), L.ptr(skip), y.data_ptr(), N * Cc, H, W, _stream()),
                "medt_up2x_relu_add_fwd")
        ctx.save_for_backward(x)
        ctx.has_skip = skip is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.lib()
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        N, Cc, H, W = x.shape
        dx = torch.empty_like(x)
        L.check(lib.medt_up2x_relu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), N * Cc, H, W, _stream()),
                "medt_up2x_relu_bwd")
        dskip = dy if ctx.has_skip else None
        if dskip is not None and ctx.skip_sink is not None and ctx.skip_sink.deposit(dskip):
            dskip = None                               # the skip tensor's block adds it in its dgrad epilogue (GradSink)
        return dx, dskip, None


def up2x_relu_add(x, skip=None, skip_sink=None):
    return UpReluAddFn.apply(x, skip, skip_sink)


# --------------------------------------------------------------------------- #
# gate network of AxialAttention_gated_data
# --------------------------------------------------------------------------- #
class GateMlpFn(torch.autograd.Function):
    """(N,C,H,W) -> (B*, 4) per-sequence gates: sigmoid(relu(fcn2(relu(fcn1(mean over the sequence of x)))))
    (reference lib/models/model_codes.py:371-380)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, axis):
        _require_device(x)
        lib = L.lib()
        x = x.contiguous()
        N, Cc, H, W = x.shape
        nseq = N * (H if axis else W)
        dev = x.device
        xn = torch.empty((nseq, Cc), device=dev, dtype=torch.float32)
        h = torch.empty_like(xn)
        o = torch.empty((nseq, 4), device=dev, dtype=torch.float32)
        gates = torch.empty_like(o)
        L.check(lib.medt_gate_mlp_fwd(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                      xn.data_ptr(), h.data_ptr(), o.data_ptr(), gates.data_ptr(), N, Cc, H, W, axis,
                                      _stream()), "medt_gate_mlp_fwd")
        ctx.save_for_backward(w1, w2, xn, h, o, gates)
        ctx.geom = (N, Cc, H, W, axis)
        return gates

    @staticmethod
    def backward(ctx, dgates):
        lib = L.lib()
        w1, w2, xn, h, o, gates = ctx.saved_tensors
        N, Cc, H, W, axis = ctx.geom
        dev = dgates.device
        nseq = gates.shape[0]
        dgates = dgates.contiguous()
        scratch = torch.empty((nseq * (4 + 2 * Cc),), device=dev, dtype=torch.float32)
        dw1, db1 = torch.empty_like(w1), torch.empty((Cc,), device=dev, dtype=torch.float32)
        dw2, db2 = torch.empty_like(w2), torch.empty((4,), device=dev, dtype=torch.float32)
        dx = torch.empty((N, Cc, H, W), device=dev, dtype=torch.float32)
        L.check(lib.medt_gate_mlp_bwd(dgates.data_ptr(), gates.data_ptr(), o.data_ptr(), h.data_ptr(), xn.data_ptr(),
                                      w1.data_ptr(), w2.data_ptr(), scratch.data_ptr(), dw1.data_ptr(), db1.data_ptr(),
                                      dw2.data_ptr(), db2.data_ptr(), dx.data_ptr(), N, Cc, H, W, axis, _stream()),
                "medt_gate_mlp_bwd")
        return dx, dw1, db1, dw2, db2, None


def gate_mlp(x, fcn1, fcn2, width: bool):
    return GateMlpFn.apply(x, fcn1.weight, fcn1.bias, fcn2.weight, fcn2.bias, 1 if width else 0)


# --------------------------------------------------------------------------- #
# LoGo patches
# --------------------------------------------------------------------------- #
def patch_gather(x, P=32, G=4):
    """(N,C,S,S) image -> (G*G*N, C, P, P) patch-major stack.  Input images carry no gradient."""
    _require_device(x)
    x = x.contiguous()
    N, Cc, S, _ = x.shape
    xp = torch.empty((G * G * N, Cc, P, P), device=x.device, dtype=torch.float32)
    L.check(L.lib().medt_patch_gather(x.data_ptr(), xp.data_ptr(), N, Cc, S, P, G, _stream()), "medt_patch_gather")
    return xp


class LogoMergeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, yp, P, G):
        _require_device(x)
        x, yp = x.contiguous(), yp.contiguous()
        N, Cc, S, _ = x.shape
        y = torch.empty_like(x)
        L.check(L.lib().medt_logo_merge_fwd(x.data_ptr(), yp.data_ptr(), y.data_ptr(), N, Cc, S, P, G, _stream()),
                "medt_logo_merge_fwd")
        ctx.geom = (N, Cc, S, P, G)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, Cc, S, P, G = ctx.geom
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        dyp = torch.empty((G * G * N, Cc, P, P), device=dy.device, dtype=torch.float32)
        L.check(L.lib().medt_logo_merge_bwd(dy.data_ptr(), dx.data_ptr(), dyp.data_ptr(), N, Cc, S, P, G, _stream()),
                "medt_logo_merge_bwd")
        return dx, dyp, None, None


def logo_merge(x, yp, P=32, G=4):
    return LogoMergeFn.apply(x, yp, P, G)


# --------------------------------------------------------------------------- #
# cross entropy
# --------------------------------------------------------------------------- #
def _nkhw(logits):
    return logits.shape[0], logits.shape[1], logits[0, 0].numel()


def _grad_buffers(logits, dloss):
    """What every loss backward starts from -> (N, K, HW), the incoming gradient as float32, an empty dlogits."""
    return _nkhw(logits), dloss.contiguous().float(), torch.empty_like(logits)


class CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        _require_device(logits)
        lib = L.lib()
        logits, target = logits.contiguous(), target.contiguous()
        if target.dtype != torch.int64:
            raise L.MedtError("cross_entropy: int64 class-index targets expected")
        N, K, HW = _nkhw(logits)
        partials = torch.empty((lib.medt_ce_partials(N, HW),), device=logits.device, dtype=torch.float32)
        out = torch.empty((3,), device=logits.device, dtype=torch.float32)
        L.check(lib.medt_ce_fwd(logits.data_ptr(), target.data_ptr(), partials.data_ptr(), out.data_ptr(), N, K, HW,
                                ignore_index, _stream()), "medt_ce_fwd")
        ctx.save_for_backward(logits, target, out)
        ctx.ignore_index = ignore_index
        loss = out[0]
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)          # no zero-fill launch for the gradient of the non-differentiable output
        return loss, out

    @staticmethod
    def backward(ctx, dloss, _dout):
        if dloss is None:
            return None, None, None
        lib = L.lib()
        logits, target, out = ctx.saved_tensors
        (N, K, HW), dloss, dlogits = _grad_buffers(logits, dloss)
        L.check(lib.medt_ce_bwd(logits.data_ptr(), target.data_ptr(), out.data_ptr(), dloss.data_ptr(),
                                dlogits.data_ptr(), N, K, HW, ctx.ignore_index, _stream()), "medt_ce_bwd")
        return dlogits, None, None


CHECK_TARGETS = os.environ.get("MEDT_CHECK_TARGETS", "1") != "0"


def cross_entropy(logits, target, ignore_index=-100):
    """F.cross_entropy(logits, target) with mean reduction (what LogNLLLoss.forward computes, metrics.py:17-20).

    Class indices outside [0, K) that are not `ignore_index` make torch raise; here the kernel counts them and this
    wrapper raises MedtError from the count (one host sync; skipped while a hipGraph is being captured -- TrainStep
    checks the same counter after the replay -- and when MEDT_CHECK_TARGETS=0)."""
    loss, out = CrossEntropyFn.apply(logits, target, ignore_index)
    return _with_ce_out(loss, out, logits.shape[1])           # [mean loss, counted pixels, out-of-range targets]


def raise_on_bad_targets(out, K):
    bad = int(out[2].item())
    if bad:
        rng = f"[0, {K})" if K > 0 else "[0, num_classes)"
        raise L.MedtError(f"cross_entropy: {bad} target value(s) outside {rng} that are not ignore_index "
                          "(torch.nn.functional.cross_entropy raises on these too)")


def _with_ce_out(loss, out, K):
    """Attach the `out` whose slot 2 counts the out-of-range targets, and raise on them where a host sync is allowed."""
    loss._medt_ce_out = out
    if CHECK_TARGETS and not torch.cuda.is_current_stream_capturing():
        raise_on_bad_targets(out, K)
    return loss


# --------------------------------------------------------------------------- #
# class-weighted cross entropy + soft Dice
# --------------------------------------------------------------------------- #
def _region_fwd(what, logits, target, weight, N, K, HW, ce, dice, eps, ignore_index):
    """The region term's forward on contiguous logits / targets -> its `out`.  `what`: the public function, for the message."""
    lib = L.lib()
    nws, nout = lib.medt_seg_loss_workspace(N, K, HW), lib.medt_seg_loss_out_floats(N, K)
    if not nws or not nout:
        raise L.MedtError(f"{what}: {lib.medt_last_error().decode()}")
    partials = torch.empty((nws,), device=logits.device, dtype=torch.float32)
    out = torch.empty((nout,), device=logits.device, dtype=torch.float32)
    L.check(lib.medt_seg_loss_fwd(logits.data_ptr(), target.data_ptr(), L.ptr(weight), partials.data_ptr(), out.data_ptr(),
                                  N, K, HW, ignore_index, ce, dice, eps, _stream()), "medt_seg_loss_fwd")
    return out


def _region_bwd(logits, target, weight, out, dloss, dlogits, N, K, HW, ce, dice, eps, ignore_index):
    """The region term's backward: writes (does not add into) every element of `dlogits`."""
    L.check(L.lib().medt_seg_loss_bwd(logits.data_ptr(), target.data_ptr(), L.ptr(weight), out.data_ptr(), dloss.data_ptr(),
                                      dlogits.data_ptr(), N, K, HW, ignore_index, ce, dice, eps, _stream()),
            "medt_seg_loss_bwd")


class SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, ce, dice, eps, ignore_index):
        _require_device(logits)
        logits, target = logits.contiguous(), target.contiguous()
        out = _region_fwd("seg_loss", logits, target, weight, *_nkhw(logits), ce, dice, eps, ignore_index)
        ctx.save_for_backward(logits, target, out, weight)
        ctx.cfg = (ce, dice, eps, ignore_index)
        loss = out[0]
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)          # no zero-fill launch for the gradient of the non-differentiable output
        return loss, out

    @staticmethod
    def backward(ctx, dloss, _dout):
        if dloss is None:
            return (None,) * 7
        logits, target, out, weight = ctx.saved_tensors
        dims, dloss, dlogits = _grad_buffers(logits, dloss)
        _region_bwd(logits, target, weight, out, dloss, dlogits, *dims, *ctx.cfg)
        return (dlogits,) + (None,) * 6


def _region_args(what, logits, weight, ce, dice, eps, required=False):
    """The checks of the region term's options -> (weight, ce, dice, eps) as the nodes take them.  required: `what` is a
    seg_<term>_loss, which refuses ce == dice == 0 and names <term>_loss() for that."""
    K = logits.shape[1]
    if weight is not None:
        if (not torch.is_tensor(weight) or weight.dtype != torch.float32 or weight.dim() != 1 or weight.numel() != K
                or weight.device != logits.device):
            raise L.MedtError(f"{what}: weight must be a float32 tensor of {K} class weights on the logits' device")
        weight = weight.detach().contiguous()
    ce, dice, eps = float(ce), float(dice), float(eps)
    if required and ce == 0.0 and dice == 0.0:
        raise L.MedtError(f"{what}: no region term (ce == dice == 0): {what[len('seg_'):]}() is the term alone")
    if dice != 0.0 and not 2 <= K <= 8:
        raise L.MedtError(f"{what}: soft Dice needs 2 <= K <= 8 classes (K = {K})")
    if not eps >= 0.0:
        raise L.MedtError(f"{what}: eps >= 0 expected")
    return weight, ce, dice, eps


def seg_loss(logits, target, weight=None, ce=1.0, dice=0.0, eps=1.0, ignore_index=-100):
    """ce * CE + dice * Dice of (N,K,H,W) float32 logits against (N,H,W) int64 class indices, p = softmax over the classes.

    CE is F.cross_entropy(logits, target, weight=weight, ignore_index=ignore_index) with mean reduction -- what the
    reference's LogNLLLoss(weight=...) computes (metrics.py:17-20): sum w[t] nll / sum w[t] over the valid pixels (target
    not `ignore_index`), NaN when nothing is counted.  `weight`: a float32 tensor of K class weights on the logits'
    device, or None (all 1).

    Dice is 1 - mean over images n and classes k of (2 I_nk + eps) / (P_nk + T_nk + eps) with I_nk = sum p_ik [t_i = k],
    P_nk = sum p_ik, T_nk = sum [t_i = k] over the valid pixels of image n ONLY (2 <= K <= 8).  `eps` (default 1) keeps an
    image whose pixels are all ignored, or a class that is neither present nor predicted, finite with a zero or finite
    gradient.  Per image, not per batch, on purpose: under data parallel with equal shards the mean of the ranks'
    gradients is then exactly the gradient of the global batch, without another collective.  The weighted CE under data
    parallel is a mean of per-rank weighted means, as with DistributedDataParallel around F.cross_entropy(weight=...).

    Either scale may be 0; that term is then left out (the weighted CE alone takes any K).  Two forward launches and one backward launch whatever the options, no float atomics: eager and replayed
    steps agree bit for bit.  Class indices outside [0, K) that are not `ignore_index` are handled as in cross_entropy()
    above: excluded, counted, raised on here (outside graph capture) and by TrainStep.check_targets()."""
    if logits.dim() < 2 or logits.dtype != torch.float32:
        raise L.MedtError("seg_loss: float32 (N,K,...) logits expected")
    if target.dtype != torch.int64 or target.device != logits.device or target.numel() * logits.shape[1] != logits.numel():
        raise L.MedtError("seg_loss: int64 (N,...) class-index targets on the logits' device expected")
    weight, ce, dice, eps = _region_args("seg_loss", logits, weight, ce, dice, eps)
    loss, out = SegLossFn.apply(logits, target, weight, ce, dice, eps, int(ignore_index))
    return _with_ce_out(loss, out, logits.shape[1])       # [loss, sum of counted weights, out-of-range targets, CE, Dice, ...]


# --------------------------------------------------------------------------- #
# region loss + one weighted extra term on maps derived from the step's own label map: the boundary loss (Kervadec et al.,
# MIDL 2019) on its signed distance map, or the border weight for touching objects (Ronneberger et al., U-Net, 2015) on the
# distances to its two nearest components
# --------------------------------------------------------------------------- #
def _boundary_maps(target, fg, ignore_index, connectivity):
    return (signed_edt_sq(target, fg, ignore_index),)


def _border_maps(target, fg, ignore_index, connectivity):
    """{target == fg} as a uint8 mask (torch), label() -> object_edt2_sq(); nothing syncs."""
    mask = torch.empty(target.shape, device=target.device, dtype=torch.uint8)
    torch.eq(target, fg, out=mask)                             # F as the uint8 mask label() takes, in one launch
    if fg == ignore_index:                                     # an ignored pixel is not in F
        mask.zero_()
    labels, _ = label(mask, connectivity)
    return object_edt2_sq(labels)


class _Term(NamedTuple):
    """An extra term of the loss: its name in messages, the attribute of the loss that holds its `out`, the int32 maps it derives
    from (target, fg, ignore_index, connectivity), its C entry points.  Forward and backward take (logits, target, *maps,
    [sigma,] ...): sigma is None for a term without one."""
    what: str
    side: str
    maps: Callable
    workspace: str
    out_floats: str
    fwd: str
    bwd: str


BOUNDARY = _Term("boundary_loss", "_medt_boundary_out", _boundary_maps, "medt_boundary_workspace", "medt_boundary_out_floats",
                 "medt_boundary_fwd", "medt_boundary_bwd")
BORDER = _Term("border_loss", "_medt_border_out", _border_maps, "medt_border_workspace", "medt_border_out_floats",
               "medt_border_fwd", "medt_border_bwd")


class SegTermFn(torch.autograd.Function):
    """region loss (medt_seg_loss_*, unchanged; left out when ce == dice == 0) + scale * one extra term as ONE node: the term's
    finalize adds the region loss on the device, the term's backward adds into the region backward's dlogits."""

    @staticmethod
    def forward(ctx, logits, target, scale, weight, ce, dice, eps, fg, ignore_index, term, connectivity, sigma):
        _require_device(logits)
        lib = L.lib()
        logits, target = logits.contiguous(), target.contiguous()
        N, K, HW = _nkhw(logits)
        region = ce != 0.0 or dice != 0.0
        rout = _region_fwd("seg_" + term.what, logits, target, weight, N, K, HW, ce, dice, eps, ignore_index) if region else None
        maps = term.maps(target, fg, ignore_index, connectivity)
        nws, nout = getattr(lib, term.workspace)(N, HW), getattr(lib, term.out_floats)(N)
        if not nws or not nout:
            raise L.MedtError(f"{term.what}: {lib.medt_last_error().decode()}")
        parts = torch.empty((nws,), device=logits.device, dtype=torch.float32)
        tout = torch.empty((nout,), device=logits.device, dtype=torch.float32)
        head = [logits.data_ptr(), target.data_ptr()] + [m.data_ptr() for m in maps] + ([] if sigma is None else [sigma])
        L.check(getattr(lib, term.fwd)(*head, scale.data_ptr(), L.ptr(rout), parts.data_ptr(), tout.data_ptr(), N, K, HW, fg,
                                       ignore_index, _stream()), term.fwd)
        ctx.save_for_backward(logits, target, tout, rout, weight, *maps)           # (rout, weight: None where there is none)
        ctx.cfg = (ce, dice, eps, ignore_index)
        ctx.term = (term, fg, sigma)
        loss = tout[0]
        outs = (tout, rout) if region else (tout,)
        ctx.mark_non_differentiable(*outs)
        ctx.set_materialize_grads(False)
        return (loss,) + outs

    @staticmethod
    def backward(ctx, dloss, *_):
        if dloss is None:
            return (None,) * 12
        term, fg, sigma = ctx.term
        logits, target, tout, rout, weight, *maps = ctx.saved_tensors
        (N, K, HW), dloss, dlogits = _grad_buffers(logits, dloss)
        region = rout is not None
        if region:
            _region_bwd(logits, target, weight, rout, dloss, dlogits, N, K, HW, *ctx.cfg)
        head = [logits.data_ptr(), target.data_ptr()] + [m.data_ptr() for m in maps] + ([] if sigma is None else [sigma])
        L.check(getattr(L.lib(), term.bwd)(*head, tout.data_ptr(), dloss.data_ptr(), dlogits.data_ptr(), N, K, HW, fg, ctx.cfg[3],
                                           int(region), _stream()), term.bwd)
        return (dlogits,) + (None,) * 11


def _seg_term(term, logits, target, scale, region, fg, ignore_index, connectivity=None, sigma=None):
    """One SegTermFn node -> loss with its side outputs.  region: (weight, ce, dice, eps) as given to a seg_<term>_loss, None for
    the term alone."""
    K = logits.shape[1]
    weight, ce, dice, eps = (None, 0.0, 0.0, 1.0) if region is None else _region_args("seg_" + term.what, logits, *region, required=True)
    loss, tout, *rout = SegTermFn.apply(logits, target, scale, weight, ce, dice, eps, int(fg), int(ignore_index), term, connectivity,
                                        sigma)
    setattr(loss, term.side, tout)
    return _with_ce_out(loss, rout[0], K) if rout else loss


def _boundary_args(what, logits, target, alpha, fg):
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise L.MedtError(f"{what}: float32 (N,K,H,W) logits expected")
    if (target.dtype != torch.int64 or target.device != logits.device or target.dim() != 3
            or tuple(target.shape) != (logits.shape[0],) + tuple(logits.shape[2:])):
        raise L.MedtError(f"{what}: int64 (N,H,W) class-index targets on the logits' device expected")
    K = logits.shape[1]
    if K < 2 or not 0 <= int(fg) < K:
        raise L.MedtError(f"{what}: two classes or more and a foreground class in [0, K) expected (K = {K}, fg = {fg})")
    if torch.is_tensor(alpha):
        if alpha.dtype != torch.float32 or alpha.numel() != 1 or alpha.device != logits.device:
            raise L.MedtError(f"{what}: alpha must be one float32 on the logits' device (or a number)")
        return alpha.detach()
    return torch.full((1,), float(alpha), device=logits.device, dtype=torch.float32)


def boundary_loss(logits, target, alpha, fg=1, ignore_index=-100):
    """alpha * B, the boundary term alone, of (N,K,H,W) float32 logits against (N,H,W) int64 class indices:
    B = mean over images n of ( sum over the valid pixels p of phi_n(p) * softmax(logits)[n,fg,p] / max(1, V_n) ),
    phi = sqrt(sd2) outside F = {target == fg}, -(sqrt(-sd2) - 1) inside (0 on the inner border), sd2 = signed_edt_sq(target, fg)
    (Kervadec's one_hot2dist, computed on the device from the step's own label map, never stored as floats).  A pixel is valid
    when its target is in [0, K) and not `ignore_index`; the others contribute nothing and receive gradient exactly 0.  Per
    image, not per batch, for seg_loss's reason (equal shards under data parallel).  alpha: a one-element float32 device tensor,
    READ ON THE DEVICE by the kernels (refill it in place and a captured step follows), or a number.  Two launches for the map,
    two forward, one backward; no float atomics.  loss._medt_boundary_out = [alpha B, B, alpha, ...]."""
    alpha = _boundary_args("boundary_loss", logits, target, alpha, fg)
    return _seg_term(BOUNDARY, logits, target, alpha, None, fg, ignore_index)


def seg_boundary_loss(logits, target, alpha, weight=None, ce=1.0, dice=0.0, eps=1.0, fg=1, ignore_index=-100):
    """seg_loss(logits, target, weight, ce, dice, eps, ignore_index) + alpha * B with B of boundary_loss(), as one
    autograd node: the region term runs through the unchanged medt_seg_loss_* entry points, the boundary finalize adds it on the
    device and the boundary backward adds into the dlogits the region backward has just written -- one gradient buffer, no torch
    add.  With alpha == 0 loss and gradient are seg_loss's, bit for bit.  loss._medt_ce_out is the region term's `out` (so
    TrainStep.check_targets() works as with seg_loss), loss._medt_boundary_out = [loss, B, alpha, ...]."""
    alpha = _boundary_args("seg_boundary_loss", logits, target, alpha, fg)
    return _seg_term(BOUNDARY, logits, target, alpha, (weight, ce, dice, eps), fg, ignore_index)


def _border_args(what, logits, target, w0, sigma, fg, connectivity):
    """_boundary_args for w0, + sigma and the connectivity -> (w0 tensor, sigma)."""
    w0 = _boundary_args(what, logits, target, w0, fg)
    sigma = float(sigma)
    if not 0.0 < sigma < float("inf"):
        raise L.MedtError(f"{what}: sigma must be positive and finite (got {sigma})")
    if connectivity not in (4, 8):
        raise L.MedtError(f"{what}: connectivity {connectivity!r} (4 or 8)")
    return w0, sigma


def border_loss(logits, target, w0, sigma=5.0, fg=1, connectivity=8, ignore_index=-100):
    """w0 * R, the border term alone, of (N,K,H,W) float32 logits against (N,H,W) int64 class indices:
    R = mean over images n of ( sum over the valid pixels p of e_n(p) * nll_n(p) / max(1, V_n) ), nll = -log softmax(logits)[target],
    e = exp(-(d1 + d2)^2 / (2 sigma^2)) at the pixels outside F = {target == fg} that have two objects to be between, 0 elsewhere;
    d1, d2: the distances to the nearest and the second-nearest connected component of F (`connectivity` 4 or 8), from
    label() and object_edt2_sq() on the device, from the step's own label map.  U-Net's weight map w = 1 + w0 e applied to the
    cross entropy is mean cross entropy + w0 R.  Valid pixels as boundary_loss(); an ignored pixel is not in F.  w0: a one-element
    float32 device tensor, READ ON THE DEVICE by the kernels (refill it in place and a captured step follows), or a number.
    No host sync, no float atomics.  loss._medt_border_out = [w0 R, R, w0, ...]."""
    w0, sigma = _border_args("border_loss", logits, target, w0, sigma, fg, connectivity)
    return _seg_term(BORDER, logits, target, w0, None, fg, ignore_index, int(connectivity), sigma)


def seg_border_loss(logits, target, w0, sigma=5.0, weight=None, ce=1.0, dice=0.0, eps=1.0, fg=1, connectivity=8, ignore_index=-100):
    """seg_loss(logits, target, weight, ce, dice, eps, ignore_index) + w0 * R with R of border_loss(), as one autograd node: the
    region term runs through the unchanged medt_seg_loss_* entry points, the border finalize adds it on the device and the border
    backward adds into the dlogits the region backward has just written.  With w0 == 0 loss and gradient are seg_loss's, bit for
    bit.  loss._medt_ce_out is the region term's `out` (so TrainStep.check_targets() works as with seg_loss),
    loss._medt_border_out = [loss, R, w0, ...]."""
    w0, sigma = _border_args("seg_border_loss", logits, target, w0, sigma, fg, connectivity)
    return _seg_term(BORDER, logits, target, w0, (weight, ce, dice, eps), fg, ignore_index, int(connectivity), sigma)


# --------------------------------------------------------------------------- #
# segmentation scoring (replaces performancemetrics_*.m)
# --------------------------------------------------------------------------- #
def seg_counts(logits, target, threshold=0.5):
    """(N,K,H,W) logits, (N,H,W) int64 labels -> (N,4) int32 {tp, fp, fn, tn} of `logits[:,1] >= threshold` vs
    `target > 0`, counted on the device."""
    _require_device(logits)
    logits, target = logits.contiguous(), target.contiguous()
    if target.dtype != torch.int64:
        raise L.MedtError("seg_counts: int64 label maps expected")
    N, K = logits.shape[0], logits.shape[1]
    HW = logits[0, 0].numel()
    counts = torch.empty((N, 4), device=logits.device, dtype=torch.int32)
    L.check(L.lib().medt_seg_counts(logits.data_ptr(), target.data_ptr(), counts.data_ptr(), N, K, HW, float(threshold),
                                    _stream()), "medt_seg_counts")
    return counts


# --------------------------------------------------------------------------- #
# sliding windows over an image larger than the network input (medt_amd.window)
# --------------------------------------------------------------------------- #
def _window_origins(oy, ox, like):
    for o in (oy, ox):
        if o.dtype != torch.int32 or o.dim() != 1 or o.numel() < 1 or o.device != like.device:
            raise L.MedtError("window origins: non-empty 1-D int32 tensors on the image's device expected")
    return oy.contiguous(), ox.contiguous()


def window_gather(image, oy, ox, S, out=None):
    """(C,H,W) image -> (len(oy)*len(ox), C, S, S) windows, row-major, window (iy, ix) cut at (oy[iy], ox[ix]) with the
    source coordinates clamped to the image.  oy / ox: int32 device tensors.  `out`: a contiguous float32 buffer whose
    first T windows are written (WindowInfer keeps the padding of its last batch behind them)."""
    _require_device(image)
    if image.dim() != 3 or image.dtype != torch.float32:
        raise L.MedtError("window_gather: a float32 (C,H,W) image expected")
    image = image.contiguous()
    oy, ox = _window_origins(oy, ox, image)
    Cc, H, W = image.shape
    T = oy.numel() * ox.numel()
    if out is None:
        out = torch.empty((T, Cc, S, S), device=image.device, dtype=torch.float32)
    elif (out.dtype != torch.float32 or not out.is_contiguous() or out.device != image.device or out.dim() != 4
          or out.shape[0] < T or tuple(out.shape[1:]) != (Cc, S, S)):
        raise L.MedtError("window_gather: out must be a contiguous float32 (>=T,C,S,S) tensor on the image's device")
    L.check(L.lib().medt_window_gather(image.data_ptr(), out.data_ptr(), oy.data_ptr(), ox.data_ptr(), Cc, H, W, S,
                                       oy.numel(), ox.numel(), _stream()), "medt_window_gather")
    return out[:T]


def window_blend(win_logits, oy, ox, H, W, threshold=0.5, want_logits=True, want_mask=True):
    """(T,K,S,S) window logits -> (blended (K,H,W) float32 or None, mask (H,W) uint8 {0,255} or None): the weighted mean of
    the windows covering each pixel (weight min(i+1, S-i) per axis), mask = blended[1] >= threshold."""
    _require_device(win_logits)
    if win_logits.dim() != 4 or win_logits.shape[2] != win_logits.shape[3] or win_logits.dtype != torch.float32:
        raise L.MedtError("window_blend: float32 (T,K,S,S) window logits expected")
    if not (want_logits or want_mask):
        raise L.MedtError("window_blend: nothing asked for")
    win_logits = win_logits.contiguous()
    oy, ox = _window_origins(oy, ox, win_logits)
    T, K, S, _ = win_logits.shape
    if T != oy.numel() * ox.numel():
        raise L.MedtError(f"window_blend: {T} windows for a plan of {oy.numel()} x {ox.numel()}")
    blended = torch.empty((K, H, W), device=win_logits.device, dtype=torch.float32) if want_logits else None
    mask = torch.empty((H, W), device=win_logits.device, dtype=torch.uint8) if want_mask else None
    L.check(L.lib().medt_window_blend(win_logits.data_ptr(), L.ptr(blended), L.ptr(mask), oy.data_ptr(), ox.data_ptr(), K,
                                      H, W, S, oy.numel(), ox.numel(), float(threshold), _stream()), "medt_window_blend")
    return blended, mask


# --------------------------------------------------------------------------- #
# test-time augmentation: flipped / transposed views and the mean of their logits (medt_amd.tta)
# --------------------------------------------------------------------------- #
def _tta_views(what, views, H, W):
    views = int(views)
    if not 0 < views <= 0xFF:
        raise L.MedtError(f"{what}: views is a bitmask 0x01 .. 0xFF over the eight view codes (got {views:#x})")
    if views & 0xF0 and H != W:
        raise L.MedtError(f"{what}: views {views:#x} transpose, which needs square maps (got {H} x {W})")
    return views, bin(views).count("1")


def tta_expand(x, views, out=None):
    """(N,C,H,W) -> (N*V,C,H,W): out[n*V + j] = the j-th view (ascending code; bit 2 transpose, bit 1 flip rows, bit 0 flip
    columns) of x[n], a bit copy.  `out`: a contiguous float32 buffer whose first N*V items are written (TtaInfer keeps the
    padding of its last batch behind them)."""
    _require_device(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise L.MedtError("tta_expand: a float32 (N,C,H,W) batch expected")
    x = x.contiguous()
    N, Cc, H, W = x.shape
    views, V = _tta_views("tta_expand", views, H, W)
    if out is None:
        out = torch.empty((N * V, Cc, H, W), device=x.device, dtype=torch.float32)
    elif (out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device or out.dim() != 4
          or out.shape[0] < N * V or tuple(out.shape[1:]) != (Cc, H, W)):
        raise L.MedtError("tta_expand: out must be a contiguous float32 (>=N*V,C,H,W) tensor on the input's device")
    L.check(L.lib().medt_tta_expand(x.data_ptr(), out.data_ptr(), N, Cc, H, W, views, _stream()), "medt_tta_expand")
    return out[:N * V]


def tta_merge(view_logits, views, threshold=0.5, want_logits=True, want_mask=True, want_votes=False):
    """(N*V,K,H,W) view logits -> (merged (N,K,H,W) float32 or None, mask (N,H,W) uint8 {0,255} or None[, votes (N,H,W) uint8]):
    merged = the views mapped back, added in ascending code and divided by V; mask = merged[:,1] >= threshold; votes = how
    many views' own mapped-back foreground logit reaches the threshold (returned as a third item when asked for)."""
    _require_device(view_logits)
    if view_logits.dim() != 4 or view_logits.dtype != torch.float32:
        raise L.MedtError("tta_merge: float32 (N*V,K,H,W) view logits expected")
    if not (want_logits or want_mask or want_votes):
        raise L.MedtError("tta_merge: nothing asked for")
    view_logits = view_logits.contiguous()
    NV, K, H, W = view_logits.shape
    views, V = _tta_views("tta_merge", views, H, W)
    if NV < V or NV % V:
        raise L.MedtError(f"tta_merge: {NV} view logits for sets of {V} views")
    N = NV // V
    dev = view_logits.device
    merged = torch.empty((N, K, H, W), device=dev, dtype=torch.float32) if want_logits else None
    mask = torch.empty((N, H, W), device=dev, dtype=torch.uint8) if want_mask else None
    votes = torch.empty((N, H, W), device=dev, dtype=torch.uint8) if want_votes else None
    L.check(L.lib().medt_tta_merge(view_logits.data_ptr(), L.ptr(merged), L.ptr(mask), L.ptr(votes), N, K, H, W, views,
                                   float(threshold), _stream()), "medt_tta_merge")
    return (merged, mask, votes) if want_votes else (merged, mask)


# --------------------------------------------------------------------------- #
# joint augmentation of uint8 batches (medt_amd.augment)
# --------------------------------------------------------------------------- #
AUG_CONTRAST = 2.0          # operation code of a contrast slot (include/medt_abi.h)
AUG_ELASTIC_SLOT = 18       # record slot of the elastic flag
AUG_ELASTIC_MAX_GRID = 8    # cells per side of the elastic deformation's grid, at most


def augment_param_floats():
    return int(L.lib().medt_augment_param_floats())


def augment_workspace(N, size):
    """Floats of workspace for N images of output size (th, tw): the partial sums of the contrast mean, then the N means."""
    n = int(L.lib().medt_augment_workspace(int(N), int(size[0]), int(size[1])))
    if n == 0:
        raise L.MedtError(f"medt_augment_workspace: {L.lib().medt_last_error().decode()}")
    return n


def augment_batch(img_u8, mask_u8, params, size, out=None, workspace=None, host_params=None, field=None):
    """uint8 (N,H,W,C) images + uint8 (N,H,W) masks -> (float32 (N,C,th,tw) in [0,1], int64 (N,th,tw)): crop, flip, colour
    jitter and affine map of each image by its record of the float32 (N,P) device table `params` (medt_amd.augment.draw_record).
    size = (th, tw).  out: an (image, mask) pair to write into (contiguous; a view that is not 16-byte aligned takes the
    kernels' element stores).  workspace: augment_workspace() floats; after the call its last N floats hold the means the
    contrast operations used.  host_params: the table as a CPU tensor, when the caller has it (the prefetcher does): the origin
    check and the choice of launches read it instead of copying `params` back, which waits for the device.
    field: the float32 (N,2,G+3,G+3) control lattices of the elastic deformation on the images' device, 1 <= G <= 8
    (medt_amd.augment.draw_field); the records whose slot 18 is set are deformed by theirs (medt_augment_warp), and a batch
    in which none is set takes the launches it takes without a field."""
    if img_u8.dtype != torch.uint8 or mask_u8.dtype != torch.uint8:
        raise L.MedtError("augment_batch: uint8 images and masks expected")
    _require_device(params)                # (a float32 device tensor; images and masks must live where the table does, below)
    if img_u8.dim() != 4 or mask_u8.dim() != 3 or tuple(mask_u8.shape) != tuple(img_u8.shape[:3]):
        raise L.MedtError("augment_batch: an (N,H,W,C) image batch and its (N,H,W) masks expected")
    N, H, W, Cc = img_u8.shape
    th, tw = int(size[0]), int(size[1])
    P = augment_param_floats()
    if (params.dtype != torch.float32 or params.dim() != 2 or tuple(params.shape) != (N, P) or not params.is_contiguous()
            or params.device != img_u8.device or mask_u8.device != img_u8.device):
        raise L.MedtError(f"augment_batch: a contiguous float32 ({N},{P}) parameter table on the images' device expected")
    host = params.cpu() if host_params is None else host_params
    if tuple(host.shape) != (N, P):
        raise L.MedtError(f"augment_batch: host_params must be the ({N},{P}) table")
    cy, cx = host[:, 0], host[:, 1]
    if not (bool((cy >= 0).all()) and bool((cx >= 0).all()) and bool((cy + th <= H).all()) and bool((cx + tw <= W).all())):
        raise L.MedtError(f"augment_batch: a crop origin puts the {th} x {tw} window outside the {H} x {W} image")
    use_stats = bool((host[:, 10:14] == AUG_CONTRAST).any())
    G = 0
    if field is not None:
        _require_device(field)
        G = int(field.shape[-1]) - 3 if field.dim() == 4 else 0
        if (field.dtype != torch.float32 or field.dim() != 4 or tuple(field.shape) != (N, 2, G + 3, G + 3)
                or not 1 <= G <= AUG_ELASTIC_MAX_GRID or not field.is_contiguous() or field.device != img_u8.device):
            raise L.MedtError(f"augment_batch: field must be a contiguous float32 ({N},2,G+3,G+3) lattice on the images' device, "
                              f"1 <= G <= {AUG_ELASTIC_MAX_GRID}")
        if not bool((host[:, AUG_ELASTIC_SLOT] != 0).any()):
            field = None                   # no record asks for it: the launches of a call without a field
    img_u8, mask_u8 = img_u8.contiguous(), mask_u8.contiguous()
    if out is None:
        out = (torch.empty((N, Cc, th, tw), device=img_u8.device, dtype=torch.float32),
               torch.empty((N, th, tw), device=img_u8.device, dtype=torch.int64))
    oi, om = out
    if (oi.dtype != torch.float32 or om.dtype != torch.int64 or tuple(oi.shape) != (N, Cc, th, tw) or tuple(om.shape) != (N, th, tw)
            or not oi.is_contiguous() or not om.is_contiguous() or oi.device != img_u8.device or om.device != img_u8.device):
        raise L.MedtError("augment_batch: out must be contiguous float32 (N,C,th,tw) and int64 (N,th,tw) tensors on the images' device")
    if workspace is None and use_stats:
        workspace = torch.empty(augment_workspace(N, (th, tw)), device=img_u8.device, dtype=torch.float32)
    if workspace is not None and (workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.device != img_u8.device
                                  or workspace.numel() < augment_workspace(N, (th, tw))):
        raise L.MedtError("augment_batch: workspace must hold augment_workspace() float32 on the images' device")
    lib = L.lib()
    if use_stats:
        L.check(lib.medt_augment_stats(img_u8.data_ptr(), params.data_ptr(), workspace.data_ptr(), N, H, W, Cc, th, tw, _stream()),
                "medt_augment_stats")
    if field is not None:
        L.check(lib.medt_augment_warp(img_u8.data_ptr(), mask_u8.data_ptr(), params.data_ptr(), field.data_ptr(), G, L.ptr(workspace),
                                      oi.data_ptr(), om.data_ptr(), N, H, W, Cc, th, tw, int(use_stats), _stream()),
                "medt_augment_warp")
        return oi, om
    L.check(lib.medt_augment_apply(img_u8.data_ptr(), mask_u8.data_ptr(), params.data_ptr(), L.ptr(workspace), oi.data_ptr(),
                                   om.data_ptr(), N, H, W, Cc, th, tw, int(use_stats), _stream()), "medt_augment_apply")
    return oi, om


# --------------------------------------------------------------------------- #
# exact squared Euclidean distance transform (metrics.surface_scores)
# --------------------------------------------------------------------------- #
EDT_NONE = 2 ** 31 - 1      # MEDT_EDT_NONE (include/medt_abi.h): what an image without a feature pixel holds everywhere


def _edt_masks(what, *masks):
    """uint8 (N,H,W) or (H,W) masks of one shape on one device -> contiguous (N,H,W) views."""
    m0 = masks[0]
    _require_device(m0.new_empty(0, dtype=torch.float32))          # (the device check; the masks themselves are uint8)
    for m in masks:
        if m.dtype != torch.uint8 or m.dim() not in (2, 3) or m.shape != m0.shape or m.device != m0.device:
            raise L.MedtError(f"{what}: uint8 (N,H,W) or (H,W) masks of one shape on one device expected")
    if m0.numel() == 0:
        raise L.MedtError(f"{what}: empty mask")
    return [m.contiguous().reshape(-1, *m.shape[-2:]) for m in masks]


def _edt_out(what, out, like):
    if out is None:
        return torch.empty(like.shape, device=like.device, dtype=torch.int32)
    if out.dtype != torch.int32 or tuple(out.shape) != tuple(like.shape) or not out.is_contiguous() or out.device != like.device:
        raise L.MedtError(f"{what}: out must be a contiguous int32 tensor of the masks' shape on their device")
    return out


def edt_sq(mask, border=False, out=None):
    """uint8 (N,H,W) or (H,W) mask -> int32 of the same shape: the exact squared Euclidean distance of every pixel to the
    nearest pixel of mask != 0 (`distance_transform_edt(mask == 0) ** 2`), or with border=True to the nearest BORDER pixel of
    mask != 0 (a foreground pixel with a 4-neighbour outside the foreground or outside the image).  EDT_NONE everywhere in an
    image without foreground.  At most 4096 pixels per side.  out: an int32 tensor to write into (a view that is not
    16-byte aligned takes the kernels' element accesses)."""
    (m,) = _edt_masks("edt_sq", mask)
    N, H, W = m.shape
    d2 = _edt_out("edt_sq", out, mask)
    g2 = torch.empty(m.shape, device=m.device, dtype=torch.int32)
    lib = L.lib()
    L.check(lib.medt_edt_cols(m.data_ptr(), g2.data_ptr(), N, H, W, int(bool(border)), _stream()), "medt_edt_cols")
    L.check(lib.medt_edt_rows(g2.data_ptr(), None, d2.data_ptr(), N, H, W, _stream()), "medt_edt_rows")
    return d2


def surface_d2(a, b, out=None):
    """Two uint8 masks (N,H,W) or (H,W) -> int32 of the same shape: at the border pixels of a != 0 the squared distance to the
    nearest border pixel of b != 0 (EDT_NONE when b has none), -1 at every other pixel.  The border of b is never stored."""
    ma, mb = _edt_masks("surface_d2", a, b)
    N, H, W = ma.shape
    d2 = _edt_out("surface_d2", out, a)
    g2 = torch.empty(ma.shape, device=ma.device, dtype=torch.int32)
    lib = L.lib()
    L.check(lib.medt_edt_cols(mb.data_ptr(), g2.data_ptr(), N, H, W, 1, _stream()), "medt_edt_cols")
    L.check(lib.medt_edt_rows(g2.data_ptr(), ma.data_ptr(), d2.data_ptr(), N, H, W, _stream()), "medt_edt_rows")
    return d2


def signed_edt_sq(target, fg=1, ignore_index=-100, out=None):
    """int64 (N,H,W) or (H,W) class indices -> int32 of the same shape: the signed squared Euclidean distance to the boundary of
    F = {target == fg}: +d^2 to the nearest pixel of F at a pixel outside F (>= 1), -d^2 to the nearest pixel outside F at a
    pixel of F (<= -1).  Ignored pixels, other classes and class indices out of range are all outside F.  An image without F
    holds 0 everywhere, and so does an image that is all F (SciPy's value for an input without a zero is arbitrary).  Exact and
    bit-identical from run to run; at most 4096 pixels per side.  out: a contiguous int32 tensor to write into (any alignment:
    the kernels use element accesses).  The label map of the training step as it stands: no uint8 copy is made."""
    _require_device(target.new_empty(0, dtype=torch.float32))      # (the device check; the label map itself is int64)
    if target.dtype != torch.int64 or target.dim() not in (2, 3):
        raise L.MedtError("signed_edt_sq: an int64 (N,H,W) or (H,W) map of class indices expected")
    if target.numel() == 0:
        raise L.MedtError("signed_edt_sq: empty label map")
    fg, ignore_index = int(fg), int(ignore_index)
    if fg < 0:
        raise L.MedtError(f"signed_edt_sq: foreground class {fg}: a class index >= 0 expected")
    t = target.contiguous().reshape(-1, *target.shape[-2:])
    N, H, W = t.shape
    sd2 = _edt_out("signed_edt_sq", out, target)
    g2 = torch.empty(t.shape, device=t.device, dtype=torch.int32)
    L.check(L.lib().medt_signed_edt(t.data_ptr(), g2.data_ptr(), sd2.data_ptr(), N, H, W, fg, ignore_index, _stream()),
            "medt_signed_edt")
    return sd2


def object_edt2_sq(labels, out=None):
    """int32 (N,H,W) or (H,W) label map (0: no object, l > 0: object l, as label() writes it) -> (d1sq, d2sq), int32 of the same
    shape: the exact squared Euclidean distances to the nearest object (0 inside one) and to the nearest object other than that
    one -- the two smallest of the per-object minimum distances; inside object l, d2sq is the distance to the nearest other
    object.  EDT_NONE where there is no such object: d1sq in an image without objects, d2sq in an image with fewer than two.
    Bit-identical from run to run; at most 4096 pixels per side.  out: a pair of contiguous int32 tensors to write into (any
    alignment: the kernels use element accesses)."""
    _require_device(labels.new_empty(0, dtype=torch.float32))      # (the device check; the label map itself is int32)
    if labels.dtype != torch.int32 or labels.dim() not in (2, 3):
        raise L.MedtError("object_edt2_sq: an int32 (N,H,W) or (H,W) label map expected")
    if labels.numel() == 0:
        raise L.MedtError("object_edt2_sq: empty label map")
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
        raise L.MedtError("object_edt2_sq: out must be a pair (d1sq, d2sq) of int32 tensors")
    lab = labels.contiguous().reshape(-1, *labels.shape[-2:])
    N, H, W = lab.shape
    d1 = _edt_out("object_edt2_sq", None if out is None else out[0], labels)
    d2 = _edt_out("object_edt2_sq", None if out is None else out[1], labels)
    scratch = torch.empty((4,) + tuple(lab.shape), device=lab.device, dtype=torch.int32)       # g1 | a | g2 | b (medt_abi.h)
    L.check(L.lib().medt_object_edt2(lab.data_ptr(), scratch.data_ptr(), d1.data_ptr(), d2.data_ptr(), N, H, W, _stream()),
            "medt_object_edt2")
    return d1, d2


# --------------------------------------------------------------------------- #
# connected-component labelling, component tables, mask clean-ups (metrics.object_scores)
# --------------------------------------------------------------------------- #
LABEL_TILE = (16, 64)       # (MEDT_LABEL_TILE_H, MEDT_LABEL_TILE_W) of include/medt_abi.h: the tile of the LDS union-find


def _label_maps(what, labels, counts):
    """int32 (N,H,W) or (H,W) label map + int32 (N,) counts on its device -> contiguous (N,H,W) view, counts."""
    _require_device(labels.new_empty(0, dtype=torch.float32))
    if labels.dtype != torch.int32 or labels.dim() not in (2, 3) or labels.numel() == 0:
        raise L.MedtError(f"{what}: an int32 (N,H,W) or (H,W) label map expected")
    lab = labels.contiguous().reshape(-1, *labels.shape[-2:])
    if counts.dtype != torch.int32 or tuple(counts.shape) != (lab.shape[0],) or counts.device != labels.device:
        raise L.MedtError(f"{what}: counts must be int32 ({lab.shape[0]},) on the label map's device")
    return lab, counts.contiguous()


def label(mask, connectivity=8, background=False, out=None):
    """uint8 (N,H,W) or (H,W) mask -> (labels, counts): the connected components of mask != 0 (background=True: of mask == 0)
    at connectivity 4 or 8.  labels: int32 of the mask's shape, 0 outside the labelled set, 1..counts[n] inside, numbered per
    image in raster order of each component's first pixel -- `scipy.ndimage.label(mask, structure)[0]` with structure None (4) or
    np.ones((3,3)) (8), bit for bit and the same on every run.  counts: int32 (N,).  Components never join across images.
    At most 4096 pixels per side.  out: an int32 tensor to write the labels into (a view that is not 16-byte aligned takes the
    kernels' element accesses)."""
    (m,) = _edt_masks("label", mask)
    N, H, W = m.shape
    if connectivity not in (4, 8):
        raise L.MedtError(f"label: connectivity {connectivity!r} (4 or 8)")
    labels = _edt_out("label", out, mask)
    counts = torch.empty(N, device=m.device, dtype=torch.int32)
    lib = L.lib()
    need = lib.medt_label_workspace_bytes(N, H, W)             # (0 for a geometry the call below refuses, with the reason)
    workspace = torch.empty(max((need + 3) // 4, 4), device=m.device, dtype=torch.int32)
    L.check(lib.medt_label_components(m.data_ptr(), labels.data_ptr(), counts.data_ptr(), workspace.data_ptr(), need, N, H, W,
                                      int(connectivity), int(bool(background)), _stream()), "medt_label_components")
    return labels, counts


def label_tables(labels, counts):
    """Label map (N,H,W) or (H,W) int32 and its counts (N,) -> (area, frame), both (N, stride) with stride = counts.max() + 1
    (one host sync): int32 area[n,l] = pixels of label l (slot 0: the unlabelled rest) and uint8 frame[n,l] = 1 when component
    l has a pixel in the first or last row or column of its image."""
    lab, cnt = _label_maps("label_tables", labels, counts)
    N, H, W = lab.shape
    top = int(cnt.max())
    stride = top + 1
    area = torch.empty(N, stride, device=lab.device, dtype=torch.int32)
    frame = torch.empty(N, stride, device=lab.device, dtype=torch.uint8)
    L.check(L.lib().medt_label_tables(lab.data_ptr(), area.data_ptr(), frame.data_ptr(), N, H, W, stride, top, _stream()),
            "medt_label_tables")
    return area, frame


def _label_select(lab, keep, mask, shape):
    N, H, W = lab.shape
    out = torch.empty(N, H, W, device=lab.device, dtype=torch.uint8)
    keep = keep.to(torch.uint8).contiguous()
    L.check(L.lib().medt_label_select(lab.data_ptr(), keep.data_ptr(), None if mask is None else mask.data_ptr(), out.data_ptr(),
                                      N, H, W, keep.shape[1], _stream()), "medt_label_select")
    return out.reshape(shape)


def remove_small_objects(mask, min_area, connectivity=8):
    """uint8 mask (N,H,W) or (H,W) -> uint8 {0,255} mask of the same shape that keeps the connected components of mask != 0
    with at least min_area pixels."""
    (m,) = _edt_masks("remove_small_objects", mask)
    labels, counts = label(m, connectivity)
    area, _ = label_tables(labels, counts)
    keep = area >= int(min_area)
    keep[:, 0] = False
    return _label_select(labels, keep, None, mask.shape)


def fill_holes(mask):
    """uint8 mask (N,H,W) or (H,W) -> uint8 {0,255} mask: mask != 0 with its holes filled,
    `scipy.ndimage.binary_fill_holes(mask != 0)` -- the 4-connected components of the background that do not reach the image's
    frame are set."""
    (m,) = _edt_masks("fill_holes", mask)
    labels, counts = label(m, 4, background=True)
    _, frame = label_tables(labels, counts)
    keep = frame == 0
    keep[:, 0] = False
    return _label_select(labels, keep, m, mask.shape)


def label_overlaps(la, ca, lb, cb):
    """Two label maps of one shape with their counts -> int64 (M,4) rows (n, a, b, |a ∩ b|) for every pair of labels a > 0 of
    la and b > 0 of lb that share a pixel of image n, sorted by (n, a, b).  (A torch.unique over an int64 key: plumbing.)"""
    A, ca = _label_maps("label_overlaps", la, ca)
    B, cb = _label_maps("label_overlaps", lb, cb)
    if A.shape != B.shape or A.device != B.device:
        raise L.MedtError("label_overlaps: label maps of one shape on one device expected")
    N = A.shape[0]
    sa, sb = int(ca.max()) + 1, int(cb.max()) + 1
    a, b = A.reshape(N, -1).long(), B.reshape(N, -1).long()
    n = torch.arange(N, device=A.device, dtype=torch.int64).unsqueeze(1).expand_as(a)
    both = (a > 0) & (b > 0)
    key, cnt = torch.unique(((n * sa + a) * sb + b)[both], return_counts=True)          # (sorted)
    return torch.stack([key // (sa * sb), key // sb % sa, key % sb, cnt], dim=1)


# --------------------------------------------------------------------------- #
# bounding boxes and per-pair directed Hausdorff distances (metrics.object_hausdorff)
# --------------------------------------------------------------------------- #
PAIR_JOB_INTS = 16                 # MEDT_PAIR_JOB_INTS of include/medt_abi.h: int32 per record of the job table
PAIR_THREADS = 256                 # work-items of a workgroup: a job takes ceil(feature columns / 256) blocks of the column launch
PAIR_SCRATCH_ELEMS = 1 << 24       # default bound of the scratch of one chunk of jobs, in int32 elements (64 MiB): the g2 of one
                                   # whole 4096 x 4096 map, the largest a single job can need, so no job ever exceeds the default


def label_boxes(labels, counts):
    """Label map (N,H,W) or (H,W) int32 and its counts (N,) -> int32 (N, stride, 4) with stride = counts.max() + 1 (one host
    sync): (y0, x0, y1, x1), inclusive, of every label; (H, W, -1, -1) for a label without a pixel and for slot 0."""
    lab, cnt = _label_maps("label_boxes", labels, counts)
    N, H, W = lab.shape
    top = int(cnt.max())
    stride = top + 1
    box = torch.empty(N, stride, 4, device=lab.device, dtype=torch.int32)
    L.check(L.lib().medt_label_boxes(lab.data_ptr(), box.data_ptr(), N, H, W, stride, top, _stream()), "medt_label_boxes")
    return box


def _pair_chunks(sizes, budget):
    """Greedy cut of the jobs, in order, into chunks [start, end) whose summed sizes stay at or below budget; a job larger than
    the budget is a chunk of its own."""
    cum = torch.cumsum(sizes, 0)
    chunks, start, J = [], 0, sizes.numel()
    while start < J:
        before = int(cum[start - 1]) if start else 0
        end = int(torch.searchsorted(cum, torch.tensor(before + budget), right=True))
        end = max(end, start + 1)
        chunks.append((start, end))
        start = end
    return chunks


def pair_hausdorff_sq(la, ca, lb, cb, pairs, max_scratch_elems=None, boxes=None):
    """Two label maps of one shape with their counts and int32 (M,3) rows (n, a, b) -> int32 (M,2) on the maps' device:
      [:,0] = max over the pixels x of object a of la[n] of min over the pixels y of object b of lb[n] of |x - y|^2,
      [:,1] = the same from b to a,
    exact integers over ALL pixels of both objects (the two directed squared Hausdorff distances of the pair).  A pair that
    names a label outside 1..count or one without a pixel is refused (MEDT_EINVAL), on the host, from the bounding boxes.
    Every pair is two jobs (one per direction) of a device job table; a job's scratch is (rows of the query object's box) x
    (columns of the feature object's box) int32, and the jobs are issued in chunks whose summed scratch stays at or below
    max_scratch_elems (default PAIR_SCRATCH_ELEMS); a job that alone is larger runs alone.  boxes: (label_boxes(la, ca),
    label_boxes(lb, cb)) when the caller has them already, on any device."""
    A, ca = _label_maps("pair_hausdorff_sq", la, ca)
    B, cb = _label_maps("pair_hausdorff_sq", lb, cb)
    if A.shape != B.shape or A.device != B.device:
        raise L.MedtError("pair_hausdorff_sq: label maps of one shape on one device expected")
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 3:
        raise L.MedtError("pair_hausdorff_sq: pairs must be int32 (M,3) rows (n, a, b)")
    N, H, W = A.shape
    M = pairs.shape[0]
    out = torch.empty(M, 2, device=A.device, dtype=torch.int32)      # (the first call below zeroes it)
    if M == 0:
        return out
    budget = PAIR_SCRATCH_ELEMS if max_scratch_elems is None else int(max_scratch_elems)
    if budget < 1:
        raise L.MedtError(f"pair_hausdorff_sq: max_scratch_elems {max_scratch_elems!r} (at least 1)")
    budget = min(budget, 2 ** 31 - 1)
    ba, bb = boxes if boxes is not None else (label_boxes(A, ca), label_boxes(B, cb))
    ba, bb = torch.as_tensor(ba).cpu().long().reshape(N, -1, 4), torch.as_tensor(bb).cpu().long().reshape(N, -1, 4)
    p = torch.as_tensor(pairs).cpu().long()
    n, a, b = p[:, 0], p[:, 1], p[:, 2]
    if bool(((n < 0) | (n >= N)).any()):
        raise L.MedtError(f"pair_hausdorff_sq failed (-1): an image index outside 0..{N - 1}")
    if bool(((a < 1) | (a >= ba.shape[1]) | (b < 1) | (b >= bb.shape[1])).any()):
        raise L.MedtError("pair_hausdorff_sq failed (-1): a pair names a label outside 1..count")
    qa, qb = ba[n, a], bb[n, b]                                    # (M,4) boxes y0, x0, y1, x1
    if bool(((qa[:, 2] < 0) | (qb[:, 2] < 0)).any()):
        bad = int(torch.nonzero((qa[:, 2] < 0) | (qb[:, 2] < 0))[0])
        raise L.MedtError(f"pair_hausdorff_sq failed (-1): pair {p[bad].tolist()} names a label without a pixel")
    # two jobs per pair, interleaved: 2m is a -> b (query in la), 2m + 1 is b -> a (query in lb)
    J = 2 * M
    q = torch.stack([qa, qb], 1).reshape(J, 4)                     # the query object's box
    f = torch.stack([qb, qa], 1).reshape(J, 4)                     # the feature object's
    table = torch.zeros(J, PAIR_JOB_INTS, dtype=torch.int64)
    table[:, 0] = n.repeat_interleave(2)
    table[:, 1] = torch.stack([a, b], 1).reshape(J)
    table[:, 2] = torch.stack([b, a], 1).reshape(J)
    table[:, 3] = torch.arange(J) % 2
    table[:, 4], table[:, 5], table[:, 6], table[:, 7] = q[:, 0], q[:, 2], q[:, 1], q[:, 3]
    table[:, 8], table[:, 9] = f[:, 1], f[:, 3]
    table[:, 10], table[:, 11] = torch.minimum(q[:, 0], f[:, 0]), torch.maximum(q[:, 2], f[:, 2])
    table[:, 13] = torch.arange(J)
    rows = q[:, 2] - q[:, 0] + 1
    cols = f[:, 3] - f[:, 1] + 1
    sizes = rows * cols
    colb = (cols + PAIR_THREADS - 1) // PAIR_THREADS
    chunks = _pair_chunks(sizes, budget)
    scratch = torch.empty(max(int(sizes[s:e].sum()) for s, e in chunks), device=A.device, dtype=torch.int32)
    lib = L.lib()
    for k, (s, e) in enumerate(chunks):
        t = table[s:e].clone()
        t[:, 12] = torch.cumsum(sizes[s:e], 0) - sizes[s:e]
        t[:, 14] = torch.cumsum(colb[s:e], 0) - colb[s:e]
        t[:, 15] = torch.cumsum(rows[s:e], 0) - rows[s:e]
        jobs = t.to(torch.int32).to(A.device)
        L.check(lib.medt_pair_hausdorff(A.data_ptr(), B.data_ptr(), jobs.data_ptr(), scratch.data_ptr(), out.data_ptr(), e - s,
                                        int(colb[s:e].sum()), int(rows[s:e].sum()), scratch.numel(), J, int(k == 0), N, H, W,
                                        _stream()), "medt_pair_hausdorff")
    return out


# --------------------------------------------------------------------------- #
# splitting touching objects: peak markers of the depth map, marker-controlled growth (test.py --split)
# --------------------------------------------------------------------------- #
SPLIT_MAX_DISTANCE = 32            # MEDT_SPLIT_MAX_DISTANCE of include/medt_abi.h: the largest window radius
SPLIT_MAX_TOLERANCE = 8            # MEDT_SPLIT_MAX_TOLERANCE
GROW_MAX_PASSES = 64               # MEDT_GROW_MAX_PASSES: passes of one medt_grow_passes call
GROW_BATCHES = (2, 4, 8, 16)       # passes issued per host read of their "changed" flags; the last size repeats


def _split_args(what, distance, tolerance, connectivity):
    if connectivity not in (4, 8):
        raise L.MedtError(f"{what}: connectivity {connectivity!r} (4 or 8)")
    if isinstance(distance, bool) or not isinstance(distance, int) or not 1 <= distance <= SPLIT_MAX_DISTANCE:
        raise L.MedtError(f"{what}: distance {distance!r} (an integer window radius, 1 .. {SPLIT_MAX_DISTANCE})")
    if isinstance(tolerance, bool) or not isinstance(tolerance, int) or not 0 <= tolerance <= SPLIT_MAX_TOLERANCE:
        raise L.MedtError(f"{what}: tolerance {tolerance!r} (an integer number of pixels, 0 .. {SPLIT_MAX_TOLERANCE})")


def _split_markers(m, distance, tolerance, connectivity):
    """Steps 1 to 5 of DESIGN.md 'Splitting touching objects' on a contiguous (N,H,W) uint8 mask -> uint8 {0,255} markers."""
    N, H, W = m.shape
    comp, cnt = label(m, connectivity)
    depth2 = edt_sq((m == 0).to(torch.uint8))
    top = int(cnt.max())                                       # (one host sync, as label_tables)
    stride = top + 1
    cmax = torch.empty(N, stride, device=m.device, dtype=torch.int32)
    marker = torch.empty(N, H, W, device=m.device, dtype=torch.uint8)
    lib = L.lib()
    L.check(lib.medt_split_cmax(depth2.data_ptr(), comp.data_ptr(), cmax.data_ptr(), N, H, W, stride, top, _stream()),
            "medt_split_cmax")
    L.check(lib.medt_split_markers(depth2.data_ptr(), comp.data_ptr(), cmax.data_ptr(), marker.data_ptr(), N, H, W, stride,
                                   distance, tolerance, _stream()), "medt_split_markers")
    return marker


def split_markers(mask, distance=7, tolerance=1, connectivity=8):
    """uint8 (N,H,W) or (H,W) mask -> uint8 {0,255} marker mask of the same shape.  With depth2 the exact squared distance of a
    pixel of mask != 0 to the nearest pixel of its image outside the mask (EDT_NONE in an image without one) and M the maximum of
    depth2 over the (2 distance + 1)^2 window around the pixel, clipped to the image, a pixel of the mask is a marker when
    sqrt(M) - sqrt(depth2) <= tolerance (evaluated exactly in integers) or when depth2 is the maximum of its component at
    `connectivity`: every component holds a marker.  distance 1 .. 32, tolerance 0 .. 8, both integers."""
    (m,) = _edt_masks("split_markers", mask)
    _split_args("split_markers", distance, tolerance, connectivity)
    return _split_markers(m, distance, tolerance, connectivity).reshape(mask.shape)


def _grow(seeds, m, connectivity, labels, dist=None):
    """The growth on contiguous (N,H,W) maps into `labels` (and `dist`) -> the number of passes issued up to and including the
    first that changed nothing."""
    N, H, W = m.shape
    lib = L.lib()
    need = lib.medt_grow_workspace_bytes(N, H, W)              # (0 for a geometry the call below refuses, with the reason)
    workspace = torch.empty(max(need // 8, 2), device=m.device, dtype=torch.int64)          # (need is a multiple of 16)
    L.check(lib.medt_grow_init(seeds.data_ptr(), m.data_ptr(), workspace.data_ptr(), need, N, H, W, _stream()), "medt_grow_init")
    changed = torch.empty(GROW_MAX_PASSES, device=m.device, dtype=torch.int32)
    issued, limit, batch, passes = 0, H * W + 1, 0, None
    while passes is None:
        if issued >= limit:
            raise L.MedtError(f"grow_labels: no fixed point after {issued} passes over {H} x {W} maps")
        k = min(GROW_BATCHES[min(batch, len(GROW_BATCHES) - 1)], limit - issued)
        L.check(lib.medt_grow_passes(workspace.data_ptr(), need, changed.data_ptr(), k, issued, N, H, W, int(connectivity),
                                     _stream()), "medt_grow_passes")
        flags = changed[:k].cpu().tolist()                     # one host read per batch
        if 0 in flags:
            passes = issued + flags.index(0) + 1
        issued += k
        batch += 1
    L.check(lib.medt_grow_labels(workspace.data_ptr(), need, labels.data_ptr(), L.ptr(dist), N, H, W, _stream()), "medt_grow_labels")
    return passes


def grow_labels(seeds, mask, connectivity=8, out=None, return_passes=False, return_distance=False):
    """int32 seed map and uint8 mask, both (N,H,W) or (H,W) -> int32 labels of the same shape: every pixel of mask != 0 takes the
    label of the seed (a pixel with seeds > 0) at the smallest geodesic distance -- the fewest steps at `connectivity` through
    the mask -- ties to the smallest label; a component of the mask without a seed stays 0, and so does everything outside the
    mask.  Negative seeds and seeds outside the mask are refused (one host sync).  The same bits on every run.  out: a
    contiguous int32 tensor to write into (any alignment).  return_passes: also the number of device passes up to and including
    the first that changed nothing; return_distance: also the int32 map of step counts (-1 where no seed was reached)."""
    (m,) = _edt_masks("grow_labels", mask)
    if connectivity not in (4, 8):
        raise L.MedtError(f"grow_labels: connectivity {connectivity!r} (4 or 8)")
    if seeds.dtype != torch.int32 or tuple(seeds.shape) != tuple(mask.shape) or seeds.device != mask.device:
        raise L.MedtError("grow_labels: seeds must be an int32 map of the mask's shape on its device")
    sd = seeds.contiguous().reshape(m.shape)
    if bool(((sd < 0) | ((sd != 0) & (m == 0))).any()):
        raise L.MedtError("grow_labels: a negative seed or a seed outside the mask")
    labels = _edt_out("grow_labels", out, mask)
    dist = torch.empty(m.shape, device=m.device, dtype=torch.int32) if return_distance else None
    passes = _grow(sd, m, connectivity, labels, dist)
    res = (labels,) + ((passes,) if return_passes else ()) + ((dist.reshape(mask.shape),) if return_distance else ())
    return res[0] if len(res) == 1 else res


def split_objects(mask, distance=7, tolerance=1, connectivity=8, out=None):
    """uint8 (N,H,W) or (H,W) mask -> (labels, counts): the objects of mask != 0 with touching ones split.  The markers of
    split_markers are labelled at `connectivity` (K = counts[n] of them, numbered in raster order of their first pixel) and every
    pixel of the mask takes the label of the marker at the smallest geodesic distance, ties to the smallest label (grow_labels).
    labels: int32 of the mask's shape, 0 outside the mask and 1..K inside, every label's pixels connected and inside one
    component of the mask; a component with a single marker comes back whole.  counts: int32 (N,).  All integers, the same bits
    on every run.  out: a contiguous int32 tensor to write the labels into (any alignment)."""
    (m,) = _edt_masks("split_objects", mask)
    _split_args("split_objects", distance, tolerance, connectivity)
    labels = _edt_out("split_objects", out, mask)
    seeds, counts = label(_split_markers(m, distance, tolerance, connectivity), connectivity)
    _grow(seeds, m, connectivity, labels)
    return labels, counts
