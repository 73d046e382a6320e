"""Test-time augmentation at inference (not in the reference): the network runs on flipped and transposed copies of its
input, each prediction is mapped back and the logits are averaged -- H&E tiles have no preferred orientation.

A view is a 3-bit code v -- bit 2 transpose, bit 1 flip rows, bit 0 flip columns, the transpose first:
    0 identity   1 left-right mirror   2 up-down mirror   3 rotation by 180 degrees
    4 transpose  5 rot90(k=-1)         6 rot90(k=1)       7 anti-transpose
and a set of views a bitmask with bit v set when code v takes part (VIEWS_FLIPS = 0x0F, VIEWS_D4 = 0xFF, 0x01 = off),
visited in ascending code.  A transposing view needs square inputs.

ops.tta_expand builds the N*V views on the device, ONE InferStep runs them `gather` per replay, ops.tta_merge maps every
view's logits back, adds them in ascending code and divides by V once -- one work-item per output element, no atomics: the
same bits on every run.  Logits are averaged, not probabilities: the project thresholds and blends logits everywhere."""
from __future__ import annotations

from . import _lib as L
from . import ops
from .trainer import InferStep, padded_batch, run_padded

VIEWS_OFF = 0x01
VIEWS_FLIPS = 0x0F
VIEWS_D4 = 0xFF
_NAMED = {"off": VIEWS_OFF, "flips": VIEWS_FLIPS, "d4": VIEWS_D4}


def parse_views(views) -> int:
    """"off" | "flips" | "d4" | a bitmask 0x01 .. 0xFF -> the bitmask."""
    if isinstance(views, str):
        if views not in _NAMED:
            raise ValueError(f"parse_views: one of {sorted(_NAMED)} or a bitmask expected (got {views!r})")
        return _NAMED[views]
    if isinstance(views, bool) or not isinstance(views, int) or not 0 < views <= 0xFF:
        raise ValueError(f"parse_views: a bitmask 0x01 .. 0xFF over the eight view codes expected (got {views!r})")
    return views


def view_codes(views) -> list:
    """The codes of a set of views, ascending: the order of tta_expand's outputs and of tta_merge's sum."""
    views = parse_views(views)
    return [v for v in range(8) if views >> v & 1]


class TtaInfer:
    """Eval-mode inference of `model` averaged over a set of views.

    infer = TtaInfer(model, "d4"); merged, mask = infer(x)                     x (N,C,S,S) on the device
                                   merged, mask, counts = infer(x, target)     target (N,S,S) int64
    merged (N,K,S,S) float32 = the mean of the views' logits mapped back, mask (N,S,S) uint8 {0,255} = merged[:,1] >= threshold
    (what test.py writes), counts (N,4) int32 {tp, fp, fn, tn} of the mask against target > 0 (ops.seg_counts).  The outputs
    are fresh tensors.  With the flip-only views x may be (N,C,H,W).

    The N*V views run `gather` per forward replay; the last, shorter batch is padded with copies of its last view and the
    padding's logits are dropped.  In eval mode the items of a batch do not interact; in train mode they would (batch
    statistics), so a model in train mode is refused.  views = 0x01 returns InferStep's bits."""

    def __init__(self, model, views, gather: int = 4, threshold: float = 0.5, use_graph: bool = True):
        self.model, self.views, self.gather, self.threshold = model, parse_views(views), max(1, int(gather)), float(threshold)
        self.V = len(view_codes(self.views))
        self.infer = InferStep(model, use_graph=use_graph, threshold=threshold)

    def __call__(self, x, target=None):
        if self.model.training:
            raise L.MedtError("TtaInfer: the model is in train mode -- batch statistics would make the views of a batch "
                              "depend on each other; call model.eval() first")
        ops._require_device(x)
        if x.dim() != 4:
            raise L.MedtError("TtaInfer: a (N,C,H,W) batch expected")
        x = x.contiguous()
        N, Cc, H, W = x.shape
        batch = padded_batch(N * self.V, self.gather, (Cc, H, W), x.device)
        ops.tta_expand(x, self.views, out=batch)
        merged, mask = ops.tta_merge(run_padded(self.infer, batch, N * self.V, self.gather), self.views, self.threshold)
        if target is None:
            return merged, mask
        return merged, mask, ops.seg_counts(merged, target.reshape(N, H, W), self.threshold)
