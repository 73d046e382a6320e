"""Oracle of test-time augmentation (medt_amd.tta, medt_tta_expand / medt_tta_merge): the normative torch expressions of
include/medt_abi.h, restated once for the CPU and the GPU tests.  A view is a 3-bit code: bit 2 transpose, bit 1 flip rows,
bit 0 flip columns, the transpose first; a set of views is a bitmask, visited in ascending code."""
import torch


def codes(views):
    assert 0 < views <= 0xFF
    return [v for v in range(8) if views >> v & 1]


def _dims(v):
    return [d for b, d in ((2, -2), (1, -1)) if v & b]


def fwd_view(a, v):
    t = a.transpose(-1, -2) if v & 4 else a
    return t.flip(_dims(v))


def inv_view(l, v):
    m = l.flip(_dims(v))
    return m.transpose(-1, -2) if v & 4 else m


def expand(x, views):
    """(N,C,H,W) -> (N V,C,H,W): item n V + j is view codes(views)[j] of x[n]."""
    return torch.stack([fwd_view(x[n], v) for n in range(x.shape[0]) for v in codes(views)]).contiguous()


def merge(view_logits, views, threshold=0.5):
    """(N V,K,H,W) -> (merged (N,K,H,W), mask (N,H,W) uint8 {0,255}, votes (N,H,W) uint8): sequential adds in ascending code in
    the dtype of the input (float32: the kernel's bits; float64: the reference of the end-to-end bound), then ONE division."""
    cs = codes(views)
    V = len(cs)
    assert view_logits.shape[0] % V == 0
    merged, votes = [], []
    for n in range(view_logits.shape[0] // V):
        back = [inv_view(view_logits[n * V + j], v) for j, v in enumerate(cs)]
        acc = back[0].clone()
        for b in back[1:]:
            acc = acc + b
        merged.append(acc / torch.tensor(float(V), dtype=acc.dtype) if V > 1 else acc)
        votes.append(sum((b[1] >= threshold).to(torch.uint8) for b in back))
    merged = torch.stack(merged).contiguous()
    return merged, (merged[:, 1] >= threshold).to(torch.uint8) * 255, torch.stack(votes)
