#!/usr/bin/env python
"""Generate the golden fixtures under tests/golden/ FROM THE REFERENCE ITSELF.

Run in the build container (needs /root/reference):

    python tests/golden/make_golden.py

The reference ships no tests / golden vectors for this path, so
the fixtures are produced by importing the reference's own
lib/models/axialnet.py (oracle/ref_loader.py), running it on CPU in float64 on
seeded inputs with a seeded, non-trivial state_dict (oracle.randomize_state),
and recording outputs, loss, gradients and updated BatchNorm buffers.

Everything an fixture consumer needs to rebuild the inputs is a (seed, shape)
pair: tests regenerate x / y / state_dict with the same CPU generators and
compare against the stored results; a checksum of x guards the RNG contract.
Full gradients would be ~6 MB per model, so model-level fixtures store, per
parameter, the L2 norm and NPROBE = 8 dot products <grad, r_j> with seeded
N(0,1) vectors r_j, plus the full gradient of every tensor of up to 512
elements and of the position tables / gates; layer-level fixtures store
everything.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import medt_oracle as O      # noqa: E402
from oracle import ref_loader            # noqa: E402


def seeded_input(seed, N, C, S, classes=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, C, S, S, generator=g, dtype=torch.float32)
    y = torch.randint(0, classes, (N, S, S), generator=g)
    return x, y


def probe_vector(name: str, numel: int, seed: int) -> torch.Tensor:
    h = (sum(ord(c) * (i + 1) for i, c in enumerate(name)) + seed) % (2 ** 31)
    g = torch.Generator().manual_seed(h)
    return torch.randn(numel, generator=g, dtype=torch.float64)


NPROBE = 8           # seeded probe vectors per gradient tensor (round 4: one probe + the norm left norm-preserving errors of the
                     # big tensors to a single 3-sigma test; eight independent dots pin an 8-dimensional projection of each)
FULL_GRAD_MAX = 512  # and every gradient tensor up to this size is stored in full (BatchNorm vectors, gates, small kernels)


def probe_matrix(name: str, numel: int, seed: int) -> torch.Tensor:
    """(NPROBE, numel): row 0 is probe_vector(name) (the round-1..3 probe), row j > 0 probe_vector(name + '#j')."""
    return torch.stack([probe_vector(name if j == 0 else f"{name}#{j}", numel, seed) for j in range(NPROBE)])


FULL_GRAD_KEYS = ("relative", "f_qr", "f_kr", "f_sv", "f_sve", "bn_similarity.weight", "adjust.weight", "adjust.bias")


FACTORY_SEED = 3000      # bench.py's initial state: torch.manual_seed(3000) BEFORE the model is built.  (The reference seeds 3000 at
                         # train.py:118-121, AFTER building the model at :95-107 -- its initial weights are unseeded, so no fixture can hold
                         # "the" state train.py starts from; this is a factory-initialised state of the same distribution, and the one
                         # bench.py times.)


def _run_reference(model_name, S, N, seed, mode, dtype, variant=0, factory_init=False):
    """mode: 'train' (batch statistics), 'eval' (no grad), 'evalgrad' (running statistics, with backward).
    variant (float32 noise sampling): 0 = as is; 1 = the images of the batch in reverse order (BatchNorm statistics and
    weight gradients are summed in another order; results are un-permuted); 2 = one host thread (other blocking of the
    reductions inside aten); 3..7 = every float32 parameter and input value moved by one unit in the last place at random
    (x * (1 +- 2^-23) or unchanged, seeded by the variant): aten's reductions give the same bits whatever the thread count,
    so more summation orders are not available -- what IS available is the sensitivity of the float32 computation to
    perturbations of the size of its own rounding, five independent samples of it."""
    torch.manual_seed(FACTORY_SEED if factory_init else seed)
    ref = ref_loader.factory(model_name)(img_size=S, imgchan=3)
    if not factory_init:
        ref.load_state_dict(O.randomize_state(ref.state_dict(), seed))
    if variant >= 3:
        g = torch.Generator().manual_seed(1000 * variant + seed)
        with torch.no_grad():
            for t in list(ref.parameters()) + [b for b in ref.buffers() if b.is_floating_point()]:
                t.mul_(1.0 + (torch.randint(-1, 2, t.shape, generator=g).to(t.dtype) * 2.0 ** -23))
    ref = ref.to(dtype)
    if not factory_init:                 # (factory state: the gates stay frozen, as train.py leaves them until epoch 10)
        for p in ref.parameters():
            p.requires_grad_(True)       # gates too (train.py:169-171 after epoch 10)
    ref.train(mode == "train")
    x, y = seeded_input(FACTORY_SEED if factory_init else seed + 1, N, 3, S)     # (bench.py's batch on rank 0: the same generator calls)
    flipped = variant == 1
    xin, yin = (x.flip(0), y.flip(0)) if flipped else (x, y)
    if variant >= 3:
        g = torch.Generator().manual_seed(2000 * variant + seed)
        xin = xin * (1.0 + (torch.randint(-1, 2, xin.shape, generator=g).to(xin.dtype) * 2.0 ** -23))
    nthreads = torch.get_num_threads()
    if variant == 2:
        torch.set_num_threads(1)
    try:
        out = ref(xin.to(dtype))
        loss = None
        if mode != "eval":
            loss = ref_loader.load_metrics().LogNLLLoss()(out, yin)
            loss.backward()
    finally:
        torch.set_num_threads(nthreads)
    if flipped:
        out = out.flip(0)
    return ref, x, out.detach().double(), loss


def model_fixture(model_name, S, N, seed, mode):
    """Reference results in float64, plus the reference's OWN float32-vs-float64 discrepancy
    ("noise"): training-mode BatchNorm makes the whole-network backward ill-conditioned in
    float32 (the reference's fp32 gradients are 0.2 % median / 10-30 % worst-case away from
    its fp64 gradients), so GPU tests bound the product's error by that floor."""
    ref, x, out, loss = _run_reference(model_name, S, N, seed, mode, torch.float64)
    ref32, _, out32, _ = _run_reference(model_name, S, N, seed, mode, torch.float32)
    # seven more float32 runs of the reference: two other summation orders (batch order, one host thread) and five with
    # every float32 input / parameter moved by at most one unit in the last place.  The per-tensor maximum over the eight is
    # the noise a float32 implementation of this network cannot be expected to beat (tests bound the product by k x this).
    # Round 2 used three runs: the maximum of three samples is itself too noisy a yardstick -- a fourth sample of the SAME
    # distribution exceeds 2.5x the max of three for ~2 % of the tensors.
    extra = [_run_reference(model_name, S, N, seed, mode, torch.float32, v) for v in (tuple(range(1, 8)) if mode == "train" else ())]
    p32x = [dict(r[0].named_parameters()) for r in extra]
    lnoise = max([((out32 - out).abs().max() / out.abs().max()).item()] +
                 [((r[2] - out).abs().max() / out.abs().max()).item() for r in extra])
    fx = {
        "meta": np.array([S, N, seed, int(mode == "train")]),
        "mode": np.array(mode),
        "x_checksum": np.array([x.double().sum().item(), (x.double() ** 2).sum().item()]),
        "logits": out.float().numpy(),
        "logits_noise": np.array([lnoise]),
        "noise_runs": np.array([1 + len(extra)]),
    }
    if mode == "eval":
        return fx
    fx["loss"] = np.array([loss.item()])
    p32 = dict(ref32.named_parameters())
    names, summ, noise, dots, dots_noise = [], [], [], [], []
    for k, p in ref.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.reshape(-1)
        g32 = p32[k].grad.double().reshape(-1)
        R = probe_matrix(k, g.numel(), seed)
        names.append(k)
        summ.append([g.norm().item(), torch.dot(g, R[0]).item()])
        gs = [g32] + [px[k].grad.double().reshape(-1) for px in p32x]
        noise.append([max((gg - g).norm().item() for gg in gs), max(abs(torch.dot(gg - g, R[0]).item()) for gg in gs)])
        dots.append((R @ g).numpy())
        dots_noise.append(max((R @ (gg - g)).abs().max().item() for gg in gs))
        if (k.endswith(FULL_GRAD_KEYS) and g.numel() <= 4096) or g.numel() <= FULL_GRAD_MAX:
            fx["grad/" + k] = p.grad.detach().numpy()
            fx["gradnoise/" + k] = np.array([max((gg - g).abs().max().item() for gg in gs)])
    fx["grad_names"] = np.array(names)
    fx["grad_summary"] = np.array(summ)
    fx["grad_noise"] = np.array(noise)
    fx["grad_dots"] = np.array(dots)                     # (tensors, NPROBE)
    fx["grad_dots_noise"] = np.array(dots_noise)         # (tensors,): max over probes and float32 runs
    if mode == "train":
        bnames, bsumm, bnoise = [], [], []
        sds = [ref32.state_dict()] + [r[0].state_dict() for r in extra]
        for k, b in ref.state_dict().items():
            if k.endswith(("running_mean", "running_var")):
                v = b.reshape(-1).double()
                bnames.append(k)
                bsumm.append([v.norm().item(), torch.dot(v, probe_vector(k, v.numel(), seed)).item()])
                bnoise.append(max((sd[k].reshape(-1).double() - v).norm().item() for sd in sds))
            elif k.endswith("num_batches_tracked"):
                bnames.append(k)
                bsumm.append([float(b.item()), 0.0])
                bnoise.append(0.0)
        fx["buf_names"] = np.array(bnames)
        fx["buf_summary"] = np.array(bsumm)
        fx["buf_noise"] = np.array(bnoise)
    return fx


def factory_fixture(model_name, S, N):
    """bench.py's initial state: FACTORY initialisation under torch.manual_seed(3000) before construction (see FACTORY_SEED), train
    mode, bench.py's synthetic batch, gates frozen.  Reference float64 logits / loss / gradient summaries, the reference's own
    float32 noise on this state (eight float32 runs), and a checksum of the initial state_dict so that a consumer can tell
    that its own same-seed initialisation is the reference's."""
    seed = FACTORY_SEED
    ref, x, out, loss = _run_reference(model_name, S, N, seed, "train", torch.float64, factory_init=True)
    runs32 = [_run_reference(model_name, S, N, seed, "train", torch.float32, v, factory_init=True) for v in range(8)]
    torch.manual_seed(FACTORY_SEED)
    init = ref_loader.factory(model_name)(img_size=S, imgchan=3).state_dict()
    fx = {
        "meta": np.array([S, N, seed, 1]),
        "mode": np.array("train"),
        "x_checksum": np.array([x.double().sum().item(), (x.double() ** 2).sum().item()]),
        "state_checksum": np.array([sum(v.double().sum().item() for v in init.values() if v.is_floating_point()),
                                    sum((v.double() ** 2).sum().item() for v in init.values() if v.is_floating_point())]),
        "logits": out.float().numpy(),
        "logits_noise_runs": np.array([((r[2] - out).abs().max() / out.abs().max()).item() for r in runs32]),
        "loss": np.array([loss.item()]),
    }
    names, summ, noise, dots, dots_noise = [], [], [], [], []
    p32x = [dict(r[0].named_parameters()) for r in runs32]
    for k, p in ref.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.reshape(-1)
        R = probe_matrix(k, g.numel(), seed)
        gs = [px[k].grad.double().reshape(-1) for px in p32x]
        names.append(k)
        summ.append([g.norm().item(), torch.dot(g, R[0]).item()])
        noise.append([max((gg - g).norm().item() for gg in gs), max(abs(torch.dot(gg - g, R[0]).item()) for gg in gs)])
        dots.append((R @ g).numpy())
        dots_noise.append(max((R @ (gg - g)).abs().max().item() for gg in gs))
    fx["grad_names"] = np.array(names)
    fx["grad_summary"] = np.array(summ)
    fx["grad_noise"] = np.array(noise)
    fx["grad_dots"] = np.array(dots)
    fx["grad_dots_noise"] = np.array(dots_noise)
    return fx


def sensitivity_fixture(model_name, S, N, seed, factory_init=False):
    """How far the REFERENCE's own float64 training-mode logits move when its input image is perturbed by one rounding of a
    given precision (relative +-eps, uniform): the conditioning of the train-mode network (batch-statistic BatchNorm through
    ~100 layers).  eps = 2^-9 is ONE bfloat16 rounding of the input -- what any bf16 storage inside the network amounts to
    at the very least; GPU tests of bf16 storage in training mode are judged against this, not against a fixed tolerance."""
    torch.manual_seed(FACTORY_SEED if factory_init else seed)
    ref = ref_loader.factory(model_name)(img_size=S, imgchan=3)
    if not factory_init:
        ref.load_state_dict(O.randomize_state(ref.state_dict(), seed))
    ref = ref.double()
    ref.train()
    x, _ = seeded_input(FACTORY_SEED if factory_init else seed + 1, N, 3, S)      # (factory state: bench.py's batch, as in factory_fixture)
    sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
    with torch.no_grad():
        base = ref(x.double())
        out = {}
        for name, eps in (("f32", 2.0 ** -24), ("2^-16", 2.0 ** -16), ("bf16", 2.0 ** -9)):
            ref.load_state_dict(sd0)                       # (running statistics moved by the previous forward)
            g = torch.Generator().manual_seed(5)
            xp = x.double() * (1 + eps * (torch.rand(x.shape, generator=g, dtype=torch.float64) * 2 - 1))
            out[name] = ((ref(xp) - base).abs().max() / base.abs().max()).item()
    return {"model": model_name, "S": S, "N": N, "seed": FACTORY_SEED if factory_init else seed, "mode": "train",
            "state": "factory" if factory_init else "randomize_state", "logits_rel_change_for_input_rounding": out}


def layer_fixture(kind, C, L, width, stride, N, seed):
    """One attention layer of the reference, everything stored in full (float64)."""
    ax = ref_loader.load()
    if kind == "gatedsig":                           # experimental zoo, lib/models/model_codes.py:215-313
        cls = ref_loader.load_model_codes().AxialAttention_gated_sig
    elif kind == "gateddata":                        # :316-443
        cls = ref_loader.load_model_codes().AxialAttention_gated_data
    else:
        cls = {"dynamic": ax.AxialAttention_dynamic, "plain": ax.AxialAttention, "wopos": ax.AxialAttention_wopos}[kind]
    torch.manual_seed(seed)
    layer = cls(C, C, groups=8, kernel_size=L, stride=stride, width=width)
    sd = O.randomize_state(layer.state_dict(), seed)
    layer.load_state_dict(sd)
    layer = layer.double()
    for p in layer.parameters():
        p.requires_grad_(True)
    g = torch.Generator().manual_seed(seed + 1)
    other = 6                                        # the non-attended spatial extent
    shape = (N, C, other, L) if width else (N, C, L, other)
    x = torch.randn(shape, generator=g, dtype=torch.float64).requires_grad_(True)
    fx = {"meta": np.array([C, L, int(width), stride, N, seed]), "x": x.detach().numpy()}
    import json
    fx["state_layout"] = np.array(json.dumps([[k, list(v.shape), str(v.dtype).replace("torch.", "")]
                                              for k, v in sd.items()]))
    layer.eval()
    fx["out_eval"] = layer(x).detach().numpy()
    layer.train()
    out = layer(x)
    w = torch.randn(out.shape, generator=g, dtype=torch.float64)
    fx["dout"] = w.numpy()
    (out * w).sum().backward()
    fx["out_train"] = out.detach().numpy()
    fx["dx"] = x.grad.numpy()
    for k, p in layer.named_parameters():
        fx["grad/" + k] = p.grad.numpy()
    for k, b in layer.state_dict().items():
        if "running" in k or "num_batches" in k:
            fx["buf/" + k] = b.numpy()
    return fx


def block_fixture(inplanes, planes, S, groups_n, npg, seed, stride=1):
    """One AxialBlock_wopos of the reference (lib/models/axialnet.py:346-391) applied to `groups_n` patch groups of `npg`
    images ONE AFTER THE OTHER -- what medt_net's patch loop (:661-700) does with every block of the local branch: each
    group is normalised with its own batch statistics, the running statistics receive the groups' updates in order, the
    parameter gradients are the sums over the groups.  Everything stored in full (float64)."""
    ax = ref_loader.load()
    torch.manual_seed(seed)
    downsample = None
    if stride != 1 or inplanes != planes * 2:
        # what medt_net._make_layer builds for the first block of a layer (lib/models/axialnet.py:596-606)
        downsample = torch.nn.Sequential(ax.conv1x1(inplanes, planes * 2, stride), torch.nn.BatchNorm2d(planes * 2))
    blk = ax.AxialBlock_wopos(inplanes, planes, stride=stride, downsample=downsample, groups=8, base_width=64, kernel_size=S)
    sd = O.randomize_state(blk.state_dict(), seed)
    blk.load_state_dict(sd)
    blk = blk.double()
    for p in blk.parameters():
        p.requires_grad_(True)
    g = torch.Generator().manual_seed(seed + 1)
    N = groups_n * npg
    x = torch.randn((N, inplanes, S, S), generator=g, dtype=torch.float64).relu_().requires_grad_(True)
    w = torch.randn((N, planes * 2, S // stride, S // stride), generator=g, dtype=torch.float64)
    import json
    fx = {"meta": np.array([inplanes, planes, S, groups_n, npg, seed] + ([stride] if stride != 1 else [])), "x": x.detach().numpy(), "dout": w.numpy(),
          "state_layout": np.array(json.dumps([[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]))}
    blk.eval()
    fx["out_eval"] = torch.cat([blk(x[i * npg:(i + 1) * npg]) for i in range(groups_n)]).detach().numpy()
    blk.train()
    outs = [blk(x[i * npg:(i + 1) * npg]) for i in range(groups_n)]          # in patch order
    out = torch.cat(outs)
    (out * w).sum().backward()
    fx["out_train"] = out.detach().numpy()
    fx["dx"] = x.grad.numpy()
    for k, p in blk.named_parameters():
        if p.grad is not None:                      # (conv1 of AxialBlock_wopos is registered and never used)
            fx["grad/" + k] = p.grad.numpy()
    for k, b in blk.state_dict().items():
        if "running" in k or "num_batches" in k:
            fx["buf/" + k] = b.numpy()
    return fx


def manifest():
    """state_dict key / shape / dtype manifest of every factory (the drop-in contract)."""
    import json
    out = {}
    for name, S in (("gatedaxialunet", 128), ("axialunet", 128), ("MedT", 128), ("logo", 128),
                    ("gatedaxialunet", 256), ("MedT", 256), ("gatedaxialunet", 64), ("axialunet", 64)):
        for chan in (3, 1):
            m = ref_loader.factory(name)(img_size=S, imgchan=chan)
            out[f"{name}/{S}/{chan}"] = {
                "state": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()],
                "params": [[k, bool(p.requires_grad)] for k, p in m.named_parameters()],
            }
    with open(os.path.join(HERE, "state_manifest.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote state_manifest.json")


def tensor_digest(t: torch.Tensor):
    """[shape, dtype, sha256 of the bytes]: bit-identity of a tensor without storing it."""
    import hashlib
    t = t.detach().contiguous().cpu()
    return [list(t.shape), str(t.dtype).replace("torch.", ""), hashlib.sha256(t.numpy().tobytes()).hexdigest()]


GATE_CASES = [(cls_name, mode, width, stride) for cls_name, mode in (("AxialAttention_gated_sig", "sigmoid"),
                                                                      ("AxialAttention_gated_data", "data"))
              for width, stride in ((False, 1), (True, 2))]


def gate_case_key(cls_name, width, stride):
    return f"{cls_name}_{'w' if width else 'h'}_s{stride}"


def gate_case_inputs(key, out_shape=None):
    """x (3, 32, 12, 12) and the output weights w of one gate-variant case, float64, from a generator seeded by the case."""
    g = torch.Generator().manual_seed(sum(ord(c) for c in key))
    x = torch.randn(3, 32, 12, 12, generator=g, dtype=torch.float64)
    return x if out_shape is None else (x, torch.randn(out_shape, generator=g, dtype=torch.float64))


def reference_surface_fixtures():
    """What tests/test_oracle_vs_reference.py, tests/test_module_surface.py and tests/test_metrics_cpu.py read from the
    reference: reference_surface.json -- digests of the reference's initial state_dicts under fixed seeds (factories and
    model_codes gate variants), key / requires_grad lists, classwise metrics on seeded inputs; gate_variants_fp64.npz -- the model_codes gate flavours (:215-313, :316-443)
    executed in float64, training mode: state, output and every gradient."""
    import json
    mc = ref_loader.load_model_codes()
    surf = {"init_seed1234_S128": {}, "gray_MedT_128_keys": list(ref_loader.factory("MedT")(img_size=128, imgchan=1).state_dict()),
            "model_codes": {}}
    for name in ("gatedaxialunet", "MedT"):
        torch.manual_seed(1234)
        ref = ref_loader.factory(name)(img_size=128, imgchan=3)
        surf["init_seed1234_S128"][name] = [[k, *tensor_digest(v)] for k, v in ref.state_dict().items()]
    for cls_name, seed, kw in (("AxialAttention_gated_sig", 9, dict(stride=2, width=True)),
                               ("AxialAttention_gated_data", 10, dict(stride=1, width=False))):
        torch.manual_seed(seed)
        m = getattr(mc, cls_name)(32, 32, groups=8, kernel_size=16, **kw)
        surf["model_codes"][cls_name] = {"seed": seed, "state": [[k, *tensor_digest(v)] for k, v in m.state_dict().items()],
                                         "params": [[k, p.requires_grad] for k, p in m.named_parameters()]}
    surf["model_codes"]["AxialBlock_gated_data_keys"] = list(mc.AxialBlock_gated_data(32, 16, kernel_size=16).state_dict())
    # the reference's metrics.py (:23-57) on the inputs of tests/test_metrics_cpu.py (float32 values are exact in JSON)
    ref_metrics = ref_loader.load_metrics()
    torch.manual_seed(2)
    out = torch.rand(3, 2, 9, 11)
    gt = torch.randint(0, 2, (3, 9, 11))
    surf["metrics_seed2"] = {f: [str(r.dtype).replace("torch.", ""), r.cpu().tolist()]
                             for f in ("classwise_iou", "classwise_f1", "jaccard_index", "f1_score")
                             for r in [getattr(ref_metrics, f)(out, gt)]}
    with open(os.path.join(HERE, "reference_surface.json"), "w") as f:
        json.dump(surf, f, separators=(",", ":"))
    print("wrote reference_surface.json")
    fx = {}
    for cls_name, mode, width, stride in GATE_CASES:
        key = gate_case_key(cls_name, width, stride)
        torch.manual_seed(5)
        layer = getattr(mc, cls_name)(32, 32, groups=8, kernel_size=12, stride=stride, width=width).double()
        for p in layer.parameters():
            if p.dim() == 0:
                p.data.uniform_(-1, 1)
            p.requires_grad_(True)
        layer.train()
        x = gate_case_inputs(key).requires_grad_(True)
        out = layer(x)
        _, w = gate_case_inputs(key, out.shape)
        (out * w).sum().backward()
        for k, v in layer.state_dict().items():             # after the forward: the state the oracle is handed
            fx[f"{key}/state/{k}"] = v.detach().numpy()
        fx[f"{key}/out"] = out.detach().numpy()
        fx[f"{key}/x_grad"] = x.grad.numpy()
        for k, p in layer.named_parameters():
            fx[f"{key}/grad/{k}"] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "gate_variants_fp64.npz"), **fx)
    print("wrote gate_variants_fp64.npz", os.path.getsize(os.path.join(HERE, "gate_variants_fp64.npz")) // 1024, "KB")


def main():
    """`python make_golden.py` regenerates everything; `python make_golden.py layer_gatedsig` only the fixtures whose
    file name starts with the given prefix (the others are deterministic re-runs of the same reference code)."""
    import sys
    only = sys.argv[1] if len(sys.argv) > 1 else ""
    torch.set_num_threads(os.cpu_count())
    if not only:
        manifest()
    if "reference_surface.json".startswith(only) or "gate_variants_fp64.npz".startswith(only):
        reference_surface_fixtures()
    layer_cases = [
        ("gatedsig", 32, 16, True, 2, 2, 17),
        ("gatedsig", 16, 32, False, 1, 2, 18),
        ("gateddata", 32, 16, True, 2, 2, 19),
        ("gateddata", 16, 32, False, 1, 2, 20),
        ("dynamic", 16, 16, False, 1, 2, 11),
        ("dynamic", 32, 8, True, 2, 2, 12),
        ("plain", 16, 8, True, 1, 2, 13),
        ("wopos", 16, 16, False, 1, 2, 14),
        ("wopos", 32, 8, True, 2, 2, 15),
        ("dynamic", 64, 32, True, 2, 1, 16),
    ]
    for case in layer_cases:
        kind, C, L, width, stride, N, seed = case
        fn = f"layer_{kind}_C{C}_L{L}_{'w' if width else 'h'}_s{stride}.npz"
        if not fn.startswith(only):
            continue
        fx = layer_fixture(*case)
        np.savez_compressed(os.path.join(HERE, fn), **fx)
        print("wrote", fn)
    # layer3_p.1-3 of MedT at BASELINE's batch size (128 -> 64 -> 128 channels on 4x4 maps, 4 images per patch group): the shape
    # the one-launch block forward (csrc/block_small.hip) is built for, here as two patch groups
    fn = "block_wopos_C128_P64_S4_G2.npz"
    if fn.startswith(only):
        np.savez_compressed(os.path.join(HERE, fn), **block_fixture(128, 64, 4, 2, 4, 21))
        print("wrote", fn)
    # layer4_p.0 of MedT at BASELINE's batch size: the stride-2 first block + its downsample path (128 -> 128 -> 256 channels, 4x4 ->
    # 2x2 maps): the shape of the one-launch stride-2 block forward (round 6), two patch groups
    fn = "block_wopos_s2_C128_P128_S4_G2.npz"
    if fn.startswith(only):
        np.savez_compressed(os.path.join(HERE, fn), **block_fixture(128, 128, 4, 2, 4, 22, stride=2))
        print("wrote", fn)
    model_cases = [
        ("gatedaxialunet", 128, 2, 101, "train"),
        ("gatedaxialunet", 128, 2, 101, "evalgrad"),
        ("MedT", 128, 2, 102, "train"),
        ("MedT", 128, 2, 102, "evalgrad"),
        ("MedT", 128, 4, 106, "train"),          # the benchmarked workload itself: BASELINE configs[2], train mode, bs 4
        ("gatedaxialunet", 128, 8, 107, "train"),    # BASELINE configs[1]'s real mode: gatedaxialunet bs 8, train (fp32 + bf16 storage)
        ("axialunet", 64, 2, 103, "train"),
        ("logo", 128, 1, 104, "evalgrad"),
        ("MedT", 256, 1, 105, "eval"),
        ("MedT", 256, 2, 108, "train"),          # BASELINE configs[4]'s per-GPU shard (bs 16 over 8 GPUs): every gradient, train mode
        ("MedT", 256, 2, 108, "evalgrad"),
    ]
    if "sensitivity_gatedaxialunet_S128_N8.json".startswith(only):
        import json
        with open(os.path.join(HERE, "sensitivity_gatedaxialunet_S128_N8.json"), "w") as f:
            json.dump(sensitivity_fixture("gatedaxialunet", 128, 8, 107), f, indent=1)
        print("wrote sensitivity_gatedaxialunet_S128_N8.json")
    # the same question at bench.py's factory state (round 6): is "no tolerance exists for bf16 storage in train mode" a property of
    # the network or of randomize_state's weights?
    if "sensitivity_factory_gatedaxialunet_S128_N8.json".startswith(only):
        import json
        with open(os.path.join(HERE, "sensitivity_factory_gatedaxialunet_S128_N8.json"), "w") as f:
            json.dump(sensitivity_fixture("gatedaxialunet", 128, 8, FACTORY_SEED, factory_init=True), f, indent=1)
        print("wrote sensitivity_factory_gatedaxialunet_S128_N8.json")
    # the trained state itself: factory initialisation under seed 3000, BASELINE configs[2] (MedT bs 4) and configs[1] (gated bs 8)
    for name, S, N in (("MedT", 128, 4), ("gatedaxialunet", 128, 8)):
        fn = f"factory_{name}_S{S}_N{N}.npz"
        if not fn.startswith(only):
            continue
        np.savez_compressed(os.path.join(HERE, fn), **factory_fixture(name, S, N))
        print("wrote", fn, os.path.getsize(os.path.join(HERE, fn)) // 1024, "KB")
    for name, S, N, seed, mode in model_cases:
        fn = f"model_{name}_S{S}_N{N}_{mode}.npz"
        if not fn.startswith(only):
            continue
        fx = model_fixture(name, S, N, seed, mode)
        np.savez_compressed(os.path.join(HERE, fn), **fx)
        print("wrote", fn, os.path.getsize(os.path.join(HERE, fn)) // 1024, "KB")


if __name__ == "__main__":
    main()
