"""Shared test helpers: golden fixtures, seeded states, comparisons."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from oracle import medt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_manifest = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(GOLDEN, "state_manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def blank_state(model_name: str, S: int, chan: int = 3):
    """Zero-filled state_dict with the reference's keys/shapes/dtypes (from the committed manifest)."""
    ent = manifest()[f"{model_name}/{S}/{chan}"]["state"]
    return {k: torch.zeros(shape, dtype=getattr(torch, dt)) for k, shape, dt in ent}


def seeded_state(model_name: str, S: int, seed: int, chan: int = 3):
    st = O.randomize_state(blank_state(model_name, S, chan), seed)
    # flatten_index is data, not randomised: rebuild it the way the reference registers it (axialnet.py:132-135)
    for k in st:
        if k.endswith("flatten_index"):
            L = int(round(st[k].numel() ** 0.5))
            ar = torch.arange(L)
            st[k] = (ar.view(L, 1) - ar.view(1, L) + L - 1).reshape(-1)
    return st


def seeded_input(seed, N, C, S, classes=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, C, S, S, generator=g, dtype=torch.float32)
    y = torch.randint(0, classes, (N, S, S), generator=g)
    return x, y


def probe_vector(name: str, numel: int, seed: int) -> torch.Tensor:
    h = (sum(ord(c) * (i + 1) for i, c in enumerate(name)) + seed) % (2 ** 31)
    g = torch.Generator().manual_seed(h)
    return torch.randn(numel, generator=g, dtype=torch.float64)


NPROBE = 8


def probe_matrix(name: str, numel: int, seed: int) -> torch.Tensor:
    """(NPROBE, numel): the probes of tests/golden/make_golden.py (row 0 = probe_vector(name))."""
    return torch.stack([probe_vector(name if j == 0 else f"{name}#{j}", numel, seed) for j in range(NPROBE)])


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


def rel_err(a, b):
    """max |a-b| / max |b|  (b = reference)."""
    a = torch.as_tensor(a, dtype=torch.float64).cpu()
    b = torch.as_tensor(b, dtype=torch.float64).cpu()
    denom = b.abs().max().item()
    return (a - b).abs().max().item() / (denom if denom > 0 else 1.0)


def param_names(model_name, S, chan=3):
    return [k for k, _ in manifest()[f"{model_name}/{S}/{chan}"]["params"]]


GATE_SUFFIXES = (".f_qr", ".f_kr", ".f_sve", ".f_sv")


def oracle_trajectory(name, st, x, y, dtype, schedule, train_keys, gate_keys=(), gates_join=None, ulp_seed=None):
    """The reference's loop (train.py:140,156-161: forward, LogNLLLoss, backward, Adam with lr 1e-3 / weight_decay 1e-5) on the
    CPU oracle, from the state `st`.  Step i runs on the first schedule[i] images of (x, y).  Parameters in `train_keys` that
    receive a gradient are updated from the first step on; those in `gate_keys` stay frozen before step `gates_join`
    (0-based) and train from it on.  Every parameter counts its own Adam step from 1 at its first update, as
    torch.optim.Adam does.  ulp_seed: the initial trained weights and the input moved by one float32 ulp in random directions
    first.  -> (loss of every step, final state)."""
    ost, xin = O.clone_state(st, dtype), x.to(dtype)
    train_keys, gate_keys = set(train_keys), set(gate_keys)
    if ulp_seed is not None:
        g = torch.Generator().manual_seed(ulp_seed)
        nudge = lambda t: torch.nextafter(t, torch.where(torch.rand(t.shape, generator=g) < 0.5, -1.0, 1.0) * float("inf"))
        ost = {k: (nudge(v) if (v.is_floating_point() and k in train_keys) else v) for k, v in ost.items()}
        xin = nudge(xin)
    mom, count, out_losses = {}, {}, []
    for i, n in enumerate(schedule):
        live = train_keys | gate_keys if (gates_join is not None and i >= gates_join) else train_keys
        leaf = {k: (v.clone().requires_grad_(True) if k in live else v) for k, v in ost.items()}
        loss = O.log_nll_loss(O.forward(name, xin[:n], leaf, True), y[:n])
        loss.backward()
        out_losses.append(loss.item())
        for k in ost:
            if k in live and leaf[k].grad is not None:
                m, v = mom.get(k, (torch.zeros_like(ost[k]), torch.zeros_like(ost[k])))
                count[k] = count.get(k, 0) + 1
                pnew, m, v = O.adam_step(ost[k], leaf[k].grad, m, v, count[k])
                ost[k], mom[k] = pnew.detach(), (m, v)
            else:
                ost[k] = leaf[k].detach()                    # buffers (running statistics) as updated by the forward
    return out_losses, ost
