"""Pin the oracle against the reference: executed live where a reference checkout exists (whole networks, every gradient),
and against what tests/golden/make_golden.py recorded from it everywhere (reference_surface.json, gate_variants_fp64.npz)."""
import hashlib
import json
import os

import pytest
import torch

import helpers as H
from oracle import medt_oracle as O
from oracle import ref_loader


def reference_surface():
    with open(os.path.join(H.GOLDEN, "reference_surface.json")) as f:
        return json.load(f)


def digest(t):
    """[shape, dtype, sha256 of the bytes] (tests/golden/make_golden.py::tensor_digest)."""
    t = t.detach().contiguous().cpu()
    return [list(t.shape), str(t.dtype).replace("torch.", ""), hashlib.sha256(t.numpy().tobytes()).hexdigest()]


MODEL_CASES = [("gatedaxialunet", 64, 2, 3), ("axialunet", 64, 1, 3), ("MedT", 128, 1, 3), ("logo", 128, 1, 3),
               # one input channel (--gray yes): the oracle tests/test_configs_gpu.py relies on
               ("gatedaxialunet", 64, 3, 1), ("axialunet", 64, 1, 1), ("MedT", 128, 3, 1), ("logo", 128, 1, 1)]


@pytest.mark.skipif(not ref_loader.available(), reason="reference checkout not present")
@pytest.mark.parametrize("name,S,N,chan", MODEL_CASES,       # (the three-channel cases keep the ids they had before `chan` was a parameter)
                         ids=[f"{n}-{s}-{b}" + ("" if c == 3 else f"-chan{c}") for n, s, b, c in MODEL_CASES])
def test_model_forward_backward_fp64(name, S, N, chan):
    torch.manual_seed(0)
    ref = ref_loader.factory(name)(img_size=S, imgchan=chan)
    sd = O.randomize_state(ref.state_dict(), 3)
    ref.load_state_dict(sd)
    ref = ref.double()
    for p in ref.parameters():
        p.requires_grad_(True)
    x, y = H.seeded_input(4, N, chan, S)
    for training in (True, False):
        ref.train(training)
        st = O.clone_state(ref.state_dict(), torch.float64, requires_grad=True)
        out_ref = ref(x.double())
        out = O.forward(name, x.double(), st, training)
        assert H.rel_err(out, out_ref) < 1e-9
        if training:
            loss_ref = ref_loader.load_metrics().LogNLLLoss()(out_ref, y)
            loss = O.log_nll_loss(out, y)
            assert abs(loss.item() - loss_ref.item()) < 1e-11
            loss_ref.backward()
            loss.backward()
            gmax = max(p.grad.abs().max().item() for p in ref.parameters() if p.grad is not None)
            for k, p in ref.named_parameters():
                if p.grad is None:
                    continue
                assert (st[k].grad - p.grad).abs().max().item() < 1e-8 * gmax, k
            for k, b in ref.state_dict().items():
                if "running" in k or "num_batches" in k:
                    assert H.rel_err(st[k].double(), b.double()) < 1e-9, k


def test_reference_gray_and_manifest_agree():
    keys = reference_surface()["gray_MedT_128_keys"]                # the reference's MedT(img_size=128, imgchan=1) state_dict keys
    ent = H.manifest()["MedT/128/1"]["state"]
    assert [k for k, _, _ in ent] == keys


@pytest.mark.parametrize("cls_name,mode", [("AxialAttention_gated_sig", "sigmoid"), ("AxialAttention_gated_data", "data")])
@pytest.mark.parametrize("width,stride", [(False, 1), (True, 2)])
def test_gate_variants_fp64(cls_name, mode, width, stride):
    """The experimental gate flavours of the reference's model_codes.py (:215-313, :316-443) against the oracle's
    gate_mode, forward + every gradient, training mode, fp64 (the reference's results: tests/golden/gate_variants_fp64.npz,
    make_golden.py::reference_surface_fixtures)."""
    from golden.make_golden import gate_case_inputs, gate_case_key
    key = gate_case_key(cls_name, width, stride)
    fx = H.load_golden("gate_variants_fp64.npz")
    pre = key + "/"
    state = {k[len(pre + "state/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(pre + "state/")}
    grads = {k[len(pre + "grad/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(pre + "grad/")}
    out_ref, x_grad = torch.from_numpy(fx[pre + "out"]), torch.from_numpy(fx[pre + "x_grad"])
    x, w = gate_case_inputs(key, out_ref.shape)
    st = O.clone_state({"L." + k: v for k, v in state.items()}, torch.float64, requires_grad=True)
    xo = x.clone().requires_grad_(True)
    out = O.axial_attention(xo, st, "L", width, stride, True, gate_mode=mode)
    (out * w).sum().backward()
    assert H.rel_err(out, out_ref) < 1e-10
    assert H.rel_err(xo.grad, x_grad) < 1e-9
    gmax = max(g.abs().max().item() for g in grads.values())
    assert grads and all(st["L." + k].requires_grad for k in grads)
    for k, g in grads.items():
        assert (st["L." + k].grad - g).abs().max().item() < 1e-9 * gmax, k


def test_gated_sig_module_surface_matches_reference():
    """The reference's side: initial state_dicts under the same seeds, as digests (reference_surface.json)."""
    import lib as droplib  # noqa: F401
    from lib.models import model_codes
    mc = reference_surface()["model_codes"]
    torch.manual_seed(9)
    b = model_codes.AxialAttention_gated_sig(32, 32, groups=8, kernel_size=16, stride=2, width=True)
    ra, sb = mc["AxialAttention_gated_sig"], b.state_dict()
    assert ra["seed"] == 9
    assert [k for k, *_ in ra["state"]] == list(sb.keys())
    for k, *dg in ra["state"]:
        assert dg == digest(sb[k]), k                      # same registration order -> same RNG stream -> same init
    assert [tuple(e) for e in ra["params"]] == [(k, p.requires_grad) for k, p in b.named_parameters()]
    torch.manual_seed(10)
    d = model_codes.AxialAttention_gated_data(32, 32, groups=8, kernel_size=16, stride=1, width=False)
    rc, sd = mc["AxialAttention_gated_data"], d.state_dict()
    assert rc["seed"] == 10
    assert [k for k, *_ in rc["state"]] == list(sd.keys())  # fcn1 / fcn2 sit between bn_output and relative, as in the reference
    for k, *dg in rc["state"]:
        assert dg == digest(sd[k]), k
    blk = model_codes.AxialBlock_gated_data(32, 16, kernel_size=16)
    assert list(blk.state_dict().keys()) == mc["AxialBlock_gated_data_keys"]
