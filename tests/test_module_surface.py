"""Drop-in boundary: the mirrored lib.models.axialnet has the reference's state_dict layout."""
import pytest
import torch

import helpers as H


def build(name, S, chan=3):
    import lib as droplib
    f = {"axialunet": droplib.models.axialunet, "gatedaxialunet": droplib.models.axialnet.gated,
         "MedT": droplib.models.axialnet.MedT, "logo": droplib.models.axialnet.logo}[name]
    return f(img_size=S, imgchan=chan)


@pytest.mark.parametrize("key", sorted(H.manifest().keys()))
def test_state_dict_layout(key):
    name, S, chan = key.split("/")
    m = build(name, int(S), int(chan))
    ent = H.manifest()[key]
    got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]
    assert got == ent["state"]
    assert [[k, bool(p.requires_grad)] for k, p in m.named_parameters()] == ent["params"]


def test_public_names():
    import lib as droplib
    ax = droplib.models.axialnet
    for n in ("AxialAttention", "AxialAttention_dynamic", "AxialAttention_wopos", "AxialBlock", "AxialBlock_dynamic",
              "AxialBlock_wopos", "ResAxialAttentionUNet", "medt_net", "axialunet", "gated", "MedT", "logo",
              "qkv_transform", "conv1x1"):
        assert hasattr(ax, n), n
    assert hasattr(droplib.models, "axialunet")          # train.py:96 uses lib.models.axialunet
    a = ax.AxialAttention_dynamic(16, 16, groups=8, kernel_size=8, stride=2, width=True)
    for attr in ("in_planes", "out_planes", "groups", "group_planes", "kernel_size", "stride", "bias", "width"):
        assert hasattr(a, attr)
    assert ax.AxialBlock_dynamic.expansion == 2


@pytest.mark.parametrize("name", ["gatedaxialunet", "MedT"])
def test_same_seed_same_init_as_reference(name):
    """The reference's initial state under torch.manual_seed(1234), as per-tensor digests (tests/golden/reference_surface.json)."""
    from test_oracle_vs_reference import digest, reference_surface
    ref = reference_surface()["init_seed1234_S128"][name]
    torch.manual_seed(1234)
    mine = build(name, 128)
    b = mine.state_dict()
    assert [k for k, *_ in ref] == list(b.keys())
    for k, *dg in ref:
        assert dg == digest(b[k]), k
    # a reference checkpoint (its keys, shapes and dtypes) loads strictly
    mine.load_state_dict({k: torch.zeros(shape, dtype=getattr(torch, dt)) for k, shape, dt, _ in ref}, strict=True)
