"""The host half of the device-side joint augmentation (medt_amd/augment.py) and the validation layer of its C ABI: no GPU.

  * the affine sampling rule of the kernels / the oracle (tests/augment_oracle.py::affine_source) against PIL's
    Image.transform(AFFINE, NEAREST), which is what the reference's torchvision F.affine ends in;
  * draw_record makes data.JointTransform2D's random draws, in its order;
  * train.py's flags;  * medt_augment_* refuse bad descriptors."""
import colorsys
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import helpers as H  # noqa: F401
import augment_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "medical-transformer_amd")


def test_affine_sampling_rule_matches_pil_nearest():
    """200 seeded maps (rotation within +-90 degrees, shear within +-45, scale 0.7 .. 2, integer translations) on four sizes:
    floor(m (x + .5, y + .5)) with the range test on the floats picks PIL's pixel everywhere except next to a pixel border,
    where PIL steps in 16.16 fixed point: pixels whose source coordinate lies within 1e-3 of an integer are left out, and
    their share is asserted (a coordinate uniform modulo 1 falls there with probability 2e-3 per axis)."""
    from medt_amd.augment import inverse_affine_matrix
    rng = np.random.RandomState(0)
    total = skipped = wrong_among_skipped = 0
    for (h, w) in ((8, 8), (13, 9), (32, 32), (33, 20)):
        ids = (1 + np.arange(h * w, dtype=np.int32)).reshape(h, w)          # 0 is the fill
        im = Image.fromarray(ids, mode="I")
        for _ in range(50):
            angle, shear, scale = rng.uniform(-90, 90), rng.uniform(-45, 45), rng.uniform(0.7, 2.0)
            tx, ty = int(rng.randint(-w, w + 1)), int(rng.randint(-h, h + 1))
            m = inverse_affine_matrix((w * 0.5, h * 0.5), angle, (tx, ty), scale, (shear, 0.0))
            got = np.array(im.transform((w, h), Image.AFFINE, m, resample=Image.NEAREST), np.int64)
            sx, sy, inside, near = AO.affine_source(m, h, w)
            want = np.where(inside, ids[sy, sx], 0)
            total += h * w
            skipped += int(near.sum())
            wrong_among_skipped += int((got != want)[near].sum())
            assert np.array_equal(got[~near], want[~near]), (h, w, m)
    print(f"affine vs PIL: {skipped} of {total} pixels within {AO.NEAR_TOL} of an integer coordinate ({100.0 * skipped / total:.2f} %), "
          f"{wrong_among_skipped} of them differ")
    assert total == 93250 and skipped <= 0.01 * total


def test_oracle_hue_matches_colorsys():
    """The oracle's hexcone round trip against the standard library's, pixel by pixel (float64)."""
    rng = np.random.RandomState(3)
    px = np.concatenate([rng.rand(60, 3), [[0.2, 0.2, 0.2], [0, 0, 0], [1, 1, 1], [1, 0, 0], [0.5, 1, 0.5]]])
    for hf in (-0.1, 0.03, 0.1, 0.5):
        got = AO.hue(px[None], np.float64(hf), AO.NP64)[0]
        for p, g in zip(px, got):
            hh, s, v = colorsys.rgb_to_hsv(*p)
            assert np.allclose(g, colorsys.hsv_to_rgb((hh + hf) % 1.0, s, v), atol=1e-12), (p, hf)


def test_draw_record_makes_the_host_transforms_draws():
    """One seed of np.random and torch: with jitter and affine off, draw_record yields the crop origins and the flips
    data.JointTransform2D applies to the same sequence of items (the image encodes its own coordinates)."""
    from medt_amd.augment import draw_record
    from medt_amd.data import JointTransform2D
    h, w, crop = 21, 17, (8, 8)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    image = np.stack([yy, xx, yy + xx], -1).astype(np.uint8)
    mask = np.zeros((h, w), np.uint8)
    for crop_arg in (crop, None):
        th, tw = crop_arg or (h, w)
        np.random.seed(11)
        torch.manual_seed(11)
        host = []
        tf = JointTransform2D(crop=crop_arg, p_flip=0.5, color_jitter_params=None, long_mask=True)
        for _ in range(12):
            img, _m = tf(image, mask)
            a = (img * 255).round().to(torch.int64)               # (3, th, tw): [0] = source y, [1] = source x
            flip = bool(a[1, 0, 0] > a[1, 0, tw - 1])
            host.append((int(a[0, 0, 0]), int(a[1, 0, tw - 1] if flip else a[1, 0, 0]), flip))
        np.random.seed(11)
        torch.manual_seed(11)
        mine = []
        for _ in range(12):
            r = draw_record(h, w, crop_arg, 0.5, None, 0.0)
            assert r.dtype == np.float32 and r.shape == (20,) and r[3] == 1.0 and not r[10:14].any()
            mine.append((int(r[0]), int(r[1]), bool(r[2])))
        assert mine == host
        assert len({m[2] for m in mine}) == 2                      # both flip states occurred


def test_draw_record_jitter_and_affine():
    from medt_amd import augment as A
    np.random.seed(5)
    torch.manual_seed(5)
    seen_orders = set()
    for _ in range(40):
        r = A.draw_record(40, 50, (32, 32), 0.5, (0.4, 0.4, 0.0, 0.1), 1.0)
        ops = [int(v) for v in r[10:14]]
        assert sorted(o for o in ops if o) == [A.OP_BRIGHTNESS, A.OP_CONTRAST, A.OP_HUE] and ops[3] == 0      # saturation range 0: dropped
        seen_orders.add(tuple(ops))
        for o, f in zip(ops, r[14:18]):
            if o in (A.OP_BRIGHTNESS, A.OP_CONTRAST):
                assert 0.6 <= f <= 1.4
            if o == A.OP_HUE:
                assert -0.1 <= f <= 0.1
        assert r[3] == 0.0 and 0 <= r[0] <= 8 and 0 <= r[1] <= 18
        m = r[4:10].astype(np.float64)
        assert abs(abs(m[0] * m[4] - m[1] * m[3]) - 0.25) < 1e-5             # scale 2 forward = determinant 1/4 backward
    assert len(seen_orders) > 1
    # the identity parameters give the identity matrix about any centre
    assert np.allclose(A.inverse_affine_matrix((16.0, 12.0), 0.0, (0, 0), 1.0, (0.0, 0.0)), (1, 0, 0, 0, 1, 0))


def _train(*argv, cwd):
    env = dict(os.environ, PYTHONPATH=PKG)
    return subprocess.run([sys.executable, os.path.join(PKG, "train.py"), *argv], env=env, capture_output=True, text=True,
                          timeout=300, cwd=cwd)


def test_cli_refuses_jitter_or_affine_without_aug_on(tmp_path):
    """Before any work: no dataset exists, no GPU is touched."""
    for extra in (["--aug_jitter", "0.2,0.2,0.2,0.05"], ["--aug_affine", "0.5"], ["--aug", "off", "--aug_affine", "0.5"]):
        r = _train("--train_dataset", str(tmp_path / "none"), *extra, cwd=str(tmp_path))
        assert r.returncode != 0 and "add --aug on" in r.stderr, r.stderr[-1000:]
        assert not (tmp_path / "none").exists()


def test_cli_refuses_malformed_jitter(tmp_path):
    for bad in ("0.2,0.2,0.2", "a,b,c,d", "0.2,0.2,0.2,0.9", "-0.1,0,0,0"):
        r = _train("--train_dataset", str(tmp_path / "none"), "--aug", "on", "--aug_jitter=" + bad, cwd=str(tmp_path))
        assert r.returncode != 0 and "--aug_jitter" in r.stderr, (bad, r.stderr[-1000:])
    r = _train("--train_dataset", str(tmp_path / "none"), "--aug", "on", "--aug_affine", "1.5", cwd=str(tmp_path))
    assert r.returncode != 0 and "--aug_affine" in r.stderr


def test_cli_defaults_are_the_old_ones():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cli_train_augment", os.path.join(PKG, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parser.parse_args(["--train_dataset", "x"])
    assert (a.aug, a.aug_jitter, a.aug_affine) == ("off", None, None)
    assert mod.make_augment(a.aug, a.aug_jitter, a.aug_affine) is None                      # the host transform
    assert mod.make_augment("on", None, None) == {"jitter": None, "p_affine": 0.0}          # crop + flip only
    assert mod.make_augment("on", "0.2,0.2,0.2,0.05", 0.5) == {"jitter": (0.2, 0.2, 0.2, 0.05), "p_affine": 0.5}


def test_host_transform_still_refuses_jitter_and_affine():
    from medt_amd.data import JointTransform2D
    with pytest.raises(NotImplementedError):
        JointTransform2D(color_jitter_params=(0.1, 0.1, 0.1, 0.1))
    with pytest.raises(NotImplementedError):
        JointTransform2D(color_jitter_params=None, p_random_affine=0.5)


def test_raw_transform_and_dataset_item(tmp_path):
    """The dataset hands the uint8 pair and the record on in front of the file name; without the raw transform an item is
    the triple it always was."""
    from medt_amd.augment import RawJointTransform2D
    from medt_amd.data import ImageToImage2D, JointTransform2D, make_synthetic_dataset
    d = make_synthetic_dataset(str(tmp_path / "d"), n=2, size=(12, 10))
    np.random.seed(0)
    torch.manual_seed(0)
    img, msk, rec, name = ImageToImage2D(d, RawJointTransform2D(crop=(8, 8)))[0]
    assert img.dtype == torch.uint8 and tuple(img.shape) == (12, 10, 3) and msk.dtype == torch.uint8 and tuple(msk.shape) == (12, 10)
    assert rec.dtype == torch.float32 and tuple(rec.shape) == (20,) and name.endswith(".png") and set(msk.unique().tolist()) <= {0, 1}
    item = ImageToImage2D(d, JointTransform2D(crop=None, p_flip=0, color_jitter_params=None, long_mask=True))[0]
    assert len(item) == 3 and item[0].dtype == torch.float32 and item[1].dtype == torch.int64


@pytest.fixture(scope="module")
def lib():
    from medt_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_abi_sizes_and_refusals(lib):
    from medt_amd import _lib, augment
    assert lib.medt_augment_param_floats() == augment.PARAM_FLOATS == AO.P
    assert lib.medt_augment_workspace(4, 128, 128) == 4 * 16 + 4                # 16 parts of 1024 pixels, then the means
    assert lib.medt_augment_workspace(3, 8, 8) == 3 + 3
    assert lib.medt_augment_workspace(1, 1000, 1000) == 32 + 1                  # at most 32 parts
    for bad in ((0, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, -3)):
        assert lib.medt_augment_workspace(*bad) == 0 and b"augment_workspace" in lib.medt_last_error()
    one = ctypes.create_string_buffer(64)                                        # a non-null stand-in: refused before any use
    p = ctypes.addressof(one)
    assert lib.medt_augment_stats(None, p, p, 1, 8, 8, 3, 8, 8, None) == -1 and b"null" in lib.medt_last_error()
    assert lib.medt_augment_stats(p, p, None, 1, 8, 8, 3, 8, 8, None) == -1
    assert lib.medt_augment_stats(p, p, p, -1, 8, 8, 3, 8, 8, None) == -1 and b"bad arguments" in lib.medt_last_error()
    assert lib.medt_augment_stats(p, p, p, 1, 8, 8, 2, 8, 8, None) == -1         # two channels
    assert lib.medt_augment_apply(None, p, p, p, p, p, 1, 8, 8, 3, 8, 8, 0, None) == -1 and b"null" in lib.medt_last_error()
    assert lib.medt_augment_apply(p, p, p, p, p, None, 1, 8, 8, 3, 8, 8, 0, None) == -1
    assert lib.medt_augment_apply(p, p, p, None, p, p, 1, 8, 8, 3, 8, 8, 1, None) == -1 and b"use_stats" in lib.medt_last_error()
    assert lib.medt_augment_apply(p, p, p, p, p, p, 1, 8, 0, 3, 8, 8, 0, None) == -1
    assert lib.medt_augment_apply(p, p, p, p, p, p, 1, 8, 8, 3, -8, 8, 0, None) == -1
    assert lib.medt_augment_apply(p, p, p, p, p, p, 4, 30000, 30000, 3, 8, 8, 0, None) == -2     # 2^31 input bytes or more
    assert lib.medt_abi_version() == _lib.ABI_VERSION == 11
