"""test.py --object_hausdorff end to end (after tests/test_label_cli.py, whose dataset, checkpoint and driver it shares): a seeded
gatedaxialunet at 32 px on a tiny dataset of blob label maps -- on the GPU, or under --emulate on the emulated device.  The
printed line is held to the numpy oracle (tests/hausdorff_oracle.py) and to metrics.object_hausdorff on the PNGs the runs
themselves wrote."""
import os

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401
import hausdorff_oracle as HO
from test_label_cli import _objects_line, _pixel_line, _png
from test_label_gpu import _dev
from test_surface_cli import _checkpoint, _dataset, _oracle_line, _run

pytestmark = pytest.mark.gpu


def _pairs(data, out):
    files = sorted(os.listdir(out))
    return files, [(_png(os.path.join(out, f)), (_png(os.path.join(data, "labelcol", f)) > 127).astype(np.uint8)) for f in files]


def _hausdorff_line(data, out, conn=8):
    """The line --object_hausdorff on prints, from the PNGs in `out` against the label maps of `data`, by brute force."""
    files, pairs = _pairs(data, out)
    rows = [HO.object_hausdorff(p, t, conn) for p, t in pairs]
    assert any(r["valid"] for r in rows), "no image with an object on both sides: the case checks nothing"
    return HO.hausdorff_line(rows, len(files))


@pytest.fixture(scope="module")
def plain(tmp_path_factory, device, emulating):
    root = tmp_path_factory.mktemp("object_hausdorff_cli")
    ckpt = _checkpoint(str(root / "gated.pth"))
    data = _dataset(str(root / "data"), 3, (32, 32), 40)
    out = _run(emulating, ckpt, data, str(root / "plain"))
    return {"root": root, "ckpt": ckpt, "data": data, "stdout": out, "dir": root / "plain"}


def test_cli_object_hausdorff_on_and_off(plain, device, emulating):
    import metrics
    root, data = plain["root"], plain["data"]
    on = _run(emulating, plain["ckpt"], data, str(root / "on"), "--object_hausdorff", "on")
    print(on)
    lines = on.strip().splitlines()
    assert lines[-2].startswith("images 3  F1 ") and lines[-1] == _hausdorff_line(data, str(root / "on")), on
    assert lines[-1].startswith("object hausdorff images ") and "objects images" not in on      # only its own line
    assert lines[:-1] == plain["stdout"].strip().splitlines()                       # the existing score line does not change
    # the printed value is metrics.object_hausdorff of the written masks
    files, pairs = _pairs(data, str(root / "on"))
    got = metrics.object_hausdorff(_dev(np.stack([p for p, _ in pairs]), device), _dev(np.stack([t for _, t in pairs]) * np.uint8(255), device))
    want = "object hausdorff images {}/{}  Hobj {:.4f}".format(int(got["valid"].sum()), len(files), got["hd"][got["valid"]].mean().item())
    assert lines[-1] == want
    # the flag at its default is a run without it: same stdout, same PNGs, byte for byte
    off = _run(emulating, plain["ckpt"], data, str(root / "off"), "--object_hausdorff", "off")
    assert off == plain["stdout"] and "hausdorff" not in off
    assert len(files) == 3 and sorted(os.listdir(root / "off")) == files
    for f in files:
        assert (root / "off" / f).read_bytes() == (plain["dir"] / f).read_bytes() == (root / "on" / f).read_bytes(), f


ALL_STAGES = ("--fill_holes", "on", "--min_object", "6", "--surface", "on", "--objects", "on", "--object_hausdorff", "on")


def test_cli_every_stage_at_once_behind_each_view_predictor(tmp_path, device, emulating, plain):
    """Every stage of test.py's one loop switched on -- both clean-ups and the three score lines -- behind --tta flips, behind
    --tta d4 at a gather that divides neither the group nor its views, and behind --window on --tta d4 on 40 x 52 images: each of
    the four printed lines is the oracle's, computed from the PNGs the run wrote, and no image is counted out.  The emulated
    device runs only the first of the three (the three together take it ten minutes); the GPU runs all."""
    wide = _dataset(str(tmp_path / "data"), 2, (40, 52), 50)
    runs = [("flips", plain["data"], 3, ("--tta", "flips")),
            ("d4", plain["data"], 3, ("--tta", "d4", "--gather", "3")),
            ("win_d4", wide, 2, ("--window", "on", "--tta", "d4"))]
    for name, data, n, flags in runs[:1] if emulating else runs:
        out_dir = str(tmp_path / name)
        out = _run(emulating, plain["ckpt"], data, out_dir, *flags, *ALL_STAGES)
        print(out)
        lines = out.strip().splitlines()
        assert lines[-4:] == [_pixel_line(data, out_dir), _oracle_line(data, out_dir), _objects_line(data, out_dir),
                              _hausdorff_line(data, out_dir)], (name, out)
        assert lines[-4].startswith("images {}  F1 ".format(n)), (name, out)
        for line, prefix in zip(lines[-3:], ("surface", "objects", "object hausdorff")):
            assert line.startswith("{} images {}/{}  ".format(prefix, n, n)), (name, line)
        assert len(os.listdir(out_dir)) == n


def test_cli_object_hausdorff_with_windows_objects_and_clean_ups(tmp_path, device, emulating, plain):
    data = _dataset(str(tmp_path / "data"), 2, (40, 52), 50)
    out = _run(emulating, plain["ckpt"], data, str(tmp_path / "win"), "--window", "on", "--objects", "on", "--object_hausdorff", "on",
               "--connectivity", "4", "--min_object", "4", "--fill_holes", "on")
    print(out)
    lines = out.strip().splitlines()
    assert lines[-3].startswith("images 2  F1 ")
    assert lines[-2] == _objects_line(data, str(tmp_path / "win"), 4), out
    assert lines[-1] == _hausdorff_line(data, str(tmp_path / "win"), 4), out
    for f in os.listdir(tmp_path / "win"):
        assert _png(tmp_path / "win" / f).shape == (40, 52)
