"""test.py --objects / --connectivity / --min_object / --fill_holes end to end (after tests/test_surface_cli.py, whose dataset
and checkpoint recipe and driver it reuses): a seeded gatedaxialunet at 32 px on a tiny dataset of blob label maps -- on the GPU,
or under --emulate on the emulated device.  The printed lines and the written PNGs are held to the numpy oracle
(tests/label_oracle.py) on the PNGs the runs themselves wrote."""
import os

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401
import label_oracle as LO
from test_surface_cli import _checkpoint, _dataset, _oracle_line as _surface_line, _run

pytestmark = pytest.mark.gpu


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"))


def _objects_line(data, out, conn=8):
    """The line --objects on prints, from the PNGs in `out` against the label maps of `data`."""
    files = sorted(os.listdir(out))
    rows = [LO.object_scores(_png(os.path.join(out, f)), _png(os.path.join(data, "labelcol", f)) > 127, conn) for f in files]
    assert any(r["valid"] and r["n_pred"] > 0 for r in rows), "no image with an object in the mask: the case checks nothing"
    return LO.objects_line(rows, len(files))


def _pixel_line(data, out):
    """The F1 / mIoU / PA line, from counts taken from the PNGs in `out`."""
    import metrics
    counts = []
    for f in sorted(os.listdir(out)):
        p, t = _png(os.path.join(out, f)) != 0, _png(os.path.join(data, "labelcol", f)) > 127
        counts.append([(p & t).sum(), (p & ~t).sum(), (~p & t).sum(), (~p & ~t).sum()])
    f1, iou, pa = metrics.segmentation_scores(torch.tensor(counts, dtype=torch.float64))
    return "images {}  F1 {:.4f}  mIoU {:.4f}  PA {:.4f}".format(len(f1), f1.mean().item(), iou.mean().item(), pa.mean().item())


@pytest.fixture(scope="module")
def plain(tmp_path_factory, device, emulating):
    """The checkpoint, the 32 x 32 dataset and a run without any of the new flags, shared by the cases."""
    root = tmp_path_factory.mktemp("label_cli")
    ckpt = _checkpoint(str(root / "gated.pth"))
    data = _dataset(str(root / "data"), 3, (32, 32), 40)
    out = _run(emulating, ckpt, data, str(root / "plain"))
    return {"root": root, "ckpt": ckpt, "data": data, "stdout": out, "dir": root / "plain"}


def test_cli_objects_on_and_defaults(plain, emulating):
    root, data = plain["root"], plain["data"]
    on = _run(emulating, plain["ckpt"], data, str(root / "on"), "--objects", "on")
    print(on)
    lines = on.strip().splitlines()
    assert lines[-2].startswith("images 3  F1 ") and lines[-1] == _objects_line(data, str(root / "on")), on
    assert lines[:-1] == plain["stdout"].strip().splitlines()                       # the existing score line does not change
    # every new flag at its default is a run without the flags: same stdout, same PNGs, byte for byte
    off = _run(emulating, plain["ckpt"], data, str(root / "off"), "--objects", "off", "--connectivity", "8", "--min_object", "0",
               "--fill_holes", "off")
    assert off == plain["stdout"] and "objects" not in off
    files = sorted(os.listdir(plain["dir"]))
    assert len(files) == 3 and sorted(os.listdir(root / "off")) == files
    for f in files:
        assert (root / "off" / f).read_bytes() == (plain["dir"] / f).read_bytes() == (root / "on" / f).read_bytes(), f


def test_cli_objects_and_surface_with_windows(tmp_path, device, emulating, plain):
    data = _dataset(str(tmp_path / "data"), 2, (40, 52), 50)
    out = _run(emulating, plain["ckpt"], data, str(tmp_path / "win"), "--window", "on", "--objects", "on", "--surface", "on",
               "--connectivity", "4")
    print(out)
    lines = out.strip().splitlines()
    assert lines[-3].startswith("images 2  F1 ")
    assert lines[-2] == _surface_line(data, str(tmp_path / "win")), out
    assert lines[-1] == _objects_line(data, str(tmp_path / "win"), 4), out
    for f in os.listdir(tmp_path / "win"):
        assert _png(tmp_path / "win" / f).shape == (40, 52)


def test_cli_clean_ups(plain, emulating):
    root, data = plain["root"], plain["data"]
    out = _run(emulating, plain["ckpt"], data, str(root / "clean"), "--min_object", "6", "--fill_holes", "on", "--objects", "on")
    print(out)
    changed = 0
    for f in sorted(os.listdir(plain["dir"])):                                      # holes first, then the small objects
        before = _png(plain["dir"] / f)
        want = LO.remove_small(LO.fill_holes(before), 6, 8)
        assert np.array_equal(_png(root / "clean" / f), want), f
        changed += int((want != before).sum())
    assert changed > 0, "the clean-ups changed no pixel: the case checks nothing"
    lines = out.strip().splitlines()
    assert lines[-2] == _pixel_line(data, str(root / "clean")), out                 # every line describes the files written
    assert lines[-1] == _objects_line(data, str(root / "clean")), out
