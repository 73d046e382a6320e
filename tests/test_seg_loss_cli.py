"""train.py --loss / --class_weights (after tests/test_cli_and_data.py::test_train_then_test_cli_roundtrip): two epochs of
gatedaxialunet with DiceCELoss(weight=[1, 3]) on synthetic images, and the refusal of a weight list of the wrong length."""
import os
import re
import subprocess
import sys

import pytest

import helpers as H  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "medical-transformer_amd")


@pytest.mark.gpu
def test_train_cli_dice_ce_with_class_weights(tmp_path, device, emulating):
    """On the GPU: the model and size of test_train_then_test_cli_roundtrip, replayed steps.  Under --emulate: train.py on the
    emulated device (tests/seg_loss_cli_driver.py), eager, 32-px images: about two minutes
    on one core (the emulator runs a step in tens of seconds; the time limit is a ceiling for a loaded host)."""
    env = dict(os.environ, PYTHONPATH=PKG)
    d, out = str(tmp_path / "data"), str(tmp_path / "run")
    if emulating:
        cmd = [sys.executable, os.path.join(ROOT, "tests", "seg_loss_cli_driver.py"), "--imgsize", "32", "--synthetic", "2",
               "--batch_size", "2", "--save_freq", "2", "--device", "cpu", "--eager"]
        saved, params = "0", None
    else:
        cmd = [sys.executable, os.path.join(PKG, "train.py"), "--imgsize", "128", "--synthetic", "8", "--batch_size", "4",
               "--save_freq", "1"]
        saved, params = "1", "Total_params: 1326850"
    r = subprocess.run(cmd + ["--train_dataset", d, "--val_dataset", d, "--direc", out, "--epoch", "2", "--modelname",
                              "gatedaxialunet", "--learning_rate", "0.001", "--gray", "no", "--loss", "ce+dice",
                              "--class_weights", "1,3"], env=env, capture_output=True, text=True, timeout=3000 if emulating else 600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert params is None or params in r.stdout
    losses = [float(v) for v in re.findall(r"epoch \[\d+/2\], loss:([0-9.naninf-]+)", r.stdout)]
    assert len(losses) == 2, r.stdout
    assert all(0.0 < v < 100.0 for v in losses), losses            # finite (nan fails every comparison)
    assert losses[1] <= losses[0], losses
    assert os.path.exists(os.path.join(out, saved, "gatedaxialunet.pth")) and os.path.exists(out + "final_model.pth")


def test_class_weights_of_the_wrong_length_are_refused(tmp_path):
    """Three weights for the two classes of the networks: a clear message, before any work (no GPU, no dataset needed)."""
    env = dict(os.environ, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--train_dataset", str(tmp_path / "none"), "--loss",
                        "ce+dice", "--class_weights", "1,2,3"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--class_weights: 3 weights given, the networks have 2 classes" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--train_dataset", str(tmp_path / "none"), "--loss",
                        "focal"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--loss" in r.stderr


def test_default_criterion_is_the_plain_cross_entropy():
    """Without the new flags: LogNLLLoss() as before; with them: the weighted / Dice criteria."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("cli_train_seg_loss", os.path.join(PKG, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from metrics import DiceCELoss, LogNLLLoss
    a = mod.parser.parse_args(["--train_dataset", "x"])
    assert (a.loss, a.class_weights) == ("ce", None)
    c = mod.make_criterion(a.loss, a.class_weights)
    assert isinstance(c, LogNLLLoss) and c.weight is None
    c = mod.make_criterion("ce", "1,3")
    assert isinstance(c, LogNLLLoss) and c.weight.tolist() == [1.0, 3.0]
    c = mod.make_criterion("ce+dice", "1,3")
    assert isinstance(c, DiceCELoss) and (c.ce, c.dice) == (1.0, 1.0) and c.weight.tolist() == [1.0, 3.0]
    c = mod.make_criterion("dice", None)
    assert isinstance(c, DiceCELoss) and (c.ce, c.dice) == (0.0, 1.0) and c.weight is None
