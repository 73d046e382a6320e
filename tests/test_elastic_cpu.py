"""The elastic deformation of the device-side joint augmentation without a GPU: the oracle (tests/elastic_oracle.py) against hand
cases, the cap on what a comparison may leave out for every shared case (tests/elastic_cases.py), the host half
(medt_amd.augment.draw_field / RawJointTransform2D, train.py's flags), the refusals of medt_augment_warp, and the kernel source
on the CPU lane emulator: work-item order must not matter, and on guard-paged memory no lattice makes a read leave a buffer."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401
import augment_oracle as AO
import elastic_cases as EC
import elastic_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "medical-transformer_amd")


# ---- the oracle against hand cases ------------------------------------------------------------------------------------------
def _identity_case(C=3):
    from medt_amd.augment import make_record
    img, mask = EC.data(11, 3, 20, 30, C)
    ops = [(AO.OP_BRIGHTNESS, 1.2), (AO.OP_CONTRAST, 0.8), (AO.OP_HUE, 0.05), (AO.OP_SATURATION, 1.3)]
    recs = np.stack([make_record(2, 3, True, None, ops, elastic=True), make_record(0, 6, False, elastic=True),
                     make_record(4, 0, True, elastic=True)])
    return img, mask, recs, (16, 24)


@pytest.mark.parametrize("backend", [EO.NP64, EO.T32], ids=["NP64", "T32"])
@pytest.mark.parametrize("C", [3, 1])
def test_zero_lattice_is_the_augment_oracle_bit_for_bit(C, backend):
    img, mask, recs, size = _identity_case(C)
    got = EO.warp(img, mask, recs, np.zeros((3, 2, 6, 6), np.float32), size, backend)
    plain = recs.copy()
    plain[:, 18] = 0
    want = AO.augment(img, mask, plain, size, backend)
    assert got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[3], want[3]) and got[3][0] > 0


def test_constant_lattice_shifts_by_whole_pixels():
    """(dx, dy) = (2, -3) under the identity flag: out[i, j] = crop[i - 3, j + 2], fill where that leaves the crop."""
    img, mask, recs, (th, tw) = _identity_case()
    recs[:, 10:18] = 0
    field = np.zeros((3, 2, 6, 6), np.float32)
    field[:, 0], field[:, 1] = 2.0, -3.0
    got_i, got_m, near, _ = EO.warp(img, mask, recs, field, (th, tw))
    plain = recs.copy()
    plain[:, 18] = 0
    crop_i, crop_m, _, _ = AO.augment(img, mask, plain, (th, tw))
    want_i, want_m = np.zeros_like(crop_i), np.zeros_like(crop_m)
    want_i[:, :, 3:, :tw - 2], want_m[:, 3:, :tw - 2] = crop_i[:, :, :th - 3, 2:], crop_m[:, :th - 3, 2:]
    assert np.array_equal(got_m, want_m) and np.abs(got_i - want_i).max() <= 1e-12
    assert not near.any() and (got_m[:, :3] == 0).all() and (got_m[:, 3:, :tw - 2] != 0).all()


@pytest.mark.parametrize("G,tw", [(1, 16), (3, 24), (8, 32)])
def test_linear_lattice_reproduces_a_linear_displacement(G, tw):
    """P_k = a (k - 1) tw / G gives d = a (j + .5): cubic B-splines reproduce linear functions.  Checked to 2e-15 in float64
    (a = 1/16 and tw / G a whole number, so the float32 lattice holds P_k exactly), and the deformation equals the pure scale
    map 1 + a through the affine path of the same oracle."""
    from medt_amd.augment import make_record
    a, th = 0.0625, tw // 2
    k = np.arange(G + 3, dtype=np.float64) - 1
    field = np.zeros((1, 2, G + 3, G + 3), np.float32)
    field[0, 0] = (a * k * tw / G)[None, :]
    field[0, 1] = (a * k * th / G)[:, None]
    assert np.array_equal(field[0, 0, 0].astype(np.float64), a * k * tw / G)
    dx, dy = EO.displacement(field[0], th, tw, EO.NP64)
    err = max(np.abs(dx - a * (np.arange(tw) + 0.5)[None, :]).max(), np.abs(dy - a * (np.arange(th) + 0.5)[:, None]).max())
    print(f"G {G}: max |d - a (j + .5)| {err:.3e}")
    assert err <= 2e-15
    img, mask = EC.data(5, 1, th, tw, 3)
    got = EO.warp(img, mask, make_record(elastic=True)[None], field, (th, tw))
    want = EO.warp(img, mask, make_record(matrix=(1 + a, 0, 0, 0, 1 + a, 0), elastic=True)[None], np.zeros_like(field), (th, tw))
    keep = ~(got[2] | want[2])
    assert np.array_equal(got[1][keep], want[1][keep]) and keep.mean() > 0.9
    assert np.abs(got[0] - want[0])[np.broadcast_to(keep[:, None], got[0].shape)].max() <= 1e-12


@pytest.mark.parametrize("G", [1, 3, 8])
def test_partition_of_unity(G):
    u = np.linspace(0.0, 1.0, 1001)
    B = EO.bspline(u)
    assert all((b >= 0).all() for b in B) and np.abs(sum(B) - 1.0).max() <= 4e-16
    field = np.empty((2, G + 3, G + 3), np.float32)
    field[0], field[1] = 1.75, -5.5
    dx, dy = EO.displacement(field, 13, 29, EO.NP64)
    assert np.abs(dx - 1.75).max() <= 2e-15 and np.abs(dy + 5.5).max() <= 4e-15


# ---- the cap on what a comparison may leave out, on the oracle alone ----------------------------------------------------------
@pytest.mark.parametrize("name", EC.NAMES, ids=EC.case_id)
def test_cap_on_the_pixels_left_out(name):
    """At most 1 % of a batch's pixels within NEAR_TOL of an integer coordinate; tiny crops (5 x 6, 7 x 8): one pixel per image."""
    c = EC.case(name)
    th, tw = c["size"]
    near = EO.warp(c["img"], c["mask"], c["recs"], c["field"], c["size"])[2]
    print(f"{EC.case_id(name)}: {int(near.sum())} of {near.size} pixels near an integer coordinate ({100 * near.mean():.2f} %), at most "
          f"{int(near.reshape(len(near), -1).sum(1).max())} in an image")
    assert EC.cap_holds(near, c["size"])
    if th >= 32 and tw >= 32:
        assert near.mean() <= 0.01
    if th * tw < 100:
        assert (near.reshape(len(near), -1).sum(1) <= 1).all()
    assert c["field"].any() and c["mask"].min() >= 1 and c["recs"].shape == (len(c["img"]), 20)


# ---- the host half -----------------------------------------------------------------------------------------------------------
def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)


def test_draw_field():
    from medt_amd.augment import draw_field
    _seed(3)
    f = draw_field(3, 4.0)
    _seed(3)
    want = np.clip(np.random.normal(0, 4.0, (2, 6, 6)), -12.0, 12.0).astype(np.float32)
    assert f.dtype == np.float32 and f.shape == (2, 6, 6) and np.array_equal(f, want)
    _seed(4)
    big = np.stack([draw_field(8, 0.5) for _ in range(200)])
    assert big.shape == (200, 2, 11, 11) and np.abs(big).max() == 1.5 and (np.abs(big) == 1.5).mean() < 0.01      # clipped to 3 sigma
    for G in (0, 9):
        with pytest.raises(ValueError):
            draw_field(G, 1.0)


def test_raw_transform_draws():
    """elastic=None: today's draws and 3-tuple; configured: the first three elements are today's (the flag apart), the lattice
    is drawn AFTER every other draw of the item, stays within 3 sigma, and is zero when the item did not draw."""
    from medt_amd.augment import RawJointTransform2D, draw_record
    img, mask = EC.data(1, 1, 21, 17, 3)
    img, mask = img[0], mask[0]
    cfg = dict(crop=(8, 8), p_flip=0.5, jitter=(0.4, 0.4, 0.0, 0.1), p_affine=0.5)
    _seed(21)
    today = [draw_record(21, 17, cfg["crop"], cfg["p_flip"], cfg["jitter"], cfg["p_affine"]) for _ in range(12)]
    after_today = np.random.rand()
    _seed(21)
    plain = RawJointTransform2D(**cfg)
    items = [plain(img, mask) for _ in range(12)]
    assert np.random.rand() == after_today
    assert all(len(it) == 3 and np.array_equal(it[2].numpy(), r) and not it[2][18] for it, r in zip(items, today))
    assert all(it[0].dtype == torch.uint8 and torch.equal(it[0], torch.from_numpy(img)) for it in items)

    elastic = {"p": 0.5, "grid": 3, "sigma": 2.0}
    tf = RawJointTransform2D(**cfg, elastic=elastic)
    flags = []
    _seed(22)
    for _ in range(40):
        state = np.random.get_state(), torch.get_rng_state()
        want = draw_record(21, 17, cfg["crop"], cfg["p_flip"], cfg["jitter"], cfg["p_affine"])
        drew = np.random.rand() < 0.5
        want_field = np.clip(np.random.normal(0, 2.0, (2, 6, 6)), -6.0, 6.0).astype(np.float32) if drew else np.zeros((2, 6, 6), np.float32)
        end = np.random.get_state()[1].copy()
        np.random.set_state(state[0])
        torch.set_rng_state(state[1])
        i, m, r, f = tf(img, mask)
        assert np.array_equal(np.random.get_state()[1], end)
        assert torch.equal(i, torch.from_numpy(img)) and torch.equal(m, torch.from_numpy(mask))
        assert np.array_equal(r.numpy()[:18], want[:18]) and r[19] == 0 and bool(r[18]) == drew
        assert f.dtype == torch.float32 and tuple(f.shape) == (2, 6, 6) and np.array_equal(f.numpy(), want_field)
        assert np.abs(f.numpy()).max() <= 6.0 and bool(f.any()) == drew
        flags.append(drew)
    assert 5 < sum(flags) < 35
    with pytest.raises(ValueError):
        RawJointTransform2D(elastic={"p": 1.0, "grid": 9, "sigma": 1.0})


def test_make_record_flag():
    from medt_amd.augment import ELASTIC_SLOT, PARAM_FLOATS, make_record
    assert ELASTIC_SLOT == EO.ELASTIC_SLOT == 18 and PARAM_FLOATS == 20
    r0, r1 = make_record(1, 2, True), make_record(1, 2, True, elastic=True)
    assert r0[18] == 0 and r1[18] == 1 and r1[19] == 0 and np.array_equal(r0[:18], r1[:18])


def _train_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cli_train_elastic", os.path.join(PKG, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_make_augment():
    mod = _train_module()
    a = mod.parser.parse_args(["--train_dataset", "x"])
    assert (a.aug_elastic, a.aug_elastic_grid, a.aug_elastic_sigma) == (None, None, None)
    assert mod.make_augment("off", None, None) is None and mod.make_augment("off", None, None, None, None, None) is None
    assert mod.make_augment("on", None, None) == {"jitter": None, "p_affine": 0.0}                           # unchanged
    assert mod.make_augment("on", "0.2,0.2,0.2,0.05", 0.5) == {"jitter": (0.2, 0.2, 0.2, 0.05), "p_affine": 0.5}
    assert mod.make_augment("on", None, None, None, None, None) == {"jitter": None, "p_affine": 0.0}
    assert mod.make_augment("on", None, None, 0.0) == {"jitter": None, "p_affine": 0.0}                      # no key at P = 0
    assert mod.make_augment("on", None, 0.5, 0.25) == {"jitter": None, "p_affine": 0.5, "elastic": {"p": 0.25, "grid": 3, "sigma": 4.0}}
    assert mod.make_augment("on", None, None, 1.0, 8, 2.5)["elastic"] == {"p": 1.0, "grid": 8, "sigma": 2.5}
    for bad in ((1.5, None, None), (-0.1, None, None), (0.5, 0, None), (0.5, 9, None), (0.5, 3, -1.0), (0.5, 3, float("inf")),
                (0.5, 3, float("nan")), (None, 3, None), (None, None, 2.0)):
        with pytest.raises(SystemExit):
            mod.make_augment("on", None, None, *bad)
    for bad in ((0.5, None, None), (None, 3, None), (None, None, 2.0)):
        with pytest.raises(SystemExit):
            mod.make_augment("off", None, None, *bad)


def _train(*argv, cwd):
    env = dict(os.environ, PYTHONPATH=PKG)
    return subprocess.run([sys.executable, os.path.join(PKG, "train.py"), *argv], env=env, capture_output=True, text=True,
                          timeout=300, cwd=cwd)


def test_cli_refusals(tmp_path):
    """Before any work: no dataset exists, no GPU is touched."""
    none = str(tmp_path / "none")
    for extra in (["--aug_elastic", "0.5"], ["--aug", "off", "--aug_elastic_grid", "3"], ["--aug_elastic_sigma", "2"]):
        r = _train("--train_dataset", none, *extra, cwd=str(tmp_path))
        assert r.returncode != 0 and "add --aug on" in r.stderr, r.stderr[-1000:]
    for extra, word in ((["--aug_elastic", "1.5"], "--aug_elastic:"), (["--aug_elastic", "0.5", "--aug_elastic_grid", "9"], "--aug_elastic_grid"),
                        (["--aug_elastic", "0.5", "--aug_elastic_sigma=-1"], "--aug_elastic_sigma"), (["--aug_elastic_grid", "3"], "add --aug_elastic")):
        r = _train("--train_dataset", none, "--aug", "on", *extra, cwd=str(tmp_path))
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr[-1000:])
    assert not (tmp_path / "none").exists()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_refusals():
    from medt_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.lib()
    one = ctypes.create_string_buffer(64)                                        # a non-null stand-in: refused before any use
    p = ctypes.addressof(one)
    call = lib.medt_augment_warp
    good = [p, p, p, p, 3, p, p, p, 1, 8, 8, 3, 8, 8, 0, None]

    def with_(**kw):
        names = ["image", "mask", "params", "field", "G", "workspace", "out_image", "out_mask", "N", "H", "W", "C", "th", "tw", "use_stats", "stream"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a
    assert call(*with_(field=None)) == -1 and b"lattice" in lib.medt_last_error()
    assert call(*with_(G=0)) == -1 and b"grid" in lib.medt_last_error()
    assert call(*with_(G=9)) == -1 and call(*with_(G=-1)) == -1
    assert call(*with_(C=2)) == -1 and b"bad arguments" in lib.medt_last_error() and b"augment_warp" in lib.medt_last_error()
    assert call(*with_(th=-8)) == -1 and call(*with_(W=0)) == -1 and call(*with_(N=-1)) == -1
    for name in ("image", "mask", "params", "out_image", "out_mask"):
        assert call(*with_(**{name: None})) == -1 and b"null" in lib.medt_last_error()
    assert call(*with_(workspace=None, use_stats=1)) == -1 and b"use_stats" in lib.medt_last_error()
    assert call(*with_(N=4, H=30000, W=30000)) == -2                             # 2^31 input bytes or more
    assert lib.medt_augment_param_floats() == 20 and lib.medt_abi_version() == _lib.ABI_VERSION == 11


# ---- the kernel source on the lane emulator ------------------------------------------------------------------------------------
def test_kernel_is_schedule_independent():
    """One case (crop, flip, jitter with a contrast mean, affine, mixed flags) under three work-item orders: identical bits."""
    import guard_driver as D
    from emu_device import emulated_device
    from medt_amd import ops
    lib = D.emu_lib()
    c = EC.case(EC.MIXED)
    runs = []
    try:
        with emulated_device(lib):
            for mode in (0, 1, 2):
                lib.emu_set_order(mode, 9)
                ws = torch.zeros(ops.augment_workspace(4, c["size"]))
                oi, om = ops.augment_batch(torch.from_numpy(c["img"].copy()), torch.from_numpy(c["mask"].copy()), torch.from_numpy(c["recs"].copy()),
                                           c["size"], workspace=ws, field=torch.from_numpy(c["field"].copy()))
                runs.append((oi.numpy().view(np.uint32).copy(), om.numpy().copy(), ws.numpy().view(np.uint32).copy()))
    finally:
        lib.emu_set_order(0, 0)
    for r in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], r))
    want_i, want_m, near, _ = EO.warp(c["img"], c["mask"], c["recs"], c["field"], c["size"])
    assert np.array_equal(runs[0][1][~near], want_m[~near]) and runs[0][0].any()


@pytest.mark.parametrize("placement", ["tail", "head"])
def test_on_guarded_memory(placement):
    """Ordinary, non-finite (NaN, +-1e30, inf) and huge finite lattices with every buffer flush against a guard page: -11 would
    mean a read or write outside a buffer; the non-finite and huge ones give all fill (asserted in the driver)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "elastic_guard_driver.py"), placement], capture_output=True,
                       text=True, timeout=900, cwd=ROOT)
    lines = r.stdout.strip().splitlines()
    last = next((ln for ln in reversed(lines) if ln.startswith("CALL ")), "(no library call announced)")
    assert r.returncode == 0, "return code %d%s\nlast announced: %s\n%s" % (
        r.returncode, " (SIGSEGV: the kernel left a buffer it was given)" if r.returncode == -11 else "", last, r.stderr[-3000:])
    s = json.loads(lines[-1])
    print(json.dumps(s))
    assert s["cases"] == 6 and s["entries"].get("medt_augment_warp") == 6 and s["entries"].get("medt_augment_stats", 0) >= 2
    assert s["unguarded"] == 0 and s["allowed"] == 0 and s["in_arena"] + s["stood_in"] == s["pointers"] and s["pointers"] >= 6 * 7
