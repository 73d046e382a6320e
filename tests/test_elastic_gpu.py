"""The elastic deformation of the device-side joint augmentation (csrc/elementwise.hip augment_warp_kernel through
medt_amd.ops.augment_batch(field=...)) against the restatement of its specification (tests/elastic_oracle.py), on the cases of
tests/elastic_cases.py.

Yardstick: that of tests/test_augment_gpu.py.  Output pixels whose coordinate lies within 1e-3 of an integer are left out (the
mask tap and the inside test are discontinuous only there), and their share is capped: 1 % of a batch, one pixel per image
for the tiny crops (asserted here and, on the oracle alone, in tests/test_elastic_cpu.py).  Everywhere else masks are exact and
images stay within max(4 x |T32 - NP64|max, 2^-20): the deviation of the SAME formulas evaluated in float32 (torch, CPU; spline,
map, floors, weights and blend) from their float64 evaluation, taken over the same pixels.  Every case prints error, noise and
ratio.  Run with `-m gpu`, or `-m gpu --emulate` on the lane emulator."""
import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401
import elastic_cases as EC
import elastic_oracle as EO

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -20
_ORACLE = {}


def _sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize()


def _oracle(name):
    """(case, float64 image, mask, near, means, float32 image): computed once per case, shared, never written."""
    if name not in _ORACLE:
        c = EC.case(name)
        want = EO.warp(c["img"], c["mask"], c["recs"], c["field"], c["size"])
        f32 = EO.warp(c["img"], c["mask"], c["recs"], c["field"], c["size"], backend=EO.T32)[0]
        for a in (*c.values(), *want, f32):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ORACLE[name] = (c, *want, f32)
    return _ORACLE[name]


def _run(device, c, field="case", recs=None, **kw):
    from medt_amd import ops
    recs = np.ascontiguousarray(c["recs"] if recs is None else recs, np.float32)
    if isinstance(field, str):
        field = c["field"]
    if field is not None:
        kw["field"] = torch.from_numpy(np.array(field, np.float32)).to(device)
    oi, om = ops.augment_batch(torch.from_numpy(c["img"].copy()).to(device), torch.from_numpy(c["mask"].copy()).to(device),
                               torch.from_numpy(recs.copy()).to(device), c["size"], host_params=torch.from_numpy(recs.copy()), **kw)
    _sync(device)
    assert oi.dtype == torch.float32 and om.dtype == torch.int64
    return oi.cpu().numpy(), om.cpu().numpy()


def _check(device, name, **kw):
    """Run the kernel on a shared case and hold it to the oracle; returns (image, mask) as numpy."""
    c, want_i, want_m, near, _, f32_i = _oracle(name)
    what = EC.case_id(name)
    keep = ~near
    sel = np.broadcast_to(keep[:, None], want_i.shape)
    noise = float(np.abs(f32_i.astype(np.float64) - want_i)[sel].max())
    tol = max(4.0 * noise, FLOOR)
    got_i, got_m = _run(device, c, **kw)
    err = float(np.abs(got_i.astype(np.float64) - want_i)[sel].max())
    print(f"{what}: max |kernel - float64| {err:.3e}, float32 noise of the formulas {noise:.3e}, ratio "
          f"{err / noise if noise else float('nan'):.2f}, tolerance {tol:.3e}; {100 * near.mean():.2f} % of the pixels near an integer "
          f"coordinate, at most {int(near.reshape(len(near), -1).sum(1).max())} in an image")
    assert EC.cap_holds(near, c["size"]), what
    assert np.array_equal(got_m[keep], want_m[keep]), what
    assert err <= tol, what
    assert np.isfinite(got_i).all() and got_i.min() >= 0.0 and got_i.max() <= 1.0
    return got_i, got_m


@pytest.mark.parametrize("name", EC.STORE, ids=EC.case_id)
def test_store_paths_and_grids(device, name):
    """tw % 4 != 0 (element tail; G = 8 is more cells than the crop has pixels), tw % 4 == 0 (16-byte stores), several rows per
    block, several blocks per image; C = 3 and 1; G = 1, 3, 8.  Elastic alone, with flip at the far corner, with an affine map."""
    got_i, got_m = _check(device, name)
    assert (got_m != 0).any() and got_i.any()


@pytest.mark.parametrize("name", EC.COMPOSITIONS, ids=EC.case_id)
def test_compositions(device, name):
    from medt_amd import ops
    c, _, _, _, means, _ = _oracle(name)
    N = len(c["img"])
    ws = torch.full((ops.augment_workspace(N, c["size"]),), 7.0, device=device)
    _check(device, name, workspace=ws)
    ws = ws.cpu().numpy()
    if (c["recs"][:, 10:14] == 2).any():             # the contrast mean is the stats launch's, of the UNWARPED crop
        assert np.abs(ws[-N:] - means).max() <= 2.0 ** -20
    else:                                            # the statistics launch was skipped: partial sums untouched, means 0
        assert (ws[:-N] == 7.0).all() and (ws[-N:] == 0.0).all()


def test_mixed_batch(device):
    """Flags [1, 0, 1, 0]: the flag-0 images are ops.augment_batch's without a field, bit for bit, whatever their neighbours
    hold; every image equals its own single-image call, bit for bit."""
    from medt_amd import ops
    c = _oracle(EC.MIXED)[0]
    assert [int(f) for f in c["recs"][:, 18]] == [1, 0, 1, 0]
    ws = torch.zeros(ops.augment_workspace(4, c["size"]), device=device)
    got_i, got_m = _check(device, EC.MIXED, workspace=ws)
    means = ws.cpu().numpy()[-4:]
    plain_i, plain_m = _run(device, c, field=None)
    for n in (1, 3):
        assert np.array_equal(got_i[n].view(np.uint32), plain_i[n].view(np.uint32)) and np.array_equal(got_m[n], plain_m[n])
    assert not np.array_equal(got_i[0], plain_i[0]) and not np.array_equal(got_i[2], plain_i[2])
    for n in range(4):
        one = {k: (v[n:n + 1] if k != "size" else v) for k, v in c.items()}
        ws1 = torch.zeros(ops.augment_workspace(1, c["size"]), device=device)
        i1, m1 = _run(device, one, workspace=ws1)
        assert np.array_equal(i1[0].view(np.uint32), got_i[n].view(np.uint32)) and np.array_equal(m1[0], got_m[n]), n
        assert ws1.cpu().numpy()[-1] == means[n]


def test_launch_choice(device):
    """A field whose records all have the flag at 0 takes medt_augment_apply: today's bits, and a workspace nobody touches
    (the records have no contrast slot, so neither launch of today's writes it -- the means slot of a workspace is written
    by either apply launch, so the means are compared with the plain call's)."""
    from medt_amd import ops
    c = _oracle(("composition", "affine"))[0]
    recs = c["recs"].copy()
    recs[:, 18] = 0.0
    N = len(recs)
    plain_ws = torch.full((ops.augment_workspace(N, c["size"]),), 7.0, device=device)
    plain_i, plain_m = _run(device, c, field=None, recs=recs, workspace=plain_ws)
    ws = torch.full((ops.augment_workspace(N, c["size"]),), 7.0, device=device)
    got_i, got_m = _run(device, c, recs=recs, workspace=ws)
    assert np.array_equal(got_i.view(np.uint32), plain_i.view(np.uint32)) and np.array_equal(got_m, plain_m)
    assert torch.equal(ws.cpu(), plain_ws.cpu()) and (ws.cpu().numpy()[:-N] == 7.0).all()
    moved_i, _ = _run(device, c)                                               # (with the flags set the lattice does act)
    assert not np.array_equal(moved_i, plain_i)


@pytest.mark.parametrize("name", [("composition", "flip_far_corner"), ("composition", "jitter")], ids=EC.case_id)
def test_zero_lattice_under_identity_gives_todays_bits(device, name):
    """Flags set, all-zero lattice, identity flag: the weights are exactly 0 and 1, the bits those of the nearest path."""
    c = _oracle(name)[0]
    assert c["recs"][:, 18].all() and c["recs"][:, 3].all()
    got_i, got_m = _run(device, c, field=np.zeros_like(c["field"]))
    plain_i, plain_m = _run(device, c, field=None)
    assert np.array_equal(got_i.view(np.uint32), plain_i.view(np.uint32)) and np.array_equal(got_m, plain_m)
    moved_i, _ = _run(device, c)
    assert not np.array_equal(moved_i, plain_i)


def test_non_finite_and_huge_lattices_are_all_fill(device):
    """NaN, +-1e30 and inf in the lattice, and a large finite lattice that pushes every coordinate far outside: image 0, mask 0
    (the classes are 1 and 2), finite output, nothing read out of bounds.  One image keeps an ordinary lattice."""
    c = _oracle(("composition", "affine"))[0]
    assert c["mask"].min() >= 1
    field = c["field"].copy()
    field[0] = np.nan
    field[1].flat[::3], field[1].flat[1::3], field[1].flat[2::3] = 1e30, -1e30, np.inf
    field[2] = 1e6
    got_i, got_m = _run(device, c, field=field)
    ref_i, ref_m = _run(device, c)
    assert np.isfinite(got_i).all()
    for n in range(3):
        assert not got_i[n].any() and not got_m[n].any(), n
    assert np.array_equal(got_i[3], ref_i[3]) and np.array_equal(got_m[3], ref_m[3]) and got_m[3].any()


def test_misaligned_output_takes_the_element_path(device):
    """An output image 4 bytes off a 16-byte boundary is written with element stores: the same bits, the canaries intact."""
    c = _oracle(("composition", "everything"))[0]
    N, (th, tw) = len(c["img"]), c["size"]
    ref_i, ref_m = _run(device, c)
    n = N * 3 * th * tw
    store = torch.full((n + 2,), -7.0, device=device)
    oi = store[1:n + 1].view(N, 3, th, tw)
    mstore = torch.full((N * th * tw + 2,), -7, device=device, dtype=torch.int64)
    om = mstore[1:-1].view(N, th, tw)
    if device.type == "cuda":
        assert oi.data_ptr() % 16 == 4
    got_i, got_m = _run(device, c, out=(oi, om))
    assert np.array_equal(got_i.view(np.uint32), ref_i.view(np.uint32)) and np.array_equal(got_m, ref_m)
    assert store[0].item() == -7.0 and store[n + 1].item() == -7.0 and mstore[0].item() == -7 and mstore[-1].item() == -7


def test_two_runs_give_the_same_bits(device):
    from medt_amd import ops
    c = _oracle(("composition", "everything"))[0]
    runs = []
    for _ in range(2):
        ws = torch.zeros(ops.augment_workspace(len(c["img"]), c["size"]), device=device)
        i, m = _run(device, c, workspace=ws)
        runs.append((i.view(np.uint32), m, ws.cpu().numpy().view(np.uint32)))
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    assert runs[0][2][-len(c["img"]):].any()                                   # the means were written


def test_wrapper_refusals(device, emulating):
    from medt_amd import MedtError, ops
    c = _oracle(("composition", "alone"))[0]
    ti, tm = torch.from_numpy(c["img"].copy()).to(device), torch.from_numpy(c["mask"].copy()).to(device)
    tp, tf = torch.from_numpy(c["recs"].copy()).to(device), torch.from_numpy(c["field"].copy()).to(device)
    N, size = len(c["img"]), c["size"]
    bad = [tf[:, :1], tf[:, :, :5], tf[:, :, :, :5], tf[:1], tf[0], tf.double(),                    # shape, square, N, rank, dtype
           torch.zeros((N, 2, 3, 3), device=device), torch.zeros((N, 2, 12, 12), device=device),      # G = 0 and 9
           torch.zeros((N, 2, 6, 12), device=device)[:, :, :, ::2]]                                    # non-contiguous
    for f in bad:
        with pytest.raises(MedtError):
            ops.augment_batch(ti, tm, tp, size, field=f)
    if not emulating:                                                                                 # (the emulated device IS the CPU)
        with pytest.raises(MedtError):
            ops.augment_batch(ti, tm, tp, size, field=tf.cpu())
    ops.augment_batch(ti, tm, tp, size, field=tf)                                                     # and the good call goes through
    _sync(device)
