"""medt_seg_loss_*: sizes and argument validation of the C ABI (no GPU: every call ends in the validation layer or in host
arithmetic; a non-NULL placeholder stands where a device pointer would, and is never dereferenced by a refused call)."""
import pytest

import helpers as H  # noqa: F401

OK, EINVAL = 0, -1
PTR = 0x1000            # "some device pointer": refused calls never launch


@pytest.fixture(scope="module")
def lib():
    from medt_amd import build, _lib
    build.build(verbose=False)          # hipcc cross-compiles for gfx950 without a GPU
    return _lib.lib()


def test_abi_version_and_sizes(lib):
    from medt_amd import _lib
    assert lib.medt_abi_version() == _lib.ABI_VERSION == 11
    # partials: one row of {sum w nll, sum w, bad targets} + 3 K Dice sums per 256-pixel block of every image
    assert lib.medt_seg_loss_workspace(3, 2, 323) == 3 * 2 * (3 + 6)
    assert lib.medt_seg_loss_workspace(2, 8, 81) == 2 * 1 * (3 + 24)
    assert lib.medt_seg_loss_workspace(2, 2, 130 * 130) == 2 * 67 * 9
    assert lib.medt_seg_loss_workspace(1, 11, 256) == 3                  # K > 8: cross entropy only
    assert lib.medt_seg_loss_out_floats(3, 2) == 5 + 2 * 3 * 2
    for bad in ((0, 2, 64), (2, 0, 64), (2, 2, 0), (-1, 2, 64), (2, -3, 64), (2, 2, -64)):
        assert lib.medt_seg_loss_workspace(*bad) == 0
    assert lib.medt_seg_loss_out_floats(0, 2) == 0 and lib.medt_seg_loss_out_floats(2, 0) == 0


def fwd(lib, logits=PTR, target=PTR, weight=None, partials=PTR, out=PTR, N=2, K=2, HW=64, ce=1.0, dice=1.0, eps=1.0):
    return lib.medt_seg_loss_fwd(logits, target, weight, partials, out, N, K, HW, -100, ce, dice, eps, None)


def bwd(lib, logits=PTR, target=PTR, weight=None, out=PTR, dloss=None, dlogits=PTR, N=2, K=2, HW=64, ce=1.0, dice=1.0, eps=1.0):
    return lib.medt_seg_loss_bwd(logits, target, weight, out, dloss, dlogits, N, K, HW, -100, ce, dice, eps, None)


def test_null_pointers_are_refused(lib):
    assert lib.medt_seg_loss_fwd(None, None, None, None, None, 2, 2, 64, -100, 1.0, 1.0, 1.0, None) == EINVAL
    assert lib.medt_seg_loss_bwd(None, None, None, None, None, None, 2, 2, 64, -100, 1.0, 1.0, 1.0, None) == EINVAL
    for name in ("logits", "target", "partials", "out"):
        assert fwd(lib, **{name: None}) == EINVAL, name
        assert b"seg_loss fwd" in lib.medt_last_error()
    for name in ("logits", "target", "out", "dlogits"):
        assert bwd(lib, **{name: None}) == EINVAL, name
        assert b"seg_loss bwd" in lib.medt_last_error()


@pytest.mark.parametrize("call", [fwd, bwd])
def test_sizes_scales_and_class_limits(lib, call):
    for kw in ({"N": 0}, {"N": -2}, {"K": 0}, {"K": -1}, {"HW": 0}, {"HW": -64}, {"eps": -1e-3}, {"eps": float("nan")}):
        assert call(lib, **kw) == EINVAL, kw
    for K in (1, 9, 64):                                       # soft Dice keeps 2 <= K <= 8 class sums in registers
        assert call(lib, K=K) == EINVAL, K
        assert b"2 <= K <= 8" in lib.medt_last_error()
    assert call(lib, N=1 << 30, HW=1 << 20, dice=0.0) < 0       # a grid beyond 2^31 workgroups
