"""TEST INFRASTRUCTURE (tests/test_augment_cli.py): `medical-transformer_amd/train.py` with torch's generator seeded BEFORE the
script builds its model -- train.py seeds only after construction (as the reference does), so two processes start from different
weights and their losses cannot be compared; with this driver they start from the same ones.
argv: gpu|emu <train.py args...>;  emu: on the emulated device (CPU tensors, libmedt_emu.so; tests/emu_device.py)."""
import contextlib
import ctypes
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "medical-transformer_amd")
for p in (ROOT, PKG, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    mode = sys.argv[1]
    sys.argv = [os.path.join(PKG, "train.py")] + sys.argv[2:]
    ctx = contextlib.nullcontext()
    if mode == "emu":
        import test_lane_emu as T
        from emu_device import emulated_device
        from medt_amd import _lib as L
        lib = ctypes.CDLL(T.build_emulator())
        for name, (res, args) in L.SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        ctx = emulated_device(lib)
    torch.manual_seed(1234)
    with ctx:
        runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main()
