"""TEST INFRASTRUCTURE (tests/test_split_cpu.py): the splitting kernels on guard-paged memory, in one process --
`python tests/split_guard_driver.py PLACEMENT` (tail | head), after tests/guard_driver.py.  medt_amd.ops.split_markers,
grow_labels and split_objects run on the CPU lane emulator with every buffer that reaches the C ABI (masks, depth and component
maps, tables, markers, seeds, the growth's workspace, pass flags, outputs) in a guard-page arena at its logical size
(tests/guarded_mem.py): a read or write outside one of them ends the process with SIGSEGV (return code -11).  The marker pass
reads an r-pixel halo and the growth a 1-pixel halo around every tile; the cases put tile edges on, one pixel inside and one
pixel past the frame, at the smallest and the largest radius.  Every result is held to the oracle.  The last line printed is a
JSON summary."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "medical-transformer_amd"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    import faulthandler
    faulthandler.enable()
    import guard_driver as D
    import guarded_mem as G
    import split_cases as SC
    import split_oracle as SO
    from medt_amd import _lib as L, ops
    from scipy import ndimage
    placement = sys.argv[1]
    lib = D.emu_lib()
    todo = [("1x1", np.ones((1, 1), np.uint8), 1, 1, 8), ("1x70 r32", np.ones((1, 70), np.uint8), 32, 1, 4),
            ("70x1 r32", np.ones((70, 1), np.uint8), 32, 0, 8), ("16x64", SC.random_discs(16, 64, 6, 2, 3, 6), 7, 1, 8),
            ("17x65", SC.random_discs(17, 65, 6, 1, 3, 6), 7, 1, 8), ("15x63 r32", SC.random_discs(15, 63, 6, 8, 3, 6), 32, 8, 4),
            ("33x129 r1", SC.random_discs(33, 129, 12, 7), 1, 0, 8), ("2 x 20x20 r32", np.stack([SC.discs(20, 20, (6, 6, 5), (13, 13, 5)),
                                                                                              np.ones((20, 20), np.uint8)]), 32, 1, 8),
            ("corridor", SC.serpentine(20, 70)[0], 2, 1, 4)]
    cases = 0
    with G.guarded_device(lib, placement, allow=D.ALLOW, announce=D.Run.announce) as (arena, proxy):
        for name, m, r, t, c in todo:
            proxy.end_case()
            proxy.case = name
            cases += 1
            print("CASE %s" % name, flush=True)
            # four images per call: the labelling's workspace (256 k + 4 bytes per image and chunk) is then a multiple of 16 bytes,
            # so that the "tail" placement hands out the 16-byte aligned pointer the call insists on
            m = np.concatenate([np.stack([i, i[::-1], i[:, ::-1], i[::-1, ::-1]]) for i in (m if m.ndim == 3 else m[None])])
            if m.shape[0] > 4:
                m = m[[0, 1, 4, 7]]
            imgs = m
            x = arena.copy_of(torch.from_numpy(m.copy()))
            mk = ops.split_markers(x, r, t, c).numpy().copy()
            lab, cnt = ops.split_objects(x, r, t, c)
            lab, cnt = lab.numpy().copy(), cnt.numpy().copy()
            want = [SO.split(i, r, t, c) for i in imgs]
            assert np.array_equal(mk, np.stack([SO.markers(i, r, t, c) for i in imgs]).reshape(m.shape)), name
            assert np.array_equal(lab, np.stack([w[0] for w in want]).reshape(m.shape)) and cnt.tolist() == [w[1] for w in want], name
            # one image alone (the labelling's workspace keeps single images out of the calls above in the "tail" placement):
            # the marker kernels through the C ABI on the oracle's component and depth maps, the growth through grow_labels below
            one = imgs[0]
            comp, k = ndimage.label(one, SO.structure(c))
            d2 = SO.depth2(one)
            h, w = one.shape
            t_d2, t_comp = arena.copy_of(torch.from_numpy(d2.astype(np.int32))), arena.copy_of(torch.from_numpy(comp.astype(np.int32)))
            t_cmax, t_mk = arena.tensor((1, k + 1), torch.int32), arena.tensor((h, w), torch.uint8)
            L.check(L.lib().medt_split_cmax(t_d2.data_ptr(), t_comp.data_ptr(), t_cmax.data_ptr(), 1, h, w, k + 1, k, 0), "medt_split_cmax")
            L.check(L.lib().medt_split_markers(t_d2.data_ptr(), t_comp.data_ptr(), t_cmax.data_ptr(), t_mk.data_ptr(), 1, h, w, k + 1, r, t, 0),
                    "medt_split_markers")
            assert np.array_equal(t_mk.numpy(), SO.markers(one, r, t, c)), name
            seeds = np.zeros(imgs[0].shape, np.int32)
            ys, xs = np.nonzero(imgs[0])
            seeds[ys[0], xs[0]], seeds[ys[-1], xs[-1]] = 2, 1
            got = ops.grow_labels(arena.copy_of(torch.from_numpy(seeds)), arena.copy_of(torch.from_numpy(imgs[0].copy())), c)
            assert np.array_equal(got.numpy(), SO.grow(seeds, imgs[0], c)[0]), name
    s = proxy.stats
    print(json.dumps({"cases": cases, "calls": s["calls"], "pointers": s["pointers"], "in_arena": s["in_arena"],
                      "stood_in": s["shadowed"], "unguarded": s["unguarded"], "allowed": s["allowed"],
                      "entries": s["entries"]}))


if __name__ == "__main__":
    main()
