"""TEST INFRASTRUCTURE: guard-paged host memory for the kernels on the CPU lane emulator (tests/lane_emu, tests/emu_device.py).

The emulator executes the kernel sources on host memory, so the MMU can check what no value comparison sees: a global load or
store one element outside a buffer the C ABI was handed.  Three pieces:

  * Arena: every allocation is an anonymous mmap of ceil(nbytes / page) + 2 pages whose first and last page are PROT_NONE.
    Placement "tail" ends the buffer on the last byte before the trailing guard page (overruns fault; the start is only as
    aligned as nbytes allows), placement "head" starts it on the first byte behind the leading guard page (underruns fault; the
    start is page aligned, so the 16-byte vector paths are taken).  No slack, no padding: the buffer has its logical size.
    Both placements give 16-byte-aligned pointers to every tensor whose byte count is a multiple of 16 -- which is every tensor
    the kernels' alignment guards look at when their shape condition (HW % 4 == 0, W even) holds: exact guarding cannot put a
    misaligned pointer in front of those guards.  Placement "offset" is the separate tool for that: the buffer ends FOUR bytes
    before the trailing guard page, so a tensor of 16k bytes starts at 12 (mod 16).  The four bytes are a canary (checked by
    check_canaries()): a write of one element past the end is seen, a read of it is not, two elements past fault.
  * guarded_torch(): a stand-in for the `torch` name of the medt_amd modules whose allocation functions hand out arena tensors.
  * GuardProxy: wraps the ctypes library, walks every pointer of every medt_* call (c_void_p arguments and, recursively, the
    pointer fields of the structures of medt_amd/_lib.py) and requires each to lie inside exactly one arena buffer.  A tensor
    that a torch operation made (clone, contiguous of a view, autograd's gradient) is copied into an arena buffer of exactly the
    tensor's size, the pointer is redirected there, and what the kernels wrote is copied back -- at the end of the call and, for
    recorded jobs, after every queue flush.  Anything else is an unguarded pointer: an AssertionError unless allow-listed.

A kernel that leaves its buffer ends the process with SIGSEGV, so cases run in child processes (tests/guard_driver.py)."""
import bisect
import contextlib
import ctypes as C
import mmap
import types

import numpy as np
import torch

PAGE = mmap.PAGESIZE
PLACEMENTS = ("tail", "head")                     # exact on one side each; "offset": see the module docstring
CANARY = 0xA5
PROT_NONE = 0
_libc = C.CDLL(None, use_errno=True)
_libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
_libc.mprotect.restype = C.c_int
_NP = {torch.float32: np.float32, torch.float64: np.float64, torch.float16: np.float16, torch.int32: np.int32,
       torch.int64: np.int64, torch.uint8: np.uint8, torch.int8: np.int8, torch.int16: np.int16, torch.bool: np.bool_}


def _perms_at(maps, addr):
    """Permissions of the region of /proc/self/maps that holds addr (slow: parses every line)."""
    for ln in maps.splitlines():
        if ln:
            rng, perms = ln.split(" ", 2)[:2]
            lo, hi = rng.split("-")
            if int(lo, 16) <= addr < int(hi, 16):
                return perms
    return None


def _guards_armed(base, npages):
    """True if /proc/self/maps shows no permissions for the page in front of and the page behind the npages data pages at
    base + PAGE.  Read only: nothing is made to fault.  Guard pages of neighbouring allocations may merge into one region, so
    each is found by the boundary it shares with the buffer's own read-write pages: the END of the leading guard's region and
    the START of the trailing guard's region."""
    with open("/proc/self/maps") as f:
        maps = "\n" + f.read()
    if npages == 0:                                          # two adjacent guard pages and nothing between them
        return _perms_at(maps, base) == "---p" and _perms_at(maps, base + PAGE) == "---p"
    lead = maps.find("-%08x " % (base + PAGE))
    trail = maps.find("\n%08x-" % (base + (npages + 1) * PAGE))
    return lead >= 0 and trail >= 0 and maps[lead:].split(" ", 2)[1] == "---p" and maps[trail:].split(" ", 2)[1] == "---p"


class Arena:
    def __init__(self, placement="tail", check_maps=True):
        assert placement in PLACEMENTS + ("offset",), placement
        self._canaries = []                # addresses of the 4 canary bytes behind every buffer of the "offset" placement
        self.placement, self.check_maps = placement, check_maps
        self._maps = []                    # the mappings: kept until release() (recorded jobs keep pointers until the flush)
        self._starts, self._sizes = [], []  # registry of live (start, nbytes), sorted by start
        self.allocations = self.bytes = 0

    # ---- raw allocation ------------------------------------------------------------------------------------------------
    def _map(self, nbytes):
        pad = 4 if self.placement == "offset" and nbytes else 0
        npages = -(-(nbytes + pad) // PAGE)
        m = mmap.mmap(-1, (npages + 2) * PAGE, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, prot=mmap.PROT_READ | mmap.PROT_WRITE)
        base = C.addressof(C.c_char.from_buffer(m))
        assert base % PAGE == 0
        trail = base + (npages + 1) * PAGE
        for g in (base, trail):
            if _libc.mprotect(g, PAGE, PROT_NONE) != 0:
                raise OSError(C.get_errno(), "mprotect")
        off = PAGE if self.placement == "head" else PAGE + npages * PAGE - nbytes - pad
        if pad:
            C.memset(base + off + nbytes, CANARY, pad)
            self._canaries.append(base + off + nbytes)
        self._maps.append(m)
        self.allocations += 1
        self.bytes += nbytes
        if self.check_maps:                                  # armed?  (read only; nothing is ever made to fault here)
            assert self.guards_armed(base, npages), "guard pages of 0x%x are not PROT_NONE" % base
        if nbytes:
            i = bisect.bisect_left(self._starts, base + off)
            self._starts.insert(i, base + off)
            self._sizes.insert(i, nbytes)
        return m, base, off, npages

    guards_armed = staticmethod(_guards_armed)

    def numpy(self, shape, dtype, fill="uninit"):
        """An arena array; fill 'uninit' (quiet NaNs for float types, 0x7f bytes for the others) or 'zeros'."""
        dtype = np.dtype(dtype)
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        m, base, off, _ = self._map(nbytes)
        a = np.frombuffer(m, dtype=np.uint8, count=nbytes, offset=off)
        if fill == "uninit" and nbytes:
            if dtype.kind == "f":
                a.view(dtype)[:] = np.nan
            else:
                a[:] = 0x7F
        return a.view(dtype).reshape(shape) if nbytes else np.zeros(shape, dtype)

    def tensor(self, shape, dtype=torch.float32, fill="uninit"):
        """An arena tensor (torch CPU, no copy: it aliases the mapping).  Zero elements: a valid empty tensor."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        item = torch.empty((), dtype=dtype).element_size()
        if n == 0:
            self._map(0)
            return torch.empty(shape, dtype=dtype)
        if dtype in _NP:
            return torch.from_numpy(self.numpy(shape, _NP[dtype], fill))
        raw = torch.from_numpy(self.numpy((n * item,), np.uint8, "zeros"))         # bfloat16: numpy has no such type
        t = raw.view(dtype).reshape(shape)
        if fill == "uninit":
            t.fill_(float("nan")) if dtype.is_floating_point else raw.fill_(0x7F)
        return t

    def copy_of(self, t):
        """An arena tensor with the shape, type and values of t (dense); requires_grad is not carried over."""
        out = self.tensor(t.shape, t.dtype, "zeros")
        with torch.no_grad():
            out.copy_(t.detach())
        return out

    # ---- registry ----------------------------------------------------------------------------------------------------------
    def owner(self, addr, nbytes=1):
        """(start, size) of the one registered buffer that holds [addr, addr + nbytes) entirely, else None."""
        i = bisect.bisect_right(self._starts, addr) - 1
        if i >= 0 and addr + nbytes <= self._starts[i] + self._sizes[i]:
            return self._starts[i], self._sizes[i]
        return None

    def check_canaries(self):
        """Placement "offset": the four bytes between every buffer and its trailing guard page are untouched."""
        want = bytes([CANARY]) * 4
        bad = [a for a in self._canaries if C.string_at(a, 4) != want]
        assert not bad, "written one element past the end of the buffer(s) ending at %s" % ", ".join("0x%x" % a for a in bad)
        return len(self._canaries)

    def release(self):
        """Forget every buffer (the mappings go when the last tensor / array on them goes)."""
        self._starts, self._sizes, self._canaries = [], [], []
        for m in self._maps:
            try:
                m.close()
            except BufferError:
                pass
        self._maps = []


# ------------------------------------------------------------------------------------------------------------------------ #
def _size(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = args[0]
    return tuple(int(s) for s in args)


def guarded_torch(arena):
    """The `torch` name for the medt_amd modules: everything of torch, with the allocation functions the modules call
    (empty, zeros, ones, full, empty_like, zeros_like, ones_like, tensor) handing out arena tensors."""
    ns = types.SimpleNamespace(**{k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})

    def make(fill, value=None):
        def alloc(*size, dtype=None, device=None, requires_grad=False):
            t = arena.tensor(_size(size), dtype or torch.float32, fill)
            if value is not None:
                t.fill_(value)
            return t.requires_grad_(requires_grad)
        return alloc

    def make_like(fill, value=None):
        def alloc(t, dtype=None, device=None, requires_grad=False):
            out = arena.tensor(tuple(t.shape), dtype or t.dtype, fill)
            if value is not None:
                out.fill_(value)
            return out.requires_grad_(requires_grad)
        return alloc

    ns.empty, ns.zeros, ns.ones = make("uninit"), make("zeros"), make("zeros", 1)
    ns.empty_like, ns.zeros_like, ns.ones_like = make_like("uninit"), make_like("zeros"), make_like("zeros", 1)
    ns.full = lambda size, fill_value, dtype=None, device=None, requires_grad=False: \
        make("zeros", fill_value)(size, dtype=dtype or torch.tensor(fill_value).dtype, requires_grad=requires_grad)
    ns.tensor = lambda data, dtype=None, device=None, requires_grad=False: \
        arena.copy_of(torch.tensor(data, dtype=dtype)).requires_grad_(requires_grad)
    return ns


# ------------------------------------------------------------------------------------------------------------------------ #
class UnguardedPointer(AssertionError):
    pass


def _bytes(t):
    return t.detach().reshape(-1).view(torch.uint8)


class _Shadow:
    """A tensor torch made, standing in the arena at its exact size for as long as the case runs."""

    def __init__(self, arena, t):
        self.orig = t
        self.copy = arena.copy_of(t)
        self.snap = _bytes(self.copy).clone()

    def refresh(self):                                       # the original changed behind our back (a torch op wrote it)
        ob = _bytes(self.orig)
        if not torch.equal(ob, self.snap):
            _bytes(self.copy).copy_(ob)
            self.snap.copy_(ob)

    def sync(self):                                          # the kernels wrote the copy: hand the result to the original
        cb = _bytes(self.copy)
        if not torch.equal(cb, self.snap):
            self.orig.data.reshape(-1).view(torch.uint8).copy_(cb)
            self.snap.copy_(cb)


class GuardProxy:
    """Forwards every attribute to the ctypes library; medt_* calls are announced, their pointers checked / redirected."""

    def __init__(self, lib, arena, allow=(), announce=None):
        from medt_amd import _lib as L
        self._lib, self._arena, self._L = lib, arena, L
        self._allow = set(allow)
        self._announce = announce
        self._seen = {}                    # data_ptr -> the dense torch tensor it was last asked of (see guarded_device)
        self._shadows = {}                 # (data_ptr, nbytes) -> _Shadow
        self.case = ""
        self.stats = {"calls": 0, "pointers": 0, "in_arena": 0, "shadowed": 0, "allowed": 0, "unguarded": 0,
                      "misaligned_calls": {}, "misaligned_pointers": {}, "entries": {}}
        self._wrappers = {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        fn = getattr(self._lib, name)
        if name not in self._L.SIGNATURES:
            return fn
        if name not in self._wrappers:
            self._wrappers[name] = self._wrap(name, fn)
        return self._wrappers[name]

    # which c_void_p arguments are no device buffers (include/medt_abi.h): every entry point's last argument is the stream, and
    # the medt_queue_* functions take only queue handles (host objects of the library) and streams
    # (tests/test_guarded_memory.py::test_handle_convention_matches_the_header holds the header to this)
    def _is_handle(self, name, i, nargs):
        return name.startswith("medt_queue_") or i == nargs - 1

    def _wrap(self, name, fn):
        argtypes = self._L.SIGNATURES[name][1]

        def call(*args):
            if self._announce:
                self._announce(name, self.case)
            st = self.stats
            st["calls"] += 1
            st["entries"][name] = st["entries"].get(name, 0) + 1
            args = list(args)
            used, restore, misaligned = [], [], [False]

            def visit(ptr, path, put):
                if not ptr:
                    return
                st["pointers"] += 1
                final = ptr
                if self._arena.owner(ptr) is not None:
                    st["in_arena"] += 1
                else:
                    t = self._seen.get(ptr)
                    if t is not None:
                        key = (ptr, t.numel() * t.element_size())
                        sh = self._shadows.get(key)
                        if sh is None:
                            sh = self._shadows[key] = _Shadow(self._arena, t)
                        else:
                            sh.orig = t
                            sh.refresh()
                        used.append(sh)
                        final = _raw_ptr(sh.copy)
                        put(final)
                        st["shadowed"] += 1
                    elif (name, path) in self._allow:
                        st["allowed"] += 1
                    else:
                        st["unguarded"] += 1
                        raise UnguardedPointer("%s: %s = 0x%x lies in no arena buffer and is no tensor torch handed out (case %s)"
                                               % (name, path, ptr, self.case))
                if final % 16:
                    misaligned[0] = True
                    key = name + ":" + path                 # which pointer: the kernels' alignment guards look at a few only
                    st["misaligned_pointers"][key] = st["misaligned_pointers"].get(key, 0) + 1

            def walk(obj, path):
                for fname, ftype in obj._fields_:
                    if ftype is C.c_void_p:
                        old = getattr(obj, fname)

                        def put(v, obj=obj, fname=fname, old=old):
                            restore.append((obj, fname, old))
                            setattr(obj, fname, v)
                        visit(old, path + "." + fname, put)
                    elif isinstance(ftype, type) and issubclass(ftype, C.Structure):
                        walk(getattr(obj, fname), path + "." + fname)

            for i, (a, at) in enumerate(zip(args, argtypes)):
                if a is None:
                    continue
                if at is C.c_void_p:
                    if self._is_handle(name, i, len(argtypes)):
                        continue
                    v = a.value if isinstance(a, C.c_void_p) else int(a)

                    def put(v, i=i):
                        args[i] = v
                    visit(v, "arg%d" % i, put)
                elif isinstance(at, type) and issubclass(at, C._Pointer):
                    obj = a._obj if hasattr(a, "_obj") else a.contents
                    walk(obj, "arg%d" % i)
            if misaligned[0]:
                st["misaligned_calls"][name] = st["misaligned_calls"].get(name, 0) + 1
            try:
                rc = fn(*args)
            finally:
                for obj, fname, old in restore:
                    setattr(obj, fname, old)
            for sh in used:
                sh.sync()
            if name.startswith("medt_queue_flush"):                 # the recorded jobs ran now: everything they may have written
                for sh in self._shadows.values():
                    sh.sync()
            return rc
        return call

    def end_case(self):
        for sh in self._shadows.values():
            sh.sync()
        self._shadows.clear()
        self._seen.clear()


_RAW_DATA_PTR = torch.Tensor.data_ptr


def _raw_ptr(t):
    return _RAW_DATA_PTR(t)


@contextlib.contextmanager
def guarded_device(lib, placement, allow=(), announce=None):
    """tests/emu_device.py::emulated_device with every buffer that reaches the C ABI in a guard-page arena.  Yields
    (arena, proxy); hand `proxy` to whatever expects the emulator library."""
    from emu_device import emulated_device
    from medt_amd import axial, block, defer, net, ops, optim, trainer, window
    arena = Arena(placement)
    proxy = GuardProxy(lib, arena, allow, announce)
    ns = guarded_torch(arena)
    mods = (axial, block, defer, net, ops, optim, trainer, window)
    saved = [(m, m.torch) for m in mods]

    def data_ptr(self):
        # every pointer the product passes comes from Tensor.data_ptr() of the tensor it passes: remember which tensor an
        # address outside the arena belongs to, so that the proxy knows its exact size
        p = _RAW_DATA_PTR(self)
        if p and self.is_contiguous() and arena.owner(p) is None:
            proxy._seen[p] = self
        return p

    with emulated_device(proxy):
        try:
            for m in mods:
                m.torch = ns
            torch.Tensor.data_ptr = data_ptr
            yield arena, proxy
        finally:
            del torch.Tensor.data_ptr
            for m, t in saved:
                m.torch = t
            proxy.end_case()
