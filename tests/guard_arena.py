"""A guard-band arena: every plane one call takes, in ONE allocation, each between two guard bands.

The suite's parity tests give every plane an allocation of its own, and an allocator pads those: a store one element
past a row tail, a tile's overhang row, a 16-byte store from a base that is only 4-byte aligned all land in padding
that nothing compares; a load past a plane reads junk that is selected away or multiplied by 0.  Here the planes sit
where a user's arena would put them, and the memory around each is known and looked at.

    arena = Arena("aligned" | "off4", "A" | "B", backend="numpy" | "device")
    arena.add("height", h, IN)                      # a numpy array: its bytes are the plane
    arena.add("out", (H, W), OUT, dtype=np.float32) # a shape: an output, prefilled with the guard pattern
    arena.build()
    before = arena.snapshot()
    call(arena.ptr("out"), arena.ptr("height"), ...)     # device: addresses; numpy: arena.view(name) is the plane
    after = arena.snapshot()
    arena.check(before, after)                      # GuardError: plane, side, byte offset of the first changed byte
    got = arena.read("out", after)

Layout, per plane and in the order of the add() calls:  [guard lo][plane][guard hi].
  guard size   at least the plane's own size and at least 4 KiB: an access within one plane-length of a plane stays
               inside the arena, so a slip is seen and does not fault
  aligned      the plane starts on a 256-byte boundary (what an allocator gives: the 16-byte kernel forms are chosen);
               guard hi begins at the very next byte after the plane's last element
  off4         the plane starts 4 bytes past a 16-byte boundary (8-byte elements and soil_rng records: 8 bytes past),
               so the scalar forms are chosen
  fills        float32 / float64 guards: A a quiet NaN with the payload 0x5EED in its low bits, B a large finite number;
               int32: two values valid for the plane's meaning, given by the caller (`fills=(a, b)`: an index inside
               the model, a mask value), so an out-of-bounds read used as an index cannot leave the arena;
               soil_rng records (16 bytes): two bit patterns
  outputs      prefilled with the guard pattern: a word the call never writes, or reads before writing, shows
  roles        IN (must be bit-unchanged afterwards), OUT, INOUT (holds data, may change), SCRATCH (contents
               unspecified afterwards; its guards must hold)

What this proves: that the call, at this shape and placement, stored nothing within one plane-length outside its
planes and left its inputs alone, and (run under both fills, results compared) that nothing it read from outside a
plane, or from an output before writing it, reached a result.  It does not see an access further away than the guard,
a load whose value is discarded under both fills, or anything in the library's internal workspace.
"""
import numpy as np

IN, OUT, INOUT, SCRATCH = "in", "out", "inout", "scratch"
PLACEMENTS = ("aligned", "off4")
FILLS = ("A", "B")
MIN_GUARD = 4096
RNG = np.dtype([("seed", "<u8"), ("offset", "<u8")])

F32_NAN = np.array([0x7FC05EED], np.uint32).view(np.float32)[0]
F64_NAN = np.array([0x7FF8000000005EED], np.uint64).view(np.float64)[0]
F32_BIG = np.float32(3.0e38)
F64_BIG = np.float64(1.0e300)


class GuardError(AssertionError):
    """A guard band or a pure input changed: `plane`, `side` ("lo", "hi" or "input"), `offset` (bytes; lo: before the
    plane's first byte, counted back from 1; hi: past its last byte, from 0; input: from the plane's first byte)."""

    def __init__(self, plane, side, offset, detail=""):
        self.plane, self.side, self.offset = plane, side, offset
        where = {"lo": "%d bytes before its first byte", "hi": "%d bytes past its last byte",
                 "input": "byte %d of the input plane itself"}[side] % offset
        AssertionError.__init__(self, "plane %r: %s changed%s" % (plane, where, detail))


def guard_value(dtype, fill, fills=None):
    """One element of the guard pattern of a plane of `dtype` under fill A or B."""
    dtype = np.dtype(dtype)
    k = FILLS.index(fill)
    if dtype == np.float32:
        return (F32_NAN, F32_BIG)[k]
    if dtype == np.float64:
        return (F64_NAN, F64_BIG)[k]
    if dtype == np.int32:
        if fills is None or len(fills) != 2 or fills[0] == fills[1]:
            raise ValueError("an int32 plane needs two different fill values that are valid for its meaning")
        return np.int32(fills[k])
    if dtype == RNG:
        return np.array([(0x0123456789ABCDEF, 0x5EED5EED5EED5EED), (0xFEDCBA9876543210, 0x0BAD0BAD0BAD0BAD)], RNG)[k]
    raise ValueError("no guard pattern for dtype %r" % dtype)


class _Plane:
    __slots__ = ("name", "role", "dtype", "shape", "data", "fills", "start", "nbytes", "lo", "hi")


class Arena:
    def __init__(self, placement, fill, backend="numpy"):
        if placement not in PLACEMENTS or fill not in FILLS or backend not in ("numpy", "device"):
            raise ValueError((placement, fill, backend))
        self.placement, self.fill, self.backend = placement, fill, backend
        self.planes, self._by_name = [], {}
        self.host = None        # the arena's bytes as built (numpy backend: the live arena)
        self._dev = None        # device backend: the silt tensor that owns the allocation
        self.base = 0           # device backend: the address of byte 0

    # ---- layout

    def add(self, name, data, role, dtype=None, fills=None):
        """A plane: `data` a numpy array (its dtype and bytes), or a shape with `dtype` (OUT and SCRATCH only)."""
        if self.host is not None or name in self._by_name or role not in (IN, OUT, INOUT, SCRATCH):
            raise ValueError("add(%r, role=%r)" % (name, role))
        p = _Plane()
        p.name, p.role, p.fills = name, role, fills
        if isinstance(data, np.ndarray):
            p.data, p.dtype, p.shape = np.ascontiguousarray(data), data.dtype, data.shape
        else:
            if role in (IN, INOUT) or dtype is None:
                raise ValueError("plane %r: an input needs its data, an output its dtype" % name)
            p.data, p.dtype, p.shape = None, np.dtype(dtype), tuple(int(d) for d in np.atleast_1d(data))
        guard_value(p.dtype, self.fill, fills)
        p.nbytes = int(np.prod(p.shape, dtype=np.int64)) * p.dtype.itemsize
        if p.nbytes == 0:
            raise ValueError("plane %r is empty" % name)
        self.planes.append(p)
        self._by_name[name] = p
        return self

    def _start(self, at, itemsize):
        """The first legal start of a plane at or after byte `at`."""
        if self.placement == "aligned":
            return -(-at // 256) * 256
        off = 4 if itemsize == 4 else 8
        return -(-(at - off) // 16) * 16 + off

    def build(self):
        at = 0
        for p in self.planes:
            g = max(p.nbytes, MIN_GUARD)
            g = -(-g // p.dtype.itemsize) * p.dtype.itemsize
            p.start = self._start(at + g, p.dtype.itemsize)
            p.lo = p.start - (p.start - at) // p.dtype.itemsize * p.dtype.itemsize    # whole elements, up to the plane
            p.hi = p.start + p.nbytes + g
            at = p.hi
        self.size = -(-at // 256) * 256
        self.host = np.zeros(self.size, np.uint8)
        for p in self.planes:
            pattern = guard_value(p.dtype, self.fill, p.fills)
            self.host[p.lo:p.hi].view(p.dtype)[:] = pattern
            if p.role in (IN, INOUT) or (p.role == SCRATCH and p.data is not None):
                self.host[p.start:p.start + p.nbytes] = p.data.reshape(-1).view(np.uint8)
        if self.backend == "device":
            from soillib_amd import silt
            self._dev = silt.tensor.from_numpy(self.host.view(np.float32)).gpu()
            self.base = self._dev.ptr
            assert self.base % 256 == 0, "the allocator's blocks start on 256 bytes"
        return self

    # ---- access

    def plane(self, name):
        return self._by_name[name]

    def ptr(self, name):
        """The plane's address (device backend), or None for a name that is None (an optional plane left out)."""
        if name is None:
            return None
        assert self.backend == "device"
        return self.base + self._by_name[name].start

    def view(self, name):
        """numpy backend: the plane itself, a writable view into the arena."""
        assert self.backend == "numpy"
        p = self._by_name[name]
        return self.host[p.start:p.start + p.nbytes].view(p.dtype).reshape(p.shape)

    def flat(self, name, before=0, after=0):
        """numpy backend: a 1-d element view that starts `before` elements ahead of the plane and ends `after`
        elements past it: what a stand-in for a faulty kernel writes or reads through."""
        assert self.backend == "numpy"
        p = self._by_name[name]
        s = p.dtype.itemsize
        return self.host[p.start - before * s:p.start + p.nbytes + after * s].view(p.dtype)

    def snapshot(self):
        """The whole arena's bytes, as a copy."""
        if self.backend == "numpy":
            return self.host.copy()
        return self._dev.cpu().numpy().view(np.uint8).copy()

    def read(self, name, snap):
        p = self._by_name[name]
        return snap[p.start:p.start + p.nbytes].view(p.dtype).reshape(p.shape).copy()

    # ---- the checker

    def check(self, before, after):
        """Every guard byte and every byte of a pure input is in `after` what it was in `before`; else GuardError
        for the first plane (in add() order) with a changed byte: its lo guard, then the plane, then its hi guard."""
        assert before.shape == after.shape == (self.size,)
        changed = before != after
        for p in self.planes:
            end = p.start + p.nbytes
            lo = np.flatnonzero(changed[p.lo:p.start])
            if lo.size:
                at = p.lo + int(lo[-1])                      # the changed byte nearest the plane
                raise GuardError(p.name, "lo", p.start - at, self._words(p, before, after, at))
            if p.role == IN:
                inside = np.flatnonzero(changed[p.start:end])
                if inside.size:
                    raise GuardError(p.name, "input", int(inside[0]), self._words(p, before, after, p.start + int(inside[0])))
            hi = np.flatnonzero(changed[end:p.hi])
            if hi.size:
                raise GuardError(p.name, "hi", int(hi[0]), self._words(p, before, after, end + int(hi[0])))
        # (bytes of the arena that belong to no plane's guards: the alignment gaps; nothing may touch them either)
        owned = np.zeros(self.size, bool)
        for p in self.planes:
            owned[p.lo:p.hi] = True
        stray = np.flatnonzero(changed & ~owned)
        if stray.size:
            near = min(self.planes, key=lambda q: abs(q.start - int(stray[0])))
            raise GuardError(near.name, "lo" if stray[0] < near.start else "hi",
                             abs(int(stray[0]) - (near.start if stray[0] < near.start else near.start + near.nbytes)))

    def _words(self, p, before, after, at):
        s = p.dtype.itemsize
        a = p.start + (at - p.start) // s * s
        if a < 0 or a + s > self.size or p.dtype == RNG:
            return ""
        return ": %r -> %r" % (before[a:a + s].view(p.dtype)[0], after[a:a + s].view(p.dtype)[0])


def bits_equal(a, b):
    """Whether two arrays of one dtype and shape hold the same bytes."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.reshape(-1).view(np.uint8) == b.reshape(-1).view(np.uint8)).all())


def assert_bits(got, want, what):
    """`got` is `want`, byte for byte (a NaN must be the same NaN)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    s = got.dtype.itemsize
    bad = (got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8)).reshape(-1, s).any(1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d elements differ, first at flat index %d: %r vs %r" % (
            what, int(bad.sum()), bad.size, i, got.reshape(-1)[i], want.reshape(-1)[i]))


# ---- one call of the library in an arena, on the device (tests/test_gpu_guard_bands*.py) ---------------------------

class Case:
    """One call under test.  `planes`: (name, role, data or shape, dtype, fills) in the order they lie in the arena;
    `call(lib, ptr)`: makes the call with ptr(name) (None for a None name) and checks its status itself;
    `want(lib, oracle)`: name -> the expected plane, or (plane, how) with how "bits" (the default: word for word),
    "naneq" (util.assert_bit_equal: word for word, a NaN for a NaN) or a function how(got, want, what) for planes
    that floating-point atomics accumulate (util.flux_close and its kin: no comparison between the fills then).  The
    name "*" stands for all planes at once: (expected, judge) with judge(planes as a dict, expected, what).  A
    function with the attribute `deterministic` set compares a plane that is one bit pattern all the same: the fills
    are compared."""

    def __init__(self, planes, call, want):
        self.planes, self.call, self.want = planes, call, want


def P(name, role, data, dtype=None, fills=None):
    return (name, role, data, dtype, fills)


def end_session_on_fault(e, what):
    """A HIP runtime call failed (SOIL_ERR_HIP, a device fault among them): the context is gone, and whatever ran
    after it on this device would only pile on: end the session here.  Every other status is a failure."""
    from soillib_amd import _abi
    if str(e).startswith("libsoil_hip error %d:" % _abi.SOIL_ERR_HIP):
        import pytest
        pytest.exit("%s: %s" % (what, e), returncode=3)


def judge_outputs(case, arena, after, want, what):
    """Every output plane of `want` read from the arena's bytes `after` and held to its reference, each the way its
    entry of `want` says (Case); returns name -> the plane as read.  Shared by run_case and tests/busy_stream.py."""
    from util import assert_bit_equal
    got = {}
    for name, exp in want.items():
        exp, how = exp if isinstance(exp, tuple) else (exp, "bits")
        if name == "*":
            how({n: arena.read(n, after) for n, *_ in case.planes}, exp, what)
            continue
        got[name] = arena.read(name, after)
        label = "%s: %s" % (what, name)
        if how == "bits":
            assert_bits(got[name], np.asarray(exp).reshape(got[name].shape), label)
        elif how == "naneq":
            assert_bit_equal(got[name], np.asarray(exp).reshape(got[name].shape), label)
        else:
            how(got[name], exp, label)
    return got


def run_case(lib, case, placement, want, what=""):
    """The four checks of a row at one placement, under both fills: the guards hold, the pure inputs are unchanged
    (Arena.check), every output is the reference's, and the outputs under fill A and fill B are the same bits."""
    from soillib_amd import _abi
    outs = {}
    for fill in FILLS:
        arena = Arena(placement, fill, "device")
        for name, role, data, dtype, fills in case.planes:
            arena.add(name, data, role, dtype=dtype, fills=fills)
        arena.build()
        before = arena.snapshot()
        assert bits_equal(before, arena.host), "the arena on the device is the arena as built"
        try:
            case.call(lib, arena.ptr)
            _abi.check(lib.soil_device_synchronize())
        except _abi.SoilError as e:
            end_session_on_fault(e, "%s %s fill %s" % (what, placement, fill))
            raise
        after = arena.snapshot()
        arena.check(before, after)
        outs[fill] = judge_outputs(case, arena, after, want, "%s %s fill %s" % (what, placement, fill))
    for name, exp in want.items():
        how = exp[1] if isinstance(exp, tuple) else "bits"
        if name != "*" and (not callable(how) or getattr(how, "deterministic", False)):
            assert_bits(outs["A"][name], outs["B"][name], "%s %s: %s under fill A against fill B" % (what, placement, name))
    return outs
