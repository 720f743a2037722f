"""The guard-band arena of tests/guard_arena.py on the host (no GPU): its layout rules, and its checker against
stand-in "ops" written in numpy, each with one of the faults the arena is there to catch.  This is the proof that the
GPU tests of tests/test_gpu_guard_bands.py would notice such a fault: they run the same class, with the same checker.

The op under test is out[x, y] = 2 * a[x, y] + b[x, y] on (H, W) float32 planes, with an int32 `graph` plane beside
them that it does not use.
"""
import numpy as np
import pytest

import guard_arena as ga
from guard_arena import IN, INOUT, OUT, SCRATCH, Arena, GuardError

SHAPES = [(5, 7), (65, 70), (33, 260), (1, 9), (9, 1)]


def _inputs(H, W):
    r = np.random.default_rng(H * 1000 + W)
    return r.random((H, W)).astype(np.float32), r.random((H, W)).astype(np.float32)


def make(placement, fill, H, W, extra=()):
    a, b = _inputs(H, W)
    arena = Arena(placement, fill)
    arena.add("a", a, IN).add("out", (H, W), OUT, dtype=np.float32).add("b", b, IN)
    arena.add("graph", np.arange(H * W, dtype=np.int32).reshape(H, W), IN, fills=(0, H * W - 1))
    for name, data, role, kw in extra:
        arena.add(name, data, role, **kw)
    return arena.build(), 2 * a + b


def good(arena):
    arena.view("out")[:] = 2 * arena.view("a") + arena.view("b")


def run(arena, op):
    before = arena.snapshot()
    op(arena)
    after = arena.snapshot()
    arena.check(before, after)
    return arena.read("out", after)


# ------------------------------------------------------------------ layout

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("placement", ga.PLACEMENTS)
def test_layout(placement, shape):
    H, W = shape
    r64 = np.arange(H * W, dtype=np.float64).reshape(H, W)
    rng = np.zeros(H * W, ga.RNG)
    arena, _ = make(placement, "A", H, W, extra=[("d", r64, INOUT, {}), ("rng", rng, INOUT, {}),
                                                 ("scratch", (3, H, W), SCRATCH, dict(dtype=np.float32))])
    end = 0
    for p in arena.planes:
        assert p.lo >= end, "the bands of two planes do not overlap"
        assert p.start - p.lo >= max(p.nbytes, 4096) and p.hi - (p.start + p.nbytes) >= max(p.nbytes, 4096)
        assert (p.start - p.lo) % p.dtype.itemsize == 0, "the guard's elements line up with the plane's"
        if placement == "aligned":
            assert p.start % 256 == 0
        else:
            assert p.start % 16 == (4 if p.dtype.itemsize == 4 else 8)
        end = p.hi
    assert end <= arena.size == arena.host.size
    # the guard begins at the very next byte, on both sides, and is the pattern throughout
    for p in arena.planes:
        want = ga.guard_value(p.dtype, "A", p.fills)
        lo = arena.host[p.lo:p.start].view(p.dtype)
        hi = arena.host[p.start + p.nbytes:p.hi].view(p.dtype)
        for band in (lo, hi):
            assert ga.bits_equal(band, np.full(band.shape, want, p.dtype))
    assert np.isnan(arena.flat("a", before=1)[0]) and np.isnan(arena.flat("a", after=1)[-1])
    assert arena.flat("graph", after=1)[-1] == 0 and arena.flat("d", before=1).view(np.uint64)[0] == 0x7FF8000000005EED


def test_fills():
    for fill, f32, f64, i32 in (("A", ga.F32_NAN, ga.F64_NAN, 3), ("B", ga.F32_BIG, ga.F64_BIG, 11)):
        assert ga.bits_equal(np.array(ga.guard_value(np.float32, fill)), np.array(f32))
        assert ga.bits_equal(np.array(ga.guard_value(np.float64, fill)), np.array(f64))
        assert ga.guard_value(np.int32, fill, (3, 11)) == i32
    assert np.isnan(ga.F32_NAN) and np.isnan(ga.F64_NAN) and np.isfinite(ga.F32_BIG) and np.isfinite(ga.F64_BIG)
    assert ga.F32_NAN.view(np.uint32) & 0x00400000, "a quiet NaN"
    a, b = ga.guard_value(ga.RNG, "A"), ga.guard_value(ga.RNG, "B")
    assert a.tobytes() != b.tobytes()
    for bad in (None, (1,), (4, 4)):
        with pytest.raises(ValueError):
            ga.guard_value(np.int32, "A", bad)
    with pytest.raises(ValueError):
        Arena("aligned", "A").add("g", np.zeros(4, np.int32), IN)          # an int plane without its two values
    with pytest.raises(ValueError):
        Arena("aligned", "A").add("x", (4,), IN, dtype=np.float32)         # an input without data


@pytest.mark.parametrize("fill", ga.FILLS)
def test_outputs_are_prefilled_and_inputs_hold_their_data(fill):
    arena, _ = make("off4", fill, 5, 7)
    a, b = _inputs(5, 7)
    assert ga.bits_equal(arena.view("a"), a) and ga.bits_equal(arena.view("b"), b)
    want = np.full((5, 7), ga.guard_value(np.float32, fill), np.float32)
    assert ga.bits_equal(arena.view("out"), want)


# ------------------------------------------------------------------ the checker

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("placement", ga.PLACEMENTS)
def test_a_correct_op_passes(placement, shape):
    outs = []
    for fill in ga.FILLS:
        arena, want = make(placement, fill, *shape)
        outs.append(run(arena, good))
        ga.assert_bits(outs[-1], want, "out")
    ga.assert_bits(outs[0], outs[1], "fill A against fill B")


def _caught(op, shape, plane, side, offset=None):
    for placement in ga.PLACEMENTS:
        for fill in ga.FILLS:
            arena, _ = make(placement, fill, *shape)
            with pytest.raises(GuardError) as e:
                run(arena, op)
            assert (e.value.plane, e.value.side) == (plane, side), str(e.value)
            if offset is not None:
                assert e.value.offset == offset, str(e.value)
            assert repr(plane) in str(e.value)


@pytest.mark.parametrize("shape", SHAPES)
def test_one_element_past_an_output(shape):
    def op(arena):
        good(arena)
        arena.flat("out", after=1)[-1] = 1.0
    _caught(op, shape, "out", "hi", 0)


@pytest.mark.parametrize("shape", SHAPES)
def test_one_element_before_an_output(shape):
    def op(arena):
        good(arena)
        arena.flat("out", before=1)[0] = 1.0
    _caught(op, shape, "out", "lo", 1)      # (the changed byte nearest the plane)


@pytest.mark.parametrize("shape", SHAPES)
def test_one_row_past_an_output(shape):
    W = shape[1]

    def op(arena):
        good(arena)
        arena.flat("out", after=W)[-W:] = 2 * arena.view("a")[-1] + arena.view("b")[-1]      # a tile's overhang row
    _caught(op, shape, "out", "hi", 0)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_store_that_happens_to_equal_the_guard_is_the_one_blind_spot(shape):
    """A stray store of the very guard pattern changes nothing; under the other fill it does."""
    def op(arena):
        good(arena)
        arena.flat("out", after=1)[-1] = ga.F32_BIG
    arena, _ = make("aligned", "B", *shape)
    run(arena, op)
    arena, _ = make("aligned", "A", *shape)
    with pytest.raises(GuardError):
        run(arena, op)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("placement", ga.PLACEMENTS)
def test_a_read_one_element_past_an_input(placement, shape):
    """The op's last cell reads a's next element, "selected away" by a multiplication by 0: no guard changes, the
    result under fill A (NaN * 0) is not the result under fill B (big * 0), and under A it is not the reference."""
    def op(arena):
        good(arena)
        arena.view("out").reshape(-1)[-1] += arena.flat("a", after=1)[-1] * np.float32(0)
    outs = []
    for fill in ga.FILLS:
        arena, want = make(placement, fill, *shape)
        outs.append(run(arena, op))
    ga.assert_bits(outs[1], want, "under the finite fill the slip is invisible")
    with pytest.raises(AssertionError):
        ga.assert_bits(outs[0], outs[1], "fill A against fill B")
    with pytest.raises(AssertionError):
        ga.assert_bits(outs[0], want, "out")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("placement", ga.PLACEMENTS)
def test_an_op_that_adds_into_an_uninitialised_output(placement, shape):
    def op(arena):
        arena.view("out")[:] += 2 * arena.view("a") + arena.view("b")
    outs = []
    for fill in ga.FILLS:
        arena, want = make(placement, fill, *shape)
        outs.append(run(arena, op))
        with pytest.raises(AssertionError):
            ga.assert_bits(outs[-1], want, "out")
    with pytest.raises(AssertionError):
        ga.assert_bits(outs[0], outs[1], "fill A against fill B")


@pytest.mark.parametrize("shape", SHAPES)
def test_an_op_that_modifies_an_input(shape):
    def op(arena):
        good(arena)
        arena.view("b").reshape(-1)[-1] = 0.0
    _caught(op, shape, "b", "input", 4 * (shape[0] * shape[1] - 1))

    def int_op(arena):
        good(arena)
        arena.view("graph")[0, 0] = 1
    _caught(int_op, shape, "graph", "input", 0)


def test_inout_and_scratch_planes_may_change_but_their_guards_may_not():
    H, W = 5, 7
    extra = [("state", np.ones((H, W), np.float32), INOUT, {}), ("scratch", (2, H, W), SCRATCH, dict(dtype=np.float32))]

    def op(arena):
        good(arena)
        arena.view("state")[:] += 1
        arena.view("scratch")[:] = 7

    arena, _ = make("off4", "A", H, W, extra)
    run(arena, op)
    assert (arena.view("state") == 2).all()

    def slip(arena):
        op(arena)
        arena.flat("scratch", after=1)[-1] = 7
    arena, _ = make("off4", "A", H, W, extra)
    with pytest.raises(GuardError) as e:
        run(arena, slip)
    assert (e.value.plane, e.value.side, e.value.offset) == ("scratch", "hi", 0)


def test_the_first_fault_in_plane_order_is_the_one_named():
    def op(arena):
        good(arena)
        arena.flat("b", after=1)[-1] = 1.0
        arena.flat("a", before=2)[0] = 1.0
    _caught(op, (5, 7), "a", "lo", 5)
