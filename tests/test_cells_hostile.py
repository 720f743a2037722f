"""The hostile inputs of the cell phase (util.hostile_cell_inputs, util.hostile_colour_inputs) and the oracle they are
compared against, without a GPU.

tests/test_gpu_cells_hostile.py compares the fused cell kernel with the oracle bit for bit on these planes.  That
comparison says something only while the planes reach the branches they were built for and most of what comes out is
a number, so both are asserted here, on the oracle's result, for every launch shape and every parameter set:

  * each launch shape is in the class it stands for (vector / scalar kernel, XCD remap, idle lanes);
  * on grids of at least 256 cells every branch of the cell phase is taken by a cell whose outputs are all finite:
    both clamps of `transfer`, a loss from the sediment alone, a loss that reaches the bedrock, the three colour
    branches, the creep tie (with equal and with different sediment);
  * at least four cells in five of every output plane are finite, on every grid;
  * the items of the builder's docstring are in the planes.

And the oracle's cell phase itself on cells whose answer can be written down by hand, with the rule its minimum and
maximum follow (soil_oracle.c: orc_fmaxf): the device rule of the reference, not the host libm's, which returns
-0 for fmaxf(+0, -0).  That order reaches one output bit: on a cell without a downhill neighbour (a pit, a plateau)
that nothing visited soil_mass_transfer adds fmaxf(0, -0 / scale.z) to delta.y, and a delta.y of -0 on entry stays -0
under the libm's order and becomes +0 under the device's.  (The fused step starts from delta = +0 and adds the creep
term afterwards: no bit of it moves.)
"""
import numpy as np
import pytest

from util import (_Placer, CELL_FLUX, CELL_OUT, COLOUR_OUT, DENORMAL, HOSTILE_SHAPES, assert_bit_equal, bits, cell_branches,
                  cell_param_sets, hostile_cell_inputs, hostile_colour_inputs, oracle_cells, oracle_colour_cells)

kBlock, kVec = 256, 4          # csrc/erosion_cells.hip

# shape -> (vector path, XCD remap, blocks, threads of the last block, live lanes of the last wave)
SHAPE_CLASS = {
    (12, 40): (True, False, 1, 120, 56),        # rows shorter than a wave
    (8, 256): (True, False, 2, 256, 64),        # a row is a wave
    (9, 260): (True, False, 3, 73, 9),          # rows of more than one wave, not a multiple of it
    (5, 1028): (True, False, 6, 5, 5),
    (256, 256): (True, True, 64, 256, 64),      # remap, blocks exactly full
    (252, 260): (True, True, 64, 252, 60),      # remap, idle lanes in the last block
    (283, 260): (True, True, 72, 219, 27),      # remap with 72 blocks
    (247, 260): (True, False, 63, 183, 55),     # 63 blocks: no remap
    (37, 53): (False, False, 8, 169, 41),       # the scalar kernel: one thread per cell
    (3, 7): (False, False, 1, 21, 21),
    (5, 1): (False, False, 1, 5, 5),
    (1, 1): (False, False, 1, 1, 1),
}


def launch_class(rows, W):
    """What erode_cells_fused launches for `rows` rows of width W (aligned planes)."""
    vec = W % kVec == 0
    total = rows * W // kVec if vec else rows * W
    nblk = -(-total // kBlock)
    remap = vec and nblk % 8 == 0 and nblk >= 64
    last = total - (nblk - 1) * kBlock
    return vec, remap, nblk, last, (last - 1) % 64 + 1


def test_every_shape_is_in_its_class():
    assert set(HOSTILE_SHAPES) == set(SHAPE_CLASS)
    for shape in HOSTILE_SHAPES:
        assert launch_class(*shape) == SHAPE_CLASS[shape], shape
    # the row ranges of the GPU tests: (1, H - 1) of (252, 260) stays in the remap class, with idle lanes
    assert launch_class(250, 260)[:3] == (True, True, 64) and launch_class(250, 260)[3] < kBlock
    # variants 1 and 3 (512 and 128 threads) want total % 512 == 0 and total % 128 == 0 and eight blocks in each XCD
    total = lambda H, W: H * W // kVec
    assert total(256, 256) % 512 == 0 and (total(256, 256) // 512) % 8 == 0
    assert total(252, 260) % 512 != 0 and total(252, 260) % 128 != 0


def _case(oracle, H, W):
    inp = hostile_cell_inputs(oracle, H, W, seed=H * 1000 + W)
    col = hostile_colour_inputs(inp, seed=H * 1000 + W)
    return inp, col


@pytest.mark.parametrize("H,W", HOSTILE_SHAPES)
def test_the_hostile_planes_reach_every_branch_and_stay_mostly_finite(oracle, H, W):
    inp, col = _case(oracle, H, W)
    n = H * W
    for name, op, scale in cell_param_sets(oracle, H, W):
        want = oracle_cells(oracle, inp, scale, op)
        want_col = oracle_colour_cells(oracle, inp, col, scale, op)
        for k in CELL_OUT:                      # the physics planes do not depend on the colour planes
            assert_bit_equal(want[k], want_col[k], "%s: %s with and without colour" % (name, k))
        for k in CELL_OUT:
            assert np.isfinite(want[k]).mean() >= 0.8, (name, k, np.isfinite(want[k]).mean())
        for k in COLOUR_OUT:
            assert np.isfinite(want_col[k]).mean() >= 0.8, (name, k)
        if n < 256:
            continue
        b = cell_branches(inp, want, scale, op)
        for branch in ("lower_clamp", "upper_clamp", "sediment_only", "reaches_bedrock", "creep_tie", "creep_tie_split"):
            assert (b[branch] & b["finite"]).any(), "%s: no finite cell takes %s" % (name, branch)
        b = cell_branches(inp, want_col, scale, op, col, want_col)
        for branch in ("colour_bedrock", "colour_mix", "colour_source_fluvial", "colour_source_debris"):
            assert (b[branch] & b["finite"]).any(), "%s: no finite cell takes %s" % (name, branch)
        # the census is no tautology: the oracle's planes show the branches where they can be read off a plane
        surf = want_col["albedoSurface"]
        took_bedrock = b["colour_bedrock"] & b["finite"]
        assert_bit_equal(surf[took_bedrock], col["albedoBedrock"][took_bedrock], name + ": the bedrock colour")
        src = b["colour_source_fluvial"] & b["finite"]
        assert_bit_equal(want_col["albedoFluvial"][src], col["albedoSurface"][src], name + ": the source colour")
        sz = np.float32(scale[2])
        cap = np.float32(0.25) * np.sqrt(np.float32(scale[0]) * np.float32(scale[0]) +
                                         np.float32(scale[1]) * np.float32(scale[1])) * np.float32(0.3)
        d = np.zeros((H, W, 2), np.float32)
        with np.errstate(all="ignore"):
            oracle.mass_transfer(d, inp["layers"], np.zeros((H, W), np.float32), want["mass"], want["velocity"],
                                 want["debris"], None, None, None, None, scale, op)
        up = b["upper_clamp"] & b["finite"]
        assert_bit_equal(d[up][:, 1], np.full(int(up.sum()), cap / sz, np.float32), name + ": the upper clamp's gain")
        only = b["sediment_only"] & b["finite"]
        assert (d[only][:, 0] == 0).all() and (d[only][:, 1] < 0).all(), name + ": a loss from the sediment alone"
        rock = b["reaches_bedrock"] & b["finite"]
        assert (d[rock][:, 0] < 0).all(), name + ": a loss that reaches the bedrock"
        assert np.allclose(d[rock][:, 1], -inp["layers"][rock][:, 1], rtol=1e-6, atol=0), name + ": ... and takes all the sediment"


@pytest.mark.parametrize("H,W", HOSTILE_SHAPES)
def test_the_hostile_planes_hold_their_items(oracle, H, W):
    inp, col = _case(oracle, H, W)
    again, col_again = _case(oracle, H, W)
    for k in inp:
        assert_bit_equal(inp[k], again[k], k + " is deterministic")
    for k in col:
        assert_bit_equal(col[k], col_again[k], k + " is deterministic")
    n, L = H * W, inp["layers"]
    neg0 = lambda a: (bits(a) == 0x80000000).any()
    denormal = lambda a: ((np.abs(a) > 0) & (np.abs(a) < np.float32(1.1754944e-38))).any()
    if n >= 64:
        for k in CELL_FLUX:
            assert (inp[k] == 0).mean() >= 0.3, k
            assert (inp[k][H - 1] == 0).all(), k + ": the all-zero row"
    if n >= 5:
        for k in CELL_FLUX:
            assert np.isnan(inp[k][0, 0]).all(), k + ": NaN in cell (0, 0)"
    if not _Placer(H, W).roomy():
        assert (H, W) in ((12, 40), (3, 7), (5, 1), (1, 1))
        return
    for k in ("layers", "waterFlux", "massFlux", "velocityFlux", "debrisFlux"):
        assert neg0(inp[k]), k + ": a -0"
    for k in ("layers", "waterFlux", "massFlux", "velocityFlux", "debrisFlux"):
        assert denormal(inp[k]), k + ": a denormal"
    assert (L == np.float32(3e38)).any() and (L == np.float32(-3e38)).any()
    assert (L[..., 1] == 0).sum() >= 16 and (L[..., 1] < 0).any()
    assert np.isposinf(inp["waterFlux"]).any() and np.isposinf(inp["debrisVelocityFlux"]).any()
    assert (inp["velocityFlux"] == np.float32(1e20)).any() and (inp["velocityFlux"] == np.float32(1e-30)).any()
    assert (inp["massFlux"] < 0).any() and (inp["debrisFlux"] < 0).any()
    for k in ("uplift", "rainfall"):
        assert (inp[k] == 0).any() and (inp[k] < 0).any() and np.isnan(inp[k]).sum() == 1, k
    # +inf, -inf and NaN: interior, the four edges, a corner, both sides of a group boundary
    for test in (np.isposinf, np.isneginf, np.isnan):
        bad = test(L).any(-1)
        assert bad[1:-1, 1:-1].any() and bad[0, 1:-1].any() and bad[-1, 1:-1].any(), test.__name__
        if H >= 8:
            assert bad[1:-1, 0].any() and bad[1:-1, -1].any(), test.__name__
        assert bad[0, 0] or bad[0, -1] or bad[-1, 0] or bad[-1, -1], test.__name__
        assert (bad[:, 3:-1:4] & bad[:, 4::4][:, :bad[:, 3:-1:4].shape[1]]).any(), test.__name__ + " across a group boundary"
    # plateaus: across a group boundary, across the wave boundary at 255 | 256, across a row's end
    h = L[..., 0] + L[..., 1]
    with np.errstate(all="ignore"):
        same = np.isfinite(h[:, :-1]) & (h[:, :-1] == h[:, 1:])
    assert same[:, 3::4].any(), "no plateau across a group boundary"
    if W > 256:
        assert same[:, 255].any(), "no plateau across columns 255 | 256"
    assert (np.isfinite(h[:-1, -1]) & (h[:-1, -1] == h[1:, 0])).any(), "no plateau across a row's end"
    # colour
    for k in col:
        assert np.isnan(col[k]).any() or np.isinf(col[k]).any(), k
    assert neg0(col["albedoSurface"]) and (col["albedoSurface"] > 1).any() and (col["albedoSurface"] < 0).any()
    for flux, a in (("massFlux", "albedoFluvial"), ("debrisFlux", "albedoDebris")):
        norm = np.abs(col[a]).sum(-1)
        assert ((inp[flux] <= 0) & (norm > 0)).any() and ((inp[flux] > 0) & (norm == 0)).any(), a
        assert (np.abs(col[a]) == np.float32(2e19)).any(), a
    assert (col["albedoFluvial"] == np.float32(3e-23)).any()
    # the gate `sqrtf(a . a) > 0` decides on its own: 3e-23 squared is the least denormal, 2e-23 squared is 0
    assert np.float32(3e-23) * np.float32(3e-23) == np.float32(1e-45) and np.float32(2e-23) * np.float32(2e-23) == 0
    assert (col["albedoDebris"] == np.float32(2e-23)).any()


# ---------------------------------------------------------------- the oracle's cell phase by hand

def _quiet_param(oracle):
    """A parameter set in powers of two under which every term of `transfer` but the one under test is an exact 0."""
    op = oracle.default_param()
    op.timeStep, op.gravity, op.uplift, op.rainfall = 1.0, 1.0, 0.0, 0.0
    op.suspensionRateFluvial = op.depositionRateFluvial = 0.0
    op.suspensionRateDebris = op.depositionRateDebris = op.landslideRateDebris = 0.0
    op.critSlopeBedrock, op.critSlopeSediment, op.yieldStress, op.exitSlope = 1.0, 0.5, 0.0, 0.03125
    op.force[0] = op.force[1] = 0.0
    return op


ONE = (1.0, 1.0, 1.0)


def _transfer(oracle, layers, op, mass=0.0, debris=0.0, delta=0.0):
    H, W = layers.shape[:2]
    f = lambda v, *c: np.full((H, W) + c, v, np.float32)
    d = f(delta, 2)
    oracle.mass_transfer(d, layers, f(0.0), f(mass), f(0.0, 2), f(debris), None, None, None, None, ONE, op)
    return d


def test_a_flat_plateau_does_not_creep(oracle):
    op = _quiet_param(oracle)
    flat = np.full((5, 6, 2), 0.25, np.float32)
    split = flat.copy()                           # equal totals, split differently between bedrock and sediment
    split[..., 1] = np.linspace(0.0, 0.4375, 30, dtype=np.float32).reshape(5, 6) // np.float32(0.0625) * np.float32(0.0625)
    split[..., 0] = np.float32(0.5) - split[..., 1]
    assert ((split[..., 0] + split[..., 1]) == 0.5).all() and len(np.unique(split[..., 1])) > 4
    for layers in (flat, split):
        d = np.zeros((5, 6, 2), np.float32)
        oracle.mass_creep(d, layers, ONE, op)
        assert_bit_equal(d, np.zeros((5, 6, 2), np.float32), "creep on a plateau")


def test_creep_moves_half_the_excess_over_the_critical_slope(oracle):
    """One step of height 2 between two flat halves, sediment 1 everywhere, critical slope 0.5: T = 0.5 (2 - 0.5) =
    0.75 on both sides of the step, a quarter of it (:708) leaves the upper cell and arrives in the lower one."""
    op = _quiet_param(oracle)
    layers = np.zeros((4, 3, 2), np.float32)
    layers[..., 1] = 1.0
    layers[2:, :, 0] = 2.0
    d = np.zeros((4, 3, 2), np.float32)
    oracle.mass_creep(d, layers, ONE, op)
    want = np.zeros((4, 3, 2), np.float32)
    want[1, :, 1], want[2, :, 1] = 0.1875, -0.1875
    assert_bit_equal(d, want, "creep across one step")


def test_a_loss_takes_the_sediment_first_and_the_bedrock_for_the_rest(oracle):
    """A ramp of slope 2 along x, critical slope 1, landslide rate 0.25: the centre cell loses 0.25 (1 x (2 - 1) x
    0.25; the clamp is at 0.25 sqrt(2) x 2).  Bare rock: all of it from the bedrock.  Sediment 0.125: that, and 0.125
    of bedrock.  Sediment 1: sediment alone."""
    op = _quiet_param(oracle)
    op.landslideRateDebris = 0.25
    for sediment, want in ((0.0, (-0.25, 0.0)), (0.125, (-0.125, -0.125)), (1.0, (0.0, -0.25))):
        layers = np.zeros((3, 3, 2), np.float32)
        layers[..., 0] = 2.0 * np.arange(3, dtype=np.float32)[:, None]
        layers[1, 1] = (2.0 - sediment, sediment)
        d = _transfer(oracle, layers, op)
        assert_bit_equal(d[1, 1], np.array(want, np.float32), "loss with sediment %g" % sediment)


def test_a_gain_goes_to_the_sediment(oracle):
    """Flat ground, debris 0.5, deposition rate 0.125, no yield stress: the debris deposits min(0.5, 0.125 x 0.5) =
    0.0625, all of it sediment; debris 16 would deposit 2, and the gain stops at the clamp 0.25 sqrt(2) x 0.3."""
    op = _quiet_param(oracle)
    op.depositionRateDebris = 0.125
    layers = np.full((3, 3, 2), 0.25, np.float32)
    assert_bit_equal(_transfer(oracle, layers, op, debris=0.5)[1, 1], np.array((0.0, 0.0625), np.float32), "gain")
    cap = np.float32(0.25) * np.sqrt(np.float32(2.0)) * np.float32(0.3)
    assert_bit_equal(_transfer(oracle, layers, op, debris=16.0)[1, 1], np.array((0.0, cap), np.float32), "clamped gain")


def test_a_cell_between_nan_neighbours_takes_the_exit_slope_on_both_axes(oracle):
    """__glocal marks a neighbour outside the grid with NaN; a NaN height inside the grid is read the same way."""
    op = _quiet_param(oracle)
    layers = np.full((3, 3, 2), np.nan, np.float32)
    layers[1, 1] = (0.5, 0.25)
    for scale in (ONE, (0.5, 2.0, 4.0)):
        assert_bit_equal(oracle.glocal(layers, 1, 1, scale, op.exitSlope), np.array((0.03125, 0.03125), np.float32), "glocal")
    # ... and so does the whole cell: velocity = A (-g grad) / |scale.y| = -0.03125 on both axes; no transfer.  Creep
    # reads the four NaN heights as ties (`hp0 > h00` is false) and its limit 0.5 ((h - NaN) - ..) as no limit at all
    # (a NaN operand loses the minimum): each neighbour takes the cell's whole sediment, 0.25 x 4 x 0.25 in all
    z = lambda *c: np.zeros((3, 3) + c, np.float32)
    with np.errstate(all="ignore"):
        w = oracle.erode_cells(layers, z(), z(), z(), z(), z(2), z(), z(2), ONE, op)
    assert_bit_equal(w["velocity"][1, 1], np.array((-0.03125, -0.03125), np.float32), "velocity")
    assert_bit_equal(w["debrisVelocity"][1, 1], np.array((-0.03125, -0.03125), np.float32), "debris velocity")
    assert_bit_equal(w["layers_next"][1, 1], np.array((0.5, 0.0), np.float32), "layers")
    assert np.isnan(w["layers_next"][0, 1]).all() and np.isnan(w["height"][1, 0])


def test_the_minimum_and_maximum_of_the_cell_phase_follow_the_device_rule(oracle):
    """A NaN operand loses and -0 orders below +0 (CUDA's fmaxf / fminf, v_max_f32 / v_min_f32), whichever operand
    comes first; both NaN: NaN."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    word = lambda v: int(bits(np.array([v], np.float32))[0])
    for a, b, hi, lo in ((0.0, -0.0, 0.0, -0.0), (-0.0, 0.0, 0.0, -0.0), (0.0, 0.0, 0.0, 0.0), (-0.0, -0.0, -0.0, -0.0),
                         (nan, -0.0, -0.0, -0.0), (-0.0, nan, -0.0, -0.0), (nan, 1.5, 1.5, 1.5), (-inf, nan, -inf, -inf),
                         (1.0, 2.0, 2.0, 1.0), (2.0, 1.0, 2.0, 1.0), (-inf, inf, inf, -inf), (-1e-45, 0.0, 0.0, -1e-45),
                         (3e38, -3e38, 3e38, -3e38)):
        assert word(oracle.fmaxf(a, b)) == word(np.float32(hi)), ("fmaxf", a, b)
        assert word(oracle.fminf(a, b)) == word(np.float32(lo)), ("fminf", a, b)
    assert np.isnan(oracle.fmaxf(nan, nan)) and np.isnan(oracle.fminf(nan, nan))


def test_the_order_of_the_zeros_reaches_one_bit_of_the_stand_alone_transfer(oracle):
    """A flat cell nothing visited: transfer = fmaxf(+0, -0.25 L x 0) = +0 under the device rule, and delta.y +=
    fmaxf(0, +0 / scale.z) turns a delta.y of -0 into +0.  (Under the libm's order both maxima are -0 and the -0
    stays.)  From delta = +0, where the fused step starts, both orders give +0."""
    for op in (_quiet_param(oracle), oracle.default_param()):
        layers = np.full((3, 3, 2), 0.25, np.float32)
        d = _transfer(oracle, layers, op, delta=-0.0)
        assert int(bits(d[1, 1])[1]) == 0, "delta.y after a transfer of +0 from -0: %r" % d[1, 1, 1]
        d = _transfer(oracle, layers, op, delta=0.0)
        assert int(bits(d[1, 1])[1]) == 0
