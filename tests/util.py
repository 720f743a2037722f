"""Shared input builders for the parity tests (seeded, deterministic)."""
import numpy as np


def terrain(oracle, H, W, seed=3.0, sediment=0.0, rng_seed=0):
    """(H, W, 2) layer plane: FBm bedrock (soil.noise parameters of
    example/erosion_gpu.py:9-15) + optional random sediment."""
    bed = oracle.noise(H, W, seed=seed, ext=(float(H), float(W)))
    layers = np.zeros((H, W, 2), np.float32)
    layers[..., 0] = bed
    if sediment > 0:
        r = np.random.default_rng(rng_seed)
        layers[..., 1] = (r.random((H, W)) * sediment).astype(np.float32)
    return layers


def script_param(oracle_or_param):
    """Parameters of example/erosion_gpu.py:75-100 mapped onto the live names
    (SURVEY.md §8a legacy->live mapping)."""
    p = oracle_or_param
    p.timeStep = 1000.0
    p.maxage = 256
    p.lrate = 1.0
    p.gravity = 9.81
    p.uplift = 0.01
    p.rainfall = 1.0
    p.evapRate = 0.0005
    p.viscosityWater = 0.000001
    p.bedShearWater = 12.5
    p.suspensionRateFluvial = 0.0008
    p.depositionRateFluvial = 0.00001
    p.fluvialExponent = 0.01
    p.exitSlope = 0.025
    p.critSlopeBedrock = 0.57
    p.landslideRateDebris = 0.0025
    p.suspensionRateDebris = 0.00025
    p.depositionRateDebris = 0.0001
    p.yieldStress = 2E6
    p.densityDebris = 2500.0
    p.viscosityDebris = 0.004
    p.bedShearDebris = 60 / 2500.0
    return p


def log_uniform(r, lo, hi):
    """One draw of numpy Generator `r`, log-uniform in [lo, hi)."""
    return float(np.exp(r.uniform(np.log(lo), np.log(hi))))


def random_param(oracle, r, force=False):
    """An oracle Param drawn with numpy Generator `r` (test_gpu_parity.test_transport_random_parameter_sets): the
    script's values, maxage in [40, 130), the rates log-uniform over several decades around the script's, and with
    `force` an external force of N(0, 0.3) per axis.  The draws come in this order, one each."""
    op = script_param(oracle.default_param())
    op.maxage = int(r.integers(40, 130))
    lu = lambda lo, hi: log_uniform(r, lo, hi)
    op.gravity = lu(1.0, 30.0)
    op.evapRate = lu(1e-5, 1e-2)
    op.viscosityWater = lu(1e-7, 1e-2)
    op.bedShearWater = lu(0.05, 60.0)
    op.frictionFactor = lu(0.01, 1.0)
    op.depositionRateFluvial = lu(1e-7, 1e-2)
    op.suspensionRateFluvial = lu(1e-5, 1e-2)
    op.fluvialExponent = lu(0.01, 1.5)
    op.viscosityDebris = lu(1e-4, 0.1)
    op.bedShearDebris = lu(1e-3, 1.0)
    op.yieldStress = lu(1e-3, 1e7)
    op.critSlopeBedrock = lu(0.02, 0.8)
    op.landslideRateDebris = lu(1e-4, 1e-1)
    op.suspensionRateDebris = lu(1e-5, 1e-2)
    op.depositionRateDebris = lu(1e-5, 1e-2)
    if force:
        op.force[0], op.force[1] = float(r.normal(0, 0.3)), float(r.normal(0, 0.3))
    return op


def copy_param(src, dst):
    """Copy a ctypes Param (oracle or product) field by field."""
    for name, _ in src._fields_:
        if name == "force":
            dst.force[0], dst.force[1] = src.force[0], src.force[1]
        elif name != "_pad":
            setattr(dst, name, getattr(src, name))
    return dst


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def assert_bit_equal(a, b, what=""):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = bits(a) == bits(b)
    both_nan = np.isnan(a) & np.isnan(b) if a.dtype.kind == "f" else np.zeros(a.shape, bool)
    bad = ~(same | both_nan)
    if bad.any():
        idx = np.argwhere(bad)[:5]
        raise AssertionError("%s: %d of %d elements differ, first at %s: %s vs %s" % (
            what, bad.sum(), bad.size, idx.tolist(), a[tuple(idx[0])], b[tuple(idx[0])]))


# ---- device helpers (GPU tests only) ----------------------------------------

def to_gpu(arr):
    from soillib_amd import silt
    return silt.tensor.from_numpy(np.ascontiguousarray(arr)).gpu()


def to_np(t):
    return t.cpu().numpy()


def rng_to_gpu(rng_np):
    """Upload an oracle rng array (structured seed/offset) as a silt.rng tensor."""
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(rng_np.astype(silt.RNG_NP)).gpu()


def product_param(oracle_param):
    """A soillib_amd.soil.param_t carrying the same values as an oracle Param."""
    from soillib_amd import soil
    p = soil.param_t()
    copy_param(oracle_param, p._c)
    return p


# ---- random_weighted: tolerance on the receiver ---------------------------

_D8 = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))   # graph.hpp:21-46


def assert_receivers_close(oracle, got, want, height, K, seed, offset, T, what="random_weighted",
                           max_frac=2e-5, edge_tol=2e-5):
    """The Gibbs weights of `random_weighted` are the reference's fast `__expf` (graph.cu:139): a
    tolerance, and with them every receiver whose draw lies within their error of a CDF edge.  The
    product's map must equal the oracle's but for a counted handful of cells, and each of those must
    be such a cell: its two receivers neighbours in the cumulative order, the draw within `edge_tol`
    of the edge between them (weights recomputed here in float64)."""
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, what
    H, W = got.shape
    bad = np.argwhere(got != want)
    assert len(bad) <= max(1, int(max_frac * got.size)), "%s: %d of %d receivers differ" % (what, len(bad), got.size)
    h = np.asarray(height, np.float64)
    for x, y in bad:
        n = int(x) * W + int(y)
        u = float(oracle.rng_uniform_cell(seed, offset, [n])[0])
        idx, cdf, z = [], [], 0.0
        for k in range(K):
            nx, ny = x + _D8[k][0], y + _D8[k][1]
            if nx < 0 or ny < 0 or nx >= H or ny >= W:
                continue
            dE = (h[x, y] - h[nx, ny]) / (1.0 if k < 4 else float(np.float32(np.sqrt(np.float32(2.0)))))
            z += np.exp(dE / T) if dE > 0 else 0.0
            idx.append(int(nx) * W + int(ny))
            cdf.append(z)
        assert z > 0, "%s: cell (%d, %d) has no downhill neighbour, receivers %d vs %d" % (what, x, y, got[x, y], want[x, y])
        edges = [c / z for c in cdf]
        near = [e for e, i in zip(edges, idx) if abs(u - e) <= edge_tol]
        assert near, "%s: cell (%d, %d): receivers %d vs %d, draw %.9f, edges %s" % (
            what, x, y, got[x, y], want[x, y], u, ["%.9f" % e for e in edges])
        assert got[x, y] in idx + [-1] and want[x, y] in idx + [-1], what


# ---- the particle launches and solve_uniform against the oracle (test_gpu_parity.py, test_gpu_cpp_ops.py) --------

def flux_close(got, want, what):
    """Same trajectories, different fp32 summation order: compare against the
    magnitude accumulated in each cell.  The absolute term covers cells of the signed (velocity)
    planes whose deposits cancel: their rounding error goes with the magnitude of the terms — up
    to the plane's maximum — not with the sum that is left (a lost or doubled deposit would show
    as an error of the order of the cell's own value)."""
    scale = np.nanmax(np.abs(want)) + 1e-30
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=4e-6 * scale, err_msg=what)
    # the same set of visited cells.  Deposits that have decayed to the edge of the fp32 range are
    # exempt: the oracle's expf_ flushes below e^-87, the attenuations' v_exp_f32 (att_exp,
    # soil_math.hpp) below 2^-126 — a deposit of 1e-38 on one side, none on the other
    assert (got[np.abs(want) > 1e-25 * scale] != 0).all(), what + ": different set of visited cells"
    assert (np.abs(got[want == 0]) <= 1e-30 * scale).all(), what + ": different set of visited cells"


def assert_fluvial_close(got, want):
    """The planes of a transport_fluvial launch, as numpy, against the oracle's: dicts with the flux planes wf, mf,
    vf, the normalised planes wh, m, v and the colour flux af."""
    for k in ("wf", "mf", "vf"):
        flux_close(got[k], want[k], "fluvial flux " + k)
    for k in ("wh", "m", "v"):
        np.testing.assert_allclose(got[k], want[k], rtol=3e-5,
                                   atol=3e-6 * (np.nanmax(np.abs(want[k])) + 1e-30), err_msg=k)
    np.testing.assert_allclose(got["af"], want["af"], rtol=1e-3, atol=1e-5)


def assert_debris_close(got, want):
    """The planes of a transport_debris launch against the oracle's: the flux planes mf, vf, the normalised m, v and
    the colour flux af."""
    np.testing.assert_allclose(got["af"], want["af"], rtol=1e-3, atol=1e-5)
    for k in ("mf", "vf"):
        flux_close(got[k], want[k], "debris flux " + k)
    for k in ("m", "v"):
        np.testing.assert_allclose(got[k], want[k], rtol=3e-5,
                                   atol=3e-6 * (np.nanmax(np.abs(want[k])) + 1e-30), err_msg=k)


def assert_solve_uniform_close(got, want):
    """solve_uniform's flux against the oracle's: the same cells finite, and those close."""
    ok = np.isfinite(want)
    assert (np.isfinite(got) == ok).all()
    np.testing.assert_allclose(got[ok], want[ok], rtol=5e-5,
                               atol=1e-6 * np.abs(want[ok]).max())


def debris_steps_match(got, want):
    """Steps a debris launch walked against the count of a side that walks every walker to the end (the oracle,
    the direct launch shape): equal — unless this process retires spent debris walkers (soil_set_debris_retire(1);
    the suite runs with them WATCHED, tests/conftest.py: walked to the end, so equal), where it may be fewer."""
    from soillib_amd import soil
    return got <= want if soil.debris_retire() == 1 else got == want



def retired_steps_close(got, r, N):
    """Steps a launch of N walkers that retires spent debris walkers walked, against the oracle's rule-aware walk `r`
    (pyoracle.particles_debris_retire).  Gate shut: nobody retires, the full walk's count exactly.  Gate open: never
    more than the full walk, and the count under the rule up to one step per 512 walkers (at least 2).  The
    trajectories are the oracle's bit for bit, but the moment an attenuation becomes an EXACT zero is not: the
    device's attenuation exponential (soil_math.hpp: att_exp, v_exp_f32) flushes below 2^-126 where the spec's expf
    flushes below e^-87, and the product of two attenuations may be subnormal on one side and zero on the other.  A
    walker whose attenuation lands in that sliver of the fp32 range is spent a step earlier or later (measured: 4
    steps for 8192 walkers at 256^2, tests/test_debris_retire.py)."""
    if not r["gate"]:
        return got == r["steps"]
    return got <= r["steps"] and abs(got - r["rule_steps"]) <= max(2, N // 512)


def debris_steps_agree(got, r, N, tiled=True):
    """The debris step count of a launch of N walkers against the oracle's rule-aware walk `r`: where this process
    retires spent walkers and the launch shape is the tiled one (the only shape that retires), retired_steps_close;
    everywhere else the full walk's count exactly."""
    from soillib_amd import soil
    if tiled and soil.debris_retire() == 1:
        return retired_steps_close(got, r, N)
    return got == r["steps"]


# ---- flow graphs for the accumulation tests (numpy, deterministic, any H x W, D4 and D8) -------------------
# A graph holds the flat index of each cell's receiver, or -1.  `accumulate` only ever compares graph[d] with the
# index of one of d's K neighbours, so any int32 is a legal entry; a value that is no neighbour's index is no edge.

def _cells(H, W):
    return np.arange(H * W, dtype=np.int64).reshape(H, W)


def graph_snake(H, W):
    """One chain through every cell: row by row, alternate rows reversed; the last cell is the only outlet."""
    idx = _cells(H, W)
    g = np.empty((H, W), np.int64)
    g[0::2, :-1] = idx[0::2, 1:]          # even rows run east ...
    g[0::2, -1] = idx[0::2, -1] + W       # ... and step down at their east end
    g[1::2, 1:] = idx[1::2, :-1]          # odd rows run west
    g[1::2, 0] = idx[1::2, 0] + W
    g[H - 1, W - 1 if (H - 1) % 2 == 0 else 0] = -1
    return g.astype(np.int32)


def _fan_centres(H, W):
    """Row and column of the centre of each cell's 3 x 3 block (blocks ragged at the far edges)."""
    x, y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return x, y, np.minimum(x // 3 * 3 + 1, H - 1), np.minimum(y // 3 * 3 + 1, W - 1)


def graph_fan(H, W, edge):
    """3 x 3 blocks whose cells all drain into the block's centre, an outlet.  D8: the centre has all 8 donors.
    D4: its 4-neighbours drain into it, each corner into the edge cell of its column."""
    x, y, cx, cy = _fan_centres(H, W)
    g = cx * W + cy
    if edge == 0:
        corner = (x != cx) & (y != cy)
        g[corner] = (cx * W + y)[corner]
    g[(x == cx) & (y == cy)] = -1
    return g.astype(np.int32)


def graph_fan_chain(H, W, edge):
    """graph_fan, but a centre drains into its east neighbour and that one east again into the next block's west
    cell (which drains into that block's centre): cells with K - 1 donors on a chain along each row of blocks."""
    x, y, cx, cy = _fan_centres(H, W)
    g = graph_fan(H, W, edge).astype(np.int64)
    idx = _cells(H, W)
    centre = (x == cx) & (y == cy) & (y + 2 < W)
    east = np.zeros((H, W), bool)
    east[:, 1:] = centre[:, :-1]
    g[centre] = idx[centre] + 1
    g[east] = idx[east] + 1
    return g.astype(np.int32)


def graph_no_edges(H, W):
    return np.full((H, W), -1, np.int32)


def graph_one_sink(H, W):
    """Every cell steps towards cell (0, 0): up, then left along row 0.  W chains that merge on one line."""
    idx = _cells(H, W)
    g = idx - W
    g[0, 1:] = idx[0, :-1]
    g[0, 0] = -1
    return g.astype(np.int32)


def graph_cycles(base, seed=5):
    """`base` (a legal graph) with about a tenth of the horizontally adjacent pairs rewired to point at each other,
    plus a few 4-cycles.  Such cells never finish; the rounds are synchronous, so the plane after the fixed number
    of rounds is still one definite plane."""
    H, W = base.shape
    g = base.astype(np.int64).copy()
    idx = _cells(H, W)
    r = np.random.default_rng(seed)
    if W >= 2:
        pair = r.random((H, W // 2)) < 0.1
        a, b = idx[:, 0:W // 2 * 2:2], idx[:, 1:W // 2 * 2:2]
        ga, gb = g[:, 0:W // 2 * 2:2], g[:, 1:W // 2 * 2:2]     # views
        ga[pair] = b[pair]
        gb[pair] = a[pair]
    if H >= 2 and W >= 2:
        for _ in range(max(1, H * W // 500)):
            x, y = int(r.integers(0, H - 1)), int(r.integers(0, W - 1))
            g[x, y], g[x, y + 1], g[x + 1, y + 1], g[x + 1, y] = idx[x, y + 1], idx[x + 1, y + 1], idx[x + 1, y], idx[x, y]
    return g.astype(np.int32)


def graph_wild(base, seed=9):
    """`base` (a legal graph) mixed with entries that are no edge: random values in [-5, 2 H W), receivers two rows
    away, across a row's end, "down-left" from column 0, the cell itself."""
    H, W = base.shape
    g = base.astype(np.int64).copy()
    idx = _cells(H, W)
    r = np.random.default_rng(seed)
    noise = r.random((H, W)) < 0.25
    g[noise] = r.integers(-5, 2 * H * W, size=(H, W))[noise]
    g[::3, ::2] = idx[::3, ::2] + 2 * W
    g[1::3, -1] = idx[1::3, -1] + 1
    g[2::3, 0] = idx[2::3, 0] + W - 1
    own = r.random((H, W)) < 0.02
    g[own] = idx[own]
    return g.astype(np.int32)


def built_graphs(H, W, edge):
    """name -> graph for the builders that need nothing but the grid."""
    return {"snake": graph_snake(H, W), "fan": graph_fan(H, W, edge), "fan_chain": graph_fan_chain(H, W, edge),
            "no_edges": graph_no_edges(H, W), "one_sink": graph_one_sink(H, W)}


def stack_graphs(tiles):
    """Tiles of (h, W) one under the other: tile t's receivers shifted by t h W, its -1 kept."""
    h, W = tiles[0].shape
    return np.concatenate([np.where(g >= 0, g + np.int32(t * h * W), g).astype(np.int32) for t, g in enumerate(tiles)])


# ---- the particle generator in numpy (solve_uniform's spawn draws) --------------------------------------------

def philox_word0(seed, subsequence, offsets):
    """Word 0 of Philox4x32-10 at counter {offset, subsequence}, key `seed`, for an array of offsets: the 32 bits
    a walker's generator (soil_oracle.c: orc_rng_next) turns into its next uniform."""
    offsets = np.asarray(offsets, np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c = [offsets & m32, offsets >> np.uint64(32), np.full_like(offsets, int(subsequence) & 0xFFFFFFFF),
         np.full_like(offsets, int(subsequence) >> 32)]
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c[0].astype(np.uint32)


def find_unit_draws(seed, subsequence, start, stop):
    """The offsets in [start, stop) at which the generator of (seed, subsequence) draws a uniform of exactly 1.0:
    ((word >> 8) + 1) 2^-24 is 1.0 when the word's upper 24 bits are all set, one draw in 2^24.  How the constants
    of tests/test_gpu_solve_uniform.py were found: find_unit_draws(1, 0, 0, 1 << 24) -> [8418514]."""
    found = []
    for lo in range(start, stop, 1 << 20):
        off = np.arange(lo, min(stop, lo + (1 << 20)), dtype=np.uint64)
        found += off[(philox_word0(seed, subsequence, off) >> np.uint32(8)) == 0xFFFFFF].tolist()
    return found


# ---- the cell phase on hostile cells (tests/test_cells_hostile.py, tests/test_gpu_cells_hostile.py) ---------------

CELL_IN = ("layers", "uplift", "rainfall", "waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux")
CELL_FLUX = ("waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux")
CELL_OUT = ("layers_next", "height", "waterHeight", "mass", "velocity", "debris", "debrisVelocity")
COLOUR_IN = ("albedoBedrock", "albedoSurface", "albedoFluvial", "albedoDebris")
COLOUR_OUT = ("albedoSurface", "albedoFluvial", "albedoDebris")

# every launch shape of the fused cell kernel (csrc/erosion_cells.hip; the class of each is asserted by
# tests/test_cells_hostile.py::test_every_shape_is_in_its_class)
HOSTILE_SHAPES = [(12, 40), (8, 256), (9, 260), (5, 1028), (256, 256), (252, 260), (283, 260), (247, 260),
                  (37, 53), (3, 7), (5, 1), (1, 1)]

DENORMAL = np.float32(1e-44)


def cell_inputs(oracle, H, W, seed=0):
    """The benign draw of the cell phase's eight input planes (test_gpu_parity._cell_inputs, the same draws)."""
    r = np.random.default_rng(seed)
    layers = terrain(oracle, H, W, sediment=0.02, rng_seed=seed)
    f1 = lambda s: (r.random((H, W)) * s).astype(np.float32)
    f2 = lambda s: (r.standard_normal((H, W, 2)) * s).astype(np.float32)
    return dict(layers=layers, uplift=f1(1.0), rainfall=f1(2.0), waterFlux=f1(3.0), massFlux=f1(0.5),
                velocityFlux=f2(2.0), debrisFlux=f1(0.2), debrisVelocityFlux=f2(1.0))


class _Placer:
    """Hands out room on an H x W grid to the items of a hostile plane, so that none lands on another: column blocks
    of 16 cells from column 16 on (a block starts on a four-cell group boundary; the first block is left to the
    colour cases and the plateau across a row's end, the last three columns to that plateau too, columns 240 - 271
    to the one across the wave boundary), in each block bands of rows from row 1 to row H - 2 with a free row
    between two bands.  An item uses columns c0 + 1 .. c0 + 11 of its band.  When the
    grid is full `take` returns None and the item is left out: the items are asked for in the order of their weight."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.blocks = [c0 for c0 in range(16, W - 14, 16) if not (W > 256 and 240 <= c0 < 272)]
        self.free = {c0: 1 for c0 in self.blocks}

    def take(self, rows=1):
        for c0 in self.blocks:
            x = self.free[c0]
            if x + rows <= self.H - 1:
                self.free[c0] = x + rows + 1
                return x, c0
        return None

    def roomy(self):
        """Whether every item of hostile_cell_inputs finds room (the bands it asks for, in its order)."""
        dry = _Placer(self.H, self.W)
        return all(dry.take(rows) for rows in (1, 1, 3, 2, 3, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1))


def hostile_cell_inputs(oracle, H, W, seed=0):
    """The eight input planes of the cell phase (cell_inputs) with the cells a benign draw never holds; the items
    are placed from (H, W) (_Placer), each one wherever the grid has room for it.

    Layers: plateaus of equal height — inside a row across a four-cell group boundary, across columns 255 / 256
    (a wave boundary within a row) where W > 256, across a row's end into the next row's start, and +inf plateaus
    (the only ties on which `hp0 > h00` against `>=` changes a value: both creep terms are 0 on a finite tie, on an
    infinite one the difference of the heights is NaN and each side's term its own sediment); neighbours of equal
    total height split differently between bedrock and sediment; patches and single cells of sediment exactly 0;
    tiny negative sediment; cliffs beside cells of large suspended mass and debris; thick and thin sediment under a
    loss; runs of (+0, -0) and (-0, +0); denormal layers; 3e38 beside -3e38; +inf, -inf and NaN in the interior, on
    the four edges, at a corner and on both sides of a group boundary.

    Flux planes: exactly 0 on at least 30 % of the cells of each plane (independently), one all-zero row, NaN in
    cell (0, 0) of all five (where walkers gone NaN park their deposits), +inf, -0, a denormal, a velocity flux of
    1e20 (its square overflows) and of (1e-30, 1e-44), a negative and a huge mass flux.
    Uplift and rainfall: 0, a negative value, a NaN.

    Below 256 cells fewer non-finite values are placed (none below 5 cells), so that four cells in five stay
    finite on every grid."""
    inp = cell_inputs(oracle, H, W, seed)
    r = np.random.default_rng(seed + 77)
    L, n = inp["layers"], H * W
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    big = n >= 256
    at = _Placer(H, W)

    def level(x, y0, y1, height):
        """cells (x, y0 .. y1 - 1) brought to one total height, each cell's sediment kept"""
        L[x, y0:y1, 0] = np.float32(height) - L[x, y0:y1, 1]
        # float32: (bedrock + sediment) must be the same number in every cell, not only nearly
        L[x, y0:y1, 0] += np.float32(height) - (L[x, y0:y1, 0] + L[x, y0:y1, 1])
        assert ((L[x, y0:y1, 0] + L[x, y0:y1, 1]) == np.float32(height)).all()

    # --- flux planes: zeros first (the special cells are written over them)
    for name in CELL_FLUX:
        inp[name][r.random((H, W)) < 0.35] = 0.0
    if H >= 3:
        for name in CELL_FLUX:                               # the all-zero row: the last one (no flux item goes there)
            inp[name][H - 1] = 0.0
    L[r.random((H, W)) < 0.05, 1] = 0.0                      # single cells of bare rock

    # --- the open slope: a gain at the upper clamp, losses at the lower one from thick, thin and no sediment
    if (p := at.take()):
        x, c = p
        inp["massFlux"][x, c + 2] = np.float32(1e12)        # deposition far above 0.075 L: upper clamp, mix colour
        L[x, c + 2, 1] = np.float32(0.01)
        inp["velocityFlux"][x, c + 2] = 0.0
        for k, sed in ((5, 50.0), (7, 1e-6), (9, 0.0)):     # the velocity's square overflows: -inf, lower clamp
            inp["velocityFlux"][x, c + k] = (1e20, 0.0)
            L[x, c + k, 1] = np.float32(sed)
            inp["massFlux"][x, c + k] = 0.0
            inp["debrisFlux"][x, c + k] = 0.0
    # --- plateaus
    if (p := at.take()):                                    # equal totals, the draw's different sediments,
        level(p[0], p[1] + 1, p[1] + 10, 0.375)             # across the group boundaries at c0 + 4 and c0 + 8
    if (p := at.take(3)):                                   # 3 x 6: ties on both axes, a middle row without any slope
        for dx in range(3):
            level(p[0] + dx, p[1] + 1, p[1] + 7, 0.4375)
    if big and (p := at.take(2)):                           # a +inf tie along x, a different sediment on each side
        L[p[0], p[1] + 5] = (inf, 0.25)
        L[p[0] + 1, p[1] + 5] = (inf, 0.0625)
    if (p := at.take(3)):                                   # three rows of height 0: the middle one has no slope at all
        x, c = p
        L[x:x + 3, c + 1:c + 6] = (0.0, -0.0)
        L[x:x + 3, c + 6:c + 12] = (-0.0, 0.0)
        for name in CELL_FLUX:                              # cells nothing visited: transfer is an exact zero there,
            inp[name][x:x + 3, c + 1:c + 12] = 0.0          # clamped against the -0 of -0.25 L * 0
        inp["debrisFlux"][x + 1, c + 3] = -0.0
        inp["velocityFlux"][x + 1, c + 4] = (-0.0, 0.0)
        inp["massFlux"][x + 1, c + 8] = -0.0
    if W > 256 and H >= 4:                                  # columns 255 | 256: a wave boundary within a row
        level(H - 2, 250, 262, 0.625)
    if H >= 4 and W >= 4:                                   # row 1's last cells and row 2's first
        level(1, W - 3, W, 0.75)
        level(2, 0, 3, 0.75)
    if (p := at.take()):                                    # a flat plateau: one bedrock, one sediment
        L[p[0], p[1] + 2:p[1] + 11] = (0.25, 0.25)
    # --- cliffs far above both critical slopes, beside large suspended mass and debris
    if (p := at.take()):
        x, c = p
        L[x, c + 2, 0] += 60.0
        L[x, c + 6, 0] += 60.0
        L[x, c + 6, 1] = 50.0                               # ... of sediment: the loss never reaches the bedrock
        L[x, c + 9, 0] += 60.0
        L[x, c + 9, 1] = np.float32(1e-6)                   # ... the loss takes all the sediment and goes on
        L[x, c + 10, 0] += 60.0
        L[x, c + 10, 1] = 0.0                               # ... bare rock
        inp["massFlux"][x, c + 1:c + 4] = np.float32(1e12)
        inp["debrisFlux"][x, c + 1:c + 4] = np.float32(1e6)
        inp["massFlux"][x, c + 5:c + 8] = 0.0
        inp["debrisFlux"][x, c + 5:c + 8] = 0.0
    # --- sediment exactly 0, tiny negative
    if (p := at.take(2)):
        L[p[0]:p[0] + 2, p[1] + 1:p[1] + 9, 1] = 0.0
    if (p := at.take()):
        L[p[0], p[1] + 1:p[1] + 4, 1] = np.float32(-1e-6)
        L[p[0], p[1] + 6, 1] = -DENORMAL
    # --- denormals, the ends of the range
    if (p := at.take()):
        L[p[0], p[1] + 1:p[1] + 4] = (DENORMAL, DENORMAL)
        L[p[0], p[1] + 4:p[1] + 7] = (np.float32(1e-39), 0.0)
    if n >= 64 and (p := at.take()):
        L[p[0], p[1] + 2] = (3e38, 0.0)
        L[p[0], p[1] + 3] = (-3e38, 0.0)
        L[p[0], p[1] + 4] = (3e38, 0.01)                    # (its height times scale.z overflows)

    # --- non-finite layers
    bad = (inf, -inf, nan)
    if big:
        if (p := at.take()):                                # the interior, three columns apart
            for k, v in enumerate(bad):
                L[p[0], p[1] + 2 + 3 * k, k % 2] = v
        if (p := at.take()):                                # both sides of the group boundaries at c0 + 4, + 8, + 12
            for k, v in enumerate(bad):
                L[p[0], p[1] + 4 * k + 3, 0] = v
                L[p[0], p[1] + 4 * k + 4, 0] = v
            L[p[0], p[1] + 3, 1], L[p[0], p[1] + 4, 1] = 0.5, 0.125     # the +inf tie along y
        if W >= 12 and H >= 3:
            for k, v in enumerate(bad):
                L[0, 3 + 3 * k, 0] = v                      # top edge
                L[H - 1, 3 + 3 * k, 1] = v                  # bottom edge
        if H >= 6 and W >= 2:                               # left and right edge (below the plateau across row 1's end)
            for k, v in enumerate(bad[:H - 5]):
                x = H - 4 - 2 * k if H >= 11 else 3 + k
                L[x, 0, 0] = v
                L[x, W - 1, 0] = v
        L[H - 1, W - 1, 0] = nan                            # corners
        L[H - 1, 0, 0] = inf
        L[0, W - 1, 0] = -inf
    elif n >= 20:
        L[H - 1, W - 1, 0] = nan

    # --- the flux planes' special cells
    if n >= 5:
        for name in CELL_FLUX:
            inp[name][0, 0] = nan
    if (p := at.take()):
        x, c = p
        if big:
            inp["waterFlux"][x, c + 1] = inf
            inp["debrisVelocityFlux"][x, c + 3] = (0.0, inf)
        inp["waterFlux"][x, c + 5] = -0.0
        inp["massFlux"][x, c + 5] = -0.0
        inp["massFlux"][x, c + 6] = DENORMAL
        inp["debrisFlux"][x, c + 6] = DENORMAL
        inp["waterFlux"][x, c + 7] = DENORMAL
        inp["velocityFlux"][x, c + 8] = (1e-30, DENORMAL)
        inp["debrisVelocityFlux"][x, c + 8] = (1e20, -1e20)
        inp["massFlux"][x, c + 9] = -0.3
        inp["debrisFlux"][x, c + 10] = -0.2
    # --- uplift and rainfall
    if (p := at.take()):
        x, c = p
        inp["uplift"][x, c + 1], inp["rainfall"][x, c + 2] = 0.0, 0.0
        inp["uplift"][x, c + 3], inp["rainfall"][x, c + 4] = -0.5, -1.5
        if n >= 64:
            inp["uplift"][x, c + 5], inp["rainfall"][x, c + 6] = nan, nan
    return inp


def colour_inputs(H, W, seed):
    """Colour flux planes with cells of |a| == 0, colours in [0, 1.3) (test_gpu_colour_step._colour_inputs)."""
    r = np.random.default_rng(seed)
    c3 = lambda s: (r.random((H, W, 3)) * s).astype(np.float32)
    a_fl, a_db = c3(4.0), c3(2.0)
    a_fl[r.random((H, W)) < 0.2] = 0.0
    a_db[r.random((H, W)) < 0.2] = 0.0
    return dict(albedoBedrock=c3(1.3), albedoSurface=c3(1.3), albedoFluvial=a_fl, albedoDebris=a_db)


def hostile_colour_inputs(inp, seed=0):
    """The four colour planes for the hostile planes `inp` (hostile_cell_inputs; adjusted in place where a case needs
    a mass flux): colour_inputs, then NaN, inf, negative, > 1 and -0 colours; a mass flux <= 0 under a non-zero
    colour flux; a colour flux of exactly (0, 0, 0) over m > 0; of (3e-23, 0, 0), whose square is the least denormal, and
    of (2e-23, 0, 0), whose square is 0, so that `sqrtf(..) > 0` alone decides; and of (2e19, 0, 0), whose square overflows."""
    H, W = inp["layers"].shape[:2]
    col = colour_inputs(H, W, seed + 2)
    n = H * W
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    if H < 3 or W < 12:
        return col
    x = H - 3 if H >= 16 else H - 2                        # a row of its own: hostile_cell_inputs fills from the top
    for name in ("massFlux", "debrisFlux"):
        inp[name][x, 1:12] = np.float32(0.25)             # m > 0 throughout, but for the cells below
    if n >= 256:
        col["albedoFluvial"][x, 1] = (nan, 0.5, 0.5)
        col["albedoDebris"][x, 2] = (inf, 0.5, 0.5)
        col["albedoSurface"][x, 3] = (0.5, nan, 0.5)
        col["albedoBedrock"][x, 3] = (inf, 0.5, 0.5)
    col["albedoSurface"][x, 4] = (-0.5, 7.0, -0.0)
    col["albedoBedrock"][x, 4] = (-0.0, 3.0, -2.0)
    col["albedoFluvial"][x, 5] = (-1.0, 2.0, -0.0)
    col["albedoDebris"][x, 5] = (5.0, -0.0, -3.0)
    inp["massFlux"][x, 6], inp["debrisFlux"][x, 6] = 0.0, -0.1          # m <= 0, a colour flux all the same
    col["albedoFluvial"][x, 6] = (0.5, 0.25, 0.125)
    col["albedoDebris"][x, 6] = (0.5, 0.25, 0.125)
    col["albedoFluvial"][x, 7] = 0.0                                    # |a| == 0 over m > 0
    col["albedoDebris"][x, 7] = 0.0
    col["albedoFluvial"][x, 8] = (3e-23, 0.0, 0.0)                      # a^2 = 9e-46 rounds to the least denormal: |a| > 0
    col["albedoDebris"][x, 8] = (2e-23, 0.0, 0.0)                       # a^2 = 4e-46 rounds to 0: the source colour
    col["albedoFluvial"][x, 9] = (2e19, 0.0, 0.0)                       # a^2 overflows
    col["albedoDebris"][x, 9] = (0.0, -2e19, 0.0)
    return col


def oracle_colour_cells(oracle, inp, col, scale, op):
    """The coloured cell phase on the oracle (test_gpu_colour_step._oracle_colour_cells): normalize_fluvial ->
    normalize_debris -> delta = 0 -> mass_transfer -> mass_creep -> add -> layer_merge, with the colour planes.
    The inputs are left as they are."""
    layers = inp["layers"]
    H, W = layers.shape[:2]
    z1 = lambda: np.zeros((H, W), np.float32)
    z2 = lambda: np.zeros((H, W, 2), np.float32)
    wh, m, v, d, dv = z1(), z1(), z2(), z1(), z2()
    af, ad, surf = col["albedoFluvial"].copy(), col["albedoDebris"].copy(), col["albedoSurface"].copy()
    oracle.normalize_fluvial(inp["waterFlux"], inp["massFlux"], inp["velocityFlux"], af, layers, inp["rainfall"], wh, m,
                             v, surf, scale, op)
    oracle.normalize_debris(inp["debrisFlux"], inp["debrisVelocityFlux"], ad, layers, d, dv, surf, scale, op)
    delta = z2()
    oracle.mass_transfer(delta, layers, inp["uplift"], m, v, d, col["albedoBedrock"], af, ad, surf, scale, op)
    oracle.mass_creep(delta, layers, scale, op)
    with np.errstate(all="ignore"):
        layers_next = layers + delta
        height = layers_next[..., 0] + layers_next[..., 1]
    return dict(layers_next=layers_next, height=height, waterHeight=wh, mass=m, velocity=v, debris=d,
                debrisVelocity=dv, albedoFluvial=af, albedoDebris=ad, albedoSurface=surf)


def oracle_cells(oracle, inp, scale, op, dom=None):
    """oracle.erode_cells on the planes of `inp`."""
    with np.errstate(all="ignore"):
        return oracle.erode_cells(*[inp[k] for k in CELL_IN], scale, op, dom)


def cell_param_sets(oracle, H, W):
    """The four (name, oracle param, scale) sets every hostile case runs under: the default parameters, the script's,
    and two drawn as test_gpu_parity.test_fused_cells_random_parameter_sets_bit_exact draws them (the same
    generator, the same order of draws)."""
    sets = [("default", oracle.default_param(), (20.0 / H, 20.0 / W, 4.0)),
            ("script", script_param(oracle.default_param()), (20.0 / H, 20.0 / W, 4.0))]
    for seed in (0, 1):
        r = np.random.default_rng(2000 + seed)
        r.integers(40, 120), r.integers(10, 30)             # (the shape's draws)
        op = script_param(oracle.default_param())
        lu = lambda lo, hi: log_uniform(r, lo, hi)
        op.timeStep = lu(1.0, 1e4)
        op.lrate = lu(0.01, 2.0)
        op.gravity = lu(1.0, 30.0)
        op.uplift = lu(1e-4, 1.0)
        op.rainfall = lu(0.01, 10.0)
        op.frictionFactor = lu(0.01, 1.0)
        op.fluvialExponent = lu(0.01, 1.5)
        op.suspensionRateFluvial = lu(1e-5, 1e-2)
        op.depositionRateFluvial = lu(1e-7, 1e-2)
        op.critSlopeBedrock = lu(0.02, 0.8)
        op.critSlopeSediment = lu(0.02, 0.8)
        op.landslideRateDebris = lu(1e-4, 1e-1)
        op.densityWater = lu(100.0, 2000.0)
        op.densityDebris = lu(500.0, 4000.0)
        sets.append(("random%d" % seed, op, (lu(0.01, 3.0), lu(0.01, 3.0), lu(0.5, 8.0))))
    return sets


def cell_branches(inp, want, scale, op, col=None, want_col=None):
    """Which cells take which branch of the cell phase: a dict of (H, W) masks.  The gradient is restated in float32
    exactly (numpy's + - * / are the IEEE operations); the raw transfer before its clamps in float64 from the
    oracle's own normalised planes, and a cell counts for a clamp only where it is past the clamp by a thousandth of
    it, so the census does not lean on the last bits of a power.  `finite`: every output of the cell is finite."""
    f32 = np.float32
    L = inp["layers"]
    H, W = L.shape[:2]
    sx, sy, sz = (f32(v) for v in scale)
    with np.errstate(all="ignore"):
        h = L[..., 0] + L[..., 1]
        pad = np.full((H + 2, W + 2), np.nan, f32)
        pad[1:-1, 1:-1] = h
        hn0, hp0, h0n, h0p = pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]
        ex = f32(op.exitSlope)

        def side(d, s, sign):
            g = d * sz / s
            lim = np.maximum(g, f32(0)) if sign > 0 else np.minimum(g, f32(0))
            return np.where(np.isnan(g), f32(sign) * ex, lim).astype(f32)
        gxn, gxp = side(h - hn0, sx, 1), side(hp0 - h, sx, -1)
        gyn, gyp = side(h - h0n, sy, 1), side(h0p - h, sy, -1)
        gx = np.where(np.abs(gxn) > 0, gxn, f32(0))
        gx = np.where(np.abs(gxp) > np.abs(gx), gxp, gx)
        gy = np.where(np.abs(gyn) > 0, gyn, f32(0))
        gy = np.where(np.abs(gyp) > np.abs(gy), gyp, gy)
        steep = np.sqrt(gx * gx + gy * gy).astype(np.float64)

        m, d = want["mass"].astype(np.float64), want["debris"].astype(np.float64)
        v = np.sqrt((want["velocity"].astype(np.float64) ** 2).sum(-1))
        v = np.where(v > 1e19, np.inf, v)                   # (its fp32 square overflows)
        step = float(op.timeStep)
        shear = 0.125 * (op.frictionFactor / 8.0) * op.densityWater * v * v
        picked = (op.suspensionRateFluvial / 64.0) * np.power(shear * steep, op.fluvialExponent)
        settled = op.depositionRateFluvial * 1.33 * m
        over = steep - op.critSlopeBedrock
        slide = np.fmax(0.0, op.landslideRateDebris * over)
        yld = op.gravity * (d * over - op.yieldStress)
        up = slide + op.suspensionRateDebris * np.fmax(0.0, yld)
        down = np.fmin(d, np.fmax(0.0, -op.depositionRateDebris * yld))
        raw = step * (settled - picked + down - up)
        diag = float(np.sqrt(sx * sx + sy * sy))
        lo, hi = -0.25 * diag * steep, 0.25 * diag * 0.3
        lower = (raw < lo * 1.001) & (lo < 0) & np.isfinite(lo)
        upper = raw > hi * 1.001
        t = np.fmin(np.fmax(raw, lo), hi)
        sed = L[..., 1].astype(np.float64) * float(sz)
        loss = t < -1e-30
        sediment_only = loss & (sed > 0) & (-sed * 0.999 < t)
        reaches_bedrock = loss & (sed >= 0) & (t < -sed * 1.001 - 1e-30)

        hz = h * sz
        tie = np.zeros((H, W), bool)
        tie_split = np.zeros((H, W), bool)
        padz = np.full((H + 2, W + 2), np.nan, f32)
        padz[1:-1, 1:-1] = hz
        pads = np.full((H + 2, W + 2), np.nan, f32)
        pads[1:-1, 1:-1] = L[..., 1]
        for dx, dy in ((0, 1), (2, 1), (1, 0), (1, 2)):
            same = padz[dx:dx + H, dy:dy + W] == hz
            tie |= same
            tie_split |= same & (pads[dx:dx + H, dy:dy + W] != L[..., 1])
        finite = np.ones((H, W), bool)
        for name in CELL_OUT:
            a = want[name]
            finite &= np.isfinite(a) if a.ndim == 2 else np.isfinite(a).all(-1)
        out = dict(lower_clamp=lower, upper_clamp=upper, sediment_only=sediment_only, reaches_bedrock=reaches_bedrock,
                   creep_tie=tie, creep_tie_split=tie_split, finite=finite)
        if col is not None:
            for name in COLOUR_OUT:
                finite = finite & np.isfinite(want_col[name]).all(-1)
            out["finite"] = finite
            out["colour_bedrock"] = L[..., 1] == 0
            eps = 1e-12
            # the transfer the colour block reads is what is left of it after the loss was taken (0 or negative then)
            out["colour_mix"] = (L[..., 1] != 0) & ((m + d) > 0) & (t > 1e-9) & (t > eps)
            for key, flux, a in (("fluvial", inp["massFlux"], col["albedoFluvial"]),
                                 ("debris", inp["debrisFlux"], col["albedoDebris"])):
                norm2 = a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2]      # float32, as written
                out["colour_source_" + key] = ~((flux > 0) & (np.sqrt(norm2) > 0))
            out["colour_source"] = out["colour_source_fluvial"] | out["colour_source_debris"]
    return out
