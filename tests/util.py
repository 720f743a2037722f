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
