"""Known-answer / property tests that pin the CPU oracle.

The reference ships no tests, fixtures or golden vectors for this path
(SURVEY.md §4, §8c), so the oracle is pinned by the analytic consequences of
the cited kernel code instead, plus — for soil.noise — by the reference's own
vendored generator compiled in place (tests/test_noise_golden.py).
"""
import math

import numpy as np
import pytest

from util import terrain

D4, D8 = 0, 1


# ------------------------------------------------------------ spec math

def test_philox_known_answers(oracle):
    # Random123 kat_vectors for philox4x32-10
    assert oracle.philox([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert oracle.philox([0xffffffff] * 4, [0xffffffff] * 2) == [
        0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert oracle.philox([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344],
                         [0xa4093822, 0x299f31d0]) == [
        0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_uniform_range_and_state(oracle):
    rng = oracle.rng_seed(4096, 7, 11)
    u = oracle.rng_uniform(rng, np.arange(4096))
    assert (u > 0).all() and (u <= 1).all()          # (0, 1] like curand_uniform
    assert (rng["offset"] == 12).all()                # one draw advances the offset by one
    assert abs(u.mean() - 0.5) < 0.03
    # addressing: (seed, subsequence, offset) — same triple, same number
    rng2 = oracle.rng_seed(1, 7, 11)
    assert oracle.rng_uniform(rng2, [5])[0] == u[5]


def test_flow_graph_draws_share_a_block_between_four_cells(oracle):
    """random_weighted's draw of cell n: word n & 3 of the Philox block (key seed; counter {offset, n >> 2})
    — one block per four cells (oracle: orc_rng_uniform_cell; device: soil_math.hpp rng_uniform_quad)."""
    seed, offset = 0x1234567890ab, 0x100000007
    cells = np.arange(40, 72)
    u = oracle.rng_uniform_cell(seed, offset, cells)
    for n, got in zip(cells, u):
        words = oracle.philox([offset & 0xffffffff, offset >> 32, int(n) >> 2, 0], [seed & 0xffffffff, seed >> 32])
        assert got == np.float32(((words[int(n) & 3] >> 8) + 1) * 2.0 ** -24)
    assert (u > 0).all() and (u <= 1).all() and len(set(u.tolist())) == len(u)
    # word 0 of a block is what a particle stream of that subsequence draws at that offset
    rng = oracle.rng_seed(1, seed, offset)
    assert oracle.rng_uniform(rng, [44 >> 2])[0] == u[44 - 40]


def test_flow_graph_draws_are_uniform_and_independent(oracle):
    """The four cells that share a Philox block take its four words: their draws have to be as good as four
    blocks' word 0 were (rounds 1-4) — uniform on (0, 1], no correlation between neighbouring cells of a row
    (same block and across blocks), between the rows of a grid, or between two realisations (offsets k, k + 1:
    example/dem_multiflow.py:43-49).  Bounds: 5 sigma of the estimators for N = 65 536 draws."""
    W = 256
    n = np.arange(W * W)
    u0 = oracle.rng_uniform_cell(0, 3, n).astype(np.float64)
    u1 = oracle.rng_uniform_cell(0, 4, n).astype(np.float64)
    N = float(u0.size)
    assert abs(u0.mean() - 0.5) < 5.0 / np.sqrt(12.0 * N)
    assert abs(u0.var() - 1.0 / 12.0) < 5.0 * np.sqrt(1.0 / 180.0 / N)
    hist = np.histogram(u0, bins=64, range=(0.0, 1.0))[0]
    chi2 = ((hist - N / 64.0) ** 2 / (N / 64.0)).sum()
    assert chi2 < 63.0 + 5.0 * np.sqrt(2.0 * 63.0)      # chi-square with 63 degrees of freedom
    corr = lambda a, b: float(np.corrcoef(a, b)[0, 1])
    g = u0.reshape(W, W)
    for lag in (1, 2, 3, 4):                              # within a block (lags 1-3) and across blocks
        assert abs(corr(g[:, :-lag].ravel(), g[:, lag:].ravel())) < 5.0 / np.sqrt(N)
    assert abs(corr(g[:-1].ravel(), g[1:].ravel())) < 5.0 / np.sqrt(N)       # the cell below
    assert abs(corr(g[:-1, :-1].ravel(), g[1:, 1:].ravel())) < 5.0 / np.sqrt(N)
    assert abs(corr(u0, u1)) < 5.0 / np.sqrt(N)           # two realisations of one cell
    # the words of one block, pairwise
    b = u0.reshape(-1, 4)
    for i in range(4):
        for j in range(i + 1, 4):
            assert abs(corr(b[:, i], b[:, j])) < 5.0 / np.sqrt(N / 4.0)


def test_expf_within_one_ulp_of_libm(oracle):
    xs = np.concatenate([np.linspace(-87, 88, 20001), np.linspace(-1, 1, 2001)]).astype(np.float32)
    mine = oracle.expf(xs).astype(np.float64)
    ref = np.exp(xs.astype(np.float64))
    ulp = np.abs(mine - ref) / np.spacing(ref.astype(np.float32)).astype(np.float64)
    assert ulp.max() < 1.0
    assert oracle.expf(np.float32(0.0)) == 1.0
    assert oracle.expf(np.float32(-90.0)) == 0.0      # flush below e^-87
    assert np.isinf(oracle.expf(np.float32(89.0)))
    assert np.isnan(oracle.expf(np.float32(np.nan)))


def test_powf_is_exp2_y_log2_x(oracle):
    r = np.random.default_rng(0)
    x = r.uniform(1e-6, 50, 5000).astype(np.float32)
    y = r.uniform(0.01, 3, 5000).astype(np.float32)
    mine = oracle.powf(x, y).astype(np.float64)
    ref = np.power(x.astype(np.float64), y.astype(np.float64))
    assert (np.abs(mine - ref) / ref).max() < 5e-6    # the error budget of CUDA's __powf
    assert oracle.powf(0.0, 2.0) == 0.0
    assert oracle.powf(1.0, 1.414) == 1.0
    assert np.isnan(oracle.powf(0.0, 0.0))            # exp2(0 * -inf), as the intrinsic


# ------------------------------------------------------- map helpers

def test_stepsize_bounds_and_ieee_edges(oracle):
    r = np.random.default_rng(1)
    for _ in range(2000):
        px, py = r.uniform(0, 50, 2)
        a = r.uniform(0, 2 * math.pi)
        s = oracle.stepsize(px, py, math.cos(a), math.sin(a))
        assert 0 < s <= 1.41421354 + 1e-6              # erosion_map.cu:61-76
    # axis-aligned direction: division by zero must resolve to sqrt(2) via fmaxf/fminf
    s = oracle.stepsize(3.25, 7.5, 1.0, 0.0)
    assert s == pytest.approx(0.5 * (0.75 + 1.41421354))
    # NaN direction (the solve_uniform OOB case): both axes clamp to sqrt(2)
    assert oracle.stepsize(1.5, 1.5, float("nan"), float("nan")) == pytest.approx(1.41421354)


def test_glocal_ramp_and_boundary(oracle):
    H, W = 8, 9
    layers = np.zeros((H, W, 2), np.float32)
    layers[..., 0] = (2.0 * np.arange(H)[:, None] + 0.0 * np.arange(W)[None, :]).astype(np.float32)
    scale = (0.5, 0.25, 4.0)
    ex = 0.02
    g = oracle.glocal(layers, 4, 4, scale, ex)
    # uphill toward +x: only the downhill (negative-x) side survives: (h - h(x-1)) * sz / sx
    assert g[0] == pytest.approx(2.0 * 4.0 / 0.5) and g[1] == 0.0
    # x = 0: the missing -x neighbour contributes +exitSlope; the +x side is uphill (clamped to 0)
    assert oracle.glocal(layers, 0, 4, scale, ex)[0] == pytest.approx(ex)
    # last row: -x side downhill slope 16 beats the -exitSlope of the missing +x neighbour
    assert oracle.glocal(layers, H - 1, 4, scale, ex)[0] == pytest.approx(16.0)
    # y borders on a field flat in y: +exitSlope at y=0 wins first (strict >), so gy = +ex;
    # at y = W-1 the n side is 0 and the p side is -ex
    assert oracle.glocal(layers, 4, 0, scale, ex)[1] == pytest.approx(ex)
    assert oracle.glocal(layers, 4, W - 1, scale, ex)[1] == pytest.approx(-ex)


# ---------------------------------------------------------- cell ops

def test_layer_merge_identity(oracle):
    layers = terrain(oracle, 16, 24, sediment=0.1)
    np.testing.assert_array_equal(oracle.layer_merge(layers), layers[..., 0] + layers[..., 1])


def test_mass_creep_conserves_sediment(oracle):
    H, W = 32, 40
    layers = terrain(oracle, H, W, sediment=0.05)
    p = oracle.default_param()
    p.critSlopeSediment = 0.01
    scale = (20.0 / H, 20.0 / W, 4.0)
    delta = np.zeros((H, W, 2), np.float32)
    oracle.mass_creep(delta, layers, scale, p)
    assert (delta[..., 0] == 0).all()                  # only delta.y is touched (erosion.cu:708)
    assert np.abs(delta[..., 1]).max() > 0
    # symmetric exchange (erosion.cu:675-706): what one cell loses its neighbour gains
    assert abs(delta[..., 1].astype(np.float64).sum()) < 1e-6 * np.abs(delta[..., 1]).sum() + 1e-9
    # never takes more than the sediment that is there
    assert (layers[..., 1] + delta[..., 1] >= -1e-7).all()


def test_mass_creep_flat_is_zero(oracle):
    layers = np.zeros((8, 8, 2), np.float32)
    layers[..., 0] = 1.0
    layers[..., 1] = 0.5
    delta = np.zeros_like(layers)
    oracle.mass_creep(delta, layers, (1, 1, 1), oracle.default_param())
    assert (delta == 0).all()


def test_mass_transfer_limits(oracle):
    H, W = 24, 24
    layers = terrain(oracle, H, W, sediment=0.02)
    p = oracle.default_param()
    scale = (20.0 / H, 20.0 / W, 4.0)
    r = np.random.default_rng(5)
    uplift = r.random((H, W)).astype(np.float32)
    mass = (r.random((H, W)) * 10).astype(np.float32)
    vel = (r.standard_normal((H, W, 2)) * 5).astype(np.float32)
    debris = (r.random((H, W)) * 3).astype(np.float32)
    delta = np.zeros((H, W, 2), np.float32)
    oracle.mass_transfer(delta, layers, uplift, mass, vel, debris, None, None, None, None, scale, p)
    L = math.hypot(scale[0], scale[1])
    total = (delta[..., 0] + delta[..., 1]) * scale[2] - p.timeStep * p.uplift * uplift
    assert (total <= 0.25 * L * 0.3 * (1 + 1e-5) + 1e-6).all()     # deposition limit, erosion.cu:528
    slope = np.array([[np.hypot(*oracle.glocal(layers, x, y, scale, p.exitSlope))
                       for y in range(W)] for x in range(H)])
    assert (total >= -0.25 * L * slope * (1 + 1e-5) - 1e-6).all()  # suspension limit, :527
    # sediment is consumed before bedrock (:535-545)
    assert (layers[..., 1] + delta[..., 1] >= -1e-6).all()


def test_normalize_fluvial_zero_flux(oracle):
    """With no flux, fields reduce to their source terms (erosion.cu:173-179)."""
    H, W = 12, 10
    layers = np.zeros((H, W, 2), np.float32)
    layers[..., 0] = np.arange(H, dtype=np.float32)[:, None] * 0.1
    p = oracle.default_param()
    scale = (2.0, 3.0, 1.0)
    z1 = np.zeros((H, W), np.float32)
    z2 = np.zeros((H, W, 2), np.float32)
    rain = np.full((H, W), 0.5, np.float32)
    wh, m, v = z1.copy(), z1.copy(), z2.copy()
    oracle.normalize_fluvial(z1, z1, z2, None, layers, rain, wh, m, v, None, scale, p)
    A = scale[0] * scale[1]
    np.testing.assert_allclose(wh, A * p.rainfall * 0.5 / scale[1], rtol=1e-6)
    assert (m == 0).all()
    g = oracle.glocal(layers, 5, 5, scale, p.exitSlope)
    np.testing.assert_allclose(v[5, 5], A * (-p.gravity * g) / scale[1], rtol=1e-6)


# ------------------------------------------------------------- graph

@pytest.mark.parametrize("edge", [D4, D8])
def test_steepest_on_ramp_and_flat(oracle, edge):
    H, W = 9, 7
    ramp = (np.arange(H, dtype=np.float32)[:, None] + np.zeros((1, W), np.float32))
    g = oracle.steepest(ramp, edge)
    d = oracle.direction(ramp, edge)
    assert (g[0] == -1).all() and (d[0] == -1).all()          # lowest row: no receiver -> -1
    n = np.arange(H * W).reshape(H, W)
    np.testing.assert_array_equal(g[1:], n[:-1])              # receiver = cell directly downhill
    assert (d[1:] == 0).all()                                 # direction k=0 is (-1, 0), graph.hpp:24
    flat = np.ones((H, W), np.float32)
    assert (oracle.steepest(flat, edge) == -1).all()          # graph.cu:43,64-68
    assert (oracle.random_weighted(flat, edge, 0, 0, 10.0) == -1).all()   # Z = 0, graph.cu:160


def test_d8_prefers_steeper_diagonal(oracle):
    h = np.zeros((3, 3), np.float32) + 10
    h[1, 1] = 20
    h[0, 0] = 0            # diagonal drop 20/sqrt(2) = 14.1 > axis drop 10
    assert oracle.steepest(h, D8)[1, 1] == 0
    assert oracle.direction(h, D8)[1, 1] == 4                 # (-1,-1) is k=4, graph.hpp:40
    assert oracle.steepest(h, D4)[1, 1] == 1                  # first axis neighbour in table order


def test_random_weighted_is_downhill_and_seeded(oracle):
    h = terrain(oracle, 32, 32)[..., 0].copy()
    a = oracle.random_weighted(h, D8, 0, 3, 10.0)
    b = oracle.random_weighted(h, D8, 0, 3, 10.0)
    c = oracle.random_weighted(h, D8, 0, 4, 10.0)
    np.testing.assert_array_equal(a, b)
    assert (a != c).any()
    flat = h.ravel()
    idx = np.nonzero(a.ravel() >= 0)[0]
    assert (flat[a.ravel()[idx]] < flat[idx]).all()           # only downhill receivers, graph.cu:139


@pytest.mark.parametrize("edge", [D4, D8])
def test_accumulate_counts_upstream_cells(oracle, edge):
    H, W = 12, 9
    ramp = (np.arange(H, dtype=np.float32)[:, None] + np.zeros((1, W), np.float32))
    g = oracle.steepest(ramp, edge)
    acc = oracle.accumulate(g, np.ones((H, W), np.float32), edge)
    # each column drains straight down: value = number of cells upstream incl. self
    expect = (H - np.arange(H))[:, None] + np.zeros((1, W))
    np.testing.assert_array_equal(acc, expect.astype(np.float32))


def test_accumulate_total_at_outlets(oracle):
    h = terrain(oracle, 40, 40)[..., 0].copy()
    g = oracle.steepest(h, D8)
    acc = oracle.accumulate(g, np.ones_like(h), D8)
    outlets = g < 0
    assert acc[outlets].sum() == h.size                       # every cell drains to exactly one outlet
    # brute-force upstream count for comparison
    order = np.argsort(-h.ravel(), kind="stable")
    val = np.ones(h.size, np.float64)
    gf = g.ravel()
    for n in order:
        if gf[n] >= 0:
            val[gf[n]] += val[n]
    np.testing.assert_array_equal(acc.ravel(), val.astype(np.float32))


def test_accumulate_decay_chain(oracle):
    H, W = 6, 1
    ramp = np.arange(H, dtype=np.float32)[:, None].copy()
    g = oracle.steepest(ramp, D4)
    decay = np.full((H, W), 0.5, np.float32)
    acc = oracle.accumulate(g, np.ones((H, W), np.float32), D4, decay=decay)
    # value[n] = 1 + 0.5 * value[n+1]  (graph.cu:478-494 with per-edge decay)
    expect = np.zeros(H)
    for n in range(H - 1, -1, -1):
        expect[n] = 1 + (0.5 * expect[n + 1] if n + 1 < H else 0)
    np.testing.assert_allclose(acc[:, 0], expect, rtol=1e-6)


def test_slope_along_graph(oracle):
    H, W = 6, 6
    ramp = (3.0 * np.arange(H, dtype=np.float32)[:, None] + np.zeros((1, W), np.float32))
    g = oracle.steepest(ramp, D8)
    s = oracle.slope(ramp, g, (2.0, 5.0))
    assert (s[0] == 0).all()                                   # no receiver -> 0, graph.cu:283
    np.testing.assert_allclose(s[1:], -3.0 / 2.0)


# ----------------------------------------------------------- stencils

def test_gradient_of_plane(oracle):
    H, W = 10, 12
    x, y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = (1.5 * x - 0.75 * y).astype(np.float32)
    g = oracle.gradient(f, (0.5, 0.25))
    np.testing.assert_allclose(g[..., 0], 1.5 / 0.5)           # one-sided fallback at borders too
    np.testing.assert_allclose(g[..., 1], -0.75 / 0.25)
    assert (oracle.gradient(np.ones((1, 1), np.float32), (1, 1)) == 0).all()  # isolated cell -> 0


def test_negslope_of_plane(oracle):
    H, W = 8, 8
    x, y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = (2.0 * x + 1.0 * y).astype(np.float32)
    s = oracle.negslope(f, (1.0, 1.0))
    assert s[0, 0] == 0                                        # the pit has no downhill neighbour
    assert s[4, 4] == pytest.approx(math.hypot(2.0, 1.0))


def test_laplacian_of_quadratic(oracle):
    H, W = 12, 12
    x, y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = (x * x + 2 * y * y).astype(np.float32)[..., None].copy()
    lap = oracle.laplacian(f, (1.0, 1.0))
    # LH = 2 + 4 = 6; LD = 0.5[(2+4)+(2+4)]... per grad.cu:178-181 the interior value is 0.5*6 + 0.5*6
    assert lap[5, 5, 0] == pytest.approx(6.0)
    const = np.full((6, 6, 2), 3.0, np.float32)
    assert (oracle.laplacian(const, (1, 1)) == 0).all()


def test_blur_of_constant_is_sum_of_weights(oracle):
    sigma = 4.0
    k = np.arange(-16, 17, dtype=np.float64)
    wsum = (np.exp(-0.5 * (k / sigma) ** 2) / (math.sqrt(2 * 3.14159265) * sigma)).sum()
    c = np.full((40, 40, 1), 2.0, np.float32)
    out = oracle.gaussian_blur(c, sigma)
    np.testing.assert_allclose(out, 2.0 * wsum * wsum, rtol=1e-5)   # un-normalised, filter.cu:47-50


def test_normal_of_plane(oracle):
    H, W = 9, 9
    x, y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = (0.5 * x + 0.25 * y).astype(np.float32)
    n = oracle.normal(f, (1.0, 1.0, 2.0))
    v = np.array([-1.0, -0.5, 1.0])
    np.testing.assert_allclose(n[4, 4], v / np.linalg.norm(v), rtol=1e-6)
    np.testing.assert_allclose(np.linalg.norm(n, axis=-1), 1.0, rtol=1e-6)


# ----------------------------------------------------- particle kernels

def _particle_inputs(oracle, H, W):
    layers = terrain(oracle, H, W, sediment=0.01)
    z1 = np.zeros((H, W), np.float32)
    z2 = np.zeros((H, W, 2), np.float32)
    return layers, z1, z2


def test_fluvial_particles_deposit_only_downstream(oracle):
    H = W = 48
    layers, z1, z2 = _particle_inputs(oracle, H, W)
    p = oracle.default_param()
    p.maxage = 64
    scale = (20.0 / H, 20.0 / W, 4.0)
    N = 2000
    rng = oracle.rng_seed(N, 0, 0)
    wf, mf, vf = z1.copy(), z1.copy(), z2.copy()
    rain = np.ones((H, W), np.float32)
    steps = oracle.particles_fluvial(wf, mf, vf, None, rng, layers, rain, z1, z2, None, scale, p)
    assert (rng["offset"] == 2).all()                # two draws per particle (erosion.cu:57-58)
    assert 0 < steps <= N * (p.maxage - 1)           # ++iter < maxage (Appendix B7)
    # Reference quirk, restated: with a zero velocity field every particle spawned on a
    # pit cell (grad = 0) has speed 0/sqrt(0) = NaN (erosion.cu:77-79), is never "oob", and
    # dumps NaN into cell (0,0) (CUDA converts NaN -> 0 when flattening the position).
    assert np.isnan(wf[0, 0])
    rest = wf.ravel()[1:]
    assert (rest >= 0).all() and rest.sum() > 0
    assert (mf.ravel()[1:] == 0).all()               # zero velocity field -> shear 0 -> no suspension
    # the same call again continues the stream: different spawn points, different flux
    wf2 = z1.copy()
    oracle.particles_fluvial(wf2, z1.copy(), z2.copy(), None, rng, layers, rain, z1, z2, None,
                             scale, p)
    assert (rng["offset"] == 4).all() and (wf2 != wf).any()


def test_slab_particles_partition_exactly(oracle):
    """Two slabs that each own half of the rows trace every particle exactly once."""
    H = W = 40
    layers, z1, z2 = _particle_inputs(oracle, H, W)
    p = oracle.default_param()
    p.maxage = 8                                     # short walks: ghost zone of 14 rows suffices
    scale = (20.0 / H, 20.0 / W, 4.0)
    N = 3000
    rain = np.ones((H, W), np.float32)
    full = z1.copy()
    oracle.particles_fluvial(full, z1.copy(), z2.copy(), None, oracle.rng_seed(N, 1, 0), layers,
                             rain, z1, z2, None, scale, p)
    G = 14
    parts = np.zeros((H, W), np.float64)
    for (x0, rows, r0, r1) in [(0, 20 + G, 0, 20), (20 - G, 20 + G, G, 20 + G)]:
        dom = oracle.domain(H, W, x0, rows, r0, r1)
        sl = slice(x0, x0 + rows)
        wf = np.zeros((rows, W), np.float32)
        oracle.particles_fluvial(wf, np.zeros((rows, W), np.float32),
                                 np.zeros((rows, W, 2), np.float32), None,
                                 oracle.rng_seed(N, 1, 0), np.ascontiguousarray(layers[sl]),
                                 np.ascontiguousarray(rain[sl]), np.zeros((rows, W), np.float32),
                                 np.zeros((rows, W, 2), np.float32), None, scale, p, dom=dom)
        parts[sl] += wf
    # cell (0,0) collects the NaN walkers (see above); a slab that does not hold global
    # row 0 has to drop its own, so that one cell is compared for NaN-ness only
    assert np.isnan(full[0, 0])
    np.testing.assert_allclose(parts.ravel()[1:], full.ravel()[1:], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("seed,start", [(0, 0), (7, 2 ** 32 - 1), (2 ** 64 - 1, 2 ** 32 - 1), (2 ** 63 + 11, 2 ** 32 - 2),
                                        (2 ** 32 + 5, 2 ** 42 + 3)])
def test_fluvial_launch_leaves_every_stream_two_draws_on(oracle, seed, start):
    """The batched step (include/soil_hip.h, soil_particles_batch) starts its debris launch from fresh streams at
    offset + 2; the oracle's debris launch continues the fluvial launch's streams.  The two agree because the
    fluvial launch takes exactly two draws of every stream: offsets start + 2 afterwards, across the 32-bit carry
    of the offset and with a 64-bit seed, and a debris launch from the continued streams equals one from fresh
    streams at start + 2 bit for bit (its planes and its step count)."""
    H, W, N = 40, 52, 700
    layers = terrain(oracle, H, W, sediment=0.01)
    r = np.random.default_rng(17)
    vel = (r.standard_normal((H, W, 2)) * 0.5).astype(np.float32)
    rain = np.ones((H, W), np.float32)
    p = oracle.default_param()
    p.maxage = 48
    p.critSlopeBedrock = 0.05                        # landslides on the synthetic terrain
    p.yieldStress = 0.001
    scale = (20.0 / H, 20.0 / W, 4.0)
    z1, z2 = np.zeros((H, W), np.float32), np.zeros((H, W, 2), np.float32)
    rng = oracle.rng_seed(N, seed, start)
    oracle.particles_fluvial(z1.copy(), z1.copy(), z2.copy(), None, rng, layers, rain, z1.copy(), vel.copy(), None,
                             scale, p)
    assert (rng["seed"] == seed).all()
    assert (rng["offset"] == start + 2).all(), np.unique(rng["offset"])
    out = []
    for streams in (rng, oracle.rng_seed(N, seed, start + 2)):
        mf, vf = z1.copy(), z2.copy()
        steps = oracle.particles_debris(mf, vf, None, streams, layers, vel.copy(), None, scale, p)
        out.append((steps, mf, vf))
    (steps_a, mf_a, vf_a), (steps_b, mf_b, vf_b) = out
    assert steps_a == steps_b > N and np.nanmax(mf_a) > 0
    assert np.array_equal(mf_a, mf_b, equal_nan=True) and np.array_equal(vf_a, vf_b, equal_nan=True)
    # the seed's high word and the offset's take part: another high word, other walks
    other = oracle.rng_seed(N, seed ^ (1 << 40), start + 2)
    mf_c = z1.copy()
    oracle.particles_debris(mf_c, z2.copy(), None, other, layers, vel.copy(), None, scale, p)
    assert not np.array_equal(mf_c, mf_a, equal_nan=True)


# ------------------------------------------------ build-defined operators (no reference definition)

def test_fill_depressions_known_answers(oracle):
    """Priority-flood surface: a bowl fills to its lowest rim, a NaN cell drains its
    neighbours like the grid border does, ramps and already drained terrain are untouched."""
    bowl = np.full((7, 7), 10.0, np.float32)
    bowl[1:-1, 1:-1] = 5.0
    bowl[3, 3] = 1.0
    bowl[0, 3] = 7.0                                   # the lowest point of the rim
    for edge in (0, 1):
        w = oracle.fill_depressions(bowl, edge)
        assert (w[1:-1, 1:-1] == 7.0).all() and w[0, 3] == 7.0 and w[0, 0] == 10.0
    # D8 reaches a diagonal gap in the rim that D4 cannot use
    gap = np.full((5, 5), 9.0, np.float32)
    gap[1:-1, 1:-1] = 2.0
    gap[0, 0] = 3.0
    assert oracle.fill_depressions(gap, 1)[2, 2] == 3.0
    assert oracle.fill_depressions(gap, 0)[2, 2] == 9.0
    hole = bowl.copy()
    hole[3, 4] = np.nan                                # NoData inside the bowl: an outlet
    w = oracle.fill_depressions(hole, 1)
    assert np.isnan(w[3, 4]) and w[3, 3] == 1.0 and w[2, 2] == 5.0
    ramp = np.add.outer(np.arange(6, dtype=np.float32), np.arange(9, dtype=np.float32))
    np.testing.assert_array_equal(oracle.fill_depressions(ramp, 1), ramp)
    r = np.random.default_rng(0)
    rough = r.standard_normal((40, 30)).astype(np.float32)
    w = oracle.fill_depressions(rough, 1)
    np.testing.assert_array_equal(oracle.fill_depressions(w, 1), w)          # idempotent
    assert (w >= rough).all()


def test_resize_known_answers(oracle):
    """Bilinear resampling at corner-aligned positions: identity at equal size, corners kept,
    a linear ramp stays linear, constants stay constant, channels are independent."""
    r = np.random.default_rng(1)
    src = r.standard_normal((9, 13)).astype(np.float32)
    np.testing.assert_array_equal(oracle.resize(src, (9, 13)), src)
    up = oracle.resize(src, (17, 25))                  # every other sample is an original one
    np.testing.assert_array_equal(up[::2, ::2], src)
    np.testing.assert_allclose(up[1::2, ::2], 0.5 * (src[:-1] + src[1:]), rtol=1e-6, atol=1e-7)
    for corner in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        assert up[corner] == src[corner]
    ramp = np.add.outer(2.0 * np.arange(5, dtype=np.float32), np.arange(8, dtype=np.float32))
    big = oracle.resize(ramp, (33, 50))
    want = np.add.outer(np.linspace(0, 8, 33), np.linspace(0, 7, 50))
    np.testing.assert_allclose(big, want, rtol=1e-5, atol=1e-5)
    assert (oracle.resize(np.full((4, 6), 2.5, np.float32), (11, 3)) == 2.5).all()
    two = r.standard_normal((6, 7, 2)).astype(np.float32)
    got = oracle.resize(two, (10, 12))
    for c in range(2):
        np.testing.assert_array_equal(got[..., c], oracle.resize(np.ascontiguousarray(two[..., c]), (10, 12)))
    assert oracle.resize(src, (1, 1))[0, 0] == src[0, 0]


# ------------------------------------------------------------ accumulate on built graphs
# What tests/test_gpu_accumulate_oracle.py leans on, pinned on the oracle alone.

def _outlets_sum(acc, g):
    return float(acc[g < 0].astype(np.float64).sum())


@pytest.mark.parametrize("H,W,edge", [(64, 64, D4), (64, 64, D8), (37, 53, D4), (37, 53, D8), (301, 257, D8),
                                      (1, 300, D8), (300, 1, D4), (1024, 1024, D8)])
def test_accumulate_snake_ends_with_every_cell_at_its_outlet(oracle, H, W, edge):
    """One chain through all H W cells: the round count 2 (ceil(log2(HW) / 2) + 1) is just enough for it."""
    from util import graph_snake
    g = graph_snake(H, W)
    assert (g < 0).sum() == 1
    acc = oracle.accumulate(g, np.ones((H, W), np.float32), edge)
    assert acc[g < 0][0] == H * W
    # and along the chain the area grows by one per cell
    order = np.empty(H * W, np.int64)
    n = 0
    for i in range(H * W):
        order[i] = n
        n = int(g.reshape(-1)[n])
    assert n == -1
    assert (acc.reshape(-1)[order] == np.arange(1, H * W + 1)).all()


@pytest.mark.parametrize("H,W", [(64, 64), (37, 53), (1, 300), (300, 1), (2, 40), (5, 1028)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_accumulate_built_graphs_drain_every_cell(oracle, H, W, edge):
    from util import built_graphs
    K = 4 if edge == D4 else 8
    ones = np.ones((H, W), np.float32)
    for name, g in built_graphs(H, W, edge).items():
        acc = oracle.accumulate(g, ones, edge)
        if name == "no_edges":
            assert (acc == 1).all()
        else:
            assert _outlets_sum(acc, g) == H * W, name
    if H >= 3 and W >= 3:
        g = built_graphs(H, W, edge)["fan"]
        acc = oracle.accumulate(g, ones, edge)
        assert acc[1, 1] == 9 and g[1, 1] == -1          # a cell with all K donors (D4: 4 + the corners behind them)
        idx = np.arange(H * W).reshape(H, W)
        assert (g == idx[1, 1]).sum() == K
        if W >= 6:
            gc = built_graphs(H, W, edge)["fan_chain"]
            assert (gc == idx[1, 4]).sum() == K - 1 and gc[1, 4] == idx[1, 5]   # K - 1 donors, on a chain


@pytest.mark.parametrize("edge", [D4, D8])
def test_accumulate_is_repeatable_and_finite_on_cycles_and_wild_graphs(oracle, edge):
    from util import graph_cycles, graph_wild
    H, W = 40, 52
    h = terrain(oracle, H, W)[..., 0].copy()
    base = oracle.random_weighted(h, edge, 0, 1, 10.0)
    r = np.random.default_rng(4)
    src = (0.5 + r.random((H, W))).astype(np.float32)
    decay = (0.8 + 0.2 * r.random((H, W))).astype(np.float32)
    for g in (graph_cycles(base), graph_wild(base)):
        assert (g != base).any()
        for d in (None, decay):
            a = oracle.accumulate(g, src, edge, decay=d)
            b = oracle.accumulate(g.copy(), src.copy(), edge, decay=None if d is None else d.copy())
            assert np.isfinite(a).all()
            assert (a.view(np.uint32) == b.view(np.uint32)).all()
    cyc = graph_cycles(base)
    idx = np.arange(H * W).reshape(H, W)
    two = (cyc.reshape(-1)[np.clip(cyc, 0, None)] == idx) & (cyc >= 0)
    assert two.sum() >= 2                                  # there are cells that point at each other
    # a cell on a cycle never finishes: it keeps collecting, so it ends above what the same cell holds without
    assert (oracle.accumulate(cyc, src, edge)[two] > src[two]).all()


@pytest.mark.parametrize("edge", [D4, D8])
def test_accumulate_of_stacked_tiles_is_the_tiles_accumulations_stacked(oracle, edge):
    """The stacking rule: T tiles one under the other, tile t's graph shifted by t h W.  A graph never drains across
    a tile border, a round is local to a connected component and a finished cell no longer changes, so the
    accumulation of the stack is the tiles' own accumulations stacked — provided every tile has finished within its
    own (smaller) round count: with unit sources its outlets then hold h W."""
    from util import stack_graphs
    T, h, W = 8, 64, 256
    graphs, srcs, decays, accs, accs_d = [], [], [], [], []
    for t in range(T):
        dem = terrain(oracle, h, W, seed=3.0 + t)[..., 0].copy()
        g = oracle.random_weighted(dem, edge, 1, t, 10.0)
        r = np.random.default_rng(100 + t)
        s = (0.5 + r.random((h, W))).astype(np.float32)
        d = (0.8 + 0.2 * r.random((h, W))).astype(np.float32)
        assert _outlets_sum(oracle.accumulate(g, np.ones((h, W), np.float32), edge), g) == h * W
        graphs.append(g), srcs.append(s), decays.append(d)
        accs.append(oracle.accumulate(g, s, edge))
        accs_d.append(oracle.accumulate(g, s, edge, decay=d))
    assert any((graphs[0] != g).any() for g in graphs[1:])
    G, S, D = stack_graphs(graphs), np.concatenate(srcs), np.concatenate(decays)
    assert G.shape == (T * h, W) and G.max() >= (T - 1) * h * W
    from util import assert_bit_equal
    assert_bit_equal(oracle.accumulate(G, S, edge), np.concatenate(accs), "stack, no decay")
    assert_bit_equal(oracle.accumulate(G, S, edge, decay=D), np.concatenate(accs_d), "stack, decay tensor")
