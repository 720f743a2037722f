"""The coloured erosion step (include/soil_hip.h: soil_colour_planes, soil_erode_cells_fused_colour,
soil_particles_pair_colour, soil_erode_step_colour; ErosionModel(colour=True)) against the oracle's
composition of the reference ops with their albedo arguments (erosion.cu:29-141, :143-187, :245-393,
:453-574, :633-757):

  * the fused colour cell kernel bit for bit, every output plane, both flags, a row sub-range;
  * both colour particle launches against the oracle's walks (forced: the same terrain on both sides),
    spent debris walkers retired (mode 1) and walked to the end (mode 0);
  * whole coloured steps, forced and free-running, and the step driver against step_unfused();
  * the edges of the retirement argument with colour: non-finite spawn colours are never retired.
"""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_oracle_fullsize import _flux_close
from test_gpu_parity import SIZES, _cell_inputs, _close_but_for_stray_walks
from util import assert_bit_equal, product_param, retired_steps_close, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

COLOUR = ("albedoBedrock", "albedoSurface", "albedoFluvial", "albedoDebris")


@pytest.fixture
def retire(hip):
    """Sets the debris retirement mode for one test; the suite's mode (watched) afterwards."""
    from soillib_amd import soil
    before = soil.debris_retire()
    yield soil.debris_retire
    soil.debris_retire(before)
    hip.soil_set_particle_mode(0)


def _colour_inputs(H, W, seed):
    """Colour flux planes with cells of |a| == 0, colours in [0, 1.3) (fminf(.., 1) bites)."""
    r = np.random.default_rng(seed)
    c3 = lambda s: (r.random((H, W, 3)) * s).astype(np.float32)
    a_fl, a_db = c3(4.0), c3(2.0)
    a_fl[r.random((H, W)) < 0.2] = 0.0
    a_db[r.random((H, W)) < 0.2] = 0.0
    return dict(albedoBedrock=c3(1.3), albedoSurface=c3(1.3), albedoFluvial=a_fl, albedoDebris=a_db)


def _oracle_colour_cells(oracle, layers, uplift, rain, wf, mf, vf, df, dvf, col, scale, op):
    """normalize_fluvial -> normalize_debris -> delta = 0 -> mass_transfer -> mass_creep -> add -> layer_merge,
    with the colour planes (the contract of soil_colour_planes, steps 5-9)."""
    H, W = layers.shape[:2]
    z1 = lambda: np.zeros((H, W), np.float32)
    z2 = lambda: np.zeros((H, W, 2), np.float32)
    wh, m, v, d, dv = z1(), z1(), z2(), z1(), z2()
    af, ad, surf = col["albedoFluvial"].copy(), col["albedoDebris"].copy(), col["albedoSurface"].copy()
    oracle.normalize_fluvial(wf, mf, vf, af, layers, rain, wh, m, v, surf, scale, op)
    oracle.normalize_debris(df, dvf, ad, layers, d, dv, surf, scale, op)
    delta = z2()
    oracle.mass_transfer(delta, layers, uplift, m, v, d, col["albedoBedrock"], af, ad, surf, scale, op)
    oracle.mass_creep(delta, layers, scale, op)
    layers_next = layers + delta
    return dict(layers_next=layers_next, height=layers_next[..., 0] + layers_next[..., 1], waterHeight=wh,
                mass=m, velocity=v, debris=d, debrisVelocity=dv, albedoFluvial=af, albedoDebris=ad,
                albedoSurface=surf)


def _planes(g):
    from soillib_amd import _abi
    planes = _abi.ErosionPlanes()
    for name in _abi._PLANES:
        setattr(planes, name, g[name].ptr)
    colour = _abi.ColourPlanes()
    for field, name in zip(_abi.COLOUR_PLANES, COLOUR):
        setattr(colour, field, g[name].ptr)
    return planes, colour


# ---------------------------------------------------------------- the colour cell kernel

CELL_SHAPES = SIZES + [(256, 256), (8, 4), (1, 8), (5, 1), (1024, 512), (40, 36), (3, 7)]


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("H,W,rows", [(h, w, None) for h, w in CELL_SHAPES] + [(96, 64, (17, 70)), (37, 53, (5, 6))])
def test_colour_cells_bit_exact(hip, oracle, H, W, rows, keep):
    """soil_erode_cells_fused_colour == the oracle's ops one after another, bit for bit, on every output plane."""
    from soillib_amd import _abi
    seed = H * 1000 + W
    inp = _cell_inputs(oracle, H, W, seed=seed)
    r = np.random.default_rng(seed + 1)
    inp["layers"][r.random((H, W)) < 0.3, 1] = 0.0        # layer.y == 0: the bedrock colour (erosion.cu:558)
    inp["layers"][0, 0, 1] = 0.0
    inp["massFlux"][r.random((H, W)) < 0.15] = 0.0        # m == 0: the source colour (:181)
    inp["debrisFlux"][r.random((H, W)) < 0.15] = 0.0
    col = _colour_inputs(H, W, seed + 2)
    op = script_param(oracle.default_param())
    pp = product_param(op)
    scale = (20.0 / H, 20.0 / W, 4.0)
    want = _oracle_colour_cells(oracle, inp["layers"], inp["uplift"], inp["rainfall"], inp["waterFlux"],
                                inp["massFlux"], inp["velocityFlux"], inp["debrisFlux"], inp["debrisVelocityFlux"],
                                col, scale, op)
    # the bedrock branch (:558-559) is taken, and on grids of some size the mix branch (:560-571) too
    assert (want["albedoSurface"] == col["albedoBedrock"]).any()
    if H * W >= 256:
        mixed = (want["albedoSurface"] != col["albedoSurface"]) & (want["albedoSurface"] != col["albedoBedrock"])
        assert mixed.any()
    g = {k: to_gpu(v) for k, v in list(inp.items()) + list(col.items())}
    out1 = lambda: np.full((H, W), np.nan, np.float32)
    out2 = lambda: np.full((H, W, 2), np.nan, np.float32)
    before = dict(layers_next=out2(), height=out1(), waterHeight=out1(), mass=out1(), velocity=out2(),
                  debris=out1(), debrisVelocity=out2())
    g.update({k: to_gpu(v) for k, v in before.items()})
    planes, colour = _planes(g)
    r0, r1 = rows if rows else (0, H)
    dom = _abi.Domain(H, W, 0, H, r0, r1)
    _abi.check(hip.soil_erode_cells_fused_colour(C.byref(planes), C.byref(colour), C.byref(dom), _abi.vec(scale, 3),
                                                 pp._ref(), _abi.SOIL_CELLS_KEEP_FLUX if keep else 0, None))
    inside = slice(r0, r1)
    outside = np.ones(H, bool)
    outside[inside] = False
    for name in ("layers_next", "height", "waterHeight", "mass", "velocity", "debris", "debrisVelocity",
                 "albedoFluvial", "albedoDebris", "albedoSurface"):
        got = to_np(g[name])
        assert_bit_equal(got[inside], want[name][inside], "colour cells " + name)
        untouched = before[name] if name in before else col[name]
        assert_bit_equal(got[outside], untouched[outside], "rows outside the range " + name)
    for name in ("waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux"):
        got = to_np(g[name])
        if keep:
            assert_bit_equal(got, inp[name], name + " kept")
        else:
            assert (got[inside] == 0).all(), name + " not re-zeroed"
            assert_bit_equal(got[outside], inp[name][outside], name + " outside the range")
    assert_bit_equal(to_np(g["albedoBedrock"]), col["albedoBedrock"], "albedo_bedrock is input only")
    assert_bit_equal(to_np(g["layers"]), inp["layers"], "input layers untouched")


def test_colour_entry_points_want_every_colour_plane(hip, oracle):
    from soillib_amd import _abi, silt
    H = W = 16
    t = lambda *s: silt.tensor(silt.float32, silt.shape(*s), silt.gpu)
    g = {name: t(H, W, 2) for name in _abi._PLANES}
    g.update({name: t(H, W, 3) for name in COLOUR})
    planes, colour = _planes(g)
    colour.albedo_debris = None
    dom = _abi.Domain(H, W, 0, H, 0, H)
    p = product_param(script_param(oracle.default_param()))
    rng = silt.tensor(silt.rng, silt.shape(64), silt.gpu)
    rng2 = silt.tensor(silt.rng, silt.shape(64), silt.gpu)
    assert hip.soil_erode_cells_fused_colour(C.byref(planes), C.byref(colour), C.byref(dom), _abi.vec((1, 1, 1), 3),
                                             p._ref(), 0, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert b"colour plane" in hip.soil_last_error()
    assert hip.soil_particles_pair_colour(C.byref(planes), C.byref(colour), rng.c_ptr, rng2.c_ptr, 64, H, W,
                                          _abi.vec((1, 1, 1), 3), p._ref(), 0, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert hip.soil_erode_step_colour(C.byref(planes), C.byref(colour), rng.c_ptr, 64, 0, 0, H, W,
                                      _abi.vec((1, 1, 1), 3), p._ref(), 0, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert hip.soil_erode_step_colour(C.byref(planes), None, rng.c_ptr, 64, 0, 0, H, W,
                                      _abi.vec((1, 1, 1), 3), p._ref(), 0, None) == _abi.SOIL_ERR_INVALID_ARGUMENT


def test_colour_model_on_a_slab_is_refused(hip):
    from soillib_amd import _abi, soil
    from soillib_amd.erosion import ErosionModel
    with pytest.raises(ValueError):
        ErosionModel(64, 32, (1.0, 1.0, 4.0), soil.param_t(), 256, dom=_abi.Domain(64, 32, 16, 24, 4, 20),
                     colour=True)


# ---------------------------------------------------------------- the particle launches

def _model(H, W, scale, pp, N):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionModel
    m = ErosionModel(H, W, scale, pp, N, seed=0, colour=True)
    silt.set(m.rainfall, 1.0)
    return m


def _colour_state(oracle, H, W, seed=5):
    r = np.random.default_rng(seed)
    z1 = lambda: np.zeros((H, W), np.float32)
    z2 = lambda: np.zeros((H, W, 2), np.float32)
    return dict(layers=terrain(oracle, H, W), wh=z1(), m=z1(), v=z2(), d=z1(), dv=z2(),
                bed=r.random((H, W, 3)).astype(np.float32), surf=r.random((H, W, 3)).astype(np.float32))


STATE_PLANES = (("layers", "layers"), ("waterHeight", "wh"), ("velocity", "v"), ("debrisVelocity", "dv"),
                ("mass", "m"), ("debris", "d"), ("albedoBedrock", "bed"), ("albedoSurface", "surf"))


def _read_state(m):
    return {key: to_np(getattr(m, name)) for name, key in STATE_PLANES}


def _force(m, st, step):
    from soillib_amd import silt
    for name, key in STATE_PLANES:
        silt.set(getattr(m, name), to_gpu(st[key]))
    m.step_index = step


def _oracle_pair(oracle, st, step, N, scale, op, threads):
    """Both colour launches of step `step` on the oracle: planes, colour fluxes, step counts."""
    H, W = st["layers"].shape[:2]
    z1 = lambda: np.zeros((H, W), np.float32)
    z2 = lambda: np.zeros((H, W, 2), np.float32)
    z3 = lambda: np.zeros((H, W, 3), np.float32)
    rain = np.ones((H, W), np.float32)
    rng = oracle.rng_seed(N, 0, step * N)
    o = dict(wf=z1(), mf=z1(), vf=z2(), af=z3(), df=z1(), dvf=z2(), ad=z3())
    o["steps_f"] = oracle.particles_fluvial(o["wf"], o["mf"], o["vf"], o["af"], rng, st["layers"], rain, st["wh"],
                                            st["v"], st["surf"], scale, op, threads=threads)
    o["debris"] = oracle.particles_debris_retire(o["df"], o["dvf"], o["ad"], rng, st["layers"], st["dv"], st["surf"],
                                                 scale, op, threads=threads)
    return o


def _pair_fluxes(m):
    return dict(wf=to_np(m.waterFlux), mf=to_np(m.massFlux), vf=to_np(m.velocityFlux), af=to_np(m.albedoFluvial),
                df=to_np(m.debrisFlux), dvf=to_np(m.debrisVelocityFlux), ad=to_np(m.albedoDebris))


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("H,W,warm", [(1024, 1024, 0), (4096, 512, 2)])
def test_colour_pair_against_the_oracle(hip, oracle, retire, H, W, warm, mode):
    """soil_particles_pair_colour from the oracle's state: the fluvial launch's step count and fluxes, colour
    included; the debris launch's count — mode 1: the oracle's walk under the retirement rule, fewer than the full
    walk (with colour planes the launch used to walk every walker to the end); mode 0: the full walk — and its
    fluxes, colour included."""
    from soillib_amd import soil
    threads = os.cpu_count() or 1
    oracle.set_threads(threads)
    N = H * W // 8
    op = script_param(oracle.default_param())
    pp = product_param(op)
    scale = (20.0 / H, 20.0 / W, 4.0)
    m = _model(H, W, scale, pp, N)
    st = _colour_state(oracle, H, W)
    try:
        if warm:   # let the device carve channels first: the launches start from its state
            _force(m, st, 0)
            for _ in range(warm):
                m.step()
            st = _read_state(m)
        retire(mode)
        _force(m, st, warm)
        m.seed_step()
        soil.particle_steps(reset=True)
        m.particles_pair()
        got_steps = soil.particle_steps(reset=True)
        got = _pair_fluxes(m)
        o = _oracle_pair(oracle, st, warm, N, scale, op, threads)
    finally:
        oracle.set_threads(1)
    assert o["debris"]["gate"] and o["debris"]["rule_steps"] < o["debris"]["steps"]
    got_debris = got_steps - o["steps_f"]
    if mode == 1:
        assert retired_steps_close(got_debris, o["debris"], N), (got_debris, o["debris"])
        assert got_debris < o["debris"]["steps"]
    else:
        assert got_debris == o["debris"]["steps"]
    assert o["steps_f"] > 20 * N
    for k in ("wf", "mf", "vf", "af", "df", "dvf", "ad"):
        _flux_close(got[k], o[k], "flux %s" % k)
    assert (o["af"] != 0).any() and (o["ad"] != 0).any()


# ---------------------------------------------------------------- whole coloured steps

def _oracle_colour_step(oracle, st, step, N, scale, op, threads):
    H, W = st["layers"].shape[:2]
    o = _oracle_pair(oracle, st, step, N, scale, op, threads)
    res = _oracle_colour_cells(oracle, st["layers"], np.zeros((H, W), np.float32), np.ones((H, W), np.float32),
                               o["wf"], o["mf"], o["vf"], o["df"], o["dvf"],
                               dict(albedoBedrock=st["bed"], albedoSurface=st["surf"], albedoFluvial=o["af"],
                                    albedoDebris=o["ad"]), scale, op)
    new = dict(layers=res["layers_next"], wh=res["waterHeight"], m=res["mass"], v=res["velocity"], d=res["debris"],
               dv=res["debrisVelocity"], bed=st["bed"], surf=res["albedoSurface"], af=res["albedoFluvial"],
               ad=res["albedoDebris"])
    return new, o


OUT_PLANES = STATE_PLANES[:6] + (("albedoSurface", "surf"), ("albedoFluvial", "af"), ("albedoDebris", "ad"))


def test_three_coloured_steps_at_1024(hip, oracle):
    """ErosionModel(colour=True).step() — soil_erode_step_colour — forced from the oracle's state and free-running,
    against the oracle's coloured composition: every physics and colour plane."""
    from soillib_amd import soil
    threads = os.cpu_count() or 1
    oracle.set_threads(threads)
    H = W = 1024
    N = H * W // 8
    op = script_param(oracle.default_param())
    pp = product_param(op)
    scale = (20.0 / H, 20.0 / W, 4.0)
    forced, free = _model(H, W, scale, pp, N), _model(H, W, scale, pp, N)
    st = _colour_state(oracle, H, W)
    _force(free, st, 0)
    try:
        for step in range(3):
            _force(forced, st, step)
            soil.particle_steps(reset=True)
            forced.step()
            got_steps = soil.particle_steps(reset=True)
            free.step()
            st, o = _oracle_colour_step(oracle, st, step, N, scale, op, threads)
            from util import debris_steps_agree
            assert debris_steps_agree(got_steps - o["steps_f"], o["debris"], N), (got_steps, o["steps_f"], o["debris"])
            for name, key in OUT_PLANES:
                want = st[key]
                tol = dict(rtol=1e-4, atol=1e-5 * (np.nanmax(np.abs(want)) + 1e-30))
                _close_but_for_stray_walks(to_np(getattr(forced, name)), want, tol["rtol"], tol["atol"], 2e-6,
                                           "step %d forced %s" % (step, name))
                _close_but_for_stray_walks(to_np(getattr(free, name)), want, tol["rtol"], tol["atol"],
                                           2e-6 if step == 0 else 2e-3, "step %d free-running %s" % (step, name))
    finally:
        oracle.set_threads(1)
    assert np.abs(st["surf"] - _colour_state(oracle, H, W)["surf"]).max() > 0   # the surface colour changed


def _close_fields(a, b, what):
    for name, _ in OUT_PLANES:
        want = to_np(getattr(b, name))
        tol = dict(rtol=1e-4, atol=1e-5 * (np.nanmax(np.abs(want)) + 1e-30))
        _close_but_for_stray_walks(to_np(getattr(a, name)), want, tol["rtol"], tol["atol"], 2e-6, what + " " + name)


def test_coloured_step_equals_step_unfused(hip, oracle):
    """The fused coloured step against the same step through the reference ops with their albedo arguments
    (step_unfused: two normalises, mass_transfer, mass_creep, add, layer_merge, one launch each)."""
    H = W = 1024
    N = H * W // 8
    op = script_param(oracle.default_param())
    pp = product_param(op)
    scale = (20.0 / H, 20.0 / W, 4.0)
    a, b = _model(H, W, scale, pp, N), _model(H, W, scale, pp, N)
    st = _colour_state(oracle, H, W)
    _force(a, st, 0)
    _force(b, st, 0)
    a.step()          # swaps: the new layers are in `layers`
    b.step_unfused()  # adds delta to `layers` in place
    _close_fields(a, b, "step vs step_unfused")


def test_coloured_step_lazy_flux_flags(hip, oracle):
    """soil_erode_step_colour with flags 0 | 0 and OUT_DIRTY | IN_DIRTY over two steps: the same fields; the
    physics flux planes zeroed at the end of either chain."""
    import ctypes as C
    from soillib_amd import _abi
    H = W = 1024
    N = H * W // 8
    op = script_param(oracle.default_param())
    pp = product_param(op)
    scale = (20.0 / H, 20.0 / W, 4.0)
    a, b = _model(H, W, scale, pp, N), _model(H, W, scale, pp, N)
    st = _colour_state(oracle, H, W)
    _force(a, st, 0)
    _force(b, st, 0)
    for step, (fa, fb) in enumerate([(0, _abi.SOIL_STEP_FLUX_OUT_DIRTY), (0, _abi.SOIL_STEP_FLUX_IN_DIRTY)]):
        for m, f in ((a, fa), (b, fb)):
            planes, colour = m._planes(), m._colour()
            _abi.check(_abi.lib().soil_erode_step_colour(C.byref(planes), C.byref(colour), m.rng.c_ptr, N, 0, step,
                                                         H, W, m._scale(), pp._ref(), f, _abi.stream()))
            m.swap_layers()
        if step == 0:
            assert (to_np(b.waterFlux) != 0).any(), "OUT_DIRTY left the flux planes as they were"
    _close_fields(a, b, "flags")
    for m in (a, b):
        for name in ("waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux"):
            assert (to_np(getattr(m, name)) == 0).all(), name


# ---------------------------------------------------------------- edges of the retirement argument

def test_non_finite_spawn_colours_are_never_retired(hip, oracle, retire):
    """NaN and inf colours on spawn cells where the gate is open: a walker that carries one can still deposit
    something that is not zero (0 * inf is NaN), so mode 1 must walk it on — the colour fluxes equal mode 0's,
    NaN positions included — while still walking fewer steps than mode 0.  Mode 2 counts nothing."""
    from soillib_amd import soil
    H = W = 1024
    N = H * W // 8
    op = script_param(oracle.default_param())
    pp = product_param(op)
    scale = (20.0 / H, 20.0 / W, 4.0)
    st = _colour_state(oracle, H, W)
    assert oracle.debris_retire_gate(st["layers"], st["dv"], scale, op)
    r = np.random.default_rng(11)
    cells = r.choice(H * W, 4000, replace=False)
    surf = st["surf"].reshape(-1, 3)
    surf[cells[:2000], r.integers(0, 3, 2000)] = np.nan
    surf[cells[2000:], r.integers(0, 3, 2000)] = np.inf
    m = _model(H, W, scale, pp, N)
    runs = {}
    for mode in (0, 1, 2):
        retire(mode)
        _force(m, st, 0)
        m.seed_step()
        soil.particle_steps(reset=True)
        m.particles_pair(overwrite=True)   # the physics flux planes hold the run before's deposits
        runs[mode] = (soil.particle_steps(reset=True), _pair_fluxes(m))
        if mode == 2:
            assert soil.debris_retire_violations(reset=True) == 0
    (s0, f0), (s1, f1), (s2, _) = runs[0], runs[1], runs[2]
    assert s1 < s0 and s2 == s0
    for k in ("ad", "af", "df", "dvf"):
        nan0, nan1 = ~np.isfinite(f0[k]), ~np.isfinite(f1[k])
        assert (nan0 == nan1).all(), k + ": non-finite cells differ"
        fin = ~nan0
        scale_k = np.abs(f0[k][fin]).max() + 1e-30
        np.testing.assert_allclose(f1[k][fin], f0[k][fin], rtol=1e-4, atol=2e-6 * scale_k, err_msg=k)
    assert (~np.isfinite(f0["ad"])).any(), "no walker carried a non-finite colour"


def test_transport_debris_with_colour_still_walks_every_walker(hip, oracle, retire):
    """soil.transport_debris with colour planes keeps its behaviour in mode 1: every walker walked to the end."""
    from soillib_amd import soil
    from util import rng_to_gpu
    H = W = 512
    N = H * W // 4                       # tiled
    op = script_param(oracle.default_param())
    pp = product_param(op)
    scale = (20.0 / H, 20.0 / W, 4.0)
    st = _colour_state(oracle, H, W)
    threads = os.cpu_count() or 1
    oracle.set_threads(threads)
    try:
        z3 = np.zeros((H, W, 3), np.float32)
        want = oracle.particles_debris_retire(np.zeros((H, W), np.float32), np.zeros((H, W, 2), np.float32), z3.copy(),
                                              oracle.rng_seed(N, 0, 0), st["layers"], st["dv"], st["surf"], scale, op,
                                              threads=threads)
    finally:
        oracle.set_threads(1)
    assert want["gate"] and want["rule_steps"] < want["steps"]
    retire(1)
    z = lambda *s: to_gpu(np.zeros(s, np.float32))
    soil.particle_steps(reset=True)
    soil.transport_debris(to_gpu(st["layers"]), to_gpu(st["dv"]), z(H, W, 2), z(H, W), z(H, W), to_gpu(st["bed"]),
                          z(H, W, 3), to_gpu(st["surf"]), rng_to_gpu(oracle.rng_seed(N, 0, 0)), scale, pp)
    assert soil.particle_steps(reset=True) == want["steps"]
