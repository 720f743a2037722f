"""GPU tests of the sharded coloured step: the slab runner with colour (soil_slab_create_colour,
SlabRunner(colour=True)) on its HIP back-end, and soil_particles_pair_colour_slab by itself.

N slabs share the one GPU in one process (tests/test_gpu_parallel.py: LocalWire, the runners taking
turns); the owned rows of all ranks, stitched together, must hold what ErosionModel(colour=True).step()
(soil_erode_step_colour) leaves on the whole grid — every physics plane and the colour planes — up to
the fp32 summation order of the flux.
"""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from parallel_gpu_colour_worker import inputs as _inputs, param as _landslide_param
from test_gpu_parallel import LocalWire
from util import product_param, rng_to_gpu, script_param, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHYSICS = ("layers", "waterHeight", "velocity", "debris", "height")
# runner plane name -> ErosionModel attribute
COLOUR = {"albedo_bedrock": "albedoBedrock", "albedo_surface": "albedoSurface", "albedo_fluvial": "albedoFluvial",
          "albedo_debris": "albedoDebris"}


@pytest.fixture
def retire(hip):
    """Sets the debris retirement mode for one test; the suite's mode (watched) afterwards."""
    from soillib_amd import soil
    before = soil.debris_retire()
    yield soil.debris_retire
    soil.debris_retire(before)


def _whole_grid(H, W, pp, steps, inp):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionModel
    m = ErosionModel(H, W, (20.0 / H, 20.0 / W, 4.0), pp, H * W // 8, seed=0, colour=True)
    m.set_layers(to_gpu(inp["layers"]))
    silt.set(m.rainfall, 1.0)
    silt.set(m.albedoBedrock, to_gpu(inp["albedo_bedrock"]))
    silt.set(m.albedoSurface, to_gpu(inp["albedo_surface"]))
    for _ in range(steps):
        m.step()
    out = {k: to_np(getattr(m, k)) for k in PHYSICS}
    out.update({k: to_np(getattr(m, a)) for k, a in COLOUR.items()})
    return out


def _run_world(world, S, W, pp, steps, inp, pair=True, trim=None, halo_need=0, info=None):
    from soillib_amd.parallel import CallbackComm, SlabRunner
    shared = LocalWire.Shared(world)
    out, errs = [None] * world, []

    def worker(rank):
        held = False
        try:
            shared.token.acquire()
            held = True
            r = SlabRunner(rows_per_rank=S, W=W, param=pp, particles_div=8, seed=0, init=False,
                           comm=CallbackComm(rank, world, LocalWire(shared, rank)), device=0, pair=pair, trim=trim,
                           halo_need=halo_need, colour=True)
            rows = slice(r.x0, r.x0 + r.rows)
            r.set_plane("layers", inp["layers"][rows])
            r.set_plane("rainfall", np.ones((r.rows, W), np.float32))
            for name in ("albedo_bedrock", "albedo_surface"):
                r.set_plane(name, inp[name][rows])
            for _ in range(steps):
                r.step()
                r.sync()
            out[rank] = {k: r.plane(k, owned=True) for k in PHYSICS + tuple(COLOUR)}
            if info is not None:
                info[rank] = dict(fallbacks=r.fallbacks, trim=r.trim, pair=r.pair, halo=r.halo_rows)
            r.close()
        except BaseException as e:  # surface worker failures in the main thread
            errs.append(e)
            try:
                shared.bar.abort()
            except Exception:
                pass
        finally:
            if held:
                shared.token.release()
    ts = [threading.Thread(target=worker, args=(k,)) for k in range(world)]
    [t.start() for t in ts]
    [t.join(600) for t in ts]
    if errs:
        raise errs[0]
    return {k: np.concatenate([o[k] for o in out], axis=0) for k in out[0]}


def _compare(got, want, inp, debris_moved=True):
    for k in want:
        w = want[k]
        np.testing.assert_allclose(got[k], w, rtol=1e-4, atol=1e-5 * (np.nanmax(np.abs(w)) + 1e-30), err_msg=k)
    # the colours moved
    assert np.nanmax(np.abs(want["albedo_fluvial"])) > 0
    assert np.nanmax(np.abs(want["albedo_debris"])) > 0 or not debris_moved
    assert (want["albedo_surface"] != inp["albedo_surface"]).any()


def _param(oracle, maxage):
    return product_param(_landslide_param(oracle.default_param(), maxage))


@pytest.mark.parametrize("world,S,W,maxage,pair,trim", [
    (2, 64, 128, 16, True, True), (2, 64, 128, 16, False, False),
    (3, 64, 64, 24, True, False), (3, 64, 64, 24, False, True),
    (4, 64, 96, 16, True, True),
    (4, 128, 768, 16, True, True),      # N = 49152: the tiled launch shape, spent debris walkers retired
    (4, 128, 768, 16, False, True),
])
def test_coloured_runner_matches_whole_grid(hip, oracle, world, S, W, maxage, pair, trim):
    pp = _param(oracle, maxage)
    steps = 3
    H = world * S
    inp = _inputs(H, W)
    info = [None] * world
    got = _run_world(world, S, W, pp, steps, inp, pair=pair, trim=trim, info=info)
    assert all(i["trim"] == trim and i["pair"] == pair for i in info)
    want = _whole_grid(H, W, pp, steps, inp)
    _compare(got, want, inp)


def test_coloured_runner_repeat_launch_fallback(hip, oracle):
    """A refresh depth too small on purpose: the launches are repeated on complete fields, colour flux
    planes and colour remote slots cleared again — the same result."""
    world, S, W, maxage, steps = 3, 96, 128, 48, 3
    pp = _param(oracle, maxage)
    H = world * S
    inp = _inputs(H, W)
    for pair in (True, False):
        info = [None] * world
        got = _run_world(world, S, W, pp, steps, inp, pair=pair, trim=True, halo_need=2, info=info)
        assert sum(i["fallbacks"] for i in info) > 0
        _compare(got, _whole_grid(H, W, pp, steps, inp), inp)


def test_migrate_mode_with_colour_is_refused(hip):
    """Migrate mode with colour is not built: the HIP colour table has no particles_pass, and the runner
    refuses the combination with a clear error (the physics runner's migrate mode is unaffected)."""
    from soillib_amd import soil
    from soillib_amd.parallel import CallbackComm, SlabRunner
    shared = LocalWire.Shared(1)
    p = soil.param_t()
    p.maxage = 8
    with pytest.raises(ValueError, match="SOIL_SLAB_MIGRATE with colour"):
        SlabRunner(rows_per_rank=64, W=64, param=p, particles_div=8, init=False, mode="migrate", device=0,
                   comm=CallbackComm(0, 1, LocalWire(shared, 0)), colour=True)


def test_coloured_runner_nan_walkers_cross_ranks(hip, oracle):
    """test_gpu_parity.py::test_particles_on_slabs_equal_whole_grid's setting (maxage 8, critSlopeBedrock
    0.05) on the runner: the NaN walkers of every rank deposit their colour into global (0, 0) through the
    16-float remote0 — NaN exactly where the whole-grid coloured step has it."""
    op = script_param(oracle.default_param())
    op.maxage = 8
    op.critSlopeBedrock = 0.05
    pp = product_param(op)
    for world, S, W in ((2, 48, 48), (3, 32, 48)):
        H = world * S
        inp = _inputs(H, W, seed=world)
        got = _run_world(world, S, W, pp, 2, inp, pair=True)
        want = _whole_grid(H, W, pp, 2, inp)
        assert np.isnan(want["waterHeight"][0, 0])          # the quirk is live here
        for k in ("albedo_fluvial", "albedo_debris", "albedo_surface"):
            np.testing.assert_array_equal(np.isnan(got[k][0, 0]), np.isnan(want[k][0, 0]), err_msg=k)
        print("world %d: (0, 0) fluvial colour %s, debris colour %s" % (world, want["albedo_fluvial"][0, 0],
                                                                       want["albedo_debris"][0, 0]))
        for k in want:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-4,
                                       atol=1e-5 * (np.nanmax(np.abs(want[k])) + 1e-30), err_msg=k)


@pytest.mark.parametrize("particle_mode", [1, 3])
def test_pair_colour_slab_parks_the_colour_of_nan_walkers(hip, oracle, particle_mode):
    """soil_particles_pair_colour_slab on slabs that do not hold global row 0: a NaN walker's colour deposit
    for (0, 0) lands in remote0[8..13].  Spawn colours (1, 1/2, 1/4) make each colour slot the mass slot
    scaled by a power of two (att * (source * c) == (att * source) * c), up to the atomics' order."""
    from soillib_amd import _abi
    H, W = 96, 48
    op = script_param(oracle.default_param())
    op.maxage = 8
    op.critSlopeBedrock = 0.05
    pp = product_param(op)
    inp = _inputs(H, W)
    G = int(hip.soil_ghost_rows(pp._ref()))
    scale = _abi.vec((20.0 / H, 20.0 / W, 4.0), 3)
    N = 6000 if particle_mode == 1 else 60000
    c = np.array([1.0, 0.5, 0.25], np.float32)
    try:
        _abi.check(hip.soil_set_particle_mode(particle_mode))
        parked = 0
        for x_own in (32, 64):
            x0 = x_own - G
            rows = min(H, x_own + 32 + G) - x0
            sl = slice(x0, x0 + rows)
            z = lambda *s: to_gpu(np.zeros((rows, W) + s, np.float32))
            g = dict(layers=to_gpu(inp["layers"][sl]), rainfall=to_gpu(np.ones((rows, W), np.float32)),
                     waterHeight=z(), waterFlux=z(), massFlux=z(), velocity=z(2), velocityFlux=z(2), debrisFlux=z(),
                     debrisVelocity=z(2), debrisVelocityFlux=z(2))
            planes = _abi.ErosionPlanes()
            for name in _abi._PLANES:
                if name in g:
                    setattr(planes, name, g[name].ptr)
            surf = to_gpu(np.broadcast_to(c, (rows, W, 3)).copy())
            af, ad = to_gpu(np.full((rows, W, 3), 7.0, np.float32)), to_gpu(np.full((rows, W, 3), 7.0, np.float32))
            colour = _abi.ColourPlanes(None, surf.ptr, af.ptr, ad.ptr)
            rem = to_gpu(np.zeros(16, np.float32))
            rf, rd = rng_to_gpu(oracle.rng_seed(N, 2, 0)), rng_to_gpu(oracle.rng_seed(N, 2, 2))
            dom = _abi.Domain(H, W, x0, rows, G, G + 32)
            _abi.check(hip.soil_particles_pair_colour_slab(C.byref(planes), C.byref(colour), rf.c_ptr, rd.c_ptr, N,
                                                           rem.c_ptr, C.byref(dom), scale, pp._ref(), 0, None))
            r = to_np(rem)
            assert (r[14:] == 0).all()
            assert not (to_np(af) == 7.0).all()          # cleared first, then deposited into
            for phys, first in ((1, 8), (4, 11)):
                want = r[phys] * c
                np.testing.assert_array_equal(np.isnan(r[first:first + 3]), np.isnan(want))
                np.testing.assert_allclose(r[first:first + 3], want, rtol=1e-5, atol=1e-30)
                parked += int(r[phys] != 0)
        assert parked > 0                                   # NaN walkers did park something
    finally:
        hip.soil_set_particle_mode(0)


def test_coloured_runner_non_finite_spawn_colours_at_a_slab_edge(hip, oracle):
    """inf and NaN spawn colours on cells next to the slab edge: their colour deposits travel in the flux halo
    (and into the reach scan: 0 * inf is NaN where a mass deposit is zero) — the non-finite positions of the
    colour planes are those of the whole-grid step."""
    world, S, W, maxage = 2, 64, 128, 16
    pp = _param(oracle, maxage)
    H = world * S
    inp = _inputs(H, W)
    r = np.random.default_rng(11)
    for row in (S - 3, S - 1, S, S + 2):
        cols = r.choice(W, 6, replace=False)
        inp["albedo_surface"][row, cols[:3]] = np.inf
        inp["albedo_surface"][row, cols[3:], 1] = np.nan
    got = _run_world(world, S, W, pp, 2, inp, pair=True, trim=True)
    want = _whole_grid(H, W, pp, 2, inp)
    for k in ("albedo_fluvial", "albedo_debris", "albedo_surface"):
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(want[k]), err_msg=k)
        np.testing.assert_array_equal(np.isinf(got[k]), np.isinf(want[k]), err_msg=k)
    # the first step's raw colour flux (before the cell phase clamps the transport colours) holds non-finite
    # deposits on both sides of the edge: they did travel in the flux halo
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionModel
    m = ErosionModel(H, W, (20.0 / H, 20.0 / W, 4.0), pp, H * W // 8, seed=0, colour=True)
    m.set_layers(to_gpu(inp["layers"]))
    silt.set(m.rainfall, 1.0)
    silt.set(m.albedoSurface, to_gpu(inp["albedo_surface"]))
    m.seed_step()
    m.particles_pair()
    raw = to_np(m.albedoFluvial)
    spawn = ~np.isfinite(inp["albedo_surface"]).all(axis=2)
    bad = ~np.isfinite(raw).all(axis=2) & ~spawn
    assert bad[:S].any() and bad[S:].any()
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-4, atol=1e-5 * (np.nanmax(np.abs(np.where(
            np.isinf(want[k]), 0, want[k]))) + 1e-30), err_msg=k)


def test_coloured_runner_retirement_modes(hip, oracle, retire):
    """Spent debris walkers walked to the end (0), retired (1), watched (2): the same planes in every mode
    (the tiled shape: N = 49152; the example's parameters, where debris walkers are spent within two steps and
    their colour flux is all zeros), and no watched violation."""
    from soillib_amd import soil
    world, S, W, maxage = 2, 256, 768, 64
    op = script_param(oracle.default_param())
    op.maxage = maxage
    pp = product_param(op)
    inp = _inputs(2 * S, W)
    res = {}
    for mode in (0, 1, 2):
        retire(mode)
        soil.debris_retire_violations(reset=True)
        res[mode] = _run_world(world, S, W, pp, 2, inp, pair=True, trim=True)
        if mode == 2:
            assert soil.debris_retire_violations(reset=True) == 0
    for mode in (1, 2):
        for k in res[0]:
            np.testing.assert_allclose(res[mode][k], res[0][k], rtol=1e-4,
                                       atol=1e-5 * (np.nanmax(np.abs(res[0][k])) + 1e-30), err_msg=(mode, k))
    _compare(res[1], _whole_grid(2 * S, W, pp, 2, inp), inp, debris_moved=False)


def test_two_processes_share_one_gpu_over_gloo_with_colour(hip, oracle, tmp_path):
    """The sharded coloured step with real process separation: two ranks launched by torch.distributed.run,
    both on GPU 0, their halos and remote sums over gloo."""
    world, S, W, maxage, steps = 2, 96, 128, 24, 3
    env = dict(os.environ, SOIL_DEVICE="0", SOIL_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    res = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
         "--master-addr", "127.0.0.1", "--master-port", "29637",
         os.path.join(ROOT, "tests", "parallel_gpu_colour_worker.py"), str(tmp_path), str(S), str(W),
         str(maxage), str(steps)],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % k)) for k in range(world)]
    got = {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0].files}
    from soillib_amd import soil
    H = world * S
    pp = _landslide_param(soil.param_t(), maxage)
    inp = _inputs(H, W)
    want = _whole_grid(H, W, pp, steps, inp)
    want = {k: want[k] for k in got}
    _compare(got, want, inp)
