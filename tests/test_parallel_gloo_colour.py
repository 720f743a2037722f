"""Multi-process (gloo, CPU) test of the library's COLOURED slab runner (soil_slab_create_colour,
csrc/slab_runner.hip): world_size 2 and 3 jobs drive it with the oracle as compute back-end, colour
table included (tests/parallel_colour_worker.py), and the owned rows of all ranks, stitched together,
must equal the same composition of the oracle's ops on the whole grid — every physics plane and the
three colour planes the step writes.  No GPU: what is under test is the runner's colour schedule —
colour flux planes in the flux halo and the reach scan, the 16-float remote0, the colour cell phase on
the banded row ranges.  The oracle parks no colour in remote0, so the terrain (a tilted plane under
the noise) is one without NaN walkers, and the worker checks that none was parked."""
import os
import subprocess
import sys

import numpy as np
import pytest

from parallel_colour_worker import OWNED, colour_cells, colour_inputs, colour_param, initial_layers
from test_parallel_gloo import _free_port
from util import script_param

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _single_domain_colour(oracle, H, W, steps, maxage):
    p = colour_param(maxage)
    scale = (20.0 / H, 20.0 / W, 4.0)
    N = H * W // 8
    layers = initial_layers(H, W)
    z1 = lambda: np.zeros((H, W), np.float32)
    z2 = lambda: np.zeros((H, W, 2), np.float32)
    z3 = lambda: np.zeros((H, W, 3), np.float32)
    st = dict(layers=layers, waterHeight=z1(), velocity=z2(), debrisVelocity=z2(), debris=z1(), height=z1())
    col = dict(colour_inputs(H, W), albedo_fluvial=z3(), albedo_debris=z3())
    rain = np.ones((H, W), np.float32)
    for step in range(steps):
        rng = oracle.rng_seed(N, 0, step * N)
        wf, mf, vf, df, dvf = z1(), z1(), z2(), z1(), z2()
        col["albedo_fluvial"], col["albedo_debris"] = z3(), z3()
        oracle.particles_fluvial(wf, mf, vf, col["albedo_fluvial"], rng, st["layers"], rain, st["waterHeight"],
                                 st["velocity"], col["albedo_surface"], scale, p)
        oracle.particles_debris(df, dvf, col["albedo_debris"], rng, st["layers"], st["debrisVelocity"],
                                col["albedo_surface"], scale, p)
        flux_seen = (np.abs(col["albedo_fluvial"]).max(), np.abs(col["albedo_debris"]).max())
        r = colour_cells(st["layers"], z1(), rain, wf, mf, vf, df, dvf, col, scale, p)
        st = dict(layers=r["layers_next"], waterHeight=r["waterHeight"], velocity=r["velocity"],
                  debrisVelocity=r["debrisVelocity"], debris=r["debris"], height=r["height"])
        col.update(albedo_fluvial=r["albedo_fluvial"], albedo_debris=r["albedo_debris"],
                   albedo_surface=r["albedo_surface"])
    return dict(st, **col), flux_seen


@pytest.mark.parametrize("world,S,W,maxage,steps,need,pair", [
    (2, 24, 32, 8, 3, None, False),
    (3, 16, 24, 6, 3, None, True),
    (2, 80, 48, 48, 3, None, True),     # deep ghost zone: trimmed halos, colour planes in the reach scan
    (3, 72, 40, 48, 3, "2", False),     # a refresh depth too small on purpose: launches repeated with colour
])
def test_coloured_slab_runner_matches_single_domain(oracle, tmp_path, world, S, W, maxage, steps, need, pair):
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        env.pop("SOIL_HALO_NEED", None)
        if need:
            env["SOIL_HALO_NEED"] = need
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", "parallel_colour_worker.py"), str(tmp_path),
             str(S), str(W), str(steps), str(maxage)] + (["pair"] if pair else []), env=env,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-3000:]

    H = world * S
    want, flux_seen = _single_domain_colour(oracle, H, W, steps, maxage)
    assert min(flux_seen) > 0                           # both launches deposited colour
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % k)) for k in range(world)]
    if need:
        assert sum(int(d["fallbacks"]) for d in parts) > 0
    for k in OWNED:
        full = np.concatenate([d[k] for d in parts], axis=0)
        w = want[k]
        np.testing.assert_allclose(full, w, rtol=2e-5, atol=1e-6 * (np.nanmax(np.abs(w)) + 1e-30), err_msg=k)
    # the colours moved: the surface was mixed, the transport colours are not zero
    first = colour_inputs(H, W)["albedo_surface"]
    assert (want["albedo_surface"] != first).any()
    assert np.abs(want["albedo_fluvial"]).max() > 0 and np.abs(want["albedo_debris"]).max() > 0


class _OneRankWire:
    """impl of parallel.CallbackComm for a world of one on host memory"""

    def exchange(self, sends, recvs):
        assert not sends and not recvs

    def all_reduce(self, addr, n):
        pass

    def barrier(self):
        pass

    def max_over_ranks(self, value):
        return value


def _runner(colour, backend):
    from soillib_amd import _abi, parallel
    from util import copy_param
    from oracle import pyoracle as o
    param = copy_param(script_param(o.default_param()), _abi.Param())
    param.maxage = 4
    return parallel.SlabRunner(rows_per_rank=8, W=8, param=param, particles_div=8, init=False,
                               ops=parallel.CallbackOps(backend), comm=parallel.CallbackComm(0, 1, _OneRankWire()),
                               colour=colour)


def test_physics_runner_refuses_colour_planes(oracle):
    from parallel_colour_worker import OracleColourOps
    from soillib_amd import parallel
    r = _runner(False, OracleColourOps())
    try:
        for name in parallel.COLOUR_PLANES:
            with pytest.raises(ValueError, match="physics-only"):
                r.plane_ptr(name)
        assert r.plane("layers").shape == (8, 8, 2)
    finally:
        r.close()
    c = _runner(True, OracleColourOps())
    try:
        for name in parallel.COLOUR_PLANES:
            a = c.plane(name)
            assert a.shape == (8, 8, 3) and not a.any()     # the colour planes start at zero
        c.set_plane("albedo_surface", np.full((8, 8, 3), 0.5, np.float32))
        assert (c.plane("albedo_surface") == 0.5).all()
    finally:
        c.close()


def test_coloured_runner_needs_a_colour_table(oracle):
    from parallel_worker import OracleOps
    with pytest.raises(ValueError, match="both"):
        _runner(True, OracleOps())


def test_migrate_mode_with_colour_needs_particles_pass(oracle):
    """The oracle's colour table has no particles_pass (nor has the HIP one): migrate mode is refused."""
    from parallel_colour_worker import OracleColourOps
    from soillib_amd import _abi, parallel
    from util import copy_param
    from oracle import pyoracle as o
    param = copy_param(script_param(o.default_param()), _abi.Param())
    param.maxage = 4
    backend = OracleColourOps()
    backend.particles_pass = lambda *a: None    # a physics hand-over exists ...
    with pytest.raises(ValueError, match="SOIL_SLAB_MIGRATE with colour"):
        parallel.SlabRunner(rows_per_rank=8, W=8, param=param, particles_div=8, init=False, mode="migrate",
                            ops=parallel.CallbackOps(backend), comm=parallel.CallbackComm(0, 1, _OneRankWire()),
                            colour=True)
