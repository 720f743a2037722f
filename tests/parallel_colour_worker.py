"""Worker of tests/test_parallel_gloo_colour.py: one rank of a world_size-N gloo job that drives the
library's COLOURED slab runner (soil_slab_create_colour, csrc/slab_runner.hip) with the CPU oracle
plugged in as compute back-end — its physics table (tests/parallel_worker.py: OracleOps) and a colour
table composed here from the oracle's ops with their albedo arguments — and gloo as the wire."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import pyoracle as o  # noqa: E402
from parallel_worker import OracleOps, _arr  # noqa: E402
from soillib_amd import _abi, parallel  # noqa: E402
from util import copy_param, script_param  # noqa: E402


def initial_layers(H, W):
    """A tilted plane under the noise: no cell of zero gradient, so no NaN walkers (OracleColourOps)."""
    x, y = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    layers = np.zeros((H, W, 2), np.float32)
    layers[..., 0] = 0.02 * x + 0.013 * y + 0.1 * o.noise(H, W, seed=3.0, ext=(float(H), float(W)))
    return layers


def colour_param(maxage, target=None):
    """The example's parameters with landslides on that terrain (a debris walker's attenuation must not
    underflow at once, or its colour flux is all zeros)."""
    p = script_param(o.default_param())
    p.maxage = maxage
    p.critSlopeBedrock = 0.0
    p.yieldStress = 0.001
    return p if target is None else copy_param(p, target)


def colour_inputs(H, W):
    """The global grid's initial colours: non-trivial, finite, per cell (the same on every rank)."""
    r = np.random.default_rng(7)
    return {"albedo_bedrock": (r.random((H, W, 3)) * 1.3).astype(np.float32),
            "albedo_surface": (r.random((H, W, 3)) * 1.3).astype(np.float32)}


class OracleColourOps(OracleOps):
    """OracleOps plus the entries of soil_slab_colour_ops (CallbackOps: the colour_* methods).

    The oracle parks no colour in remote0, so a NaN walker that another rank's (0, 0) would receive
    takes its colour deposit with it: the inputs of the tests are chosen free of such walkers, and
    every launch here checks that nothing was parked (remote0 all zero on ranks that do not hold row 0)."""

    @staticmethod
    def _colour(cp, dom):
        c, d = cp.contents, dom.contents
        return {n: _arr(getattr(c, n), (d.rows, d.W, 3)) for n in _abi.COLOUR_PLANES}

    @staticmethod
    def _nothing_parked(remote0, dom):
        if dom.contents.x0 > 0:
            r = _arr(remote0, (16,))
            assert not r.any(), "a NaN walker parked a deposit for (0, 0): these inputs must be free of them %s" % r

    def colour_particles_fluvial(self, pl, cp, rng, N, remote0, dom, scale, param):
        P, d = self._planes(pl, dom)
        c = self._colour(cp, dom)
        c["albedo_fluvial"][:] = 0
        o.particles_fluvial(P["waterFlux"], P["massFlux"], P["velocityFlux"], c["albedo_fluvial"], self._rng(rng, N),
                            P["layers"], P["rainfall"], P["waterHeight"], P["velocity"], c["albedo_surface"],
                            [scale[i] for i in range(3)], self._param(param), dom=self._dom(d),
                            remote0=_arr(remote0, (8,)))
        self._nothing_parked(remote0, dom)

    def colour_particles_debris(self, pl, cp, rng, N, remote0, dom, scale, param):
        P, d = self._planes(pl, dom)
        c = self._colour(cp, dom)
        c["albedo_debris"][:] = 0
        o.particles_debris(P["debrisFlux"], P["debrisVelocityFlux"], c["albedo_debris"], self._rng(rng, N),
                           P["layers"], P["debrisVelocity"], c["albedo_surface"], [scale[i] for i in range(3)],
                           self._param(param), dom=self._dom(d), remote0=_arr(remote0, (8,)))
        self._nothing_parked(remote0, dom)

    def colour_cells(self, pl, cp, dom, scale, param):
        P, d = self._planes(pl, dom)
        c = self._colour(cp, dom)
        r0, r1 = d.r0, d.r1
        if r1 <= r0:
            return
        res = colour_cells(P["layers"], P["uplift"], P["rainfall"], P["waterFlux"], P["massFlux"],
                           P["velocityFlux"], P["debrisFlux"], P["debrisVelocityFlux"], c,
                           [scale[i] for i in range(3)], self._param(param), self._dom(d))
        for name in ("layers_next", "height", "waterHeight", "mass", "velocity", "debris", "debrisVelocity"):
            P[name][r0:r1] = res[name][r0:r1]
        for name in ("albedo_surface", "albedo_fluvial", "albedo_debris"):
            c[name][r0:r1] = res[name][r0:r1]
        for name in parallel.FLUX_PLANES:      # the fused kernel re-zeroes the physics flux it consumed
            P[name][r0:r1] = 0


def colour_cells(layers, uplift, rain, wf, mf, vf, df, dvf, c, scale, op, dom=None):
    """normalize_fluvial -> normalize_debris -> delta = 0 -> mass_transfer -> mass_creep -> add, with the
    colour planes (soil_colour_planes, steps 5-9), on copies of the colour planes."""
    rows, W = layers.shape[:2]
    dom = dom or o.domain(rows, W)
    z1 = lambda: np.zeros((rows, W), np.float32)
    z2 = lambda: np.zeros((rows, W, 2), np.float32)
    wh, m, v, d, dv = z1(), z1(), z2(), z1(), z2()
    af, ad, surf = c["albedo_fluvial"].copy(), c["albedo_debris"].copy(), c["albedo_surface"].copy()
    o.normalize_fluvial(wf, mf, vf, af, layers, rain, wh, m, v, surf, scale, op, dom)
    o.normalize_debris(df, dvf, ad, layers, d, dv, surf, scale, op, dom)
    delta = z2()
    o.mass_transfer(delta, layers, uplift, m, v, d, c["albedo_bedrock"], af, ad, surf, scale, op, dom)
    o.mass_creep(delta, layers, scale, op, dom)
    layers_next = layers + delta
    return dict(layers_next=layers_next, height=layers_next[..., 0] + layers_next[..., 1], waterHeight=wh,
                mass=m, velocity=v, debris=d, debrisVelocity=dv, albedo_fluvial=af, albedo_debris=ad,
                albedo_surface=surf)


OWNED = ("layers", "waterHeight", "velocity", "debris", "height") + parallel.COLOUR_PLANES


def main():
    out_dir, S, W, steps, maxage = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), \
        int(sys.argv[5])
    pair = len(sys.argv) > 6 and sys.argv[6] == "pair"
    param = colour_param(maxage, _abi.Param())
    backend = OracleColourOps()
    if pair:    # both launches "overlapped": the fluvial one draws from rng, the debris one from rng_debris
        def colour_particles_pair(pl, cp, rng, rng_debris, N, remote0, dom, scale, prm):
            backend.colour_particles_fluvial(pl, cp, rng, N, remote0, dom, scale, prm)
            backend.colour_particles_debris(pl, cp, rng_debris, N, remote0, dom, scale, prm)
        backend.colour_particles_pair = colour_particles_pair
    wire = parallel.GlooWire(device=False)
    comm = parallel.CallbackComm(wire.dist.get_rank(), wire.dist.get_world_size(), wire)
    runner = parallel.SlabRunner(rows_per_rank=S, W=W, param=param, particles_div=8, seed=0,
                                 ops=parallel.CallbackOps(backend), comm=comm, pair=pair, colour=True, init=False)
    rows = slice(runner.x0, runner.x0 + runner.rows)
    runner.set_plane("layers", initial_layers(runner.H, W)[rows])
    runner.set_plane("rainfall", np.ones((runner.rows, W), np.float32))
    col = colour_inputs(runner.H, W)
    for name, a in col.items():
        runner.set_plane(name, a[rows])
    for _ in range(steps):
        runner.step()
    np.savez(os.path.join(out_dir, "rank%d.npz" % runner.rank),
             fallbacks=runner.fallbacks, G=runner.G,
             **{k: runner.plane(k, owned=True).copy() for k in OWNED})
    runner.barrier()
    runner.shutdown()


if __name__ == "__main__":
    main()
