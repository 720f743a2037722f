#!/usr/bin/env python
"""The sharded coloured step (SlabRunner(colour=True), soil_slab_create_colour; DESIGN.md 5, "Colour on slabs") as ONE rank of
a `world`-way split of a size^2 grid, emulated on one GPU: an interior rank (world // 2) in deep-halo mode with
halos trimmed to the measured reach, on a wire that moves nothing but counts what the rank sends.  Every kernel
the rank would launch runs at its real size; the wire time is missing.  Prints one JSON line:
  colour_ms, physics_ms         ms per step of the coloured and the physics-only runner, timed in this run
  flux_halo_bytes_per_neighbour bytes of the flux halo this rank sends one neighbour per step (mean of the
                                two), coloured and physics-only; field_halo_bytes_per_neighbour the same for
                                the field halo (the same planes either way: no colour field halo)
  whole_grid_colour_ms          soil_erode_step_colour on the whole size^2 grid (ErosionModel(colour=True)),
                                if it fits (--no-whole skips it)
The script's parameters (example/erosion_gpu.py), maxage 256, N = cells / 8, noise terrain, uniform colours.

    python tools/bench_colour_slab.py [--size 16384] [--world 4] [--steps 4] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("SOIL_HALO_FULL", "0")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from soillib_amd import _abi, silt, soil  # noqa: E402
from soillib_amd.parallel import FIELD_PLANES, FLUX_PLANES, CallbackComm, SlabRunner  # noqa: E402
from util import script_param  # noqa: E402


class CountingWire:
    """impl of parallel.CallbackComm that moves nothing and counts the bytes sent, by plane kind and peer"""

    def __init__(self):
        self.ranges = []       # (first byte, end, kind)
        self.sent = {}         # (kind, peer) -> bytes

    def watch(self, runner, names, kind):
        for n in names:
            p, rows, ch = runner.plane_ptr(n)
            self.ranges.append((p.value, p.value + 4 * rows * runner.W * ch, kind))

    def exchange(self, sends, recvs):
        for addr, n, peer in sends:
            kind = next((k for a, b, k in self.ranges if a <= addr < b), "other")
            self.sent[(kind, peer)] = self.sent.get((kind, peer), 0) + n

    def all_reduce(self, addr, n):
        pass

    def barrier(self):
        pass

    def max_over_ranks(self, value):
        return value


def rank_of_world(args, colour):
    param = script_param(soil.param_t())
    param.maxage = 256
    world, size = args.world, args.size
    wire = CountingWire()
    cell = 20.0 / size
    r = SlabRunner(rows_per_rank=size // world, W=size, param=param, particles_div=8, seed=0,
                   comm=CallbackComm(world // 2, world, wire), scale=[cell, cell, 4.0], noise_rows=size,
                   mode="deep", colour=colour)
    if colour:
        for name, v in (("albedo_bedrock", 0.3), ("albedo_surface", 0.6)):
            p, rows, ch = r.plane_ptr(name)
            _abi.check(_abi.lib().soil_set_f32(p, v, rows * r.W * ch, None))
        _abi.check(_abi.lib().soil_device_synchronize())
    flux = FLUX_PLANES + (("albedo_fluvial", "albedo_debris") if colour else ())
    wire.watch(r, flux, "flux")
    wire.watch(r, FIELD_PLANES + ("layers_next",), "field")
    for _ in range(args.warmup):
        r.step()
    r.sync()
    wire.sent.clear()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        r.step()
    r.sync()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    peers = sorted({p for _, p in wire.sent})
    per = lambda kind: sum(v for (k, _), v in wire.sent.items() if k == kind) / max(len(peers), 1) / args.steps
    out = dict(ms=ms, flux=per("flux"), field=per("field"), other=per("other"), rows=r.rows, S=r.S, G=r.G,
               fallbacks=r.fallbacks, reach=r.reach_hist)
    r.close()
    del r
    silt.empty_cache()
    return out


def whole_grid(args):
    from soillib_amd.erosion import ErosionModel
    S = args.size
    param = script_param(soil.param_t())
    param.maxage = 256
    p = soil.noise_t()
    p.seed = 3.0
    p.ext = [S, S]
    m = ErosionModel(S, S, (20.0 / S, 20.0 / S, 4.0), param, S * S // 8, seed=0, colour=True)
    bed = soil.noise(silt.shape(S, S), p, host=silt.gpu)
    zero = silt.tensor(silt.float32, silt.shape(S, S), silt.gpu)
    silt.set(zero, 0.0)
    _abi.check(_abi.lib().soil_layers_from_planes(m.layers.c_ptr, bed.c_ptr, zero.c_ptr, S * S, None))
    del bed, zero
    silt.set(m.rainfall, 1.0)
    silt.set(m.albedoBedrock, 0.3)
    silt.set(m.albedoSurface, 0.6)
    for _ in range(args.warmup):
        m.step()
    _abi.check(_abi.lib().soil_device_synchronize())
    t0 = time.perf_counter()
    for _ in range(args.steps):
        m.step()
    _abi.check(_abi.lib().soil_device_synchronize())
    return (time.perf_counter() - t0) * 1e3 / args.steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--world", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-whole", action="store_true")
    args = ap.parse_args()
    soil.debris_retire(1)
    c = rank_of_world(args, True)
    f = rank_of_world(args, False)
    out = dict(note="emulated on one GPU, no wire measured", size=args.size, world=args.world,
               rank=args.world // 2, mode="deep", trim=os.environ.get("SOIL_HALO_FULL") != "1",
               steps=args.steps, warmup=args.warmup, rows=c["rows"], owned_rows=c["S"], ghost_rows_per_side=c["G"],
               colour_ms=c["ms"], physics_ms=f["ms"],
               flux_halo_bytes_per_neighbour=dict(colour=c["flux"], physics=f["flux"]),
               field_halo_bytes_per_neighbour=dict(colour=c["field"], physics=f["field"]),
               other_bytes_per_neighbour=dict(colour=c["other"], physics=f["other"]),
               repeated_launches=dict(colour=c["fallbacks"], physics=f["fallbacks"]),
               reach=dict(colour=c["reach"], physics=f["reach"]))
    if not args.no_whole:
        try:
            out["whole_grid_colour_ms"] = whole_grid(args)
        except MemoryError as e:
            out["whole_grid_colour_ms"] = None
            out["whole_grid_skipped"] = str(e)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
