#!/usr/bin/env python
"""The coloured erosion step (include/soil_hip.h: soil_erode_step_colour) on an S^2 grid,
N = cells / 8, maxage 256 and the script's parameters (example/erosion_gpu.py), against the same step
through the reference ops (ErosionModel.step_unfused with colour) and the physics-only step, all in one
process.  Prints one JSON line: ms per step of
  colour_retire1   soil_erode_step_colour, spent debris walkers retired (soil_set_debris_retire(1))
  colour_retire0   the same, every walker walked to the end
  colour_unfused   step_unfused() with colour: two transport launches, then one launch per cell op
  physics          soil_erode_step (no colour), retirement as in colour_retire1
For the colour cell kernel's own time run this under rocprofv3 --kernel-trace --stats (168 bytes per cell,
DESIGN.md 3.4)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from soillib_amd import _abi, silt, soil  # noqa: E402
from soillib_amd.erosion import ErosionModel  # noqa: E402
from util import script_param  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=8192)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
S = args.size
lib = _abi.lib()
param = script_param(soil.param_t())
param.maxage = 256
scale = (20.0 / S, 20.0 / S, 4.0)
N = S * S // 8
p = soil.noise_t()
p.seed = 3.0
p.ext = [S, S]
bed = soil.noise(silt.shape(S, S), p, host=silt.gpu)
layers0 = silt.tensor(silt.float32, silt.shape(S, S, 2), silt.gpu)
zero = silt.tensor(silt.float32, silt.shape(S, S), silt.gpu)
silt.set(zero, 0.0)
_abi.check(lib.soil_layers_from_planes(layers0.c_ptr, bed.c_ptr, zero.c_ptr, S * S, None))


def model(colour):
    m = ErosionModel(S, S, scale, param, N, seed=0, colour=colour)
    m.set_layers(layers0)
    silt.set(m.rainfall, 1.0)
    if colour:
        silt.set(m.albedoBedrock, 0.3)
        silt.set(m.albedoSurface, 0.6)
    return m


def per_step(m, step):
    """ms per step over args.steps steps after args.warmup, from the same terrain each time."""
    m.set_layers(layers0)
    m.step_index = 0
    for _ in range(args.warmup):
        step()
    _abi.check(lib.soil_device_synchronize())
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    _abi.check(lib.soil_device_synchronize())
    return (time.perf_counter() - t0) * 1e3 / args.steps


out = dict(size=S, N=N, maxage=256, steps=args.steps, warmup=args.warmup)
soil.debris_retire(1)
c = model(True)
out["colour_retire1_ms"] = per_step(c, c.step)
soil.debris_retire(0)
out["colour_retire0_ms"] = per_step(c, c.step)
soil.debris_retire(1)
out["colour_unfused_ms"] = per_step(c, c.step_unfused)
del c
f = model(False)
out["physics_ms"] = per_step(f, f.step)
out["colour_speedup_vs_unfused"] = out["colour_unfused_ms"] / out["colour_retire1_ms"]
print(json.dumps(out))
