#!/usr/bin/env python
"""Flats and filled lakes (include/soil_hip.h: soil_flat_distance, soil_flat_receivers and their _batch forms;
DESIGN.md 3.5 "Flats and filled lakes"), timed in one process:

  --single H,...   at H x H under D8, on two DEMs:
      c3         the bench.py --config c3 DEM (noise x 100, seed 3), filled by soil.fill_depressions
      quantised  floor(noise x 20), unfilled: many natural flats of every shape
    distance     soil.flat_distance(dem)                          with the launches and looks of soil_flat_distance_info
    receivers    soil.flat_receivers(steepest(dem), dem, dist)
    fill         soil.fill_depressions on the same UNFILLED DEM: the yardstick, code this library had before
  --batch H:B,...  soil.flat_distance_batch + flat_receivers_batch on B filled models (another seed each) against the
                   single-grid calls on the same models one at a time

One JSON line per size and DEM.  A figure is the median of --repeats medians, each over --iters calls (device events
around every call) after --warmup calls, the routes alternated repeat by repeat; the spread beside it is the greatest
minus the least of those medians.  `fill_over_flats`: fill / (distance + receivers).

--count N: the distance and the receivers alone, N calls each and nothing else timed, for a kernel trace:
    rocprofv3 --kernel-trace --stats -- python tools/bench_flats.py --single 4096 --count 10"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402
from tools.bench_flow_batch import model_view  # noqa: E402
from tools.bench_flow_paths import emit, figures  # noqa: E402

SINGLE = "1024,4096,8192"
BATCH = "256:8,256:64,256:256"


def dem(H, seed, factor, floor=False):
    p = soil.noise_t()
    p.seed = float(seed)
    p.ext = [H, H]
    h = soil.noise(silt.shape(H, H), p, host=silt.gpu)
    silt.multiply(h, factor)
    if floor:
        h.view_torch().floor_()
        _abi.check(_abi.lib().soil_device_synchronize())
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default=None, help="H,... (default with neither option: %s)" % SINGLE)
    ap.add_argument("--batch", default=None, help="H:B,... (default with neither option: %s)" % BATCH)
    ap.add_argument("--iters", type=int, default=10, help="timed calls per median")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=0, help="the new calls alone, this many each, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.single is None and args.batch is None:
        args.single, args.batch = SINGLE, BATCH
    lib = _abi.lib()
    edge = soil.d8
    for H in [int(v) for v in (args.single or "").split(",") if v]:
        for name in ("c3", "quantised"):
            raw = dem(H, 3, 100.0) if name == "c3" else dem(H, 3, 20.0, floor=True)
            h = soil.fill_depressions(raw, edge) if name == "c3" else raw
            graph = soil.steepest(h, edge)
            dist = soil.flat_distance(h, edge)
            info = soil.flat_distance_info()
            line = {"H": H, "dem": name, "what": "single", "flat_cells": int((dist.view_torch() > 0).sum().item()),
                    "unreached": int((dist.view_torch() < 0).sum().item()),
                    "largest_distance": int(dist.view_torch().max().item())}
            line.update(info)
            if args.count:
                for _ in range(args.count):
                    soil.flat_receivers(graph, h, soil.flat_distance(h, edge), edge)
                _abi.check(lib.soil_stream_synchronize(_abi.stream()))
                line["count"] = args.count
                emit(line, args)
                continue
            line.update(figures(lib, [("distance", lambda: soil.flat_distance(h, edge)),
                                      ("receivers", lambda: soil.flat_receivers(graph, h, dist, edge)),
                                      ("fill", lambda: soil.fill_depressions(raw, edge))], args))
            both = line["distance_ms"] + line["receivers_ms"]
            line["flats_ms"] = round(both, 4)
            line["fill_over_flats"] = round(line["fill_ms"] / both, 2)
            emit(line, args)
            raw = h = graph = dist = None
            silt.empty_cache()
    for cfg in [v for v in (args.batch or "").split(",") if v]:
        H, B = (int(v) for v in cfg.split(":"))
        hb = silt.tensor(silt.float32, silt.shape(B, H, H), silt.gpu)
        per = hb.nbytes() // B
        for b in range(B):
            one = soil.fill_depressions(dem(H, 5 + b, 100.0), edge)
            _abi.check(lib.soil_memcpy_d2d(C.c_void_p(hb.ptr + b * per), one.c_ptr, per, _abi.stream()))
        _abi.check(lib.soil_stream_synchronize(_abi.stream()))
        gb = soil.steepest_batch(hb, edge)
        models = [(model_view(hb, b), model_view(gb, b)) for b in range(B)]

        def batch():
            return soil.flat_receivers_batch(gb, hb, soil.flat_distance_batch(hb, edge), edge)

        def single():
            out = None
            for h, g in models:
                out = soil.flat_receivers(g, h, soil.flat_distance(h, edge), edge)
            return out

        line = {"H": H, "B": B, "what": "batch"}
        single()
        line["single_launches_last_model"] = soil.flat_distance_info()["launches"]
        batch()
        line["batch_launches"] = soil.flat_distance_info()["launches"]
        line["batch_kernels_per_call"] = line["batch_launches"] + 1
        if args.count:
            for _ in range(args.count):
                batch()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            line["count"] = args.count
            emit(line, args)
            continue
        line.update(figures(lib, [("batch", batch), ("single", single)], args))
        line["single_over_batch"] = round(line["single_ms"] / line["batch_ms"], 2)
        emit(line, args)
        hb = gb = models = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
