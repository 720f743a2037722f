#!/usr/bin/env python
"""Downstream walks along a receiver graph (include/soil_hip.h: soil_flow_paths, soil_flow_paths_batch; DESIGN.md 3.5
"Basins and flow length"), timed in one process against what a user had before them:

  --single H,...   on the `steepest` D8 graph of the bench terrain (noise x 100) at H x H:
      paths_terminal   soil.basins(graph)                                the new call, terminal only
      paths_all        soil.flow_paths(graph, scale)                     the new call, all three outputs
      torch            ptr = where(graph >= 0, graph, n); ptr = ptr.gather(0, ptr), ceil(log2(H W)) times — the
                       device-side route a user has today (terminals only, int64 indices as gather wants them)
      accumulate       soil.accumulate(graph, ones): the yardstick of the same algorithm class
  --batch H:B,...  soil.flow_paths_batch on B models against soil.flow_paths on the same models one at a time

One JSON line per size.  A figure is the median of --repeats medians, each over --iters calls (device events around
every call) after --warmup calls, the routes alternated repeat by repeat; the spread beside it is the greatest minus
the least of those medians.  `holds` (single): both new figures lie below torch's by more than both spreads;
(batch): for B >= 8 the batch lies below the one-at-a-time route by more than that route's spread, for B = 1 it is not
above it by more than that spread.

--count N: the batch route alone, N calls and nothing else on the device (graphs come from the host), for a kernel
trace:  rocprofv3 --kernel-trace --stats -- python tools/bench_flow_paths.py --batch 256:8 --count 10"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402
from tools.bench_flow_batch import model_view, timed  # noqa: E402

SINGLE = "256,1024,4096,8192"
BATCH = "256:1,256:8,256:64,256:256,512:1,512:8,512:64,512:256,1024:1,1024:8,1024:64,1024:256"
SCALE = (0.25, 3.0)


def graphs(B, H, on_host=False):
    """The `steepest` D8 graphs of B bench terrains (noise x 100, another seed per model), (B, H, H)."""
    p = soil.noise_t()
    p.ext = [H, H]
    out = silt.tensor(silt.int32, silt.shape(B, H, H), silt.gpu)
    per = out.nbytes() // B
    for b in range(B):
        p.seed = float(5 + b)
        if on_host:
            one = silt.tensor.from_numpy(soil.noise(silt.shape(H, H), p).numpy() * np.float32(100.0)).gpu()
        else:
            one = soil.noise(silt.shape(H, H), p, host=silt.gpu)
            silt.multiply(one, 100.0)
        g = soil.steepest(one, soil.d8)
        _abi.check(_abi.lib().soil_memcpy_d2d(C.c_void_p(out.ptr + b * per), g.c_ptr, per, _abi.stream()))
    _abi.check(_abi.lib().soil_stream_synchronize(_abi.stream()))
    return out


def figures(lib, routes, args):
    for _, call in routes:
        for _ in range(args.warmup):
            call()
    medians = {key: [] for key, _ in routes}
    for _ in range(args.repeats):
        for key, call in routes:
            medians[key].append(statistics.median(timed(lib, call, args.iters)))
    line = {"iters": args.iters, "repeats": args.repeats, "warmup": args.warmup}
    for key, meds in medians.items():
        line[key + "_ms"] = round(statistics.median(meds), 4)
        line[key + "_ms_spread"] = round(max(meds) - min(meds), 4)
    return line


def emit(line, args):
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default=None, help="H,... (default with neither option: %s)" % SINGLE)
    ap.add_argument("--batch", default=None, help="H:B,... (default with neither option: %s)" % BATCH)
    ap.add_argument("--iters", type=int, default=20, help="timed calls per median")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=0, help="the new route alone, this many calls, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.single is None and args.batch is None:
        args.single, args.batch = SINGLE, BATCH
    lib = _abi.lib()
    edge = soil.d8
    for H in [int(v) for v in (args.single or "").split(",") if v]:
        graph = model_view(graphs(1, H, on_host=bool(args.count)), 0)
        if args.count:
            for _ in range(args.count):
                soil.flow_paths(graph, edge, SCALE)
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "count": args.count, "route": "flow_paths, all three outputs"}, args)
            continue
        import torch
        g64 = graph.view_torch().view(-1).long()
        own = torch.arange(H * H, device="cuda")
        rounds = max(1, int(np.ceil(np.log2(H * H))))
        ones = silt.tensor(silt.float32, silt.shape(H, H), silt.gpu)
        silt.set(ones, 1.0)

        def by_torch():
            ptr = torch.where(g64 >= 0, g64, own)
            for _ in range(rounds):
                ptr = ptr.gather(0, ptr)
            return ptr

        line = {"H": H, "what": "single", "torch_rounds": rounds}
        line.update(figures(lib, [("paths_terminal", lambda: soil.basins(graph, edge)),
                                  ("paths_all", lambda: soil.flow_paths(graph, edge, SCALE)),
                                  ("torch", by_torch),
                                  ("accumulate", lambda: soil.accumulate(graph, ones, edge))], args))
        worst = max(line["paths_terminal_ms"] + line["paths_terminal_ms_spread"],
                    line["paths_all_ms"] + line["paths_all_ms_spread"])
        line["holds"] = bool(worst < line["torch_ms"] - line["torch_ms_spread"])
        line["torch_over_paths_all"] = round(line["torch_ms"] / line["paths_all_ms"], 2)
        line["accumulate_over_paths_all"] = round(line["accumulate_ms"] / line["paths_all_ms"], 2)
        emit(line, args)
        g64 = own = ones = graph = None
        torch.cuda.empty_cache()
        silt.empty_cache()
    for cfg in [v for v in (args.batch or "").split(",") if v]:
        H, B = (int(v) for v in cfg.split(":"))
        graph = graphs(B, H, on_host=bool(args.count))
        scales = [(SCALE[0] * (1 + b % 3), SCALE[1]) for b in range(B)]
        if args.count:
            for _ in range(args.count):
                soil.flow_paths_batch(graph, edge, scales)
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "B": B, "count": args.count, "route": "flow_paths_batch, all three outputs"}, args)
            continue
        models = [model_view(graph, b) for b in range(B)]

        def single():
            out = None
            for b, g in enumerate(models):
                out = soil.flow_paths(g, edge, scales[b])
            return out

        line = {"H": H, "B": B, "what": "batch"}
        line.update(figures(lib, [("batch", lambda: soil.flow_paths_batch(graph, edge, scales)), ("single", single)], args))
        a, s, spread = line["batch_ms"], line["single_ms"], line["single_ms_spread"]
        line["batch_ms_per_model"] = round(a / B, 5)
        line["single_over_batch"] = round(s / a, 2)
        line["holds"] = bool(a <= s + spread) if B == 1 else bool(a < s - spread)
        emit(line, args)
        graph = models = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
