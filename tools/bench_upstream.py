#!/usr/bin/env python
"""Upstream extrema and breaching (include/soil_hip.h: soil_upstream_extreme and its _batch form; DESIGN.md 3.5
"Upstream extrema and breaching"), timed in one process against the same-shaped reduction the library had and against
what a user writes today, on the conditioned D8 graph of the bench terrain (noise x 100, soil.condition) at H x H with
the ORIGINAL heights as the value plane — the breaching call:

  --single H,...
      upstream         soil.upstream_min(graph, height)             out alone
      upstream_arg     soil.upstream_min(graph, height, arg=True)   out and arg: the same kernels, one more store
      accumulate       soil.accumulate(graph, ones)                 the upstream SUM on the same graph, in a fixed order
      torch            the device-side loop a user writes today: int64 keys of the heights, int64 pointers,
                       M = M.scatter_reduce(0, J, M, "amin"); J = J[J], ceil(log2(H W)) times, the keys turned back
                       into floats — the same bits (checked before timing); no edge rule (the pointers are handed to
                       it ready-made), no arg
      condition / condition_breached   for information: what carving costs on top of filling and routing
  --batch H:B,...  soil.upstream_min_batch on B models against soil.upstream_min on the same models one at a time

One JSON line per size.  A figure is the median of --repeats medians, each over --iters calls (device events around
every call) after --warmup calls, the routes alternated repeat by repeat; the spread beside it is the greatest minus
the least of those medians.  `holds_a`: upstream is no slower than accumulate by more than the two spreads together;
`holds_b`: upstream lies below torch by more than both spreads; (batch) `holds`: the batch lies below the
one-at-a-time route by more than that route's spread.

--count N, for a kernel trace: N calls of upstream_min (with --batch: of upstream_min_batch), untimed; the set-up's
kernels (noise, the conditioning) are in the trace once.
    rocprofv3 --kernel-trace --stats -- python tools/bench_upstream.py --single 1024 --count 10"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402
from tools.bench_flow_batch import model_view  # noqa: E402
from tools.bench_flow_paths import emit, figures  # noqa: E402

SINGLE = "256,1024,4096,8192"
BATCH = "256:8,256:64,256:256"


def terrains(B, H):
    """B bench terrains (noise x 100, another seed per model) and their conditioned D8 graphs, (B, H, H) on the
    device."""
    p = soil.noise_t()
    p.ext = [H, H]
    height = silt.tensor(silt.float32, silt.shape(B, H, H), silt.gpu)
    per = height.nbytes() // B
    for b in range(B):
        p.seed = float(5 + b)
        one = soil.noise(silt.shape(H, H), p, host=silt.gpu)
        silt.multiply(one, 100.0)
        _abi.check(_abi.lib().soil_memcpy_d2d(height.ptr + b * per, one.c_ptr, per, _abi.stream()))
    _, graph = soil.condition_batch(height, soil.d8)
    _abi.check(_abi.lib().soil_stream_synchronize(_abi.stream()))
    return height, graph


def torch_route(height, graph, H):
    """The loop of the issue: the pointers are prepared outside the timed window, the keys inside it."""
    import torch
    g = graph.view_torch().view(-1).long()
    own = torch.arange(H * H, device="cuda")
    ptr0 = torch.where(g >= 0, g, own)                             # (a conditioned graph: an entry >= 0 is an edge)
    h = height.view_torch().view(-1)
    rounds = max(1, int(np.ceil(np.log2(H * H))))

    def run():
        u = h.view(torch.int32).long() & 0xFFFFFFFF
        M = torch.where(u >> 31 != 0, ~u & 0xFFFFFFFF, u | 0x80000000)          # (no NaN on the bench terrain)
        J = ptr0
        for _ in range(rounds):
            M = M.scatter_reduce(0, J, M, "amin", include_self=True)
            J = J[J]
        bits = torch.where(M >> 31 != 0, M & 0x7FFFFFFF, ~M & 0xFFFFFFFF)
        return torch.where(bits >= 1 << 31, bits - (1 << 32), bits).int().view(torch.float32)
    return run, rounds


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
        import torch
        height, graph = (model_view(t, 0) for t in terrains(1, H))
        if args.count:
            for _ in range(args.count):
                soil.upstream_min(graph, height, edge)
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "count": args.count, "route": "upstream_min", "info": soil.upstream_info()}, args)
            continue
        ones = silt.tensor(silt.float32, silt.shape(H, H), silt.gpu)
        silt.set(ones, 1.0)
        by_torch, rounds = torch_route(height, graph, H)
        ours = soil.upstream_min(graph, height, edge).view_torch().view(-1).view(torch.int32)
        theirs = by_torch().view(torch.int32)
        cut = int((ours != height.view_torch().view(-1).view(torch.int32)).sum())
        line = {"H": H, "what": "single", "rounds": rounds, "torch_same_bits": bool((ours == theirs).all()),
                "cells_cut": cut}
        line.update(figures(lib, [("upstream", lambda: soil.upstream_min(graph, height, edge)),
                                  ("upstream_arg", lambda: soil.upstream_min(graph, height, edge, arg=True)),
                                  ("accumulate", lambda: soil.accumulate(graph, ones, edge)),
                                  ("torch", by_torch)], args))
        few = argparse.Namespace(iters=3, repeats=3, warmup=1)     # (the fill synchronises and is slow: for information)
        info = figures(lib, [("condition", lambda: soil.condition(height, edge)),
                             ("condition_breached", lambda: soil.condition_breached(height, edge))], few)
        line.update({k: v for k, v in info.items() if k.startswith("condition")})
        spread = line["upstream_ms_spread"]
        line["holds_a"] = bool(line["upstream_ms"] <= line["accumulate_ms"] + spread + line["accumulate_ms_spread"])
        line["holds_a_arg"] = bool(line["upstream_arg_ms"] <= line["accumulate_ms"] + line["upstream_arg_ms_spread"] +
                                   line["accumulate_ms_spread"])
        line["holds_b"] = bool(line["upstream_ms"] + spread < line["torch_ms"] - line["torch_ms_spread"])
        line["upstream_over_accumulate"] = round(line["upstream_ms"] / line["accumulate_ms"], 3)
        line["upstream_arg_over_accumulate"] = round(line["upstream_arg_ms"] / line["accumulate_ms"], 3)
        line["torch_over_upstream"] = round(line["torch_ms"] / line["upstream_ms"], 2)
        line["condition_breached_over_condition"] = round(line["condition_breached_ms"] / line["condition_ms"], 3)
        emit(line, args)
        height = graph = ones = by_torch = ours = theirs = None
        torch.cuda.empty_cache()
        silt.empty_cache()
    for cfg in [v for v in (args.batch or "").split(",") if v]:
        H, B = (int(v) for v in cfg.split(":"))
        height, graph = terrains(B, H)
        if args.count:
            for _ in range(args.count):
                soil.upstream_min_batch(graph, height, edge)
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "B": B, "count": args.count, "route": "upstream_min_batch", "info": soil.upstream_info()}, args)
            continue
        models = [[model_view(t, b) for t in (graph, height)] for b in range(B)]

        def single():
            out = None
            for g, h in models:
                out = soil.upstream_min(g, h, edge)
            return out

        line = {"H": H, "B": B, "what": "batch"}
        line.update(figures(lib, [("batch", lambda: soil.upstream_min_batch(graph, height, edge)), ("single", single)], args))
        a, s, spread = line["batch_ms"], line["single_ms"], line["single_ms_spread"]
        line["batch_ms_per_model"] = round(a / B, 5)
        line["single_over_batch"] = round(s / a, 2)
        line["holds"] = bool(a < s - spread)
        emit(line, args)
        height = graph = models = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
