#!/usr/bin/env python
"""Downstream sums and the implicit stream-power step (include/soil_hip.h: soil_downstream, soil_stream_power and
their _batch forms; DESIGN.md 3.5 "Downstream sums and the stream-power step"), timed in one process against what a
user had before them, on the conditioned D8 graph of the bench terrain (noise x 100, soil.condition) at H x H:

  --single H,...
      downstream       soil.downstream(graph, scale=...)        a == b == 1, t == 0: the records alone, no B plane
      flow_paths       soil.flow_paths(graph, scale)            all three outputs: the same rounds, the same bytes
      stream_power     soil.stream_power(filled, graph, k, scale, dt, uplift)
      torch            the device-side loop a user writes today: fp64 coefficients made by torch from the same planes,
                       int64 pointers, A += B * A[p]; B *= B[p]; p = p[p], ceil(log2(H W)) times — no edge rule (the
                       pointers and the edge lengths are handed to it ready-made), no cycle mark
      accumulate       soil.accumulate(graph, ones): the yardstick of the same algorithm class
  --batch H:B,...  soil.stream_power_batch on B models against soil.stream_power on the same models one at a time

One JSON line per size.  A figure is the median of --repeats medians, each over --iters calls (device events around
every call) after --warmup calls, the routes alternated repeat by repeat; the spread beside it is the greatest minus
the least of those medians.  `holds_a`: downstream is no slower than flow_paths by more than the two spreads
together; `holds_b`: stream_power lies below torch by more than both spreads; (batch) `holds`: for B >= 8 the batch
lies below the one-at-a-time route by more than that route's spread.

--count N, for a kernel trace: with --batch the batch route alone, N calls; with --single N calls each of downstream,
flow_paths and stream_power, one route after the other.  Nothing is timed; the set-up's kernels (noise, the
conditioning, the drainage area) are in the trace once.
    rocprofv3 --kernel-trace --stats -- python tools/bench_downstream.py --batch 256:8 --count 10"""
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
BATCH = "256:8,256:64,256:256,512:8,512:64"
SCALE = (0.25, 3.0)
DT, K, M = 50.0, 2e-3, 0.5


def terrains(B, H):
    """B bench terrains (noise x 100, another seed per model) conditioned for D8: filled, graph, erosivity, uplift,
    each (B, H, H) on the device."""
    p = soil.noise_t()
    p.ext = [H, H]
    height = silt.tensor(silt.float32, silt.shape(B, H, H), silt.gpu)
    per = height.nbytes() // B
    for b in range(B):
        p.seed = float(5 + b)
        one = soil.noise(silt.shape(H, H), p, host=silt.gpu)
        silt.multiply(one, 100.0)
        _abi.check(_abi.lib().soil_memcpy_d2d(height.ptr + b * per, one.c_ptr, per, _abi.stream()))
    filled, graph = soil.condition_batch(height, soil.d8)
    ones = silt.tensor(silt.float32, silt.shape(B, H, H), silt.gpu)
    silt.set(ones, 1.0)
    k = soil.erosivity(soil.accumulate_batch(graph, ones, soil.d8), K, M)
    silt.set(ones, 0.01)                                           # the uplift plane
    _abi.check(_abi.lib().soil_stream_synchronize(_abi.stream()))
    return filled, graph, k, ones


def torch_route(filled, graph, k, uplift, H):
    """The loop of the issue, on planes prepared outside the timed window: int64 pointers and the edge lengths."""
    import torch
    g = graph.view_torch().view(-1).long()
    own = torch.arange(H * H, device="cuda")
    edge = g >= 0                                                  # (a conditioned graph: an entry >= 0 is an edge)
    ptr0 = torch.where(edge, g, own)
    dx, dy = ptr0 // H - own // H, ptr0 % H - own % H
    sx, sy = float(np.float32(SCALE[0])), float(np.float32(SCALE[1]))
    L = torch.full((H * H,), float(np.sqrt(sx * sx + sy * sy)), dtype=torch.float64, device="cuda")
    L[dx == 0], L[dy == 0] = sy, sx
    h, kk, u = (t.view_torch().view(-1) for t in (filled, k, uplift))
    rounds = max(1, int(np.ceil(np.log2(H * H))))

    def run():
        F = kk.double() * DT / L
        d = 1.0 + F
        A = torch.where(edge, (h.double() + DT * u.double()) / d, h.double())
        B = torch.where(edge, F / d, torch.zeros_like(F))
        p = ptr0
        for _ in range(rounds):
            A = A + B * A[p]
            B = B * B[p]
            p = p[p]
        return A.float()
    return run, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default=None, help="H,... (default with neither option: %s)" % SINGLE)
    ap.add_argument("--batch", default=None, help="H:B,... (default with neither option: %s)" % BATCH)
    ap.add_argument("--iters", type=int, default=20, help="timed calls per median")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=0, help="the routes alone, this many calls each, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.single is None and args.batch is None:
        args.single, args.batch = SINGLE, BATCH
    lib = _abi.lib()
    edge = soil.d8
    for H in [int(v) for v in (args.single or "").split(",") if v]:
        import torch
        filled, graph, k, uplift = (model_view(t, 0) for t in terrains(1, H))
        if args.count:
            for call in (lambda: soil.downstream(graph, edge, scale=SCALE), lambda: soil.flow_paths(graph, edge, SCALE),
                         lambda: soil.stream_power(filled, graph, k, edge, SCALE, DT, uplift)):
                for _ in range(args.count):
                    call()
                _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "count": args.count, "routes": "downstream, flow_paths, stream_power"}, args)
            continue
        ones = silt.tensor(silt.float32, silt.shape(H, H), silt.gpu)
        silt.set(ones, 1.0)
        by_torch, rounds = torch_route(filled, graph, k, uplift, H)
        ours = soil.stream_power(filled, graph, k, edge, SCALE, DT, uplift).view_torch()
        theirs = by_torch().view(H, H)
        line = {"H": H, "what": "single", "rounds": rounds,
                "torch_max_rel_diff": float(((ours - theirs).abs() / theirs.abs().clamp(min=1e-3)).max())}
        line.update(figures(lib, [("downstream", lambda: soil.downstream(graph, edge, scale=SCALE)),
                                  ("flow_paths", lambda: soil.flow_paths(graph, edge, SCALE)),
                                  ("stream_power", lambda: soil.stream_power(filled, graph, k, edge, SCALE, DT, uplift)),
                                  ("torch", by_torch),
                                  ("accumulate", lambda: soil.accumulate(graph, ones, edge))], args))
        line["holds_a"] = bool(line["downstream_ms"] <= line["flow_paths_ms"] + line["downstream_ms_spread"] + line["flow_paths_ms_spread"])
        line["holds_b"] = bool(line["stream_power_ms"] + line["stream_power_ms_spread"] < line["torch_ms"] - line["torch_ms_spread"])
        line["downstream_over_flow_paths"] = round(line["downstream_ms"] / line["flow_paths_ms"], 3)
        line["torch_over_stream_power"] = round(line["torch_ms"] / line["stream_power_ms"], 2)
        line["stream_power_over_accumulate"] = round(line["stream_power_ms"] / line["accumulate_ms"], 2)
        emit(line, args)
        filled = graph = k = uplift = ones = by_torch = ours = theirs = None
        torch.cuda.empty_cache()
        silt.empty_cache()
    for cfg in [v for v in (args.batch or "").split(",") if v]:
        H, B = (int(v) for v in cfg.split(":"))
        filled, graph, k, uplift = terrains(B, H)
        scales = [(SCALE[0] * (1 + b % 3), SCALE[1]) for b in range(B)]
        if args.count:
            for _ in range(args.count):
                soil.stream_power_batch(filled, graph, k, edge, scales, DT, uplift)
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "B": B, "count": args.count, "route": "stream_power_batch"}, args)
            continue
        models = [[model_view(t, b) for t in (filled, graph, k, uplift)] for b in range(B)]

        def single():
            out = None
            for b, (f, g, kk, u) in enumerate(models):
                out = soil.stream_power(f, g, kk, edge, scales[b], DT, u)
            return out

        line = {"H": H, "B": B, "what": "batch"}
        line.update(figures(lib, [("batch", lambda: soil.stream_power_batch(filled, graph, k, edge, scales, DT, uplift)),
                                  ("single", single)], args))
        a, s, spread = line["batch_ms"], line["single_ms"], line["single_ms_spread"]
        line["batch_ms_per_model"] = round(a / B, 5)
        line["single_over_batch"] = round(s / a, 2)
        line["holds"] = bool(a < s - spread)
        emit(line, args)
        filled = graph = k = uplift = models = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
