#!/usr/bin/env python
"""The stream-power step with sediment deposition (include/soil_hip.h: soil_stream_power_deposit and its _batch form;
DESIGN.md 3.5 "Erosion-deposition"), timed in one process on the conditioned D8 graph of the bench terrain (noise x
100, soil.condition) at H x H, `--n` iterations a call (default 8):

  --single H,...
      deposit     soil.stream_power_deposit(filled, graph, k, g, scale, dt, uplift, iters=n)
      floor       (a) n x (soil.accumulate_batch + soil.stream_power) on the same graph: the work the call contains,
                  through entries this feature left as they were
      composed    (b) the route through the public Python calls a user had before: per iteration q by torch,
                  soil.accumulate_batch, the coefficients by torch in fp64 squeezed into float32 `a` / `b` planes,
                  soil.downstream(a, b, terminal); F, g, d, B0 and the lifted heights are made once, outside the timed
                  window
  --batch H:B,...
      batch       soil.stream_power_deposit_batch on B models
      single      (c) soil.stream_power_deposit on the same models one at a time

One JSON line per size.  A figure is the median of --repeats medians, each over --iters calls (device events around
every call) after --warmup calls, the routes alternated repeat by repeat; the spread beside it is the greatest minus
the least of those medians.  `deposit_over_floor` is the ratio to (a); `not_slower_than_composed`: deposit lies below
(b) plus both spreads; (batch) `batch_faster`: the batch lies below the loop by more than the loop's spread.  None of
them is a threshold: the figures are what is reported.

--count N, for a kernel trace: N calls of deposit (or of the batch route), untimed.
    rocprofv3 --kernel-trace --stats -- python tools/bench_deposition.py --single 1024 --count 10"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402
from tools.bench_downstream import DT, SCALE, terrains  # noqa: E402
from tools.bench_flow_batch import model_view  # noqa: E402
from tools.bench_flow_paths import emit, figures  # noqa: E402

SINGLE = "256,1024,4096"
BATCH = "256:8,256:64,256:256"
G = 1.0


def planes(B, H):
    """terrains() and the deposition plane G cell / area of the same graphs, each (B, H, H) on the device."""
    filled, graph, k, uplift = terrains(B, H)
    ones = silt.tensor(silt.float32, silt.shape(B, H, H), silt.gpu)
    silt.set(ones, 1.0)
    g = soil.deposition(soil.accumulate_batch(graph, ones, soil.d8), G, SCALE[0] * SCALE[1])
    _abi.check(_abi.lib().soil_stream_synchronize(_abi.stream()))
    return filled, graph, k, uplift, g


def composed_route(filled, graph, k, uplift, g, H, n):
    """(b): `filled` ... `g` are the (1, H, H) tensors; every plane that does not change with the iterate is made here."""
    import numpy as np
    import torch
    gr = graph.view_torch().view(-1).long()
    own = torch.arange(H * H, device="cuda")
    edge = gr >= 0                                                 # (a conditioned graph: an entry >= 0 is an edge)
    ptr = torch.where(edge, gr, own)
    dx, dy = ptr // H - own // H, ptr % H - own % H
    sx, sy = float(np.float32(SCALE[0])), float(np.float32(SCALE[1]))
    L = torch.full((H * H,), float(np.sqrt(sx * sx + sy * sy)), dtype=torch.float64, device="cuda")
    L[dx == 0], L[dy == 0] = sy, sx
    h, kk, u, gg = (t.view_torch().view(-1).double() for t in (filled, k, uplift, g))
    F = kk * DT / L
    d = (1.0 + F) + gg
    b = h + DT * u
    lead = (1.0 + gg) * b
    B0 = silt.tensor.from_torch(torch.where(edge, F / d, torch.zeros_like(F)).float().view(H, H).contiguous())
    graph2, height2 = model_view(graph, 0), model_view(filled, 0)
    zero = torch.zeros((), dtype=torch.float32, device="cuda")

    def run():
        x = torch.where(edge, b, h)
        for i in range(n):
            q = torch.where(edge, (b - x).float(), zero)
            if i:
                Qs = soil.accumulate_batch(graph, silt.tensor.from_torch(q.view(1, H, H)), soil.d8).view_torch().view(-1)
                A0 = (lead + gg * (Qs.double() - q.double())) / d
            else:
                A0 = lead / d
            a = silt.tensor.from_torch(A0.float().view(H, H))
            x = soil.downstream(graph2, soil.d8, a=a, b=B0, terminal=height2, double=True).view_torch().view(-1)
        return x
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default=None, help="H,... (default with neither option: %s)" % SINGLE)
    ap.add_argument("--batch", default=None, help="H:B,... (default with neither option: %s)" % BATCH)
    ap.add_argument("--n", type=int, default=8, help="iterations of a deposit call")
    ap.add_argument("--iters", type=int, default=20, help="timed calls per median")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=0, help="the new route alone, this many calls, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.single is None and args.batch is None:
        args.single, args.batch = SINGLE, BATCH
    lib = _abi.lib()
    edge, n = soil.d8, args.n
    for H in [int(v) for v in (args.single or "").split(",") if v]:
        import torch
        batch1 = planes(1, H)
        filled, graph, k, uplift, g = (model_view(t, 0) for t in batch1)
        deposit = lambda: soil.stream_power_deposit(filled, graph, k, g, edge, SCALE, DT, uplift, n)  # noqa: E731
        if args.count:
            for _ in range(args.count):
                deposit()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "count": args.count, "n": n, "route": "stream_power_deposit", "info": soil.stream_power_deposit_info()}, args)
            continue
        ones = silt.tensor(silt.float32, silt.shape(1, H, H), silt.gpu)
        silt.set(ones, 1.0)

        def floor():
            out = None
            for _ in range(n):
                soil.accumulate_batch(batch1[1], ones, edge)
                out = soil.stream_power(filled, graph, k, edge, SCALE, DT, uplift)
            return out

        composed = composed_route(*batch1, H, n)
        ours = soil.stream_power_deposit(filled, graph, k, g, edge, SCALE, DT, uplift, n, True, residual=True)
        theirs = composed().view(H, H)
        line = {"H": H, "what": "single", "n": n, "G": G, "residual": float(ours[1].view_torch()[0]),
                "composed_max_abs_diff": float((ours[0].view_torch() - theirs).abs().max()),
                "info": soil.stream_power_deposit_info()}
        line.update(figures(lib, [("deposit", deposit), ("floor", floor), ("composed", composed)], args))
        line["deposit_over_floor"] = round(line["deposit_ms"] / line["floor_ms"], 3)
        line["composed_over_deposit"] = round(line["composed_ms"] / line["deposit_ms"], 3)
        line["not_slower_than_composed"] = bool(
            line["deposit_ms"] <= line["composed_ms"] + line["deposit_ms_spread"] + line["composed_ms_spread"])
        emit(line, args)
        batch1 = filled = graph = k = uplift = g = ones = composed = ours = theirs = None
        torch.cuda.empty_cache()
        silt.empty_cache()
    for cfg in [v for v in (args.batch or "").split(",") if v]:
        H, B = (int(v) for v in cfg.split(":"))
        filled, graph, k, uplift, g = planes(B, H)
        scales = [(SCALE[0] * (1 + b % 3), SCALE[1]) for b in range(B)]
        batch = lambda: soil.stream_power_deposit_batch(filled, graph, k, g, edge, scales, DT, uplift, n)  # noqa: E731
        if args.count:
            for _ in range(args.count):
                batch()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "B": B, "count": args.count, "n": n, "route": "stream_power_deposit_batch"}, args)
            continue
        models = [[model_view(t, b) for t in (filled, graph, k, g, uplift)] for b in range(B)]

        def single():
            out = None
            for b, (f, gr, kk, gg, u) in enumerate(models):
                out = soil.stream_power_deposit(f, gr, kk, gg, edge, scales[b], DT, u, n)
            return out

        line = {"H": H, "B": B, "what": "batch", "n": n, "G": G}
        line.update(figures(lib, [("batch", batch), ("single", single)], args))
        a, s, spread = line["batch_ms"], line["single_ms"], line["single_ms_spread"]
        line["batch_ms_per_model"] = round(a / B, 5)
        line["single_over_batch"] = round(s / a, 2)
        line["batch_faster"] = bool(a < s - spread)
        emit(line, args)
        filled = graph = k = uplift = g = models = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
