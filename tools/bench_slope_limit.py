#!/usr/bin/env python
"""Threshold hillslopes (include/soil_hip.h: soil_slope_limit, soil_slope_limit_batch; DESIGN.md 3.5 "Threshold
hillslopes"), timed in one process against what a user had before it, on the bench terrain of tools/bench_diffuse.py
(noise x 100) after one soil.stream_power step on its conditioned graph, at H x H, D8.  The generator stretches one
noise field over the grid whatever H is, so the cell size is 256 / H along both axes: the terrain keeps its extent and
its slopes from size to size, and one critical slope stays informative at every size:

  --single H,...
      slope_limit      soil.slope_limit(carved, scale, slope)
      torch            the device-side loop a user writes today: per sweep eight shifted adds and torch.minimum on the
                       same plane (float32, +inf beyond the border), torch.equal with the plane of --torch-check sweeps
                       before to decide whether to go on.  Its result must be the same bits.
      fill, diffuse    soil.fill_depressions and soil.diffuse on the same grid: the sibling terms of a step
  --batch H:B,...  soil.slope_limit_batch on B models against soil.slope_limit on the same models one at a time

The slope: of --slopes, the one whose share of lowered cells at 256^2 lies nearest one half (it must lie in 0.2 .. 0.8;
the share is counted on the numpy restatement of tests/slope_limit_ref.py there, and on the call's own result, which
equals the torch route's bit for bit, at every size).  One JSON line per size with the share, the launches and the
looks.  A figure is the median of --repeats medians, each over --iters calls (device events around every call) after
--warmup calls, the routes alternated repeat by repeat; the spread beside it is the greatest minus the least of those
medians.  `holds_torch`: slope_limit lies below the torch route by more than both spreads; (batch) `holds`: for B >= 8
the batch lies below the one-at-a-time route by more than that route's spread.

--count N, for a kernel trace: N calls of slope_limit (or of the batch route) and nothing else timed:
    rocprofv3 --kernel-trace --stats -- python tools/bench_slope_limit.py --single 4096 --count 10"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402
from tools.bench_diffuse import heights  # noqa: E402
from tools.bench_flow_batch import model_view  # noqa: E402
from tools.bench_flow_paths import emit, figures  # noqa: E402

SINGLE = "256,1024,4096,8192"
BATCH = "256:8,256:64,256:256,512:8,512:64"
KC, M, DT = 2e-3, 0.5, 7.0                                           # the stream-power step that carves the terrain
DX = (-1, 0, 0, 1, -1, -1, 1, 1)
DY = (0, -1, 1, 0, -1, 1, -1, 1)


def cell(H):
    return (256.0 / H, 256.0 / H)


def carved(height):
    """One stream_power step of every model of a (B, H, H) tensor on its conditioned graph."""
    scale = cell(height.shape[1])
    filled, graph = soil.condition_batch(height, soil.d8)
    ones = silt.tensor(silt.float32, silt.shape(*height.shape), silt.gpu)
    silt.set(ones, 1.0)
    k = soil.erosivity(soil.accumulate_batch(graph, ones, soil.d8), KC, M)
    return soil.stream_power_batch(filled, graph, k, soil.d8, scale, DT)


def share(h, w):
    return float((w.view_torch() < h.view_torch()).float().mean())


def torch_route(h, scale, slope, check):
    """(run, sweeps): the Jacobi loop in torch; sweeps[0] is the number of sweeps of the last run."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    H, W = h.shape
    c = [float(np.float32(np.float64(np.float32(slope)) * L)) for L in (float(scale[0]), float(scale[1]), np.sqrt(float(scale[0]) ** 2 + float(scale[1]) ** 2))]
    step = [c[2] if k >= 4 else (c[0] if DX[k] else c[1]) for k in range(8)]
    sweeps = [0]

    def run():
        w = h.view_torch().clone()
        n = 0
        while True:
            before = w
            for _ in range(check):
                p = F.pad(w, (1, 1, 1, 1), value=float("inf"))
                for k in range(8):
                    w = torch.minimum(w, p[1 + DX[k]:1 + DX[k] + H, 1 + DY[k]:1 + DY[k] + W] + step[k])
                n += 1
            if torch.equal(w, before):
                sweeps[0] = n
                return w
    return run, sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default=None, help="H,... (default with neither option: %s)" % SINGLE)
    ap.add_argument("--batch", default=None, help="H:B,... (default with neither option: %s)" % BATCH)
    ap.add_argument("--slopes", default="0.05,0.1,0.2,0.4,0.8,1.6,3.2", help="the candidates for the critical slope")
    ap.add_argument("--slope", type=float, default=None, help="the critical slope, without the choice at 256^2")
    ap.add_argument("--iters", type=int, default=20, help="timed calls per median")
    ap.add_argument("--torch-iters", type=int, default=1, help="timed calls per median of the torch route")
    ap.add_argument("--torch-check", type=int, default=8, help="sweeps of the torch route between two torch.equal")
    ap.add_argument("--no-torch-above", type=int, default=8192, help="no torch route above this H")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=0, help="the new route alone, this many calls, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.single is None and args.batch is None:
        args.single, args.batch = SINGLE, BATCH
    lib = _abi.lib()
    import torch
    slope = args.slope
    if slope is None:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import slope_limit_ref as ref
        h = model_view(carved(heights(1, 256)), 0)
        sc = cell(256)
        shares = {s: share(h, soil.slope_limit(h, sc, s)) for s in (float(v) for v in args.slopes.split(","))}
        slope = min(shares, key=lambda s: abs(shares[s] - 0.5))
        want = ref.jacobi(h.cpu().numpy(), sc, slope, ref.D8)
        got = soil.slope_limit(h, sc, slope).cpu().numpy()
        line = {"what": "slope", "slope": slope, "shares_at_256": shares, "reference_share": ref.lowered_share(h.cpu().numpy(), want),
                "same_bits_as_reference": ref.same_bits(got, want)}
        emit(line, args)
        assert 0.2 <= line["reference_share"] <= 0.8 and line["same_bits_as_reference"], line
    for H in [int(v) for v in (args.single or "").split(",") if v]:
        height = model_view(heights(1, H), 0)
        h = model_view(carved(heights(1, H)), 0)
        sc = cell(H)
        call = lambda: soil.slope_limit(h, sc, slope)
        if args.count:
            for _ in range(args.count):
                call()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "count": args.count, "route": "slope_limit", "slope": slope, **soil.slope_limit_info()}, args)
            continue
        ours = call()
        line = {"H": H, "what": "single", "slope": slope, "cell": sc[0], "share": round(share(h, ours), 4), **soil.slope_limit_info()}
        routes = [("slope_limit", call), ("fill", lambda: soil.fill_depressions(height, soil.d8)),
                  ("diffuse", lambda: soil.diffuse(height, sc, DT, kappa=sc[0] * sc[0]))]
        line.update(figures(lib, routes, args))
        if H <= args.no_torch_above:
            by_torch, sweeps = torch_route(h, sc, slope, args.torch_check)
            line["torch_same_bits"] = bool(torch.equal(by_torch().view(torch.int32), ours.view_torch().view(torch.int32)))
            line["torch_sweeps"] = sweeps[0]
            t_args = argparse.Namespace(iters=args.torch_iters, repeats=min(args.repeats, 3), warmup=1)
            t_line = figures(lib, [("torch", by_torch)], t_args)
            line.update({"torch_ms": t_line["torch_ms"], "torch_ms_spread": t_line["torch_ms_spread"],
                         "torch_iters": t_args.iters, "torch_repeats": t_args.repeats})
            line["holds_torch"] = bool(line["slope_limit_ms"] + line["slope_limit_ms_spread"] < line["torch_ms"] - line["torch_ms_spread"])
            line["torch_over_slope_limit"] = round(line["torch_ms"] / line["slope_limit_ms"], 1)
        line["slope_limit_over_fill"] = round(line["slope_limit_ms"] / line["fill_ms"], 2)
        line["slope_limit_over_diffuse"] = round(line["slope_limit_ms"] / line["diffuse_ms"], 2)
        emit(line, args)
        height = h = ours = by_torch = None
        torch.cuda.empty_cache()
        silt.empty_cache()
    for cfg in [v for v in (args.batch or "").split(",") if v]:
        H, B = (int(v) for v in cfg.split(":"))
        hs = carved(heights(B, H))
        sc = cell(H)
        scales = [(sc[0] * (1 + b % 3), sc[1]) for b in range(B)]
        batch = lambda: soil.slope_limit_batch(hs, scales, slope)
        if args.count:
            for _ in range(args.count):
                batch()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "B": B, "count": args.count, "route": "slope_limit_batch", "slope": slope, **soil.slope_limit_info()}, args)
            continue
        models = [model_view(hs, b) for b in range(B)]
        launches = []

        def single():
            out = None
            del launches[:]
            for b, m in enumerate(models):
                out = soil.slope_limit(m, scales[b], slope)
                launches.append(soil.slope_limit_info()["launches"])
            return out

        together = batch()
        info = soil.slope_limit_info()
        single()
        line = {"H": H, "B": B, "what": "batch", "slope": slope, "share": round(share(hs, together), 4),
                "batch_launches": info["launches"], "batch_looks": info["looks"], "single_launches_max": max(launches),
                "single_launches_sum": sum(launches)}
        line.update(figures(lib, [("batch", batch), ("single", single)], args))
        a, s, spread = line["batch_ms"], line["single_ms"], line["single_ms_spread"]
        line["batch_ms_per_model"] = round(a / B, 5)
        line["single_over_batch"] = round(s / a, 2)
        line["holds"] = bool(a < s - spread)
        emit(line, args)
        hs = models = together = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
