#!/usr/bin/env python
"""The implicit hillslope-diffusion step (include/soil_hip.h: soil_diffuse, soil_diffuse_batch; DESIGN.md 3.5
"Hillslope diffusion and the evolve step"), timed in one process against what a user had before it, on the bench
terrain (noise x 100) at H x H with w = kappa dt / s^2 = 7 along both axes, border = 1:

  --single H,...
      diffuse          soil.diffuse(height, scale, dt, kappa)
      torch            the device-side restatement a user writes today: the same two sweeps in fp64 torch, vectorised
                       across the lines and serial along them (no void cells, no mask, no diffusivity plane: the
                       coefficients of a scalar kappa are made once per position on the host)
      explicit         the explicit route at its stability limit: ceil(4 w) sub-steps of soil.laplacian +
                       silt.multiply + silt.add (another scheme: its result is compared loosely, not bit for bit)
      stream_power     soil.stream_power on the conditioned graph of the same grid: the sibling term of an evolve step
  --batch H:B,...  soil.diffuse_batch on B models against soil.diffuse on the same models one at a time

One JSON line per size.  A figure is the median of --repeats medians, each over --iters calls (device events around
every call) after --warmup calls, the routes alternated repeat by repeat; the spread beside it is the greatest minus
the least of those medians.  The torch route runs 4 H small kernels' worth of Python a call: it is timed over
--torch-iters calls a median.  `holds_torch`, `holds_explicit`: diffuse lies below the route by more than both spreads;
(batch) `holds`: for B >= 8 the batch lies below the one-at-a-time route by more than that route's spread.
`roofline_share`: the algorithmic bytes of a call with a scalar kappa and a float output — the first sweep reads h and
writes e and g (20), reads them back with h and writes x (28); the second reads h and x and writes e and g (28), reads
them back with h and writes the output (24): 100 bytes a cell — over the time, against 8 TB/s.

--count N, for a kernel trace: N calls of diffuse (or of the batch route) and nothing else timed:
    rocprofv3 --kernel-trace --stats -- python tools/bench_diffuse.py --single 4096 --count 10"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402
from tools.bench_flow_batch import model_view  # noqa: E402
from tools.bench_flow_paths import emit, figures  # noqa: E402

SINGLE = "256,1024,4096,8192"
BATCH = "256:8,256:64,256:256,512:8,512:64"
SCALE = (1.0, 1.0)
KAPPA, DT = 1.0, 7.0                                                 # w = 7 along both axes
BYTES_PER_CELL = 100                                                 # a step: 20 + 28 + 28 + 24 (the docstring)
PEAK = 8e12


def heights(B, H):
    """B bench terrains (noise x 100, another seed per model), (B, H, H) on the device."""
    p = soil.noise_t()
    p.ext = [H, H]
    height = silt.tensor(silt.float32, silt.shape(B, H, H), silt.gpu)
    per = height.nbytes() // B
    for b in range(B):
        p.seed = float(5 + b)
        one = soil.noise(silt.shape(H, H), p, host=silt.gpu)
        silt.multiply(one, 100.0)
        _abi.check(_abi.lib().soil_memcpy_d2d(height.ptr + b * per, one.c_ptr, per, _abi.stream()))
    _abi.check(_abi.lib().soil_stream_synchronize(_abi.stream()))
    return height


def torch_route(height, H):
    """The two sweeps in fp64 torch, border = 1, scalar kappa: p, q and the g of every position made once on the host
    (they do not depend on the heights), the e recurrence and the back-substitution a Python loop over the line."""
    import torch
    h = height.view_torch()
    w = KAPPA * DT / (SCALE[0] * SCALE[0])
    free = torch.ones(H, dtype=torch.bool)
    free[0] = free[-1] = False
    p = torch.where(free, torch.full((H,), w, dtype=torch.float64), torch.zeros(H, dtype=torch.float64))
    q = p.clone()
    den, g = [0.0] * H, [0.0] * H
    for i in range(H):
        b = 1.0 + float(p[i]) + float(q[i])
        den[i] = b - float(p[i]) * (g[i - 1] if i else 0.0)
        g[i] = float(q[i]) / den[i]
    p_l, inner = [float(v) for v in p], torch.ones(H, dtype=torch.bool, device="cuda")
    inner[0] = inner[-1] = False                                     # lines on the border are fixed from end to end

    def sweep(d):                                                    # along dim 0 of d (n, lines)
        e = torch.empty_like(d)
        e[0] = d[0]
        for i in range(1, H):
            e[i] = torch.where(inner, (d[i] + p_l[i] * e[i - 1]) / den[i], d[i])
        x = torch.empty_like(d)
        x[H - 1] = e[H - 1]
        for i in range(H - 2, -1, -1):
            x[i] = torch.where(inner, e[i] + g[i] * x[i + 1], e[i]) if p_l[i] else e[i]
        return x

    def run():
        x = sweep(h.double())
        return sweep(x.t().contiguous()).t().float()
    return run


def explicit_route(height, H):
    """ceil(4 w) explicit sub-steps: h += (kappa dt / n) laplacian(h)."""
    n = int(math.ceil(4.0 * KAPPA * DT / (SCALE[0] * SCALE[0])))
    src = silt.tensor.from_device(height.ptr, silt.float32, silt.shape(H, H, 1), keepalive=height)

    def run():
        h = silt.clone(src)
        for _ in range(n):
            lap = soil.laplacian(h, SCALE)
            silt.multiply(lap, KAPPA * DT / n)
            silt.add(h, lap)
        return h
    return run, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default=None, help="H,... (default with neither option: %s)" % SINGLE)
    ap.add_argument("--batch", default=None, help="H:B,... (default with neither option: %s)" % BATCH)
    ap.add_argument("--iters", type=int, default=20, help="timed calls per median")
    ap.add_argument("--torch-iters", type=int, default=1, help="timed calls per median of the torch route")
    ap.add_argument("--no-torch-above", type=int, default=8192, help="no torch route above this H")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=0, help="the new route alone, this many calls, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.single is None and args.batch is None:
        args.single, args.batch = SINGLE, BATCH
    lib = _abi.lib()
    for H in [int(v) for v in (args.single or "").split(",") if v]:
        import torch
        height = model_view(heights(1, H), 0)
        call = lambda: soil.diffuse(height, SCALE, DT, kappa=KAPPA)
        if args.count:
            for _ in range(args.count):
                call()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "count": args.count, "route": "diffuse"}, args)
            continue
        filled, graph = soil.condition(height, soil.d8)
        ones = silt.tensor(silt.float32, silt.shape(H, H), silt.gpu)
        silt.set(ones, 1.0)
        k = soil.erosivity(soil.accumulate(graph, ones, soil.d8), 2e-3, 0.5)
        by_explicit, substeps = explicit_route(height, H)
        ours = call().view_torch()
        line = {"H": H, "what": "single", "w": KAPPA * DT / SCALE[0] ** 2, "explicit_substeps": substeps,
                "explicit_max_abs_diff": float((ours - by_explicit().view_torch().view(H, H)).abs().max())}
        routes = [("diffuse", call), ("explicit", by_explicit),
                  ("stream_power", lambda: soil.stream_power(filled, graph, k, soil.d8, SCALE, DT))]
        line.update(figures(lib, routes, args))
        if H <= args.no_torch_above:
            by_torch = torch_route(height, H)
            line["torch_max_abs_diff"] = float((ours - by_torch()).abs().max())
            t_args = argparse.Namespace(iters=args.torch_iters, repeats=min(args.repeats, 3), warmup=1)
            t_line = figures(lib, [("torch", by_torch)], t_args)
            line.update({"torch_ms": t_line["torch_ms"], "torch_ms_spread": t_line["torch_ms_spread"],
                         "torch_iters": t_args.iters, "torch_repeats": t_args.repeats})
            line["holds_torch"] = bool(line["diffuse_ms"] + line["diffuse_ms_spread"] < line["torch_ms"] - line["torch_ms_spread"])
            line["torch_over_diffuse"] = round(line["torch_ms"] / line["diffuse_ms"], 1)
        line["holds_explicit"] = bool(line["diffuse_ms"] + line["diffuse_ms_spread"] < line["explicit_ms"] - line["explicit_ms_spread"])
        line["explicit_over_diffuse"] = round(line["explicit_ms"] / line["diffuse_ms"], 2)
        line["diffuse_over_stream_power"] = round(line["diffuse_ms"] / line["stream_power_ms"], 2)
        line["roofline_share"] = round(BYTES_PER_CELL * H * H / (line["diffuse_ms"] * 1e-3) / PEAK, 4)
        emit(line, args)
        height = filled = graph = k = ones = by_explicit = ours = None
        torch.cuda.empty_cache()
        silt.empty_cache()
    for cfg in [v for v in (args.batch or "").split(",") if v]:
        H, B = (int(v) for v in cfg.split(":"))
        height = heights(B, H)
        scales = [(SCALE[0] * (1 + b % 3), SCALE[1]) for b in range(B)]
        batch = lambda: soil.diffuse_batch(height, scales, DT, kappa=KAPPA)
        if args.count:
            for _ in range(args.count):
                batch()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "B": B, "count": args.count, "route": "diffuse_batch"}, args)
            continue
        models = [model_view(height, b) for b in range(B)]

        def single():
            out = None
            for b, m in enumerate(models):
                out = soil.diffuse(m, scales[b], DT, kappa=KAPPA)
            return out

        line = {"H": H, "B": B, "what": "batch"}
        line.update(figures(lib, [("batch", batch), ("single", single)], args))
        a, s, spread = line["batch_ms"], line["single_ms"], line["single_ms_spread"]
        line["batch_ms_per_model"] = round(a / B, 5)
        line["single_over_batch"] = round(s / a, 2)
        line["holds"] = bool(a < s - spread)
        line["roofline_share"] = round(BYTES_PER_CELL * B * H * H / (a * 1e-3) / PEAK, 4)
        emit(line, args)
        height = models = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
