#!/usr/bin/env python
"""The stream-power step with a slope exponent above 1 (include/soil_hip.h: soil_stream_power_n and its _batch form;
DESIGN.md 3.5 "Slope exponents above 1"), timed in one process on the conditioned D8 graph of the bench terrain (noise
x 100, soil.condition) at H x H, exponent `--exponent` (default 2), `--n` Newton steps a call (default 8):

  --single H,...
      power_n     soil.stream_power_n(filled, graph, k, scale, dt, exponent, uplift, iters=n)
      floor       (n + 1) x soil.stream_power on the same planes: the engine work the call contains (the start and n
                  solves), through an entry this feature left as it was.  What the call adds to it is the new init
                  pass's 8-byte gather of the receiver's iterate and its fp64 power, and the iterate kept by the final
  --batch H:B,...
      batch       soil.stream_power_n_batch on B models
      single      soil.stream_power_n on the same models one at a time
  --convergence H,...
      the residual after 1, 2, ... `--steps` Newton steps for the exponents 1.5, 2 and 3 (one call per count: a call
      reports the change of its last step), and the first count at which it is below 1e-9 of the height range

One JSON line per size.  A figure is the median of --repeats medians, each over --iters calls (device events around
every call) after --warmup calls, the routes alternated repeat by repeat; the spread beside it is the greatest minus
the least of those medians.  `power_n_over_floor` is the ratio of the two, `ratio_low` / `ratio_high` what the spreads
leave of it; (batch) `batch_faster`: the batch lies below the loop by more than the loop's spread.  None of them is a
threshold: the figures are what is reported.

--count N, for a kernel trace: N calls of power_n (or of the batch route), untimed.
    rocprofv3 --kernel-trace --stats -- python tools/bench_stream_power_n.py --single 1024 --count 10"""
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
BATCH = "256:8,256:64"
CONVERGENCE = "1024"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default=None, help="H,... (default with no option: %s)" % SINGLE)
    ap.add_argument("--batch", default=None, help="H:B,... (default with no option: %s)" % BATCH)
    ap.add_argument("--convergence", default=None, help="H,... (default with no option: %s)" % CONVERGENCE)
    ap.add_argument("--exponent", type=float, default=2.0, help="the slope exponent of the timed calls")
    ap.add_argument("--n", type=int, default=8, help="Newton steps of a timed call")
    ap.add_argument("--steps", type=int, default=16, help="the largest count of --convergence")
    ap.add_argument("--iters", type=int, default=20, help="timed calls per median")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=0, help="the new route alone, this many calls, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.single is None and args.batch is None and args.convergence is None:
        args.single, args.batch, args.convergence = SINGLE, BATCH, CONVERGENCE
    lib = _abi.lib()
    edge, n, expo = soil.d8, args.n, args.exponent
    for H in [int(v) for v in (args.single or "").split(",") if v]:
        import torch
        batch1 = terrains(1, H)
        filled, graph, k, uplift = (model_view(t, 0) for t in batch1)
        power_n = lambda: soil.stream_power_n(filled, graph, k, edge, SCALE, DT, expo, uplift, None, n)  # noqa: E731
        if args.count:
            for _ in range(args.count):
                power_n()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "count": args.count, "n": n, "exponent": expo, "route": "stream_power_n",
                  "info": soil.stream_power_n_info()}, args)
            continue

        def floor():
            out = None
            for _ in range(n + 1):
                out = soil.stream_power(filled, graph, k, edge, SCALE, DT, uplift)
            return out

        ours = soil.stream_power_n(filled, graph, k, edge, SCALE, DT, expo, uplift, None, n, True, True)
        start = soil.stream_power(filled, graph, k, edge, SCALE, DT, uplift, double=True)
        line = {"H": H, "what": "single", "n": n, "exponent": expo, "residual": float(ours[1].view_torch()[0]),
                "max_abs_from_the_n1_step": float((ours[0].view_torch() - start.view_torch()).abs().max()),
                "info": soil.stream_power_n_info()}
        line.update(figures(lib, [("power_n", power_n), ("floor", floor)], args))
        a, f = line["power_n_ms"], line["floor_ms"]
        da, df = line["power_n_ms_spread"], line["floor_ms_spread"]
        line["power_n_over_floor"] = round(a / f, 3)
        line["ratio_low"], line["ratio_high"] = round((a - da) / (f + df), 3), round((a + da) / max(f - df, 1e-9), 3)
        emit(line, args)
        batch1 = filled = graph = k = uplift = ours = start = None
        torch.cuda.empty_cache()
        silt.empty_cache()
    for cfg in [v for v in (args.batch or "").split(",") if v]:
        H, B = (int(v) for v in cfg.split(":"))
        filled, graph, k, uplift = terrains(B, H)
        scales = [(SCALE[0] * (1 + b % 3), SCALE[1]) for b in range(B)]
        batch = lambda: soil.stream_power_n_batch(filled, graph, k, edge, scales, DT, expo, uplift, None, n)  # noqa: E731
        if args.count:
            for _ in range(args.count):
                batch()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "B": B, "count": args.count, "n": n, "exponent": expo, "route": "stream_power_n_batch"}, args)
            continue
        models = [[model_view(t, b) for t in (filled, graph, k, uplift)] for b in range(B)]

        def single():
            out = None
            for b, (f, gr, kk, u) in enumerate(models):
                out = soil.stream_power_n(f, gr, kk, edge, scales[b], DT, expo, u, None, n)
            return out

        line = {"H": H, "B": B, "what": "batch", "n": n, "exponent": expo}
        line.update(figures(lib, [("batch", batch), ("single", single)], args))
        a, s, spread = line["batch_ms"], line["single_ms"], line["single_ms_spread"]
        line["batch_ms_per_model"] = round(a / B, 5)
        line["single_over_batch"] = round(s / a, 2)
        line["batch_faster"] = bool(a < s - spread)
        emit(line, args)
        filled = graph = k = uplift = models = None
        silt.empty_cache()
    for H in [int(v) for v in (args.convergence or "").split(",") if v]:
        filled, graph, k, uplift = (model_view(t, 0) for t in terrains(1, H))
        h = filled.view_torch()
        span = float(h.max() - h.min())
        for e in (1.5, 2.0, 3.0):
            res = []
            for steps in range(1, args.steps + 1):
                r = soil.stream_power_n(filled, graph, k, edge, SCALE, DT, e, uplift, None, steps, False, True)[1]
                res.append(float(r.view_torch()[0]))
            below = [i + 1 for i, v in enumerate(res) if v < 1e-9 * span]
            emit({"H": H, "what": "convergence", "exponent": e, "height_range": round(span, 3),
                  "residual_after": [float("%.3g" % v) for v in res], "first_below_1e-9_of_range": below[0] if below else None}, args)
        filled = graph = k = uplift = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
