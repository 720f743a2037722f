#!/usr/bin/env python
"""The erosion-deposition step at a slope exponent above 1 (include/soil_hip.h: soil_stream_power_deposit_n and its
_batch form; DESIGN.md 3.5 "Erosion-deposition at slope exponents above 1"), timed in one process on the conditioned D8
graph of the bench terrain (noise x 100, soil.condition) at H x H, exponent `--exponent` (default 2), G = 1, `--n`
iterations a call (default 8):

  --single H,...
      deposit_n   soil.stream_power_deposit_n(filled, graph, k, g, scale, dt, exponent, uplift, iters=n)
      floor       n x (soil.accumulate_batch + soil.stream_power) + soil.stream_power on the same planes: the engine
                  work the call contains (the start, n accumulations and n solves), through entries this feature left
                  as they were.  What the call adds to it is the q pass, the new init pass's 8-byte gather of the
                  receiver's iterate and its fp64 power, and the iterate kept by the final
      deposit     soil.stream_power_deposit at the same `iters`: the step at n = 1, the entry the library had
  --batch H:B,...
      batch       soil.stream_power_deposit_n_batch on B models
      single      soil.stream_power_deposit_n on the same models one at a time
  --map H,...
      the residual after 1, 2, ... `--steps` iterations (one call per count: a call reports the change of its last
      iteration) for the exponents 1.5, 2 and 3, G 0.5, 1 and 2, and K dt at the bench value and 100 times it: the first
      count at which it is below 1e-9 of the height range, and what it does otherwise — `floor`: the last four
      residuals lie within a factor of two of each other, far below the first; `diverges`: the last residual exceeds
      that of a quarter of the way; `falling`: neither yet; and `settled_at`, the first count from which every
      residual is within a factor of two of the least one (None where the last is not)
  --table FILE
      no device: the table of DESIGN.md from the --map lines of FILE, one row per (K dt, n, G), a cell per size

One JSON line per size (per case for --map).  A figure is the median of --repeats medians, each over --iters calls
(device events around every call) after --warmup calls, the routes alternated repeat by repeat; the spread beside it is
the greatest minus the least of those medians.  `deposit_n_over_floor` is the ratio of the two, `ratio_low` /
`ratio_high` what the spreads leave of it; (batch) `batch_faster`: the batch lies below the loop by more than the loop's
spread.  None of them is a threshold: the figures are what is reported.

--count N, for a kernel trace: N calls of deposit_n (or of the batch route), untimed.
    rocprofv3 --kernel-trace --stats -- python tools/bench_deposit_n.py --single 1024 --count 10"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402
from tools.bench_deposition import planes  # noqa: E402
from tools.bench_downstream import DT, SCALE  # noqa: E402
from tools.bench_flow_batch import model_view  # noqa: E402
from tools.bench_flow_paths import emit, figures  # noqa: E402

SINGLE = "256,1024,4096"
BATCH = "256:8,256:64"
MAP = "256,1024,4096"


def classify(res, span):
    """What the residuals of 1 .. len(res) iterations show: (first count below 1e-9 of the range or None, a word)."""
    below = [i + 1 for i, v in enumerate(res) if v < 1e-9 * span]
    if below:
        return below[0], "converges"
    tail = res[-4:]
    if max(tail) <= 2.0 * min(tail) and max(tail) < 1e-3 * max(res[:4]):
        return None, "floor"
    if res[-1] > res[len(res) // 4]:
        return None, "diverges"
    return None, "falling"


def settled_at(res):
    """The first count from which every residual is within a factor of two of the least one, or None."""
    least = min(res)
    return next((j + 1 for j in range(len(res)) if max(res[j:]) <= 2.0 * least), None)


def table(path):
    """The rows of DESIGN.md's table from the --map lines of `path`.  A cell: the first count below 1e-9 of the range;
    else `floor r from j` (r the least residual, j settled_at); else `falling: r (x f)` (the residual at the last count
    and its factor an iteration over the last eight); else `diverges (a -> b)` (after 4 counts and after the last)."""
    import json
    rows, sizes = {}, []
    for line in open(path):
        d = json.loads(line)
        if d.get("what") != "map":
            continue
        res = d["residual_after"]
        first, word = classify(res, d["height_range"])
        if first:
            cell = "%d" % first
        elif word == "floor":
            cell = "floor %.2g from %s" % (min(res), settled_at(res))
        elif word == "diverges":
            cell = "diverges (%.2g -> %.2g)" % (res[3], res[-1])
        else:
            cell = "falling: %.2g (x %.2f)" % (res[-1], (res[-1] / res[-9]) ** 0.125)
        rows.setdefault((d["K_dt_times"], d["exponent"], d["G"]), {})[d["H"]] = cell
        if d["H"] not in sizes:
            sizes.append(d["H"])
    print("| K dt | n | G | " + " | ".join("%d^2" % H for H in sizes) + " |")
    for (times, e, G), cells in rows.items():
        print("| %s | %g | %g | " % ("bench" if times == 1.0 else "x %g" % times, e, G)
              + " | ".join(cells.get(H, "") for H in sizes) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default=None, help="H,... (default with no option: %s)" % SINGLE)
    ap.add_argument("--batch", default=None, help="H:B,... (default with no option: %s)" % BATCH)
    ap.add_argument("--map", default=None, help="H,... (default with no option: %s)" % MAP)
    ap.add_argument("--exponent", type=float, default=2.0, help="the slope exponent of the timed calls")
    ap.add_argument("--n", type=int, default=8, help="iterations of a timed call")
    ap.add_argument("--steps", type=int, default=40, help="the largest count of --map")
    ap.add_argument("--iters", type=int, default=20, help="timed calls per median")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=0, help="the new route alone, this many calls, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--table", default=None, help="print DESIGN.md's table from the --map lines of this file; no device")
    args = ap.parse_args()
    if args.table:
        return table(args.table)
    if args.single is None and args.batch is None and args.map is None:
        args.single, args.batch, args.map = SINGLE, BATCH, MAP
    lib = _abi.lib()
    edge, n, expo = soil.d8, args.n, args.exponent
    for H in [int(v) for v in (args.single or "").split(",") if v]:
        import torch
        batch1 = planes(1, H)
        filled, graph, k, uplift, g = (model_view(t, 0) for t in batch1)
        deposit_n = lambda: soil.stream_power_deposit_n(filled, graph, k, g, edge, SCALE, DT, expo, uplift, n)  # noqa: E731
        if args.count:
            for _ in range(args.count):
                deposit_n()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "count": args.count, "n": n, "exponent": expo, "route": "stream_power_deposit_n",
                  "info": soil.stream_power_deposit_n_info()}, args)
            continue
        ones = silt.tensor(silt.float32, silt.shape(1, H, H), silt.gpu)
        silt.set(ones, 1.0)

        def floor():
            for _ in range(n):
                soil.accumulate_batch(batch1[1], ones, edge)
                soil.stream_power(filled, graph, k, edge, SCALE, DT, uplift)
            return soil.stream_power(filled, graph, k, edge, SCALE, DT, uplift)

        deposit = lambda: soil.stream_power_deposit(filled, graph, k, g, edge, SCALE, DT, uplift, n)  # noqa: E731
        ours = soil.stream_power_deposit_n(filled, graph, k, g, edge, SCALE, DT, expo, uplift, n, True, residual=True)
        plain = soil.stream_power_n(filled, graph, k, edge, SCALE, DT, expo, uplift, None, n, True)
        line = {"H": H, "what": "single", "n": n, "exponent": expo, "G": 1.0, "residual": float(ours[1].view_torch()[0]),
                "max_abs_from_stream_power_n": float((ours[0].view_torch() - plain.view_torch()).abs().max()),
                "info": soil.stream_power_deposit_n_info()}
        line.update(figures(lib, [("deposit_n", deposit_n), ("floor", floor), ("deposit", deposit)], args))
        a, f = line["deposit_n_ms"], line["floor_ms"]
        da, df = line["deposit_n_ms_spread"], line["floor_ms_spread"]
        line["deposit_n_over_floor"] = round(a / f, 3)
        line["ratio_low"], line["ratio_high"] = round((a - da) / (f + df), 3), round((a + da) / max(f - df, 1e-9), 3)
        line["deposit_n_over_deposit"] = round(a / line["deposit_ms"], 3)
        emit(line, args)
        batch1 = filled = graph = k = uplift = g = ones = ours = plain = None
        torch.cuda.empty_cache()
        silt.empty_cache()
    for cfg in [v for v in (args.batch or "").split(",") if v]:
        H, B = (int(v) for v in cfg.split(":"))
        filled, graph, k, uplift, g = planes(B, H)
        scales = [(SCALE[0] * (1 + b % 3), SCALE[1]) for b in range(B)]
        batch = lambda: soil.stream_power_deposit_n_batch(filled, graph, k, g, edge, scales, DT, expo, uplift, n)  # noqa: E731
        if args.count:
            for _ in range(args.count):
                batch()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "B": B, "count": args.count, "n": n, "exponent": expo, "route": "stream_power_deposit_n_batch"}, args)
            continue
        models = [[model_view(t, b) for t in (filled, graph, k, g, uplift)] for b in range(B)]

        def single():
            out = None
            for b, (f, gr, kk, gg, u) in enumerate(models):
                out = soil.stream_power_deposit_n(f, gr, kk, gg, edge, scales[b], DT, expo, u, n)
            return out

        line = {"H": H, "B": B, "what": "batch", "n": n, "exponent": expo, "G": 1.0}
        line.update(figures(lib, [("batch", batch), ("single", single)], args))
        a, s, spread = line["batch_ms"], line["single_ms"], line["single_ms_spread"]
        line["batch_ms_per_model"] = round(a / B, 5)
        line["single_over_batch"] = round(s / a, 2)
        line["batch_faster"] = bool(a < s - spread)
        emit(line, args)
        filled = graph = k = uplift = g = models = None
        silt.empty_cache()
    for H in [int(v) for v in (args.map or "").split(",") if v]:
        filled, graph, k, uplift, g = (model_view(t, 0) for t in planes(1, H))
        h = filled.view_torch()
        span = float(h.max() - h.min())
        for times in (1.0, 100.0):
            kk = silt.tensor.from_torch((k.view_torch() * times).contiguous())
            for e in (1.5, 2.0, 3.0):
                for G in (0.5, 1.0, 2.0):
                    gg = silt.tensor.from_torch((g.view_torch() * G).contiguous())      # (the bench plane is G = 1)
                    res = []
                    for steps in range(1, args.steps + 1):
                        r = soil.stream_power_deposit_n(filled, graph, kk, gg, edge, SCALE, DT, e, uplift, steps, False,
                                                        residual=True)[1]
                        res.append(float(r.view_torch()[0]))
                    first, word = classify(res, span)
                    emit({"H": H, "what": "map", "K_dt_times": times, "exponent": e, "G": G, "height_range": round(span, 3),
                          "first_below_1e-9_of_range": first, "verdict": word, "least": float("%.3g" % min(res)),
                          "least_at": res.index(min(res)) + 1, "settled_at": settled_at(res), "residual_after": [float("%.3g" % v) for v in res]}, args)
        filled = graph = k = uplift = g = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
