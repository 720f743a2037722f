#!/usr/bin/env python
"""Exact multiple-flow accumulation (include/soil_hip.h: soil_mfd_weights, soil_mfd_accumulate and their _batch forms;
DESIGN.md 3.5 "Exact multiple-flow accumulation") against one realisation of soil_multiflow, the Monte-Carlo loop it is
the limit of.  JSON lines, one per figure group; --out appends them to a file (profiles/mfd/bench.jsonl).

  --single H,...   the config-C3 terrain (bench_configs.py: noise seed 3 x 100), D8, unit source, T = 10, twice: raw, and
                   filled with the flat distance as `dist`.  Routes, alternated:
      mfd          soil.mfd_accumulate
      weights      soil.mfd_weights alone
      multiflow    soil.multiflow with --realisations graphs; the line holds the time of ONE of them
                   `break_even_K` = mfd_ms / multiflow_one_ms: the realisations mfd_accumulate costs.  `holds`: it lies
                   below 512, the K of example/dem_multiflow.py.  launches / tiles / looks: soil.mfd_info.
  --batch H:B,...  soil.mfd_accumulate_batch on B terrains (seeds 5 ..) against soil.mfd_accumulate on the same models
                   one at a time; `holds`: the batch lies below the loop by more than both spreads.

Every figure is the median of --repeats medians of --iters calls, from one primed state; `_spread` is max - min of those
medians.  --count N, for a kernel trace: N calls of mfd_accumulate (or of the batch route) and nothing else timed:
    rocprofv3 --kernel-trace --stats -- python tools/bench_mfd.py --single 4096 --count 10"""
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
BATCH = "256:8,256:64,256:256"
T = 10.0


def c3_terrain(H):
    p = soil.noise_t()
    p.seed = 3.0
    p.ext = [H, H]
    h = soil.noise(silt.shape(H, H), p, host=silt.gpu)
    silt.multiply(h, 100.0)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default=None, help="H,... (default with neither option: %s)" % SINGLE)
    ap.add_argument("--batch", default=None, help="H:B,... (default with neither option: %s)" % BATCH)
    ap.add_argument("--realisations", type=int, default=16, help="graphs of a timed soil.multiflow call")
    ap.add_argument("--iters", type=int, default=10, help="timed calls per median")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--count", type=int, default=0, help="the new route alone, this many calls, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.single is None and args.batch is None:
        args.single, args.batch = SINGLE, BATCH
    lib = _abi.lib()
    e = soil.d8
    for H in [int(v) for v in (args.single or "").split(",") if v]:
        raw = c3_terrain(H)
        filled = soil.fill_depressions(raw, e)
        dist = soil.flat_distance(filled, e)
        rain = silt.tensor(silt.float32, silt.shape(H, H), silt.gpu)
        silt.set(rain, 1.0)
        for name, h, d in (("raw", raw, None), ("filled", filled, dist)):
            mfd = lambda: soil.mfd_accumulate(h, None, e, T=T, dist=d)
            if args.count:
                for _ in range(args.count):
                    mfd()
                emit({"H": H, "terrain": name, "count": args.count, "route": "mfd_accumulate", **soil.mfd_info()}, args)
                continue
            out = mfd()
            line = {"H": H, "what": "single", "terrain": name, "T": T, **soil.mfd_info()}
            w = soil.mfd_weights(h, e, T=T, dist=d).view_torch()
            line["terminals"] = int((w.sum(0) == 0).sum())
            line["sum_at_terminals_over_cells"] = float(out.view_torch().double()[w.sum(0) == 0].sum() / (H * H))
            del w
            K = args.realisations
            routes = [("mfd", mfd), ("weights", lambda: soil.mfd_weights(h, e, T=T, dist=d)),
                      ("multiflow", lambda: soil.multiflow(h, rain, K, T, e))]
            line.update(figures(lib, routes, args))
            line["realisations"] = K
            line["multiflow_one_ms"] = round(line["multiflow_ms"] / K, 4)
            line["break_even_K"] = round(line["mfd_ms"] / line["multiflow_one_ms"], 1)
            line["holds"] = bool(line["break_even_K"] < 512)
            emit(line, args)
    for H, B in [tuple(int(x) for x in v.split(":")) for v in (args.batch or "").split(",") if v]:
        hs = heights(B, H)
        models = [model_view(hs, b) for b in range(B)]
        batch = lambda: soil.mfd_accumulate_batch(hs, None, e, T=T)

        def loop():
            for m in models:
                soil.mfd_accumulate(m, None, e, T=T)
        if args.count:
            for _ in range(args.count):
                batch()
            emit({"H": H, "B": B, "count": args.count, "route": "mfd_accumulate_batch", **soil.mfd_info()}, args)
            continue
        batch()
        line = {"H": H, "B": B, "what": "batch", "T": T, **soil.mfd_info()}
        line.update(figures(lib, [("batch", batch), ("loop", loop)], args))
        line["loop_over_batch"] = round(line["loop_ms"] / line["batch_ms"], 2)
        line["holds"] = bool(line["batch_ms"] + line["batch_ms_spread"] < line["loop_ms"] - line["loop_ms_spread"])
        emit(line, args)


if __name__ == "__main__":
    main()
