#!/usr/bin/env python
"""Stream order (include/soil_hip.h: soil_stream_order and its _batch form; DESIGN.md 3.5 "Stream order and channel
segments"), timed in one process against the closure work it contains at most, on the conditioned D8 graph of the bench
terrain (noise x 100, soil.condition) at H x H with its drainage area (soil.accumulate of ones):

  --single H,...
      few              soil.stream_order(graph, area=area, threshold=T)   the channels at T cells of drainage
      all              soil.stream_order(graph)                           every cell a channel cell
      few_wide / all_wide   the same under SOIL_STREAM_ORDER_NARROW=0: every channel cell in every closure's work set
      up_few / up_all  `levels` calls of soil.upstream_max(graph, area) — soil_upstream_extreme, op 1 —, levels that of
                       the call beside it: one full closure per level, which is the most the call can contain
  --batch H:B,...  soil.stream_order_batch on B models (area, threshold T) against soil.stream_order model by model

One JSON line per size.  A figure is the median of --repeats medians, each over --iters calls (device events around
every call) after --warmup calls, the routes alternated repeat by repeat; the spread beside it is the greatest minus
the least of those medians.  `few_over_up`, `all_over_up`: the call over the `levels` closures; `holds_*`: the call is
no slower than them by more than the two spreads together.  `narrow_gain_*`: wide over narrow.

--count N, for a kernel trace: N calls of the thresholded route (with --batch: of stream_order_batch), untimed; the
set-up's kernels (noise, the conditioning, the accumulation) are in the trace once.
    rocprofv3 --kernel-trace --stats -- python tools/bench_stream_order.py --single 1024 --count 6"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402
from tools.bench_flow_batch import model_view  # noqa: E402
from tools.bench_flow_paths import emit, figures  # noqa: E402
from tools.bench_upstream import terrains  # noqa: E402

SINGLE = "256,1024,4096,8192"
BATCH = "256:8,256:64,256:256"
THRESHOLD = 100.0


def areas(graph, B, H):
    ones = silt.tensor(silt.float32, silt.shape(B, H, H), silt.gpu)
    silt.set(ones, 1.0)
    return soil.accumulate_batch(graph, ones, soil.d8)


def wide(call):
    def run():
        os.environ["SOIL_STREAM_ORDER_NARROW"] = "0"              # (read per call)
        try:
            return call()
        finally:
            del os.environ["SOIL_STREAM_ORDER_NARROW"]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default=None, help="H,... (default with neither option: %s)" % SINGLE)
    ap.add_argument("--batch", default=None, help="H:B,... (default with neither option: %s)" % BATCH)
    ap.add_argument("--iters", type=int, default=20, help="timed calls per median")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=THRESHOLD, help="cells of drainage that make a channel")
    ap.add_argument("--count", type=int, default=0, help="the new route alone, this many calls, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.single is None and args.batch is None:
        args.single, args.batch = SINGLE, BATCH
    lib = _abi.lib()
    edge, T = soil.d8, args.threshold
    for H in [int(v) for v in (args.single or "").split(",") if v]:
        import torch
        _, graph3 = terrains(1, H)
        area = model_view(areas(graph3, 1, H), 0)
        graph = model_view(graph3, 0)
        few = lambda: soil.stream_order(graph, edge, area=area, threshold=T)   # noqa: E731
        every = lambda: soil.stream_order(graph, edge)                         # noqa: E731
        if args.count:
            for _ in range(args.count):
                few()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "count": args.count, "route": "stream_order", "info": soil.stream_order_info()}, args)
            continue
        order = few().view_torch()
        levels_few = soil.stream_order_info()["levels"]
        share = float((order > 0).float().mean())
        assert bool((order == wide(few)().view_torch()).all()), "the narrowed closures change the result"
        top = every().view_torch()
        levels_all = soil.stream_order_info()["levels"]
        assert int(top.max()) == levels_all and int(order.max()) == levels_few
        assert bool((top == wide(every)().view_torch()).all()), "the narrowed closures change the result"

        def closures(n):
            def run():
                out = None
                for _ in range(n):
                    out = soil.upstream_max(graph, area, edge)
                return out
            return run

        line = {"H": H, "what": "single", "threshold": T, "channel_share": round(share, 4), "levels_few": levels_few,
                "levels_all": levels_all, "rounds": soil.stream_order_info()["rounds"]}
        line.update(figures(lib, [("few", few), ("all", every), ("few_wide", wide(few)), ("all_wide", wide(every)),
                                  ("up_few", closures(levels_few)), ("up_all", closures(levels_all))], args))
        for k in ("few", "all"):
            a, u = line[k + "_ms"], line["up_" + k + "_ms"]
            line[k + "_over_up"] = round(a / u, 3)
            line["holds_" + k] = bool(a <= u + line[k + "_ms_spread"] + line["up_" + k + "_ms_spread"])
            line["narrow_gain_" + k] = round(line[k + "_wide_ms"] / a, 3)
        emit(line, args)
        graph3 = graph = area = order = top = None
        torch.cuda.empty_cache()
        silt.empty_cache()
    for cfg in [v for v in (args.batch or "").split(",") if v]:
        H, B = (int(v) for v in cfg.split(":"))
        _, graph = terrains(B, H)
        area = areas(graph, B, H)
        batch = lambda: soil.stream_order_batch(graph, edge, area=area, threshold=T)   # noqa: E731
        if args.count:
            for _ in range(args.count):
                batch()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            emit({"H": H, "B": B, "count": args.count, "route": "stream_order_batch", "info": soil.stream_order_info()}, args)
            continue
        models = [[model_view(t, b) for t in (graph, area)] for b in range(B)]

        def single():
            out = None
            for g, a in models:
                out = soil.stream_order(g, edge, area=a, threshold=T)
            return out

        batch()
        line = {"H": H, "B": B, "what": "batch", "threshold": T, "levels": soil.stream_order_info()["levels"]}
        line.update(figures(lib, [("batch", batch), ("single", single)], args))
        a, s, spread = line["batch_ms"], line["single_ms"], line["single_ms_spread"]
        line["batch_ms_per_model"] = round(a / B, 5)
        line["single_over_batch"] = round(s / a, 2)
        line["holds"] = bool(a < s - spread)
        emit(line, args)
        graph = area = models = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
