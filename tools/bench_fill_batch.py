#!/usr/bin/env python
"""The fill of a batch (include/soil_hip.h: soil_fill_depressions_batch; DESIGN.md 3.5 "Filling a batch"), timed in
one process.  The models are the bench.py --config c3 DEM (noise x 100) with another seed each, D8.

  --batch H:B,...   soil.fill_depressions_batch on B models of H x H against the route there was before it: a loop of
                    soil.fill_depressions over the same models (the single-grid kernel and its schedule are what they
                    were), with the launches and looks of both from soil.fill_info
  --one H,...       B = 1 through the batch entry against the single call on the same model (the batch's overhead)
  --chain H:B,...   ErosionBatch.conditioned() + drainage(graph=g) against the one-at-a-time route
                    fill_depressions -> resolve_flats -> accumulate over the same models

One JSON line per point.  A figure is the median of --repeats medians, each over --iters calls (device events around
every call) after --warmup calls, the routes alternated repeat by repeat; the spread beside it is the greatest minus
the least of those medians.

--count N: the batch call alone, N calls per point and nothing else timed, for a kernel trace:
    rocprofv3 --kernel-trace --stats -- python tools/bench_fill_batch.py --batch 256:1,256:8,256:64 --count 10"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402
from tools.bench_flats import dem  # noqa: E402
from tools.bench_flow_batch import model_view  # noqa: E402
from tools.bench_flow_paths import emit, figures  # noqa: E402

BATCH = "256:8,256:64,256:256,512:8,512:64,1024:8"
ONE = "1024,4096"
CHAIN = "256:8,256:64"


def models_of(lib, H, B):
    hb = silt.tensor(silt.float32, silt.shape(B, H, H), silt.gpu)
    per = hb.nbytes() // B
    for b in range(B):
        one = dem(H, 5 + b, 100.0)
        _abi.check(lib.soil_memcpy_d2d(C.c_void_p(hb.ptr + b * per), one.c_ptr, per, _abi.stream()))
    _abi.check(lib.soil_stream_synchronize(_abi.stream()))
    return hb


def pairs(text):
    return [tuple(int(v) for v in cfg.split(":")) for cfg in (text or "").split(",") if cfg]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default=None, help="H:B,... (default with no option: %s)" % BATCH)
    ap.add_argument("--one", default=None, help="H,... (default with no option: %s)" % ONE)
    ap.add_argument("--chain", default=None, help="H:B,... (default with no option: %s)" % CHAIN)
    ap.add_argument("--iters", type=int, default=10, help="timed calls per median")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--count", type=int, default=0, help="the batch call alone, this many per point, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.batch is None and args.one is None and args.chain is None:
        args.batch, args.one, args.chain = BATCH, ONE, CHAIN
    lib = _abi.lib()
    edge = soil.d8
    points = [("batch", H, B) for H, B in pairs(args.batch)] + [("one", int(v), 1) for v in (args.one or "").split(",") if v]
    for what, H, B in points:
        hb = models_of(lib, H, B)
        models = [model_view(hb, b) for b in range(B)]

        def batch():
            return soil.fill_depressions_batch(hb, edge)

        def loop():
            out = None
            for h in models:
                out = soil.fill_depressions(h, edge)
            return out

        line = {"H": H, "B": B, "what": what}
        launches = looks = 0
        per_level = None
        for h in models:
            soil.fill_depressions(h, edge)
            info = soil.fill_info()
            launches, looks = launches + info["launches"], looks + info["looks"]
            per_level = info["per_level"] if per_level is None else [max(a, b) for a, b in zip(per_level, info["per_level"])]
        line.update(loop_launches=launches, loop_looks=looks, loop_per_level_max=per_level)
        batch()
        info = soil.fill_info()
        line.update(batch_launches=info["launches"], batch_looks=info["looks"], batch_per_level=info["per_level"],
                    levels=info["levels"])
        if args.count:
            for _ in range(args.count):
                batch()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            line["count"] = args.count
            emit(line, args)
        else:
            line.update(figures(lib, [("batch", batch), ("loop", loop)], args))
            line["loop_over_batch"] = round(line["loop_ms"] / line["batch_ms"], 2)
            emit(line, args)
        hb = models = None
        silt.empty_cache()
    if args.count:
        return
    for H, B in pairs(args.chain):
        from soillib_amd.erosion import ErosionBatch
        hb = models_of(lib, H, B)
        bt = ErosionBatch(B, H, H, (20.0 / H, 20.0 / H, 4.0), soil.param_t(), 64, list(range(B)))
        silt.set(bt.height, hb)
        models = [model_view(hb, b) for b in range(B)]
        ones = silt.tensor(silt.float32, silt.shape(H, H), silt.gpu)
        silt.set(ones, 1.0)

        def chain_batch():
            _, g = bt.conditioned()
            return bt.drainage(graph=g)

        def chain_loop():
            out = None
            for h in models:
                filled = soil.fill_depressions(h, edge)
                out = soil.accumulate(soil.resolve_flats(filled, edge), ones, edge)
            return out

        line = {"H": H, "B": B, "what": "chain"}
        line.update(figures(lib, [("batch", chain_batch), ("loop", chain_loop)], args))
        line["loop_over_batch"] = round(line["loop_ms"] / line["batch_ms"], 2)
        emit(line, args)
        hb = bt = models = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
