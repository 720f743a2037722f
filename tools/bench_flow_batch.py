#!/usr/bin/env python
"""The drainage of B models of one (H, W) in one call (include/soil_hip.h: soil_steepest_batch + soil_accumulate_batch;
DESIGN.md 3.5 "Flow routing over a batch") against the same B models through soil.steepest + soil.accumulate one at a
time, the only route before the batch entries, both timed in one process:

  batch    steepest_batch(height) then accumulate_batch(graph, source[, decay])                       one call
  single   for b in range(B): steepest(height[b]) then accumulate[_decay](graph, source[b][, decay[b]])   B calls

One JSON line per H:B (square grids) and per decay setting.  A figure is the median of --repeats medians, each over
--iters calls (device events around every call) after --warmup calls, the two routes alternated repeat by repeat; the
spread beside it is the greatest minus the least of those medians.  `holds`: for B >= 8 the batch's time per model lies
below the single route's by more than the single route's spread; for B = 1 it is not above it by more than that spread.

--count N: the batch route alone, N calls and nothing else on the device (inputs come from the host), for a kernel
trace:  rocprofv3 --kernel-trace --stats -- python tools/bench_flow_batch.py --configs 256:8 --count 10"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402

DEFAULT = "256:1,256:8,256:64,256:256,512:1,512:8,512:64,512:256,1024:1,1024:8,1024:64"


class Events:
    def __init__(self, lib):
        self.lib, self.ev = lib, []

    def record(self):
        e = C.c_void_p()
        _abi.check(self.lib.soil_event_create(C.byref(e)))
        _abi.check(self.lib.soil_event_record(e, _abi.stream()))
        self.ev.append(e)

    def intervals(self):
        _abi.check(self.lib.soil_stream_synchronize(_abi.stream()))
        out = []
        for a, b in zip(self.ev[:-1], self.ev[1:]):
            ms = C.c_float()
            _abi.check(self.lib.soil_event_elapsed_ms(a, b, C.byref(ms)))
            out.append(ms.value)
        for e in self.ev:
            self.lib.soil_event_destroy(e)
        return out


def timed(lib, call, n):
    ev = Events(lib)
    ev.record()
    for _ in range(n):
        call()
        ev.record()
    return ev.intervals()


def model_view(t, b):
    dims = tuple(t.shape)[1:]
    per = t.nbytes() // t.shape[0]
    return silt.tensor.from_device(t.ptr + b * per, t.type, silt.shape(*dims), keepalive=t)


def inputs(B, H, on_host):
    """Heights (noise x 100, another seed per model), sources in [0.5, 1.5) and decays in [0.8, 1).  `on_host`: the
    heights come from the host generator, so that no kernel but the timed ones runs (--count)."""
    p = soil.noise_t()
    p.ext = [H, H]
    height = silt.tensor(silt.float32, silt.shape(B, H, H), silt.gpu)
    per = height.nbytes() // B
    for b in range(B):
        p.seed = float(5 + b)
        if on_host:
            one = silt.tensor.from_numpy(soil.noise(silt.shape(H, H), p).numpy() * np.float32(100.0)).gpu()
        else:
            one = soil.noise(silt.shape(H, H), p, host=silt.gpu)
            silt.multiply(one, 100.0)
        _abi.check(_abi.lib().soil_memcpy_d2d(C.c_void_p(height.ptr + b * per), one.c_ptr, per, _abi.stream()))
    r = np.random.default_rng(H + B)
    up = lambda a: silt.tensor.from_numpy(a).gpu()
    return (height, up((0.5 + r.random((B, H, H), dtype=np.float32))), up((0.8 + 0.2 * r.random((B, H, H), dtype=np.float32))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT, help="H:B,... (default: %s)" % DEFAULT)
    ap.add_argument("--iters", type=int, default=20, help="timed calls per median")
    ap.add_argument("--repeats", type=int, default=5, help="medians per figure, the routes alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--edge", default="d8", choices=("d4", "d8"))
    ap.add_argument("--no-single", action="store_true", help="the batch route alone")
    ap.add_argument("--count", type=int, default=0, help="the batch route alone, this many calls, untimed (kernel traces)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    lib = _abi.lib()
    edge = soil.d8 if args.edge == "d8" else soil.d4
    for cfg in args.configs.split(","):
        H, B = (int(v) for v in cfg.split(":"))
        height, source, decay = inputs(B, H, on_host=bool(args.count))
        models = [(model_view(height, b), model_view(source, b), model_view(decay, b)) for b in range(B)]

        def batch(with_decay):
            return soil.accumulate_batch(soil.steepest_batch(height, edge), source, edge, decay if with_decay else None)

        def single(with_decay):
            out = None
            for h, s, d in models:
                g = soil.steepest(h, edge)
                out = soil.accumulate_decay(g, s, d, edge) if with_decay else soil.accumulate(g, s, edge)
            return out

        if args.count:
            for _ in range(args.count):
                batch(False)
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
            print(json.dumps({"H": H, "B": B, "count": args.count, "route": "batch, no decay"}), flush=True)
            continue
        for with_decay in (False, True):
            routes = [("batch", lambda: batch(with_decay))]
            if not args.no_single:
                routes.append(("single", lambda: single(with_decay)))
            for _, call in routes:
                for _ in range(args.warmup):
                    call()
            medians = {key: [] for key, _ in routes}
            for _ in range(args.repeats):
                for key, call in routes:
                    medians[key].append(statistics.median(timed(lib, call, args.iters)))
            line = {"H": H, "B": B, "edge": args.edge, "decay": with_decay, "iters": args.iters,
                    "repeats": args.repeats, "warmup": args.warmup}
            for key, meds in medians.items():
                line[key + "_ms"] = round(statistics.median(meds), 4)
                line[key + "_ms_spread"] = round(max(meds) - min(meds), 4)
                line[key + "_ms_per_model"] = round(statistics.median(meds) / B, 5)
            if "single_ms" in line:
                a, b, spread = line["batch_ms"], line["single_ms"], line["single_ms_spread"]
                line["single_over_batch"] = round(b / a, 2)
                line["holds"] = bool(a <= b + spread) if B == 1 else bool(a < b - spread)
            print(json.dumps(line), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
        height = source = decay = models = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
