#!/usr/bin/env python
"""Per-cell order statistics and exceedance maps across the B models of a batch (include/soil_hip.h:
soil_erode_batch_quantiles, soil_erode_batch_exceedance, one launch each; DESIGN.md 3.5 "Order statistics") against
what a user had before them, all timed in one process:

  torch_quantiles   torch.sort over the model axis of view_torch() of the planes (the six channels stacked, height
                    added in fp32), then per position the gather of the two order statistics and the fp64 lerp;
  torch_exceedance  (x > t).sum(0) / B over the same stack.

(torch.quantile refuses inputs of this size.)  Both use nothing newer than view_torch, so this file also runs on a
build without the two entry points (--baseline-only).

One JSON line per H:B (square grids): ms per call of each route (device events around each call, the median over
--rounds x --iters calls after --warmup, the routes alternated round by round, and the least and greatest median of
a round as the spread), the ratios, the path that served the quantiles, and the algorithmic bytes (20 per cell and
model read, 24 per cell and position written) with bytes/s and the share of 8 TB/s.  --paths also times every path
SOIL_QUANTILE_PATH can force at that B (reg to 64, lds to 256, bisect any): where each B should go.  The kernels
alone are in a kernel trace (--no-baseline under rocprofv3 --kernel-trace --stats)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, silt, soil  # noqa: E402
from soillib_amd.erosion import ErosionBatch  # noqa: E402

DEFAULT = "256:1,256:8,256:64,256:256,512:1,512:8,512:32,1024:8,256:300"
PEAK = 8.0e12   # bytes/s of HBM
READ = ("layers", "waterHeight", "mass", "debris")
PATH_MAX = (("reg", 64), ("lds", 256), ("bisect", None))


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


def auto_path(B):
    """What the entry takes unforced (csrc/erosion_quantiles.hip)."""
    return "reg" if B <= 16 else "lds" if B <= 256 else "bisect"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT, help="H:B,... (default: %s)" % DEFAULT)
    ap.add_argument("--q", default="0.1,0.5,0.9", help="the quantiles of a call")
    ap.add_argument("--iters", type=int, default=5, help="timed calls per round")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the routes")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--paths", action="store_true", help="also every path that can be forced at this B")
    ap.add_argument("--no-baseline", action="store_true", help="the two device calls alone")
    ap.add_argument("--baseline-only", action="store_true", help="the torch routes alone")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    lib = _abi.lib()
    param = soil.param_t()
    q = [float(v) for v in args.q.split(",")]
    for cfg in args.configs.split(","):
        H, B = (int(v) for v in cfg.split(":"))
        n = H * H
        batch = ErosionBatch(B, H, H, (20.0 / H, 20.0 / H, 4.0), param, 16, list(range(B)))
        gen = torch.Generator(device="cuda")
        gen.manual_seed(H + B)
        views = {name: getattr(batch, name).view_torch() for name in READ}
        for view in views.values():   # heavy-tailed, every model its own values
            view.copy_(torch.randn(view.shape, generator=gen, device=view.device).exp_())
        torch.cuda.synchronize()
        pos = [v * (B - 1) for v in q]
        thresholds = [1.0, 1.0, 2.0, 1.0, 1.0, 1.0]
        t_dev = torch.tensor(thresholds, device=views["mass"].device)

        def stacked():
            l = views["layers"]
            return torch.stack([l[..., 0], l[..., 1], l[..., 0] + l[..., 1], views["waterHeight"], views["mass"],
                                views["debris"]], dim=-1)

        def torch_quantiles():
            s = torch.sort(stacked(), dim=0).values
            out = []
            for p in pos:
                lo = int(p)
                frac = p - lo
                a, b = s[lo], s[min(lo + 1, B - 1)]
                out.append(a if frac == 0 else torch.where(a == b, a, (a.double() + frac * (b.double() - a.double())).float()))
            return torch.stack(out)

        def torch_exceedance():
            return ((stacked() > t_dev).sum(0).double() / B).float()

        def forced(path):
            def call():
                os.environ["SOIL_QUANTILE_PATH"] = path   # read at every call
                try:
                    return batch.quantiles(q)
                finally:
                    os.environ.pop("SOIL_QUANTILE_PATH", None)
            return call

        routes = []   # (key, call)
        if not args.baseline_only:
            routes.append(("quantiles", lambda: batch.quantiles(q)))
            routes.append(("exceedance", lambda: batch.exceedance(thresholds)))
            if args.paths:
                routes += [("quantiles_" + name, forced(name)) for name, top in PATH_MAX if top is None or B <= top]
        if not args.no_baseline:
            routes.append(("torch_quantiles", torch_quantiles))
            routes.append(("torch_exceedance", torch_exceedance))
        for _, call in routes:
            for _ in range(args.warmup):
                call()
        times = {key: [] for key, _ in routes}
        for _ in range(args.rounds):
            for key, call in routes:
                times[key].append(timed(lib, call, args.iters))
        nbytes = {"quantiles": B * n * 20 + n * 24 * len(q), "exceedance": B * n * 20 + n * 24}
        line = {"H": H, "B": B, "q": q, "path": auto_path(B), "iters": args.iters, "rounds": args.rounds,
                "warmup": args.warmup, "bytes": nbytes}
        for key, rounds in times.items():
            meds = [statistics.median(v) for v in rounds]
            line[key + "_ms"] = round(statistics.median([v for rnd in rounds for v in rnd]), 4)
            line[key + "_ms_rounds_min_max"] = [round(min(meds), 4), round(max(meds), 4)]
        for key in ("quantiles", "exceedance"):
            if key + "_ms" in line:
                rate = nbytes[key] / (line[key + "_ms"] * 1e-3)
                line[key + "_bytes_per_s"] = round(rate, 0)
                line[key + "_share_of_8TBps"] = round(rate / PEAK, 4)
                if "torch_%s_ms" % key in line:
                    line["torch_over_" + key] = round(line["torch_%s_ms" % key] / line[key + "_ms"], 2)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        batch = views = None
        silt.empty_cache()


if __name__ == "__main__":
    main()
