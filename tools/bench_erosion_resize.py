#!/usr/bin/env python
"""A batch of B erosion models resampled to a new resolution by ErosionBatch.resized() (include/soil_hip.h:
soil_erode_resize_batch, one launch for every plane of every model) against the per-plane route a
user had before it, both timed in one process: a new ErosionBatch of the new size, then for every model and every
persistent plane a soil_memcpy_d2d out of the model-major tensor (B > 1 only), legacy.resize (soil_resize), a
copy back, then silt.set(..., 0) on the five flux planes and soil.layer_merge for `height`.  The per-plane route
uses nothing newer than soil_resize, so this file also runs on a build without soil_erode_resize_batch
(--baseline-only).

One JSON line per Ho:Hn:B (square grids Ho^2 -> Hn^2): ms per call of both (device events around each call, the
median over --rounds x --iters calls after --warmup, the two alternated round by round, and the least and
greatest median of a round as the spread), their ratio, and the algorithmic bytes (resize_bytes below) and
bytes/s of the fused call, allocation of the new batch and the zeroing of its layers_next included.  --colour:
coloured batches.  --no-baseline: the fused call alone (the profiling run: rocprofv3 --kernel-trace --stats).
--yardsticks: after each configuration one single-channel soil_resize and one fused cell phase at the new size,
--iters times each, for a kernel trace to hold the two kernels the resample's share of the roofline is compared
with."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soillib_amd import _abi, legacy, silt, soil  # noqa: E402
from soillib_amd.erosion import ErosionBatch  # noqa: E402

DEFAULT = "256:512:1,256:512:8,256:512:64,256:512:256,512:1024:1,512:1024:8,512:1024:32,4096:8192:1"
COLOUR_DEFAULT = "256:512:1,256:512:8,256:512:64,256:512:256,512:1024:1,512:1024:8,512:1024:32"
RESAMPLED = (("layers", 2), ("uplift", 1), ("rainfall", 1), ("waterHeight", 1), ("mass", 1), ("debris", 1),
             ("velocity", 2), ("debrisVelocity", 2))
COLOUR = tuple((name, 3) for name in ErosionBatch.PLANES_3)
FLUX = ("waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux")


def resize_bytes(B, Ho, Wo, Hn, Wn, colour=False):
    """Algorithmic bytes of one soil_erode_resize_batch: per new cell 48 of state (12 floats), 4 of height and 28
    of zeros (the five flux planes) written, with colour 48 more (four vec3 planes); per old cell 44 read (the
    state without height), with colour 48 more, every source cell counted once."""
    written = B * Hn * Wn * (80 + (48 if colour else 0))
    read = B * Ho * Wo * (44 + (48 if colour else 0))
    return {"written": written, "read": read, "total": written + read}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=None, help="Ho:Hn:B,... (default: %s; with --colour %s)" % (
        DEFAULT, COLOUR_DEFAULT))
    ap.add_argument("--iters", type=int, default=5, help="timed calls per round")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two routes")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--colour", action="store_true")
    ap.add_argument("--no-baseline", action="store_true", help="the fused call alone")
    ap.add_argument("--baseline-only", action="store_true", help="the per-plane route alone")
    ap.add_argument("--yardsticks", action="store_true", help="also run soil_resize (1 channel) and the cell phase")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    lib = _abi.lib()
    param = soil.param_t()
    for cfg in (args.configs or (COLOUR_DEFAULT if args.colour else DEFAULT)).split(","):
        Ho, Hn, B = (int(v) for v in cfg.split(":"))
        scale, N, seeds = (20.0 / Ho, 20.0 / Ho, 4.0), 16, list(range(B))
        batch = ErosionBatch(B, Ho, Ho, scale, param, N, seeds, colour=args.colour)
        for k, (name, _) in enumerate(RESAMPLED + (COLOUR if args.colour else ())):
            silt.set(getattr(batch, name), 0.25 + 0.125 * k)
        planes = RESAMPLED + (COLOUR if args.colour else ())
        # the per-plane route's staging: one source and one destination plane per channel count
        stage = {c: (silt.tensor(silt.float32, silt.shape(Ho, Ho, c), silt.gpu),
                     silt.tensor(silt.float32, silt.shape(Hn, Hn, c), silt.gpu))
                 for c in sorted({c for _, c in planes})} if B > 1 else {}

        def per_plane():
            new = ErosionBatch(B, Hn, Hn, (20.0 / Hn, 20.0 / Hn, 4.0), param, N, seeds, colour=args.colour)
            for name, c in planes:
                src, dst = getattr(batch, name), getattr(new, name)
                if B == 1:
                    legacy.resize(dst, src, (Hn, Hn), (Ho, Ho))
                    continue
                s, d = stage[c]
                for b in range(B):
                    _abi.check(lib.soil_memcpy_d2d(s.c_ptr, C.c_void_p(src.ptr + b * s.nbytes()), s.nbytes(),
                                                   _abi.stream()))
                    legacy.resize(d, s, (Hn, Hn), (Ho, Ho))
                    _abi.check(lib.soil_memcpy_d2d(C.c_void_p(dst.ptr + b * d.nbytes()), d.c_ptr, d.nbytes(),
                                                   _abi.stream()))
            for name in FLUX:
                silt.set(getattr(new, name), 0.0)
            soil.layer_merge(new.height, new.layers)
            return new

        fused = (lambda: batch.resized(Hn, Hn)) if not args.baseline_only else None
        base = per_plane if not args.no_baseline else None
        for call in (fused, base):
            for _ in range(args.warmup if call else 0):
                call()
        t_fused, t_base = [], []
        for _ in range(args.rounds):
            if fused:
                t_fused.append(timed(lib, fused, args.iters))
            if base:
                t_base.append(timed(lib, base, args.iters))
        nbytes = resize_bytes(B, Ho, Ho, Hn, Hn, args.colour)
        line = {"Ho": Ho, "Hn": Hn, "B": B, "colour": args.colour, "iters": args.iters, "rounds": args.rounds,
                "warmup": args.warmup, "bytes": nbytes}
        for key, rounds in (("fused", t_fused), ("per_plane", t_base)):
            if rounds:
                meds = [statistics.median(r) for r in rounds]
                line[key + "_ms"] = round(statistics.median([v for r in rounds for v in r]), 4)
                line[key + "_ms_rounds_min_max"] = [round(min(meds), 4), round(max(meds), 4)]
        if t_fused:
            line["fused_bytes_per_s"] = round(nbytes["total"] / (line["fused_ms"] * 1e-3), 0)
        if t_fused and t_base:
            line["per_plane_over_fused"] = round(line["per_plane_ms"] / line["fused_ms"], 3)
        if args.yardsticks:
            s = silt.tensor(silt.float32, silt.shape(Ho, Ho), silt.gpu)
            d = silt.tensor(silt.float32, silt.shape(Hn, Hn), silt.gpu)
            silt.set(s, 0.5)
            new = batch.resized(Hn, Hn) if fused else per_plane()
            for _ in range(args.iters):
                legacy.resize(d, s, (Hn, Hn), (Ho, Ho))
                new.cells_fused()
            _abi.check(lib.soil_stream_synchronize(_abi.stream()))
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
