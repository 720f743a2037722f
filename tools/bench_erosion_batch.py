#!/usr/bin/env python
"""A batch of B independent erosion models stepped together (include/soil_hip.h: soil_erode_step_batch,
ErosionBatch) against the same B models stepped one after the other through
ErosionModel.step() on the same stream, both timed in one process.  N = cells / 8 (8192 at 256^2), maxage 256
and the script's parameters (example/erosion_gpu.py), every model its own noise terrain and seed.

One JSON line per (size, B): ms per batch step and per model-step (median over --steps device-event-timed
steps after --warmup), the sequential loop's ms per model-step, and seq / batch.  --no-seq leaves the loop
out (the profiling run: rocprofv3 --kernel-trace --stats).  --colour times the coloured batch
(ErosionBatch(colour=True), soil_erode_step_batch_colour) against ErosionModel(colour=True).step(), bedrock and
surface colours set on every model.  --sweep times a parameter sweep (ErosionBatch with a sequence of B param_t,
soil_erode_step_batch_params; with --colour the coloured one) against the uniform batch at the same shapes: B
separate param_t of equal values, so that both walk the same walks and only the sweep's mechanism differs, the
two alternated --rounds times in blocks of --steps steps, medians of each.  No sequential loop then.
--models times a batch of different models (soil_erode_step_batch_models) in one of two modes: (a) equal
records, the uniform batch, the sweep of B equal param_t and a batch of B equal records (scale, N and param per
model), alternated as --sweep alternates two (with --colour the coloured ones); (b) with --mixed, models that
differ: N_b = cells / 8, 16, 32, 64 and z-scale 2, 4, 8 in turn, against the same models stepped one at a time
through ErosionModel.step() on the same stream, the two alternated --rounds times."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from soillib_amd import _abi, silt, soil  # noqa: E402
from soillib_amd.erosion import ErosionBatch, ErosionModel  # noqa: E402
from util import script_param  # noqa: E402

DEFAULT = "256:1,256:8,256:64,256:256,512:1,512:8,512:32,1024:1,1024:8,1024:32"
COLOUR_DEFAULT = "256:1,256:8,256:64,256:256,512:1,512:8,512:32,1024:1,1024:8"
SWEEP_DEFAULT = "256:1,256:8,256:64,256:256,512:8,512:32"
MIXED_DEFAULT = "256:8,256:64,512:8,512:32"

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default=None, help="size:B,size:B,... (default: %s; with --colour %s)" % (
    DEFAULT, COLOUR_DEFAULT))
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-seq", action="store_true")
ap.add_argument("--out", default=None, help="also append the lines to this file")
ap.add_argument("--colour", action="store_true", help="the coloured batch against coloured single models")
ap.add_argument("--sweep", action="store_true", help="a parameter sweep against the uniform batch (default configs: %s)"
                % SWEEP_DEFAULT)
ap.add_argument("--models", action="store_true", help="a batch of different models: (a) equal records against the "
                "uniform batch and the sweep (default configs: %s)" % SWEEP_DEFAULT)
ap.add_argument("--mixed", action="store_true", help="--models: (b) models of different N and z-scale against "
                "the one-at-a-time loop (default configs: %s)" % MIXED_DEFAULT)
ap.add_argument("--rounds", type=int, default=5, help="--sweep, --models: alternations")
args = ap.parse_args()
if args.configs is None:
    args.configs = (MIXED_DEFAULT if args.models and args.mixed else SWEEP_DEFAULT if args.sweep or args.models
                    else COLOUR_DEFAULT if args.colour else DEFAULT)
lib = _abi.lib()
param = script_param(soil.param_t())
param.maxage = 256


class Events:
    def __init__(self):
        self.ev = []

    def record(self):
        e = C.c_void_p()
        _abi.check(lib.soil_event_create(C.byref(e)))
        _abi.check(lib.soil_event_record(e, _abi.stream()))
        self.ev.append(e)

    def intervals(self):
        _abi.check(lib.soil_stream_synchronize(_abi.stream()))
        out = []
        for a, b in zip(self.ev[:-1], self.ev[1:]):
            ms = C.c_float()
            _abi.check(lib.soil_event_elapsed_ms(a, b, C.byref(ms)))
            out.append(ms.value)
        for e in self.ev:
            lib.soil_event_destroy(e)
        return out


def terrain_into(layers_ptr, S, b):
    """layers[..., 0] = noise of seed 3 + b, layers[..., 1] = 0 (on the device)."""
    p = soil.noise_t()
    p.seed = 3.0 + b
    p.ext = [S, S]
    bed = soil.noise(silt.shape(S, S), p, host=silt.gpu)
    _abi.check(lib.soil_layers_from_planes(C.c_void_p(layers_ptr), bed.c_ptr, None, S * S, _abi.stream()))


def colours_into(m):
    """Bedrock and surface colours of a coloured batch or model (the transport colours are the step's own)."""
    if args.colour:
        silt.set(m.albedoBedrock, 0.6)
        silt.set(m.albedoSurface, 0.3)


def timed(step, n):
    ev = Events()
    ev.record()
    for _ in range(n):
        step()
        ev.record()
    return statistics.median(ev.intervals())


def run(S, B):
    N = S * S // 8
    scale = (20.0 / S, 20.0 / S, 4.0)
    seeds = [1000 + b for b in range(B)]
    batch = ErosionBatch(B, S, S, scale, param, N, seeds, colour=args.colour)
    for b in range(B):
        terrain_into(batch.layers.ptr + b * S * S * 8, S, b)
    silt.set(batch.rainfall, 1.0)
    colours_into(batch)
    for _ in range(args.warmup):
        batch.step()
    ms_batch = timed(batch.step, args.steps)
    line = {"size": S, "B": B, "N": N, "colour": args.colour, "maxage": param.maxage, "steps": args.steps, "warmup": args.warmup,
            "batch_ms_per_step": round(ms_batch, 4), "batch_ms_per_model_step": round(ms_batch / B, 5)}
    del batch
    if not args.no_seq:
        models = []
        for b in range(B):
            m = ErosionModel(S, S, scale, param, N, seed=seeds[b], colour=args.colour)
            terrain_into(m.layers.ptr, S, b)
            silt.set(m.rainfall, 1.0)
            colours_into(m)
            models.append(m)

        def one_round():
            for m in models:
                m.step()
        for _ in range(args.warmup):
            one_round()
        ms_seq = timed(one_round, args.steps)
        line.update({"seq_ms_per_round": round(ms_seq, 4), "seq_ms_per_model_step": round(ms_seq / B, 5),
                     "seq_over_batch": round(ms_seq / ms_batch, 3)})
        del models
    silt.empty_cache()
    _abi.check(lib.soil_workspace_release())
    return line


def run_sweep(S, B):
    """The uniform batch and a sweep of B equal params, alternated in blocks of args.steps steps."""
    N = S * S // 8
    scale = (20.0 / S, 20.0 / S, 4.0)
    seeds = [1000 + b for b in range(B)]
    params = []
    for _ in range(B):
        p = soil.param_t()
        for name in soil.param_t._FIELDS + ("force",):
            setattr(p, name, getattr(param, name))
        params.append(p)
    batches = {}
    for kind, prm in (("uniform", param), ("sweep", params)):
        bt = ErosionBatch(B, S, S, scale, prm, N, seeds, colour=args.colour)
        for b in range(B):
            terrain_into(bt.layers.ptr + b * S * S * 8, S, b)
        silt.set(bt.rainfall, 1.0)
        colours_into(bt)
        for _ in range(args.warmup):
            bt.step()
        batches[kind] = bt
    ms = {"uniform": [], "sweep": []}
    for _ in range(args.rounds):
        for kind in ("uniform", "sweep"):
            ms[kind].append(timed(batches[kind].step, args.steps))
    u, w = statistics.median(ms["uniform"]), statistics.median(ms["sweep"])
    line = {"size": S, "B": B, "N": N, "colour": args.colour, "sweep": True, "maxage": param.maxage,
            "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
            "uniform_ms_per_step": round(u, 4), "sweep_ms_per_step": round(w, 4),
            "uniform_rounds_ms": [round(v, 4) for v in ms["uniform"]],
            "sweep_rounds_ms": [round(v, 4) for v in ms["sweep"]],
            "sweep_over_uniform": round(w / u, 4)}
    del batches
    silt.empty_cache()
    _abi.check(lib.soil_workspace_release())
    return line


def equal_params(B):
    """B separate param_t of the script's values."""
    out = []
    for _ in range(B):
        p = soil.param_t()
        for name in soil.param_t._FIELDS + ("force",):
            setattr(p, name, getattr(param, name))
        out.append(p)
    return out


def alternated(steppers):
    """{kind: step function}, each timed in blocks of args.steps steps, the kinds alternated args.rounds times."""
    ms = {kind: [] for kind in steppers}
    for _ in range(args.rounds):
        for kind, step in steppers.items():
            ms[kind].append(timed(step, args.steps))
    return ms


def run_models(S, B):
    """(a) The uniform batch, a sweep of B equal params and a batch of B equal records, alternated."""
    N = S * S // 8
    scale = (20.0 / S, 20.0 / S, 4.0)
    seeds = [1000 + b for b in range(B)]
    batches = {}
    for kind, sc, prm, n in (("uniform", scale, param, N), ("sweep", scale, equal_params(B), N),
                             ("models", [list(scale)] * B, equal_params(B), [N] * B)):
        bt = ErosionBatch(B, S, S, sc, prm, n, seeds, colour=args.colour)
        assert bt._per_model() == (kind == "models")
        for b in range(B):
            terrain_into(bt.layers.ptr + b * S * S * 8, S, b)
        silt.set(bt.rainfall, 1.0)
        colours_into(bt)
        for _ in range(args.warmup):
            bt.step()
        batches[kind] = bt
    ms = alternated({kind: bt.step for kind, bt in batches.items()})
    med = {kind: statistics.median(v) for kind, v in ms.items()}
    line = {"size": S, "B": B, "N": N, "colour": args.colour, "models": "equal", "maxage": param.maxage,
            "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
    for kind in ms:
        line[kind + "_ms_per_step"] = round(med[kind], 4)
    for kind in ms:
        line[kind + "_rounds_ms"] = [round(v, 4) for v in ms[kind]]
    line["models_over_sweep"] = round(med["models"] / med["sweep"], 4)
    line["models_over_uniform"] = round(med["models"] / med["uniform"], 4)
    del batches
    silt.empty_cache()
    _abi.check(lib.soil_workspace_release())
    return line


def run_mixed(S, B):
    """(b) Model b with N_b = cells / (8, 16, 32, 64)[b % 4] and z-scale (2, 4, 8)[b % 3]: the batch of different
    models against the same models stepped one at a time, alternated."""
    Ns = [S * S // (8, 16, 32, 64)[b % 4] for b in range(B)]
    scales = [[20.0 / S, 20.0 / S, (2.0, 4.0, 8.0)[b % 3]] for b in range(B)]
    seeds = [1000 + b for b in range(B)]
    bt = ErosionBatch(B, S, S, scales, param, Ns, seeds, colour=args.colour)
    for b in range(B):
        terrain_into(bt.layers.ptr + b * S * S * 8, S, b)
    silt.set(bt.rainfall, 1.0)
    colours_into(bt)
    models = []
    for b in range(B):
        m = ErosionModel(S, S, scales[b], param, Ns[b], seed=seeds[b], colour=args.colour)
        terrain_into(m.layers.ptr, S, b)
        silt.set(m.rainfall, 1.0)
        colours_into(m)
        models.append(m)

    def one_round():
        for m in models:
            m.step()
    for _ in range(args.warmup):
        bt.step()
        one_round()
    ms = alternated({"batch": bt.step, "seq": one_round})
    b_ms, s_ms = statistics.median(ms["batch"]), statistics.median(ms["seq"])
    line = {"size": S, "B": B, "Ns": sorted(set(Ns), reverse=True), "z_scales": [2.0, 4.0, 8.0],
            "colour": args.colour, "models": "mixed", "maxage": param.maxage, "steps": args.steps,
            "warmup": args.warmup, "rounds": args.rounds,
            "batch_ms_per_step": round(b_ms, 4), "seq_ms_per_round": round(s_ms, 4),
            "batch_rounds_ms": [round(v, 4) for v in ms["batch"]], "seq_rounds_ms": [round(v, 4) for v in ms["seq"]],
            "seq_over_batch": round(s_ms / b_ms, 3)}
    del bt, models
    silt.empty_cache()
    _abi.check(lib.soil_workspace_release())
    return line


name = C.create_string_buffer(256)
lib.soil_device_name(name, 256)
for cfg in args.configs.split(","):
    S, B = (int(v) for v in cfg.split(":"))
    if args.models:
        line = run_mixed(S, B) if args.mixed else run_models(S, B)
    else:
        line = run_sweep(S, B) if args.sweep else run(S, B)
    line["device"] = name.value.decode()
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(s + "\n")
