"""Guard bands around every plane of the erosion entry points of include/soil_hip.h: the stand-alone cell and colour
ops, the fused cell phase, the particle launches, whole steps, batches of models, resampling and the summaries.  The
method, the four checks of a row and the shapes are those of tests/test_gpu_guard_bands.py, which also holds the
completeness test over both tables; the struct-taking entry points fill soil_erosion_planes / soil_colour_planes
from the arena by name.

What differs here:

  particle rows   the launch shape of the particle kernels does not follow from shape and alignment, so these rows run
                  under every mode of tests/test_gpu_parity.py's `particle_mode` at one of its SIZES, (37, 53) with
                  700 walkers.  The flux planes are sums of floating-point atomics: held to util.flux_close (and the
                  helpers built on it) in both runs, never compared between the fills.
  whole steps     soil_erode_step*, soil_erode and the batch steps are compositions of rows of this table (the
                  particle launches and the cell phase).  Their planes derive from atomic sums, so they are held to
                  the oracle's composition of the step with the tolerance tests/test_gpu_colour_step.py holds a step
                  to; soil_erode_step_ex runs with both flux flags, which leaves the flux planes behind: those are
                  held to util.flux_close and the cell phase, fed with them, to the oracle bit for bit.
  batch particle  B = 3 of (5, 7), (65, 67) and (33, 260), below and above the 1024 walkers at which a batch goes
  rows            from the direct to the staged shape.
  cell launch     the vector cell kernels pick their launch form by the number of work-groups: the cell rows also run
  forms           at (256, 256) and (252, 260), the shapes of tests/test_gpu_cells_hostile.py at which the XCD remap,
                  the 512- and 128-thread kernels and DIRECT are taken, soil_erode_cells_fused_ex there under
                  SOIL_CELLS_VARIANT 1 .. 6 (read on every call), and the batch rows at B = 2 of those shapes.

Out of scope, as there: include/soil_slab.h and the library's internal workspace (the particle streams of the batch
entries and of soil_erode live in it).
"""
import ctypes as C
import os

import numpy as np
import pytest

import guard_arena as ga
import util
from guard_arena import IN, INOUT, OUT, Case, P
from test_gpu_guard_bands import BATCH, F32, F64, GRID, I32, Row, case_list, dims, extras, fl, memo, ok, run_row, shape_args
from test_gpu_parity import particle_mode  # noqa: F401  (a fixture: every launch shape of the particle kernels)

ROWS = {}
PHYSICS = ("layers", "layers_next", "height", "uplift", "rainfall", "waterHeight", "waterFlux", "mass", "massFlux",
           "velocity", "velocityFlux", "debris", "debrisFlux", "debrisVelocity", "debrisVelocityFlux")
CH = dict(layers=2, layers_next=2, velocity=2, velocityFlux=2, debrisVelocity=2, debrisVelocityFlux=2,
          albedo_bedrock=3, albedo_surface=3, albedo_fluvial=3, albedo_debris=3)
FLUX = util.CELL_FLUX
CELL_OUT = util.CELL_OUT
COLOUR = dict(albedo_bedrock="albedoBedrock", albedo_surface="albedoSurface", albedo_fluvial="albedoFluvial",
              albedo_debris="albedoDebris")
PARTICLE_SIZE = (37, 53)            # of tests/test_gpu_parity.py's SIZES: ragged, W % 4 != 0
N_PARTICLES = 700
BATCH_PARTICLES = [(3, 5, 7, "N200"), (3, 5, 7, "N1100"), (3, 65, 67, "N200"), (3, 65, 67, "N1100"), (3, 33, 260, "N1100")]


def row(entry, cases, ref, composed=False, modes=False):
    def deco(build):
        assert entry not in ROWS, entry
        ROWS[entry] = r = Row(entry, list(cases), build, ref, composed=composed)
        r.modes = modes
        return build
    return deco


def tail(name):
    return (CH[name],) if name in CH else ()


def plane_shape(key, name):
    return shape_args(key) + tail(name)


def structs(p, colour, prefix=""):
    """soil_erosion_planes (and soil_colour_planes) filled from the arena by name; a plane the arena does not hold is NULL."""
    from soillib_amd import _abi
    pl = _abi.ErosionPlanes()
    for n in PHYSICS:
        setattr(pl, n, p(prefix + n))
    cp = None
    if colour:
        cp = _abi.ColourPlanes()
        for n in COLOUR:
            setattr(cp, n, p(prefix + n))
    return pl, cp


def lenient(p, names):
    """ptr(name) of the arena, None for a plane the case does not hold."""
    return lambda name: p(name) if name in names else None


def pparam(op):
    return util.product_param(op)


def scale_of(H, W):
    return (20.0 / H, 20.0 / W, 4.0)


def whole(H, W):
    from soillib_amd import _abi
    return _abi.Domain(H, W, 0, H, 0, H)


# ------------------------------------------------------------------ the stand-alone cell and colour ops

@memo
def cell_in(H, W, seed):
    from oracle import pyoracle
    return util.cell_inputs(pyoracle, H, W, seed)


@memo
def colour_in(H, W, seed):
    return util.colour_inputs(H, W, seed)


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


@row("soil_mass_transfer", GRID, "oracle.mass_transfer with the colour planes; delta and albedo_surface are in/out; waterHeight "
     "and momentumDebris are accepted and unread")
def _(key, oracle):
    H, W = key
    inp, col = cell_in(H, W, 1), colour_in(H, W, 2)
    r = np.random.default_rng(3)
    f1 = lambda s: (r.random((H, W)) * s).astype(F32)
    f2 = lambda s: (r.standard_normal((H, W, 2)) * s).astype(F32)
    m, v, d, wh, md = f1(0.5), f2(2.0), f1(0.2), f1(1.0), f2(1.0)
    delta = (r.standard_normal((H, W, 2)) * 0.01).astype(F32)
    op, sc = util.script_param(oracle.default_param()), scale_of(H, W)

    def want(lib, oracle):
        dd, surf = delta.copy(), col["albedoSurface"].copy()
        oracle.mass_transfer(dd, inp["layers"], inp["uplift"], m, v, d, col["albedoBedrock"], col["albedoFluvial"],
                             col["albedoDebris"], surf, sc, op)
        return dict(delta=(dd, "naneq"), albedo_surface=(surf, "naneq"))
    pp = pparam(op)
    return Case([P("delta", INOUT, delta), P("layers", IN, inp["layers"]), P("uplift", IN, inp["uplift"]), P("waterHeight", IN, wh),
                 P("mass", IN, m), P("velocityFluvial", IN, v), P("albedo_surface", INOUT, col["albedoSurface"]),
                 P("debris", IN, d), P("momentumDebris", IN, md), P("albedo_bedrock", IN, col["albedoBedrock"]),
                 P("albedoFluxFluvial", IN, col["albedoFluvial"]), P("albedoFluxDebris", IN, col["albedoDebris"])],
                lambda lib, p: ok(lib.soil_mass_transfer(
                    p("delta"), p("layers"), p("uplift"), p("waterHeight"), p("mass"), p("velocityFluvial"), p("debris"),
                    p("momentumDebris"), p("albedo_bedrock"), p("albedoFluxFluvial"), p("albedoFluxDebris"), p("albedo_surface"),
                    H, W, fl(*sc), pp._ref(), None)), want)


@row("soil_mass_creep", GRID, "oracle.mass_creep; delta is in/out")
def _(key, oracle):
    H, W = key
    layers = cell_in(H, W, 1)["layers"]
    delta = (np.random.default_rng(4).standard_normal((H, W, 2)) * 0.01).astype(F32)
    op, sc = util.script_param(oracle.default_param()), scale_of(H, W)

    def want(lib, oracle):
        dd = delta.copy()
        oracle.mass_creep(dd, layers, sc, op)
        return dict(delta=(dd, "naneq"))
    pp = pparam(op)
    return Case([P("layers", IN, layers), P("delta", INOUT, delta)],
                lambda lib, p: ok(lib.soil_mass_creep(p("delta"), p("layers"), H, W, fl(*sc), pp._ref(), None)), want)


@row("soil_layer_merge", GRID, "oracle.layer_merge")
def _(key, oracle):
    H, W = key
    layers = cell_in(H, W, 1)["layers"]
    return Case([P("height", OUT, key, F32), P("layers", IN, layers)],
                lambda lib, p: ok(lib.soil_layer_merge(p("height"), p("layers"), H * W, None)),
                lambda lib, oracle: dict(height=(oracle.layer_merge(layers), "naneq")))


@row("soil_layers_from_planes", GRID, "numpy: the two planes interleaved")
def _(key, oracle):
    H, W = key
    layers = cell_in(H, W, 1)["layers"]
    bed, sed = np.ascontiguousarray(layers[..., 0]), np.ascontiguousarray(layers[..., 1])
    return Case([P("bedrock", IN, bed), P("layers", OUT, key + (2,), F32), P("sediment", IN, sed)],
                lambda lib, p: ok(lib.soil_layers_from_planes(p("layers"), p("bedrock"), p("sediment"), H * W, None)),
                lambda lib, oracle: dict(layers=np.stack([bed, sed], axis=-1)))


@row("soil_layers_to_planes", GRID, "numpy: the layer plane split")
def _(key, oracle):
    H, W = key
    layers = cell_in(H, W, 1)["layers"]
    return Case([P("bedrock", OUT, key, F32), P("layers", IN, layers), P("sediment", OUT, key, F32)],
                lambda lib, p: ok(lib.soil_layers_to_planes(p("bedrock"), p("sediment"), p("layers"), H * W, None)),
                lambda lib, oracle: dict(bedrock=np.ascontiguousarray(layers[..., 0]), sediment=np.ascontiguousarray(layers[..., 1])))


@row("soil_albedo_stratum", GRID, "oracle.albedo_stratum")
def _(key, oracle):
    H, W = key
    inp = cell_in(H, W, 1)
    op, sc = oracle.default_param(), (1.0, 1.0, 80.0)
    a, b = (0.9, 0.5, 0.1), (0.2, 0.3, 0.4)

    def want(lib, oracle):
        out = np.zeros((H, W, 3), F32)
        oracle.albedo_stratum(out, inp["uplift"], inp["layers"], sc, op, a, b, 5e4, 2.5)
        return dict(albedoBedrock=(out, "naneq"))
    pp = pparam(op)
    return Case([P("uplift", IN, inp["uplift"]), P("albedoBedrock", OUT, key + (3,), F32), P("layers", IN, inp["layers"])],
                lambda lib, p: ok(lib.soil_albedo_stratum(p("albedoBedrock"), p("uplift"), p("layers"), H * W, fl(*sc), pp._ref(),
                                                          fl(*a), fl(*b), 5e4, 2.5, None)), want)


@row("soil_albedo_layer", GRID, "oracle.albedo_layer")
def _(key, oracle):
    H, W = key
    layers, col = cell_in(H, W, 1)["layers"], colour_in(H, W, 2)
    bed, sed = col["albedoBedrock"], col["albedoSurface"]

    def want(lib, oracle):
        out = np.zeros((H, W, 3), F32)
        oracle.albedo_layer(out, bed, sed, layers, 12.0, (0.1, 0.2, 0.3))
        return dict(albedo=(out, "naneq"))
    return Case([P("albedoBedrock", IN, bed), P("albedo", OUT, key + (3,), F32), P("albedoSediment", IN, sed), P("layers", IN, layers)],
                lambda lib, p: ok(lib.soil_albedo_layer(p("albedo"), p("albedoBedrock"), p("albedoSediment"), p("layers"), H * W, 12.0,
                                                        fl(0.1, 0.2, 0.3), None)), want)


@row("soil_albedo_discharge", GRID, "oracle.albedo_discharge; albedo is in/out")
def _(key, oracle):
    H, W = key
    alb = colour_in(H, W, 2)["albedoSurface"]
    dis = (np.random.default_rng(5).standard_normal((H, W)) * 40).astype(F32)

    def want(lib, oracle):
        out = alb.copy()
        oracle.albedo_discharge(out, dis, (0.1, 0.3, 0.8), 0.05, 0.7)
        return dict(albedo=(out, "naneq"))
    return Case([P("albedo", INOUT, alb), P("discharge", IN, dis)],
                lambda lib, p: ok(lib.soil_albedo_discharge(p("albedo"), p("discharge"), H * W, fl(0.1, 0.3, 0.8), 0.05, 0.7, None)),
                want)


@row("soil_ghost_extent", GRID, "tests/parallel_worker.py: OracleOps.ghost_extent; depth is in/out (accumulated with max)")
def _(key, oracle):
    H, W = key
    r0 = H // 3
    r1 = max(r0 + 1, 2 * H // 3)
    plane = np.zeros((H, W), F32)
    r = np.random.default_rng(6)
    for x in range(H):
        if (x < r0 or x >= r1) and r.random() < 0.5 and min(abs(x - r0), abs(x - r1)) < H // 4 + 1:
            plane[x, r.integers(W)] = 1.0 if x % 2 else -2.5

    def want(lib, oracle):
        import parallel_worker
        depth = [0, 0]
        parallel_worker.OracleOps().ghost_extent(plane.ctypes.data, H, W, r0, r1, depth)
        return dict(depth=np.array(depth, I32))
    return Case([P("plane", IN, plane), P("depth", INOUT, np.zeros(2, I32), fills=(0, 1))],
                lambda lib, p: ok(lib.soil_ghost_extent(p("depth"), p("plane"), H, W, r0, r1, None)), want)


# ------------------------------------------------------------------ the fused cell phase, single models and batches

def cell_sets(oracle, key, form):
    """(op, scale) of every model: one set for all, or a set per model for the sweep and the batch of models."""
    B, H, W = dims(key)
    sets = {n: (op, sc) for n, op, sc in util.cell_param_sets(oracle, H, W)}
    names = ("script", "random0", "random1") if form in ("params", "models") else ("script",) * 3
    out = [sets[n] for n in names[:B or 1]]
    if form == "params":
        out = [(op, sets["script"][1]) for op, _ in out]            # a sweep shares its scale
    return out


def cell_case(entry, key, oracle, colour, form=None):
    from soillib_amd import _abi
    B, H, W = dims(key)
    keep = "keep" in extras(key)
    variant = [e[1:] for e in extras(key) if e.startswith("v")]
    nb = B or 1
    sets = cell_sets(oracle, key, form)
    inps = [cell_in(H, W, H * W + b) for b in range(nb)]
    cols = [colour_in(H, W, 7 + b) for b in range(nb)]
    stack = lambda arrays: arrays[0] if B is None else np.stack(arrays)
    planes = []
    for n in PHYSICS:
        if n in util.CELL_IN:
            role = IN if (n not in FLUX or keep) else INOUT
            planes.append(P(n, role, stack([i[n] for i in inps])))
        else:
            planes.append(P(n, OUT, plane_shape(key, n), F32))
    if colour:
        for n, k in COLOUR.items():
            planes.append(P(n, IN if n == "albedo_bedrock" else INOUT, stack([c[k] for c in cols])))

    def want(lib, oracle):
        outs = [util.oracle_colour_cells(oracle, inps[b], cols[b], sets[b][1], sets[b][0]) for b in range(nb)]
        w = {n: (stack([o[n] for o in outs]), "naneq") for n in CELL_OUT}
        if colour:
            w.update({n: (stack([o[k] for o in outs]), "naneq") for n, k in COLOUR.items() if n != "albedo_bedrock"})
        if not keep:
            w.update({n: np.zeros(plane_shape(key, n), F32) for n in FLUX})
        return w

    flags = _abi.SOIL_CELLS_KEEP_FLUX if keep else 0
    pps = [pparam(op) for op, _ in sets]

    def call(lib, p):
        pl, cp = structs(p, colour)
        cref = C.byref(cp) if colour else None
        sc = fl(*sets[0][1])
        dom = whole(H, W)
        if form == "params":
            params = (_abi.Param * nb)()
            for b in range(nb):
                util.copy_param(sets[b][0], params[b])
        if form == "models":
            recs = (_abi.BatchModel * nb)()
            for b in range(nb):
                util.copy_param(sets[b][0], recs[b].param)
                for i in range(3):
                    recs[b].scale[i] = sets[b][1][i]
        before = os.environ.get("SOIL_CELLS_VARIANT")
        if variant:
            os.environ["SOIL_CELLS_VARIANT"] = variant[0]
        try:
            if entry == "soil_erode_cells_fused":
                rc = lib.soil_erode_cells_fused(C.byref(pl), C.byref(dom), sc, pps[0]._ref(), None)
            elif entry == "soil_erode_cells_fused_ex":
                rc = lib.soil_erode_cells_fused_ex(C.byref(pl), C.byref(dom), sc, pps[0]._ref(), flags, None)
            elif entry == "soil_erode_cells_fused_colour":
                rc = lib.soil_erode_cells_fused_colour(C.byref(pl), cref, C.byref(dom), sc, pps[0]._ref(), flags, None)
            elif entry == "soil_erode_cells_fused_batch":
                rc = lib.soil_erode_cells_fused_batch(C.byref(pl), B, H, W, sc, pps[0]._ref(), flags, None)
            elif entry == "soil_erode_cells_fused_batch_colour":
                rc = lib.soil_erode_cells_fused_batch_colour(C.byref(pl), cref, B, H, W, sc, pps[0]._ref(), flags, None)
            elif entry == "soil_erode_cells_fused_batch_params":
                rc = lib.soil_erode_cells_fused_batch_params(C.byref(pl), cref, B, H, W, sc, params, flags, None)
            else:
                rc = lib.soil_erode_cells_fused_batch_models(C.byref(pl), cref, B, H, W, recs, flags, None)
            ok(rc)
        finally:
            if variant:
                if before is None:
                    del os.environ["SOIL_CELLS_VARIANT"]
                else:
                    os.environ["SOIL_CELLS_VARIANT"] = before
    return Case(planes, call, want)


KEEP = lambda shapes: [s + ("keep",) for s in shapes]                                        # noqa: E731
# The launch form of the vector cell kernels follows from the number of four-cell groups, not from the shape's edges
# (csrc/erosion_cells.hip: erode_cells_fused, cells_batch): the XCD remap needs at least 64 work-groups and a multiple
# of 8, SOIL_CELLS_VARIANT 1 / 3 a group count that 512 / 128 divides.  So the shapes are those of
# tests/test_gpu_cells_hostile.py::test_every_launch_variant_is_the_same_function: at (256, 256) variant 1 is the
# 512-thread kernel, 3 the 128-thread one, 4 DIRECT, 2 the kernel without the remap, 5 the split (84-byte kernel and
# zeroing pass), 6 names none (the one re-zeroing kernel under remap), 0 the default (the split under remap); at
# (252, 260) — 16380 groups in 64 work-groups, the remap with idle lanes — 1 and 3 fall through to the 256-thread
# kernels.  With `keep` every variant is the 84-byte kernel.  Aligned placements only take these forms; off4 takes the
# scalar kernel at the same sizes.  The arenas of these cases are 16.5 MB (26 MB with colour).
REMAP = [(256, 256), (252, 260)]
VARIANTS = [s + ("v%d" % v,) for s in REMAP for v in range(1, 7)] + [s + ("v%d" % v, "keep") for s in REMAP for v in (1, 5)]
# ... and a batch whose models are that large: the remap instantiations of cells_batch (B = 2: 33 MB, 52 MB with colour)
REMAP_BATCH = [(2, 256, 256), (2, 252, 260)]
_REF_CELLS = "util.oracle_colour_cells (the oracle's cell phase), the re-zeroed flux planes all +0; with `keep` the flux planes are inputs"
_REF_REMAP = "; 256x256 and 252x260: the work-group counts at which the XCD remap and the variants' kernels are taken"

row("soil_erode_cells_fused", GRID + REMAP, _REF_CELLS + _REF_REMAP)(
    lambda key, oracle: cell_case("soil_erode_cells_fused", key, oracle, False))
row("soil_erode_cells_fused_ex", GRID + KEEP(GRID) + REMAP + KEEP(REMAP) + VARIANTS,
    _REF_CELLS + _REF_REMAP + "; v1 .. v6: SOIL_CELLS_VARIANT there")(
    lambda key, oracle: cell_case("soil_erode_cells_fused_ex", key, oracle, False))
row("soil_erode_cells_fused_colour", GRID + KEEP(GRID) + REMAP + KEEP(REMAP), _REF_CELLS + _REF_REMAP)(
    lambda key, oracle: cell_case("soil_erode_cells_fused_colour", key, oracle, True))
row("soil_erode_cells_fused_batch", BATCH + KEEP(BATCH[:1] + BATCH[-1:]) + REMAP_BATCH + KEEP(REMAP_BATCH), _REF_CELLS + _REF_REMAP)(
    lambda key, oracle: cell_case("soil_erode_cells_fused_batch", key, oracle, False))
row("soil_erode_cells_fused_batch_colour", BATCH + KEEP(BATCH[:1] + BATCH[-1:]) + REMAP_BATCH + KEEP(REMAP_BATCH[1:]),
    _REF_CELLS + _REF_REMAP)(lambda key, oracle: cell_case("soil_erode_cells_fused_batch_colour", key, oracle, True))
row("soil_erode_cells_fused_batch_params", BATCH + KEEP(BATCH[:1] + BATCH[-1:]) + REMAP_BATCH[1:],
    _REF_CELLS + _REF_REMAP + "; a param per model, with colour")(
    lambda key, oracle: cell_case("soil_erode_cells_fused_batch_params", key, oracle, True, "params"))
row("soil_erode_cells_fused_batch_models", BATCH + KEEP(BATCH[:1] + BATCH[-1:]) + REMAP_BATCH + KEEP(REMAP_BATCH[:1]),
    _REF_CELLS + _REF_REMAP + "; a param and a scale per model, no colour")(
    lambda key, oracle: cell_case("soil_erode_cells_fused_batch_models", key, oracle, False, "models"))


# ------------------------------------------------------------------ resampling and the summaries of a batch

STATE = ("layers", "uplift", "rainfall", "waterHeight", "mass", "debris", "velocity", "debrisVelocity")


@memo
def read_planes(B, H, W, seed):
    import test_gpu_erosion_stats as stats
    return _frozen(stats._random_read_planes(B, H, W, seed))


@row("soil_erode_resize_batch", BATCH, "oracle.resize of every plane of every model, from ((H + 1) / 2, W + 3); height the fp32 sum "
     "of the resampled layers; the flux planes +0; dst.layers_next is not touched: an input here")
def _(key, oracle):
    B, H, W = key
    Ho, Wo = (H + 1) // 2, W + 3
    r = np.random.default_rng([8, H, W])
    src = {n: r.standard_normal((B, Ho, Wo) + tail(n)).astype(F32) for n in STATE + tuple(COLOUR)}
    untouched = r.standard_normal((B, H, W, 2)).astype(F32)
    planes = []
    for n in STATE + tuple(COLOUR):
        planes += [P("src." + n, IN, src[n]), P("dst." + n, OUT, (B, H, W) + tail(n), F32)]
    planes += [P("dst.height", OUT, (B, H, W), F32), P("dst.layers_next", IN, untouched)]
    planes += [P("dst." + n, OUT, (B, H, W) + tail(n), F32) for n in FLUX]
    names = {p[0] for p in planes}

    def want(lib, oracle):
        w = {}
        for n in STATE + tuple(COLOUR):
            w["dst." + n] = (np.stack([oracle.resize(src[n][b], (H, W)) for b in range(B)]), "naneq")
        lay = w["dst.layers"][0]
        w["dst.height"] = (lay[..., 0] + lay[..., 1], "naneq")
        w.update({"dst." + n: np.zeros((B, H, W) + tail(n), F32) for n in FLUX})
        return w

    def call(lib, p):
        q = lenient(p, names)
        dpl, dcp = structs(q, True, "dst.")
        spl, scp = structs(q, True, "src.")
        ok(lib.soil_erode_resize_batch(C.byref(dpl), C.byref(spl), C.byref(dcp), C.byref(scp), B, H, W, Ho, Wo, None))
    return Case(planes, call, want)


def _summary_planes(key, names):
    B, H, W = key
    host = read_planes(B, H, W, H + 3 * W + B)
    return host, [P(n, IN, host[n]) for n in names]


@row("soil_erode_batch_stats", BATCH, "tests/test_gpu_erosion_stats.py: _check_model on every record; the records under the two "
     "fills byte for byte")
def _(key, oracle):
    import test_gpu_erosion_stats as stats
    from soillib_amd.erosion import STATS_DTYPE
    B, H, W = key
    host, planes = _summary_planes(key, stats.READ)
    names = set(stats.READ)

    def judge(got, exp, what):
        rec = np.ascontiguousarray(got).view(STATS_DTYPE).reshape(B, 10)
        for b in range(B):
            stats._check_model(rec[b], host, b, what + ": ")
    judge.deterministic = True
    return Case(planes[:3] + [P("out", OUT, (B, 40), F64)] + planes[3:],
                lambda lib, p: ok(lib.soil_erode_batch_stats(C.byref(structs(lenient(p, names), False)[0]), B, H, W, p("out"), None)),
                lambda lib, oracle: dict(out=(None, judge)))


@row("soil_erode_batch_ensemble", BATCH, "tests/test_gpu_erosion_stats.py: _ensemble_expected, mean and var")
def _(key, oracle):
    import test_gpu_erosion_stats as stats
    B, H, W = key
    host, planes = _summary_planes(key, stats.ENSEMBLE_READ)
    names = set(stats.ENSEMBLE_READ)

    def want(lib, oracle):
        mean, var = stats._ensemble_expected(host, B)
        return dict(mean=(mean, "naneq"), var=(var, "naneq"))
    return Case([P("mean", OUT, (H, W, 6), F32)] + planes + [P("var", OUT, (H, W, 6), F32)],
                lambda lib, p: ok(lib.soil_erode_batch_ensemble(C.byref(structs(lenient(p, names), False)[0]), B, H, W, p("mean"),
                                                                p("var"), None)), want)


@row("soil_erode_batch_quantiles", BATCH, "tests/test_gpu_erosion_quantiles.py: _expected with _assert_bits, four positions")
def _(key, oracle):
    import test_gpu_erosion_quantiles as quant
    import test_gpu_erosion_stats as stats
    B, H, W = key
    host, planes = _summary_planes(key, stats.ENSEMBLE_READ)
    names = set(stats.ENSEMBLE_READ)
    pos = [0.0, (B - 1) / 2.0, float(B - 1), 0.5]

    def want(lib, oracle):
        bits, generated = quant._expected(quant._channels(host), pos)
        judge = lambda got, exp, what: quant._assert_bits(got, exp[0], exp[1], what)          # noqa: E731
        judge.deterministic = True
        return dict(out=((bits, generated), judge))
    return Case(planes[:2] + [P("out", OUT, (len(pos), H, W, 6), F32)] + planes[2:],
                lambda lib, p: ok(lib.soil_erode_batch_quantiles(C.byref(structs(lenient(p, names), False)[0]), B, H, W,
                                                                 (C.c_double * len(pos))(*pos), len(pos), p("out"), None)), want)


@row("soil_erode_batch_exceedance", BATCH, "tests/test_gpu_erosion_quantiles.py: _exceedance_expected")
def _(key, oracle):
    import test_gpu_erosion_quantiles as quant
    import test_gpu_erosion_stats as stats
    B, H, W = key
    host, planes = _summary_planes(key, stats.ENSEMBLE_READ)
    names = set(stats.ENSEMBLE_READ)
    t = [0.0, -0.5, 1.0, 0.25, -1.0, 2.0]
    return Case(planes + [P("out", OUT, (H, W, 6), F32)],
                lambda lib, p: ok(lib.soil_erode_batch_exceedance(C.byref(structs(lenient(p, names), False)[0]), B, H, W, fl(*t),
                                                                  p("out"), None)),
                lambda lib, oracle: dict(out=quant._exceedance_expected(quant._channels(host), t)))


# ------------------------------------------------------------------ the particle launches and whole steps of one model

def particle_op(oracle, maxage=64):
    op = util.script_param(oracle.default_param())
    op.maxage = maxage
    op.critSlopeBedrock = 0.05          # landslides on the synthetic terrain (tests/test_gpu_parity.py)
    op.yieldStress = 0.001
    return op


_STATES = {}


def particle_state(oracle, H, W, b=0):
    """One model's state for a particle launch: the draws of tests/test_gpu_parity.py's transport tests."""
    k = (H, W, b)
    if k not in _STATES:
        r = np.random.default_rng(21 + b)
        c3 = lambda: r.random((H, W, 3)).astype(F32)                                           # noqa: E731
        st = dict(layers=util.terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.01, rng_seed=b),
                  rainfall=(0.5 + r.random((H, W))).astype(F32), uplift=(0.5 * r.random((H, W))).astype(F32),
                  waterHeight=(r.random((H, W)) * 0.1).astype(F32), velocity=(r.standard_normal((H, W, 2)) * 2).astype(F32),
                  debrisVelocity=(r.standard_normal((H, W, 2)) * 0.5).astype(F32), albedoSurface=c3(), albedoBedrock=c3(),
                  stale3=c3(), stale2=r.standard_normal((H, W, 2)).astype(F32), stale1=r.random((H, W)).astype(F32))
        _STATES[k] = _frozen(st)
    return _STATES[k]


def stale(st, name):
    """Numbers a plane holds before a call that must not read them."""
    return st["stale3"] if name in CH and CH[name] == 3 else st["stale2"] if name in CH else st["stale1"]


def rng_at(oracle, N, seed, offset):
    return oracle.rng_seed(N, seed, offset).astype(ga.RNG)


SEED, STEP = 5, 2


def oracle_pair(oracle, st, N, seed, offset, sc, op, colour):
    from test_gpu_erosion_batch_oracle import _oracle_particles
    return _oracle_particles(oracle, st, N, seed, offset, sc, op, colour)[0]


def flux_judges(want_flux):
    return {n: (a, lambda got, exp, what: util.flux_close(got, exp, what)) for n, a in want_flux.items()}


@row("soil_transport_fluvial", [PARTICLE_SIZE], "oracle.transport_fluvial with util.assert_fluvial_close; the rng states word for word; "
     "waterHeight, velocity, the flux planes and rng are in/out", modes=True)
def _(key, oracle):
    H, W = key
    N, st, op, sc = N_PARTICLES, particle_state(oracle, H, W), particle_op(oracle, 128), scale_of(H, W)
    z = lambda *c: np.zeros((H, W) + c, F32)                                                   # noqa: E731
    names = dict(wh="waterHeight", wf="waterFlux", m="mass", mf="massFlux", v="velocity", vf="velocityFlux", af="albedoFlux")

    def want(lib, oracle):
        o = dict(wh=st["waterHeight"].copy(), wf=z(), m=z(), mf=z(), v=st["velocity"].copy(), vf=z(2), af=z(3))
        rng = oracle.rng_seed(N, SEED, 100)
        oracle.transport_fluvial(st["layers"], st["rainfall"], o["wh"], o["wf"], o["m"], o["mf"], o["v"], o["vf"], o["af"],
                                 st["albedoSurface"], rng, sc, op)
        judge = lambda got, exp, what: util.assert_fluvial_close({k: got[n] for k, n in names.items()}, exp)   # noqa: E731
        return {"*": (o, judge), "rng": rng.astype(ga.RNG)}
    pp = pparam(op)
    return Case([P("layers", IN, st["layers"]), P("waterHeight", INOUT, st["waterHeight"]), P("rainfall", IN, st["rainfall"]),
                 P("waterFlux", INOUT, z()), P("mass", OUT, key, F32), P("massFlux", INOUT, z()), P("velocity", INOUT, st["velocity"]),
                 P("velocityFlux", INOUT, z(2)), P("albedoSource", IN, st["albedoSurface"]), P("albedoFlux", INOUT, z(3)),
                 P("rng", INOUT, rng_at(oracle, N, SEED, 100))],
                lambda lib, p: ok(lib.soil_transport_fluvial(
                    p("layers"), p("rainfall"), p("waterHeight"), p("waterFlux"), p("mass"), p("massFlux"), p("velocity"),
                    p("velocityFlux"), None, p("albedoFlux"), p("albedoSource"), p("rng"), N, H, W, fl(*sc), pp._ref(), None)), want)


@row("soil_transport_debris", [PARTICLE_SIZE], "oracle.transport_debris with util.assert_debris_close; the rng states word for word; "
     "velocity, the flux planes and rng are in/out", modes=True)
def _(key, oracle):
    H, W = key
    N, st, op, sc = N_PARTICLES, particle_state(oracle, H, W), particle_op(oracle, 128), scale_of(H, W)
    z = lambda *c: np.zeros((H, W) + c, F32)                                                   # noqa: E731
    names = dict(v="velocity", vf="velocityFlux", m="mass", mf="massFlux", af="albedoFlux")

    def want(lib, oracle):
        o = dict(v=st["debrisVelocity"].copy(), vf=z(2), m=z(), mf=z(), af=z(3))
        rng = oracle.rng_seed(N, SEED + 1, 0)
        oracle.transport_debris(st["layers"], o["v"], o["vf"], o["m"], o["mf"], o["af"], st["albedoSurface"], rng, sc, op)
        judge = lambda got, exp, what: util.assert_debris_close({k: got[n] for k, n in names.items()}, exp)    # noqa: E731
        return {"*": (o, judge), "rng": rng.astype(ga.RNG)}
    pp = pparam(op)
    return Case([P("velocity", INOUT, st["debrisVelocity"]), P("layers", IN, st["layers"]), P("velocityFlux", INOUT, z(2)),
                 P("mass", OUT, key, F32), P("albedoSource", IN, st["albedoSurface"]), P("massFlux", INOUT, z()),
                 P("albedoFlux", INOUT, z(3)), P("rng", INOUT, rng_at(oracle, N, SEED + 1, 0))],
                lambda lib, p: ok(lib.soil_transport_debris(
                    p("layers"), p("velocity"), p("velocityFlux"), p("mass"), p("massFlux"), None, p("albedoFlux"), p("albedoSource"),
                    p("rng"), N, H, W, fl(*sc), pp._ref(), None)), want)


@row("soil_particles_fluvial_slab", [PARTICLE_SIZE], "oracle.particles_fluvial with util.flux_close, the colour flux too; rng word for "
     "word; remote0 stays +0 on a whole grid; the flux planes, rng and remote0 are in/out", modes=True)
def _(key, oracle):
    H, W = key
    N, st, op, sc = N_PARTICLES, particle_state(oracle, H, W), particle_op(oracle), scale_of(H, W)
    z = lambda *c: np.zeros((H, W) + c, F32)                                                   # noqa: E731

    def want(lib, oracle):
        o = dict(waterFlux=z(), massFlux=z(), velocityFlux=z(2), albedoFlux=z(3))
        rng = oracle.rng_seed(N, SEED, 100)
        oracle.particles_fluvial(o["waterFlux"], o["massFlux"], o["velocityFlux"], o["albedoFlux"], rng, st["layers"], st["rainfall"],
                                 st["waterHeight"], st["velocity"], st["albedoSurface"], sc, op)
        return dict(flux_judges(o), rng=rng.astype(ga.RNG), remote0=np.zeros(8, F32))
    pp = pparam(op)
    dom = whole(H, W)
    return Case([P("waterFlux", INOUT, z()), P("layers", IN, st["layers"]), P("massFlux", INOUT, z()), P("rainfall", IN, st["rainfall"]),
                 P("velocityFlux", INOUT, z(2)), P("waterHeight", IN, st["waterHeight"]), P("albedoFlux", INOUT, z(3)),
                 P("velocity", IN, st["velocity"]), P("remote0", INOUT, np.zeros(8, F32)), P("albedoSource", IN, st["albedoSurface"]),
                 P("rng", INOUT, rng_at(oracle, N, SEED, 100))],
                lambda lib, p: ok(lib.soil_particles_fluvial_slab(
                    p("waterFlux"), p("massFlux"), p("velocityFlux"), p("albedoFlux"), p("rng"), N, p("layers"), p("rainfall"),
                    p("waterHeight"), p("velocity"), p("albedoSource"), p("remote0"), C.byref(dom), fl(*sc), pp._ref(), None)), want)


@row("soil_particles_debris_slab", [PARTICLE_SIZE], "oracle.particles_debris with util.flux_close, the colour flux too; rng word for "
     "word; remote0 stays +0; the flux planes, rng and remote0 are in/out", modes=True)
def _(key, oracle):
    H, W = key
    N, st, op, sc = N_PARTICLES, particle_state(oracle, H, W), particle_op(oracle), scale_of(H, W)
    z = lambda *c: np.zeros((H, W) + c, F32)                                                   # noqa: E731

    def want(lib, oracle):
        o = dict(massFlux=z(), velocityFlux=z(2), albedoFlux=z(3))
        rng = oracle.rng_seed(N, SEED + 1, 0)
        oracle.particles_debris(o["massFlux"], o["velocityFlux"], o["albedoFlux"], rng, st["layers"], st["debrisVelocity"],
                                st["albedoSurface"], sc, op)
        return dict(flux_judges(o), rng=rng.astype(ga.RNG), remote0=np.zeros(8, F32))
    pp = pparam(op)
    dom = whole(H, W)
    return Case([P("layers", IN, st["layers"]), P("massFlux", INOUT, z()), P("velocity", IN, st["debrisVelocity"]),
                 P("velocityFlux", INOUT, z(2)), P("remote0", INOUT, np.zeros(8, F32)), P("albedoFlux", INOUT, z(3)),
                 P("albedoSource", IN, st["albedoSurface"]), P("rng", INOUT, rng_at(oracle, N, SEED + 1, 0))],
                lambda lib, p: ok(lib.soil_particles_debris_slab(
                    p("massFlux"), p("velocityFlux"), p("albedoFlux"), p("rng"), N, p("layers"), p("velocity"), p("albedoSource"),
                    p("remote0"), C.byref(dom), fl(*sc), pp._ref(), None)), want)


def model_planes(key, sts, roles, colour, colour_roles=None):
    """The planes of soil_erosion_planes (and soil_colour_planes) for the states `sts` (one per model): `roles` maps a
    physics plane to (role, "state" | "zero" | "stale" | None for an output)."""
    B = dims(key)[0]
    _, H, W = dims(key)
    stack = lambda arrays: arrays[0] if B is None else np.stack(arrays)                        # noqa: E731
    planes = []
    for n in PHYSICS:
        role, what = roles[n]
        if what is None:
            planes.append(P(n, role, plane_shape(key, n), F32))
        elif what == "state":
            planes.append(P(n, role, stack([st[n] for st in sts])))
        elif what == "zero":
            planes.append(P(n, role, np.zeros(plane_shape(key, n), F32)))
        else:
            planes.append(P(n, role, stack([stale(st, n) for st in sts])))
    if colour:
        for n, k in COLOUR.items():
            role, what = colour_roles[n]
            planes.append(P(n, role, stack([st[k] if what == "state" else stale(st, n) for st in sts])))
    return planes


# what a particle launch does with the planes of soil_erosion_planes: the state is read, the flux planes are added to,
# the cell phase's other outputs are not touched (so they are inputs here, and must come back bit for bit)
PARTICLE_ROLES = dict(layers=(IN, "state"), layers_next=(IN, "stale"), height=(IN, "stale"), uplift=(IN, "state"),
                      rainfall=(IN, "state"), waterHeight=(IN, "state"), mass=(IN, "stale"), velocity=(IN, "state"),
                      debris=(IN, "stale"), debrisVelocity=(IN, "state"))
PARTICLE_COLOUR = dict(albedo_bedrock=(IN, "state"), albedo_surface=(IN, "state"), albedo_fluvial=(INOUT, "stale"),
                       albedo_debris=(INOUT, "stale"))
# ... and a whole step: the state planes are read by the launches and written by the cell phase
STEP_ROLES = dict(layers=(IN, "state"), layers_next=(OUT, None), height=(OUT, None), uplift=(IN, "state"), rainfall=(IN, "state"),
                  waterHeight=(INOUT, "state"), mass=(OUT, None), velocity=(INOUT, "state"), debris=(OUT, None),
                  debrisVelocity=(INOUT, "state"))
STEP_COLOUR = dict(albedo_bedrock=(IN, "state"), albedo_surface=(INOUT, "state"), albedo_fluvial=(INOUT, "stale"),
                   albedo_debris=(INOUT, "stale"))


def with_flux(roles, what):
    return dict(roles, **{n: (INOUT, what) for n in FLUX})


def pair_case(entry, key, oracle, colour, overwrite):
    from soillib_amd import _abi
    H, W = key
    N, st, op, sc = N_PARTICLES, particle_state(oracle, H, W), particle_op(oracle), scale_of(H, W)
    offset = STEP * N
    slab = entry.endswith("_slab") or entry.endswith("_slab_ex")
    planes = model_planes(key, [st], with_flux(PARTICLE_ROLES, "stale" if overwrite else "zero"), colour, PARTICLE_COLOUR)
    planes += [P("rng_fluvial", INOUT, rng_at(oracle, N, SEED, offset)), P("rng_debris", INOUT, rng_at(oracle, N, SEED, offset + 2))]
    if slab:
        planes.insert(3, P("remote0", INOUT, np.zeros(16 if colour else 8, F32)))

    def want(lib, oracle):
        o = oracle_pair(oracle, st, N, SEED, offset, sc, op, colour)
        w = flux_judges({n: o[n] for n in FLUX})
        if colour:
            w.update(flux_judges({"albedo_fluvial": o["albedoFluvial"], "albedo_debris": o["albedoDebris"]}))
        w.update(rng_fluvial=rng_at(oracle, N, SEED, offset + 2), rng_debris=rng_at(oracle, N, SEED, offset + 4))
        if slab:
            w["remote0"] = np.zeros(16 if colour else 8, F32)
        return w
    pp = pparam(op)
    flags = _abi.SOIL_FLUX_OVERWRITE if overwrite else 0

    def call(lib, p):
        pl, cp = structs(p, colour)
        dom = whole(H, W)
        tail_args = (C.byref(dom), fl(*sc), pp._ref())
        if entry == "soil_particles_pair_slab":
            rc = lib.soil_particles_pair_slab(C.byref(pl), p("rng_fluvial"), p("rng_debris"), N, p("remote0"), *tail_args, None)
        elif entry == "soil_particles_pair_slab_ex":
            rc = lib.soil_particles_pair_slab_ex(C.byref(pl), p("rng_fluvial"), p("rng_debris"), N, p("remote0"), *tail_args, flags, None)
        elif entry == "soil_particles_pair_colour":
            rc = lib.soil_particles_pair_colour(C.byref(pl), C.byref(cp), p("rng_fluvial"), p("rng_debris"), N, H, W, fl(*sc),
                                                pp._ref(), flags, None)
        else:
            rc = lib.soil_particles_pair_colour_slab(C.byref(pl), C.byref(cp), p("rng_fluvial"), p("rng_debris"), N, p("remote0"),
                                                     *tail_args, flags, None)
        ok(rc)
    return Case(planes, call, want)


_REF_PAIR = ("the oracle's two launches (tests/test_gpu_erosion_batch_oracle.py: _oracle_particles) with util.flux_close; the rng "
             "states word for word; the planes a launch does not touch are inputs; the flux planes and rng are in/out")
row("soil_particles_pair_slab", [PARTICLE_SIZE], _REF_PAIR, modes=True)(
    lambda key, oracle: pair_case("soil_particles_pair_slab", key, oracle, False, False))
row("soil_particles_pair_slab_ex", [PARTICLE_SIZE], _REF_PAIR + "; SOIL_FLUX_OVERWRITE over stale flux planes", modes=True)(
    lambda key, oracle: pair_case("soil_particles_pair_slab_ex", key, oracle, False, True))
row("soil_particles_pair_colour", [PARTICLE_SIZE], _REF_PAIR + "; the colour flux planes stale on entry", modes=True)(
    lambda key, oracle: pair_case("soil_particles_pair_colour", key, oracle, True, False))
row("soil_particles_pair_colour_slab", [PARTICLE_SIZE], _REF_PAIR + "; SOIL_FLUX_OVERWRITE; the colour flux planes stale on entry",
    modes=True)(lambda key, oracle: pair_case("soil_particles_pair_colour_slab", key, oracle, True, True))


def step_close(got, want, what):
    """A step's planes against the oracle's composition of the step from the same state: the bar of
    tests/test_gpu_colour_step.py (the same trajectories; the fp32 order of the flux sums differs)."""
    from test_gpu_parity import _close_but_for_stray_walks
    # Cells that are equal on both sides are set aside first, and the absolute bar is taken from the finite values: on
    # strongly anisotropic cells (3 x 33 x 260: 0.61 x 0.077) the debris flux of a few cells overflows to +inf on the
    # device and in the oracle alike, and the comparator takes inf - inf, a NaN, for a difference.
    same = got == want
    finite = np.abs(want[np.isfinite(want)])
    atol = 1e-5 * ((finite.max() if finite.size else 0.0) + 1e-30)
    _close_but_for_stray_walks(np.where(same, F32(0), got), np.where(same, F32(0), want), 1e-4, atol, 2e-6, what)


def oracle_step(oracle, st, N, seed, offset, sc, op, colour):
    """The oracle's step of one model from state `st`: the cell phase's planes by the names of soil_erosion_planes."""
    from test_gpu_erosion_batch_oracle import _oracle_cells
    flux = oracle_pair(oracle, st, N, seed, offset, sc, op, colour)
    cells = _oracle_cells(oracle, st, flux, sc, op, colour)
    out = {n: cells[n] for n in CELL_OUT}
    if colour:
        out.update({n: cells[k] for n, k in COLOUR.items() if n != "albedo_bedrock"})
    return out, flux


def step_case(entry, key, oracle, colour, flags):
    H, W = key
    N, st, op, sc = N_PARTICLES, particle_state(oracle, H, W), particle_op(oracle), scale_of(H, W)
    offset = STEP * N
    dirty = bool(flags)
    planes = model_planes(key, [st], with_flux(STEP_ROLES, "stale" if dirty else "zero"), colour, STEP_COLOUR)
    planes.insert(5, P("rng", OUT, (N,), ga.RNG))

    def want(lib, oracle):
        cells, flux = oracle_step(oracle, st, N, SEED, offset, sc, op, colour)
        w = dict(rng=rng_at(oracle, N, SEED, offset + 4))
        if not dirty:
            w.update({n: (a, step_close) for n, a in cells.items()})
            w.update({n: np.zeros(plane_shape(key, n), F32) for n in FLUX})
            return w
        # both flux flags: the flux planes are left behind, and the cell phase is the oracle's on them, bit for bit
        w.update(flux_judges({n: flux[n] for n in FLUX}))

        def judge(got, exp, what):
            res = oracle.erode_cells(st["layers"], st["uplift"], st["rainfall"], *[got[n].copy() for n in FLUX], sc, op)
            for n in CELL_OUT:
                util.assert_bit_equal(got[n], res[n], "%s: %s from the flux planes left behind" % (what, n))
        w["*"] = (None, judge)
        return w
    pp = pparam(op)

    def call(lib, p):
        pl, cp = structs(p, colour)
        head = (p("rng"), N, SEED, STEP, H, W, fl(*sc), pp._ref())
        if entry == "soil_erode_step":
            rc = lib.soil_erode_step(C.byref(pl), *head, None)
        elif entry == "soil_erode_step_ex":
            rc = lib.soil_erode_step_ex(C.byref(pl), *head, flags, None)
        else:
            rc = lib.soil_erode_step_colour(C.byref(pl), C.byref(cp), *head, flags, None)
        ok(rc)
    return Case(planes, call, want)


_REF_STEP = ("composed (the particle launches + the cell phase): the oracle's composition of the step with the tolerance of "
             "tests/test_gpu_colour_step.py (rtol 1e-4, atol 1e-5 of the plane's largest value); the flux planes come back +0; rng "
             "(re-seeded by the step: an output) word for word; waterHeight, velocity and debrisVelocity are in/out")
row("soil_erode_step", [PARTICLE_SIZE], _REF_STEP, composed=True, modes=True)(
    lambda key, oracle: step_case("soil_erode_step", key, oracle, False, 0))
row("soil_erode_step_ex", [PARTICLE_SIZE], "composed: SOIL_STEP_FLUX_IN_DIRTY | SOIL_STEP_FLUX_OUT_DIRTY over stale flux planes: the flux "
    "planes left behind with util.flux_close, and the cell phase against oracle.erode_cells on those very planes bit for bit",
    composed=True, modes=True)(lambda key, oracle: step_case("soil_erode_step_ex", key, oracle, False, 3))
row("soil_erode_step_colour", [PARTICLE_SIZE], _REF_STEP + "; the colour planes of the step", composed=True, modes=True)(
    lambda key, oracle: step_case("soil_erode_step_colour", key, oracle, True, 0))


@row("soil_erode", [PARTICLE_SIZE], "composed (one step on the legacy containers): the oracle's composition with the tolerances of "
     "tests/test_gpu_api_surface.py; the track planes, stale on entry, come back +0; height, sediment, discharge and the momenta are "
     "in/out", composed=True, modes=True)
def _(key, oracle):
    from soillib_amd import _abi
    H, W = key
    N, op, sc = N_PARTICLES, particle_op(oracle), scale_of(H, W)
    # the data planes start from zero, as the containers of tests/test_gpu_api_surface.py do
    st = dict(particle_state(oracle, H, W), waterHeight=np.zeros((H, W), F32), velocity=np.zeros((H, W, 2), F32),
              debrisVelocity=np.zeros((H, W, 2), F32))
    bed, sed = np.ascontiguousarray(st["layers"][..., 0]), np.ascontiguousarray(st["layers"][..., 1])
    data = dict(discharge="waterHeight", momentum="velocity", debris_momentum="debrisVelocity")
    outs = dict(mass="mass", debris="debris")
    track = dict(discharge_track="waterFlux", mass_track="massFlux", momentum_track="velocityFlux", debris_track="debrisFlux",
                 debris_momentum_track="debrisVelocityFlux")
    planes = [P("height", INOUT, bed), P("uplift", IN, st["uplift"]), P("sediment", INOUT, sed), P("rainfall", IN, st["rainfall"])]
    planes += [P(n, INOUT, st[k]) for n, k in data.items()]
    planes += [P(n, OUT, plane_shape(key, k), F32) for n, k in outs.items()]
    planes += [P(n, INOUT, stale(st, k)) for n, k in track.items()]

    def close(atol_of):
        return lambda got, exp, what: np.testing.assert_allclose(got, exp, rtol=1e-4, atol=atol_of(exp), err_msg=what)
    rel = close(lambda a: 1e-5 * (np.nanmax(np.abs(a)) + 1e-30))

    def want(lib, oracle):
        cells, _ = oracle_step(oracle, st, N, SEED, STEP * N, sc, op, False)
        w = dict(height=(cells["layers_next"][..., 0], close(lambda a: 1e-6)), sediment=(cells["layers_next"][..., 1], close(lambda a: 1e-6)))
        w.update({n: (cells[k], rel) for n, k in dict(data, **outs).items()})
        w.update({n: np.zeros(plane_shape(key, k), F32) for n, k in track.items()})
        return w
    pp = pparam(op)

    def call(lib, p):
        m = _abi.ErodeModel()
        for n in _abi._ERODE_MODEL:
            setattr(m, n, p(n))
        ok(lib.soil_erode(C.byref(m), H, W, N, SEED, STEP, 1, fl(*sc), pp._ref(), None))
    return Case(planes, call, want)


# ------------------------------------------------------------------ the particle launches and whole steps of a batch

BATCH_SEEDS = (11, 2 ** 40 + 5, 7)


def batch_n(key):
    return int([e for e in extras(key) if e.startswith("N")][0][1:])


def batch_models(oracle, key, form):
    """(op, scale, N) of every model of a batch: one for all, a param per model (the sweep), or everything per model."""
    B, H, W = dims(key)
    N = batch_n(key)
    base = particle_op(oracle, 33)
    if form is None:
        return [(base, scale_of(H, W), N)] * B
    ops = []
    for b in range(B):
        op = particle_op(oracle, (33, 12, 64)[b])
        op.evapRate *= 1.0 + b
        op.gravity *= 1.0 + 0.25 * b
        ops.append(op)
    if form == "params":
        return [(ops[b], scale_of(H, W), N) for b in range(B)]
    return [(ops[b], tuple(s * (1.0 + 0.5 * b) for s in scale_of(H, W)), (N, N // 2, 0)[b]) for b in range(B)]


def batch_flux_close(got, want, what):
    from test_gpu_erosion_batch_oracle import _flux_close_at_any_scale
    for b in range(len(want)):
        _flux_close_at_any_scale(got[b], want[b], "%s, model %d" % (what, b))


def batch_step_close(got, want, what):
    for b in range(len(want)):
        step_close(got[b], want[b], "%s, model %d" % (what, b))


def batch_case(entry, key, oracle, colour, form, step):
    from soillib_amd import _abi
    B, H, W = dims(key)
    N = batch_n(key)
    sts = [particle_state(oracle, H, W, b) for b in range(B)]
    mods = batch_models(oracle, key, form)
    roles = with_flux(STEP_ROLES if step else PARTICLE_ROLES, "zero")
    planes = model_planes(key, sts, roles, colour, STEP_COLOUR if step else PARTICLE_COLOUR)

    def want(lib, oracle):
        outs = [oracle_step(oracle, sts[b], mods[b][2], BATCH_SEEDS[b], STEP * mods[b][2], mods[b][1], mods[b][0], colour)
                for b in range(B)]
        if step:
            w = {n: (np.stack([o[0][n] for o in outs]), batch_step_close) for n in outs[0][0]}
            w.update({n: np.zeros(plane_shape(key, n), F32) for n in FLUX})
            return w
        w = {n: (np.stack([o[1][n] for o in outs]), batch_flux_close) for n in FLUX}
        if colour:
            w.update({n: (np.stack([o[1][COLOUR[n]] for o in outs]), batch_flux_close) for n in ("albedo_fluvial", "albedo_debris")})
        return w
    pps = [pparam(m[0]) for m in mods]

    def call(lib, p):
        pl, cp = structs(p, colour)
        cref = C.byref(cp) if colour else None
        seeds = (C.c_uint64 * B)(*BATCH_SEEDS)
        sc = fl(*mods[0][1])
        if form == "params":
            params = (_abi.Param * B)()
            for b in range(B):
                util.copy_param(mods[b][0], params[b])
        if form == "models":
            recs = (_abi.BatchModel * B)()
            for b in range(B):
                util.copy_param(mods[b][0], recs[b].param)
                for i in range(3):
                    recs[b].scale[i] = mods[b][1][i]
                recs[b].N, recs[b].seed, recs[b].step_index = mods[b][2], BATCH_SEEDS[b], STEP
        fn = getattr(lib, entry)
        if form == "models":
            rc = fn(C.byref(pl), cref, B, H, W, recs, None)
        elif form == "params":
            rc = fn(C.byref(pl), cref, B, H, W, N, seeds, STEP, sc, params, None)
        elif colour:
            rc = fn(C.byref(pl), cref, B, H, W, N, seeds, STEP, sc, pps[0]._ref(), None)
        else:
            rc = fn(C.byref(pl), B, H, W, N, seeds, STEP, sc, pps[0]._ref(), None)
        ok(rc)
    return Case(planes, call, want)


_REF_BP = ("the oracle's two launches of every model from streams (seeds[b], n, step_index N) with "
           "tests/test_gpu_erosion_batch_oracle.py's _flux_close_at_any_scale; the planes a launch does not touch are inputs")
_REF_BS = ("composed (soil_particles_batch* + soil_erode_cells_fused_batch*): the oracle's composition of every model's step with the "
           "tolerance of tests/test_gpu_colour_step.py; the flux planes come back +0")
for _entry, _colour, _form, _note in (("soil_particles_batch", False, None, ""),
                                      ("soil_particles_batch_colour", True, None, "; with the colour planes"),
                                      ("soil_particles_batch_params", True, "params", "; a param per model, with colour"),
                                      ("soil_particles_batch_models", False, "models", "; a param, scale and walker count per model (the last: 0)")):
    row(_entry, BATCH_PARTICLES, _REF_BP + _note)(
        lambda key, oracle, e=_entry, c=_colour, f=_form: batch_case(e, key, oracle, c, f, False))
for _entry, _colour, _form, _note in (("soil_erode_step_batch", False, None, ""),
                                      ("soil_erode_step_batch_colour", True, None, "; with the colour planes"),
                                      ("soil_erode_step_batch_params", False, "params", "; a param per model, no colour"),
                                      ("soil_erode_step_batch_models", True, "models", "; a param, scale and walker count per model, with colour")):
    row(_entry, BATCH_PARTICLES, _REF_BS + _note, composed=True)(
        lambda key, oracle, e=_entry, c=_colour, f=_form: batch_case(e, key, oracle, c, f, True))


# ------------------------------------------------------------------ the tests

PLAIN = {e: r for e, r in ROWS.items() if not r.modes}
MODES = {e: r for e, r in ROWS.items() if r.modes}


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ga.PLACEMENTS)
@pytest.mark.parametrize("entry,key", case_list(PLAIN))
def test_guard_bands(hip, oracle, entry, key, placement):
    run_row(hip, oracle, ROWS, entry, key, placement)


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ga.PLACEMENTS)
@pytest.mark.parametrize("entry,key", case_list(MODES))
def test_guard_bands_in_every_particle_launch_shape(hip, oracle, particle_mode, entry, key, placement):   # noqa: F811
    run_row(hip, oracle, ROWS, entry, key, placement)
