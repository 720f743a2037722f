"""Guard bands around every plane of every call: no entry point of include/soil_hip.h that takes a device plane reads
or writes outside its planes.  One table row per entry point, called through soillib_amd._abi with the pointers of a
guard-band arena (tests/guard_arena.py: ONE allocation, every plane between two guard bands at least as large as the
plane, outputs prefilled with the guard pattern).  For every row, at every shape, placement ("aligned": 256-byte
starts, the 16-byte kernel forms; "off4": 4 bytes past a 16-byte boundary, the scalar forms) and under both guard
fills (A a quiet NaN, B a large finite number; int32 planes: two valid values):

  1. guards    every guard byte is unchanged after the call
  2. inputs    every pure input plane is bit-unchanged (in/out and scratch planes are marked as such in the row)
  3. outputs   every output is the reference the op's own test file uses (the CPU oracle, tests/*_ref.py, tests/util.py),
               compared the way that file compares it: word for word, or util.flux_close and its kin for planes that
               floating-point atomics accumulate
  4. fills     the outputs under fill A and under fill B are the same bits (atomic planes: both within the tolerance)

This file: the rows of the runtime, the stencils, the flow graphs and everything that works on one (H, W) plane or a
batch of them; tests/test_gpu_guard_bands_erosion.py: the erosion step, its phases, batches and summaries.  The
completeness test at the end walks _abi.SIGNATURES: an entry point is a row or is in EXEMPT, which holds only entry
points without a device plane argument.

Shapes.  GRID: (5, 7) below any tile or vector width, (65, 70) across the 64-cell tiles with W % 4 == 2, (33, 260)
with W % 4 == 0 (the 16-byte form), (1, 9) and (9, 1).  BATCH: B = 3 of each of those and of (65, 67), whose odd
H * W puts model 1 four bytes off every wider alignment.  (1, 1) is left to the existing tests: no second valid index
exists for an int guard.

Knobs.  SOIL_PATHS_IDX64=1 is read once per process: the rows of the pointer-doubling engine run again in one child
process that has it set.  (SOIL_CELLS_VARIANT is read on every call: tests/test_gpu_guard_bands_erosion.py.)

Out of scope: include/soil_slab.h (the multi-GPU runner; its planes are its own allocations), and the library's
internal workspace, which cannot be guarded from outside.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):      # run as a script (the child process, the table): nothing is preset
    if _p not in sys.path:
        sys.path.insert(0, _p)

import deposit_n_ref as dnref  # noqa: E402
import deposit_ref as depref
import diffuse_ref as difref
import downstream_ref as dref
import fill_ref
import flats_ref
import flow_paths_ref as fref
import guard_arena as ga
import mfd_ref as mref
import power_n_ref as pnref
import slope_limit_ref as slref
import stream_order_ref as soref
import upstream_ref as uref
from guard_arena import IN, INOUT, OUT, SCRATCH, Case, P
from util import assert_solve_uniform_close

D4, D8 = 0, 1
GRID = [(5, 7), (65, 70), (33, 260), (1, 9), (9, 1)]
BATCH = [(3,) + s for s in GRID] + [(3, 65, 67)]
SC2 = (1.5, 2.0)
SC3 = (0.4, 1.7, 3.0)
F32, F64, I32 = np.float32, np.float64, np.int32


class Row:
    def __init__(self, entry, cases, build, ref, planes="", composed=False):
        self.entry, self.cases, self.build, self.ref, self.planes, self.composed = entry, cases, build, ref, planes, composed


ROWS = {}


def row(entry, cases, ref, composed=False):
    def deco(build):
        assert entry not in ROWS, entry
        ROWS[entry] = Row(entry, list(cases), build, ref, composed=composed)
        return build
    return deco


def ok(rc):
    from soillib_amd import _abi
    _abi.check(rc)


def fl(*v):
    return (C.c_float * len(v))(*[float(x) for x in v])


def key_id(key):
    return "x".join(str(k) for k in key)


def case_list(rows):
    return [pytest.param(entry, key, id="%s-%s" % (entry, key_id(key))) for entry, r in rows.items() for key in r.cases]


_WANT = {}


def run_row(lib, oracle, rows, entry, key, placement):
    """The case of row `entry` at `key`; its reference is made once and shared by the placements."""
    case = rows[entry].build(key, oracle)
    if (entry, key) not in _WANT:
        _WANT[entry, key] = case.want(lib, oracle)
    ga.run_case(lib, case, placement, _WANT[entry, key], "%s %s" % (entry, key_id(key)))


# ------------------------------------------------------------------ inputs, made once

_MEMO = {}


def memo(fn):
    def wrapped(*a):
        k = (fn.__name__,) + a
        if k not in _MEMO:
            v = fn(*a)
            for x in (v if isinstance(v, tuple) else (v,)):
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)
            _MEMO[k] = v
        return _MEMO[k]
    return wrapped


def dims(key):
    """(B or None, H, W) of a row's key; the strings of a key are its extras (a mode, a flag, a walker count)."""
    key = tuple(k for k in key if not isinstance(k, str))
    return (None,) + key if len(key) == 2 else key


def extras(key):
    return tuple(k for k in key if isinstance(k, str))


def stacked(key, fn):
    """fn(b) per model, stacked for a batch key; fn(0) for a grid key."""
    B = dims(key)[0]
    return fn(0) if B is None else np.stack([fn(b) for b in range(B)])


def per_model(key, fn, *planes):
    """fn(plane slices of model b ...) stacked over the models of a batch key, or fn(planes) for a grid key; a None
    plane stays None; fn may return a tuple or dict of planes."""
    B = dims(key)[0]
    if B is None:
        return fn(0, *planes)
    outs = [fn(b, *[None if p is None else p[b] for p in planes]) for b in range(B)]
    if isinstance(outs[0], dict):
        return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}
    if isinstance(outs[0], tuple):
        return tuple(None if outs[0][i] is None else np.stack([o[i] for o in outs]) for i in range(len(outs[0])))
    return np.stack(outs)


@memo
def height(H, W, seed):
    return mref.fractal(H, W, seed=seed)


@memo
def graph(H, W, edge, seed):
    """A downhill receiver graph (acyclic) with a few entries that are no edge: -1s, the cell itself, INT32_MIN."""
    g = fref.descent(fref.terrain(H, W, seed), edge).copy()
    r = np.random.default_rng(seed)
    flat = g.reshape(-1)
    n = flat.size
    for value, share in ((None, 0.03), (fref.INT32_MIN, 0.02)):
        at = np.flatnonzero(r.random(n) < share)
        flat[at] = at if value is None else value
    return g


@memo
def rand(H, W, seed, channels=0, lo=0.0, hi=1.0):
    r = np.random.default_rng([seed, H, W])
    return (lo + (hi - lo) * r.random((H, W) + ((channels,) if channels else ()))).astype(F32)


@memo
def mask(H, W, seed, share):
    return (np.random.default_rng([seed, H, W, 7]).random((H, W)) < share).astype(I32)


def hs(key, seed=3):
    _, H, W = dims(key)
    return stacked(key, lambda b: height(H, W, seed + 10 * b))


def gs(key, edge, seed=2):
    _, H, W = dims(key)
    return stacked(key, lambda b: graph(H, W, edge, seed + b))


def rs(key, seed, channels=0, lo=0.0, hi=1.0):
    _, H, W = dims(key)
    return stacked(key, lambda b: rand(H, W, seed + 100 * b, channels, lo, hi))


def ms(key, seed, share):
    _, H, W = dims(key)
    return stacked(key, lambda b: mask(H, W, seed + b, share))


def cells(key):
    _, H, W = dims(key)
    return H * W


def idx_fills(key):
    """Two valid indices inside a model, for the guards of graph planes."""
    return (0, cells(key) - 1)


def scales_of(key):
    """The scale argument(s) of a row: one pair for a grid, B pairs and their count for a batch; and the pairs."""
    B = dims(key)[0]
    if B is None:
        return (fl(*SC2),), [SC2]
    pairs = [(SC2[0] * (1 + 0.5 * b), SC2[1] / (1 + b)) for b in range(B)]
    return (fl(*[v for p in pairs for v in p]), B), pairs


def shape_args(key):
    return tuple(d for d in dims(key) if d is not None)


def out_shape(key, *tail):
    return shape_args(key) + tail


def batch_suffix(key):
    return "" if dims(key)[0] is None else "_batch"


# ------------------------------------------------------------------ the runtime's element-wise ops (csrc/runtime.hip)

@row("soil_set_f32", GRID, "numpy.full")
def _(key, oracle):
    n = cells(key)
    return Case([P("t", OUT, key, F32)], lambda lib, p: ok(lib.soil_set_f32(p("t"), 2.5, n, None)),
                lambda lib, oracle: dict(t=np.full(key, 2.5, F32)))


@row("soil_set_i32", GRID, "numpy.full")
def _(key, oracle):
    n = cells(key)
    return Case([P("t", OUT, key, I32, idx_fills(key))], lambda lib, p: ok(lib.soil_set_i32(p("t"), -7, n, None)),
                lambda lib, oracle: dict(t=np.full(key, -7, I32)))


@row("soil_add_f32", GRID, "numpy: t + other in float32")
def _(key, oracle):
    t, other = rs(key, 1), rs(key, 2, lo=-1.0)
    return Case([P("t", INOUT, t), P("other", IN, other)],
                lambda lib, p: ok(lib.soil_add_f32(p("t"), p("other"), t.size, None)),
                lambda lib, oracle: dict(t=t + other))


@row("soil_multiply_f32", GRID, "numpy: t * value in float32")
def _(key, oracle):
    t = rs(key, 3, lo=-1.0)
    return Case([P("t", INOUT, t)], lambda lib, p: ok(lib.soil_multiply_f32(p("t"), 0.3, t.size, None)),
                lambda lib, oracle: dict(t=t * F32(0.3)))


@row("soil_rng_seed", GRID, "oracle.rng_seed")
def _(key, oracle):
    n = cells(key)
    return Case([P("rng", OUT, (n,), ga.RNG)], lambda lib, p: ok(lib.soil_rng_seed(p("rng"), n, 2 ** 40 + 3, 2 ** 33 + 1, None)),
                lambda lib, oracle: dict(rng=oracle.rng_seed(n, 2 ** 40 + 3, 2 ** 33 + 1).astype(ga.RNG)))


@row("soil_selftest_math", GRID, "oracle.expf / log2f / powf (ops 0, 1, 2), as tests/test_gpu_parity.py")
def _(key, oracle):
    a, b = rs(key, 4, lo=0.0, hi=50.0), rs(key, 5, lo=0.005, hi=3.0)
    x = rs(key, 6, lo=-80.0, hi=80.0)

    def call(lib, p):
        ok(lib.soil_selftest_math(p("exp"), p("x"), p("x"), x.size, 0, None))
        ok(lib.soil_selftest_math(p("log2"), p("a"), p("a"), a.size, 1, None))
        ok(lib.soil_selftest_math(p("pow"), p("a"), p("b"), a.size, 2, None))
    return Case([P("a", IN, a), P("exp", OUT, key, F32), P("b", IN, b), P("log2", OUT, key, F32), P("x", IN, x),
                 P("pow", OUT, key, F32)], call,
                lambda lib, oracle: dict(exp=(oracle.expf(x), "naneq"), log2=(oracle.log2f(a), "naneq"),
                                         pow=(oracle.powf(a, b), "naneq")))


def _pow_close(got, want, what):
    """tests/test_gpu_mfd.py::test_the_power_function_is_the_pow_the_restatement_assumes: the device's fp64 pow is
    deterministic and not correctly rounded; it is numpy's to 1e-14 relative."""
    assert np.allclose(got, want, rtol=1e-14, atol=0.0), what


_pow_close.deterministic = True         # an element-wise plane: the two fills are compared bit for bit


@row("soil_selftest_math64", GRID, "numpy.power to 1e-14 relative, as tests/test_gpu_mfd.py holds it; the fills bit for bit")
def _(key, oracle):
    a = rs(key, 7, lo=1e-3, hi=40.0).astype(F64)
    b = np.full(key, 1.1, F64)

    def want(lib, oracle):
        return dict(out=(np.power(a, b), _pow_close))
    case = Case([P("a", IN, a), P("out", OUT, key, F64), P("b", IN, b)],
                lambda lib, p: ok(lib.soil_selftest_math64(p("out"), p("a"), p("b"), a.size, 0, None)), want)
    return case


# ------------------------------------------------------------------ stencils (csrc/stencil.hip), noise, resize, path

@row("soil_gradient", GRID, "oracle.gradient")
def _(key, oracle):
    h = hs(key)
    return Case([P("out", OUT, key + (2,), F32), P("in", IN, h)],
                lambda lib, p: ok(lib.soil_gradient(p("out"), p("in"), *key, fl(*SC2), None)),
                lambda lib, oracle: dict(out=(oracle.gradient(h, SC2), "naneq")))


@row("soil_negslope", GRID, "oracle.negslope")
def _(key, oracle):
    h = hs(key)
    return Case([P("in", IN, h), P("out", OUT, key, F32)],
                lambda lib, p: ok(lib.soil_negslope(p("out"), p("in"), *key, fl(*SC2), None)),
                lambda lib, oracle: dict(out=(oracle.negslope(h, SC2), "naneq")))


@row("soil_laplacian", GRID, "oracle.laplacian (D = 2)")
def _(key, oracle):
    t = rs(key, 8, channels=2, lo=-1.0)
    return Case([P("out", OUT, key + (2,), F32), P("in", IN, t)],
                lambda lib, p: ok(lib.soil_laplacian(p("out"), p("in"), *key, 2, fl(*SC2), None)),
                lambda lib, oracle: dict(out=(oracle.laplacian(t, SC2), "naneq")))


@row("soil_gaussian_blur", GRID, "oracle.gaussian_blur (C = 2); tensor is in/out, scratch is scratch")
def _(key, oracle):
    t = rs(key, 9, channels=2, lo=-1.0)
    return Case([P("tensor", INOUT, t), P("scratch", SCRATCH, key + (2,), F32)],
                lambda lib, p: ok(lib.soil_gaussian_blur(p("tensor"), p("scratch"), *key, 2, 1.3, None)),
                lambda lib, oracle: dict(tensor=(oracle.gaussian_blur(t, 1.3), "naneq")))


@row("soil_normal", GRID, "oracle.normal")
def _(key, oracle):
    h = hs(key)
    return Case([P("in", IN, h), P("out", OUT, key + (3,), F32)],
                lambda lib, p: ok(lib.soil_normal(p("out"), p("in"), *key, fl(*SC3), None)),
                lambda lib, oracle: dict(out=(oracle.normal(h, SC3), "naneq")))


def _noise_param(ext0, ext1):
    from soillib_amd import _abi
    q = _abi.NoiseParam()
    _abi.lib().soil_noise_param_default(C.byref(q))
    q.seed, q.ext[0], q.ext[1] = 3.0, float(ext0), float(ext1)
    return q


@row("soil_noise", GRID, "oracle.noise")
def _(key, oracle):
    H, W = key
    q = _noise_param(H, W)
    return Case([P("out", OUT, key, F32)], lambda lib, p: ok(lib.soil_noise(p("out"), H, W, C.byref(q), None)),
                lambda lib, oracle: dict(out=(oracle.noise(H, W, seed=3.0, ext=(float(H), float(W))), "naneq")))


@row("soil_noise_window", GRID, "rows x0 .. x0 + H of oracle.noise of the (H + 6, W) map")
def _(key, oracle):
    H, W = key
    q = _noise_param(H + 6, W)
    return Case([P("out", OUT, key, F32)], lambda lib, p: ok(lib.soil_noise_window(p("out"), H, W, 2, C.byref(q), None)),
                lambda lib, oracle: dict(out=(oracle.noise(H + 6, W, seed=3.0, ext=(float(H + 6), float(W)))[2:2 + H], "naneq")))


@row("soil_resize", GRID, "oracle.resize (D = 2), from ((H + 1) / 2, W + 3) to (H, W)")
def _(key, oracle):
    H, W = key
    old = ((H + 1) // 2, W + 3)
    src = rand(old[0], old[1], 10, 2, -1.0, 1.0)
    return Case([P("src", IN, src), P("dst", OUT, key + (2,), F32)],
                lambda lib, p: ok(lib.soil_resize(p("dst"), p("src"), H, W, old[0], old[1], 2, None)),
                lambda lib, oracle: dict(dst=(oracle.resize(src, key), "naneq")))


@row("soil_solve_uniform", GRID, "oracle.solve_uniform with util.assert_solve_uniform_close (K = 2): flux is added to "
     "with atomics; the rng plane word for word")
def _(key, oracle):
    H, W = key
    N = 300
    sc = (0.05, 0.05)
    flow = np.ascontiguousarray(-oracle.gradient(hs(key) * F32(0.02), sc))
    src, decay = rs(key, 11, channels=2, hi=1e-3), rs(key, 12, hi=0.01)
    rng = oracle.rng_seed(N, 1, 0).astype(ga.RNG)

    def want(lib, oracle):
        r = oracle.rng_seed(N, 1, 0)
        flux = oracle.solve_uniform(flow, src, decay, r, sc, N)
        return dict(flux=(flux, lambda got, exp, what: assert_solve_uniform_close(got, exp)), rng=r.astype(ga.RNG))
    return Case([P("flow", IN, flow), P("flux", OUT, key + (2,), F32), P("source", IN, src), P("rng", INOUT, rng),
                 P("decay", IN, decay)],
                lambda lib, p: ok(lib.soil_solve_uniform(p("flux"), p("flow"), p("source"), p("decay"), p("rng"), N, H, W, 2,
                                                         fl(*sc), N, None)), want)


# ------------------------------------------------------------------ flow graphs (csrc/graph.hip)

def _graph_row(entry, ref_name):
    for batch in (False, True):
        @row(entry + ("_batch" if batch else ""), BATCH if batch else GRID, "oracle.%s, model by model" % ref_name)
        def _(key, oracle, entry=entry, ref_name=ref_name):
            h = hs(key)
            name = entry + batch_suffix(key)
            return Case([P("height", IN, h), P("graph", OUT, shape_args(key), I32, idx_fills(key))],
                        lambda lib, p: ok(getattr(lib, name)(p("graph"), p("height"), *shape_args(key), D8, None)),
                        lambda lib, oracle: dict(graph=per_model(key, lambda b, x: getattr(oracle, ref_name)(x, D8), h)))


_graph_row("soil_direction", "direction")
_graph_row("soil_steepest", "steepest")

RW_SEEDS = (11, 2 ** 40 + 5, 7)


def _rw_want(lib, oracle, key, h, offset, T):
    import test_gpu_random_weighted as rw
    return per_model(key, lambda b, x: rw.restate(lib, oracle, x, D8, RW_SEEDS[b], offset, T), h)


@row("soil_random_weighted", GRID, "the bit-exact restatement of tests/test_gpu_random_weighted.py (restate)")
def _(key, oracle):
    h = hs(key)
    return Case([P("graph", OUT, key, I32, idx_fills(key)), P("height", IN, h)],
                lambda lib, p: ok(lib.soil_random_weighted(p("graph"), p("height"), *key, D8, RW_SEEDS[0], 5, 10.0, None)),
                lambda lib, oracle: dict(graph=_rw_want(lib, oracle, key, h, 5, 10.0)))


@row("soil_random_weighted_batch", BATCH, "the same restatement, model b with seeds[b]")
def _(key, oracle):
    h = hs(key)
    seeds = (C.c_uint64 * 3)(*RW_SEEDS)
    return Case([P("graph", OUT, key, I32, idx_fills(key)), P("height", IN, h)],
                lambda lib, p: ok(lib.soil_random_weighted_batch(p("graph"), p("height"), *key, D8, seeds, 5, 10.0, None)),
                lambda lib, oracle: dict(graph=_rw_want(lib, oracle, key, h, 5, 10.0)))


for _batch in (False, True):
    @row("soil_slope" + ("_batch" if _batch else ""), BATCH if _batch else GRID, "oracle.slope on oracle.steepest's graph")
    def _(key, oracle):
        h = hs(key)
        flow = per_model(key, lambda b, x: oracle.steepest(x, D8), h)
        args, pairs = scales_of(key)
        return Case([P("slope", OUT, shape_args(key), F32), P("tensor", IN, h), P("flow", IN, flow, fills=idx_fills(key))],
                    lambda lib, p: ok(getattr(lib, "soil_slope" + batch_suffix(key))(p("slope"), p("tensor"), p("flow"),
                                                                                    *shape_args(key), *args, None)),
                    lambda lib, oracle: dict(slope=(per_model(key, lambda b, x, f: oracle.slope(x, f, pairs[b]), h, flow), "naneq")))

    @row("soil_accumulate" + ("_batch" if _batch else ""), BATCH if _batch else GRID, "oracle.accumulate with a decay plane")
    def _(key, oracle):
        g, src, decay = gs(key, D8), rs(key, 13), rs(key, 14, lo=0.5, hi=1.0)
        return Case([P("graph", IN, g, fills=idx_fills(key)), P("out", OUT, shape_args(key), F32), P("source", IN, src),
                     P("decay", IN, decay)],
                    lambda lib, p: ok(getattr(lib, "soil_accumulate" + batch_suffix(key))(
                        p("out"), p("graph"), p("source"), p("decay"), *shape_args(key), D8, None)),
                    lambda lib, oracle: dict(out=(per_model(key, lambda b, a, s, d: oracle.accumulate(a, s, D8, d), g, src, decay),
                                                  "naneq")))


@row("soil_multiflow", GRID, "the mean of tests/test_gpu_accumulate_oracle.py (_mean) over oracle.accumulate of the "
     "restated random_weighted graphs, K = 3; sum is in/out (accumulated into, zero on entry)")
def _(key, oracle):
    h, src = hs(key), rs(key, 15)
    K, seed, T = 3, 11, 10.0

    def want(lib, oracle):
        import test_gpu_accumulate_oracle as acc
        import test_gpu_random_weighted as rw
        terms = {k: oracle.accumulate(rw.restate(lib, oracle, h, D8, seed, k, T), src, D8) for k in range(K)}
        return dict(sum=acc._mean(terms, range(K), K, key))
    return Case([P("sum", INOUT, np.zeros(key, F64)), P("height", IN, h), P("source", IN, src)],
                lambda lib, p: ok(lib.soil_multiflow(p("sum"), p("height"), p("source"), *key, D8, seed, 0, 1, K, K, T, None)),
                want)


# ------------------------------------------------------------------ conditioning (csrc/conditioning.hip, flats.hip)

@memo
def dem(H, W, seed):
    return fill_ref.pitted(H, W, seed) if H * W >= 64 else fill_ref.small(H, W, seed)


def dems(key):
    _, H, W = dims(key)
    return stacked(key, lambda b: dem(H, W, b))


_FILLED = {}


def filled(oracle, key):
    if key not in _FILLED:
        _FILLED[key] = per_model(key, lambda b, z: oracle.fill_depressions(z, D8), dems(key))
        _FILLED[key].setflags(write=False)
    return _FILLED[key]


for _batch in (False, True):
    @row("soil_fill_depressions" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "oracle.fill_depressions with fill_ref.compare")
    def _(key, oracle):
        z = dems(key)
        return Case([P("out", OUT, shape_args(key), F32), P("height", IN, z)],
                    lambda lib, p: ok(getattr(lib, "soil_fill_depressions" + batch_suffix(key))(
                        p("out"), p("height"), *shape_args(key), D8, None)),
                    lambda lib, oracle: dict(out=(filled(oracle, key), lambda got, want, what: fill_ref.compare(got, want, z, what))))

    @row("soil_flat_distance" + ("_batch" if _batch else ""), BATCH if _batch else GRID, "flats_ref.distance_bfs on a filled DEM")
    def _(key, oracle):
        z = filled(oracle, key)
        return Case([P("height", IN, z), P("dist", OUT, shape_args(key), I32, (0, 1))],
                    lambda lib, p: ok(getattr(lib, "soil_flat_distance" + batch_suffix(key))(
                        p("dist"), p("height"), *shape_args(key), D8, None)),
                    lambda lib, oracle: dict(dist=per_model(key, lambda b, x: flats_ref.distance_bfs(x, D8), z)))

    @row("soil_flat_receivers" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "flats_ref.receivers on oracle.steepest's graph of a filled DEM and flats_ref.distance_bfs")
    def _(key, oracle):
        z = filled(oracle, key)
        g = per_model(key, lambda b, x: oracle.steepest(x, D8), z)
        dist = per_model(key, lambda b, x: flats_ref.distance_bfs(x, D8), z)
        return Case([P("in", IN, g, fills=idx_fills(key)), P("out", OUT, shape_args(key), I32, idx_fills(key)),
                     P("height", IN, z), P("dist", IN, dist, fills=(0, 1))],
                    lambda lib, p: ok(getattr(lib, "soil_flat_receivers" + batch_suffix(key))(
                        p("out"), p("in"), p("height"), p("dist"), *shape_args(key), D8, None)),
                    lambda lib, oracle: dict(out=per_model(key, lambda b, a, x, d: flats_ref.receivers(a, x, d, D8), g, z, dist)))

    # ---- threshold hillslopes (csrc/slope_limit.hip)
    @row("soil_slope_limit" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "slope_limit_ref.jacobi and excess, a slope plane")
    def _(key, oracle):
        _, H, W = dims(key)
        h = stacked(key, lambda b: slref.smooth(H, W, 5 + b))
        sp = stacked(key, lambda b: slref.lithology(H, W, 5 + b, 0.3))
        args, pairs = scales_of(key)

        def want(lib, oracle):
            w = per_model(key, lambda b, x, s: slref.jacobi(x, pairs[b], s, D8), h, sp)
            return dict(out=w, excess=per_model(key, lambda b, x, y: slref.excess(x, y), h, w))
        return Case([P("out", OUT, shape_args(key), F32), P("height", IN, h), P("excess", OUT, shape_args(key), F32),
                     P("slope_plane", IN, sp)],
                    lambda lib, p: ok(getattr(lib, "soil_slope_limit" + batch_suffix(key))(
                        p("out"), p("excess"), p("height"), p("slope_plane"), 0.0, *shape_args(key), *args, D8, None)), want)

    # ---- exact multiple-flow accumulation (csrc/mfd.hip)
    @row("soil_mfd_weights" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "mfd_ref.weights, kind power p = 1.1 with the device's own pow (tests/test_gpu_mfd.py: dev_pow), a dist plane")
    def _(key, oracle):
        B, H, W = dims(key)
        h = hs(key)
        dist = per_model(key, lambda b, x: flats_ref.distance_bfs(x, D8), h)
        args, pairs = scales_of(key)

        def want(lib, oracle):
            from test_gpu_mfd import dev_pow
            return dict(weights=per_model(key, lambda b, x, d: mref.weights(x, D8, p=1.1, scale=pairs[b], dist=d, pow_=dev_pow), h, dist))
        return Case([P("height", IN, h), P("weights", OUT, ((B,) if B else ()) + (8, H, W), F32), P("dist", IN, dist, fills=(0, 1))],
                    lambda lib, p: ok(getattr(lib, "soil_mfd_weights" + batch_suffix(key))(
                        p("weights"), p("height"), p("dist"), 1, 1.1, *shape_args(key), *args, D8, None)), want)

    @row("soil_mfd_accumulate" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "mfd_ref.accumulate of mfd_ref.weights, kind Gibbs T = 10 with the device's own exp2 (dev_exp2); out and out64")
    def _(key, oracle):
        h, src = hs(key, 4), rs(key, 16)
        dist = per_model(key, lambda b, x: flats_ref.distance_bfs(x, D8), h)
        args, pairs = scales_of(key)

        def want(lib, oracle):
            from test_gpu_mfd import dev_exp2
            a = per_model(key, lambda b, x, s, d: mref.accumulate(mref.weights(x, D8, T=10.0, dist=d, exp2=dev_exp2), s)[0],
                          h, src, dist)
            return dict(out64=a, out=a.astype(F32))
        return Case([P("out", OUT, shape_args(key), F32), P("height", IN, h), P("out64", OUT, shape_args(key), F64),
                     P("source", IN, src), P("dist", IN, dist, fills=(0, 1))],
                    lambda lib, p: ok(getattr(lib, "soil_mfd_accumulate" + batch_suffix(key))(
                        p("out"), p("out64"), p("height"), p("source"), p("dist"), 0, 10.0, *shape_args(key), *args, D8, None)),
                    want)

    # ---- the pointer-doubling engine (csrc/flow_paths.hip, downstream.hip, upstream.hip, stream_order.hip)
    @row("soil_flow_paths" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "flow_paths_ref.walk_doubling: terminal, steps and length, a stop plane")
    def _(key, oracle):
        g, stop = gs(key, D8), ms(key, 1, 0.05)
        args, pairs = scales_of(key)
        names = ("terminal", "steps", "length")
        return Case([P("terminal", OUT, shape_args(key), I32, idx_fills(key)), P("graph", IN, g, fills=idx_fills(key)),
                     P("steps", OUT, shape_args(key), I32, (0, 1)), P("stop", IN, stop, fills=(0, 1)),
                     P("length", OUT, shape_args(key), F32)],
                    lambda lib, p: ok(getattr(lib, "soil_flow_paths" + batch_suffix(key))(
                        p("terminal"), p("steps"), p("length"), p("graph"), p("stop"), *shape_args(key), D8, *args, None)),
                    lambda lib, oracle: dict(zip(names, per_model(key, lambda b, a, s: fref.walk_doubling(a, D8, pairs[b], s), g, stop))))

    @row("soil_downstream" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "downstream_ref.solve_doubling: out and out64; a, b, t and stop planes")
    def _(key, oracle):
        g, stop = gs(key, D8), ms(key, 2, 0.05)
        a, b, t = rs(key, 17), rs(key, 18, lo=0.5, hi=1.0), rs(key, 19, lo=-1.0)
        args, pairs = scales_of(key)

        def want(lib, oracle):
            o = per_model(key, lambda m, G, A, Bp, T, S: dref.solve_doubling(G, D8, A, Bp, T, pairs[m], S), g, a, b, t, stop)
            return dict(out=o[0], out64=o[1])
        return Case([P("out", OUT, shape_args(key), F32), P("graph", IN, g, fills=idx_fills(key)), P("a", IN, a),
                     P("out64", OUT, shape_args(key), F64), P("b", IN, b), P("t", IN, t), P("stop", IN, stop, fills=(0, 1))],
                    lambda lib, p: ok(getattr(lib, "soil_downstream" + batch_suffix(key))(
                        p("out"), p("out64"), p("graph"), p("a"), p("b"), p("t"), p("stop"), *shape_args(key), D8, *args, None)),
                    want)

    @row("soil_stream_power" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "downstream_ref.solve_doubling(power=...): out and out64; uplift and stop planes")
    def _(key, oracle):
        g, stop = gs(key, D8), ms(key, 3, 0.05)
        h, k, u = hs(key, 5), rs(key, 20, hi=0.5), rs(key, 21, hi=0.1)
        args, pairs = scales_of(key)
        dt = 0.75

        def want(lib, oracle):
            o = per_model(key, lambda m, G, Hh, K, U, S: dref.solve_doubling(G, D8, scale=pairs[m], stop=S, power=(Hh, K, U, dt)),
                          g, h, k, u, stop)
            return dict(out=o[0], out64=o[1])
        return Case([P("height", IN, h), P("out", OUT, shape_args(key), F32), P("graph", IN, g, fills=idx_fills(key)),
                     P("erosivity", IN, k), P("out64", OUT, shape_args(key), F64), P("uplift", IN, u),
                     P("stop", IN, stop, fills=(0, 1))],
                    lambda lib, p: ok(getattr(lib, "soil_stream_power" + batch_suffix(key))(
                        p("out"), p("out64"), p("height"), p("graph"), p("erosivity"), p("uplift"), p("stop"), *shape_args(key),
                        D8, *args, dt, None)), want)

    @row("soil_upstream_extreme" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "upstream_ref.extreme: out and arg, a stop plane; op min on the grid, max on the batch")
    def _(key, oracle):
        g, stop, v = gs(key, D8), ms(key, 4, 0.05), rs(key, 22, lo=-1.0)
        op = uref.MIN if dims(key)[0] is None else uref.MAX

        def want(lib, oracle):
            o = per_model(key, lambda m, G, V, S: uref.extreme(G, V, D8, op, S), g, v, stop)
            return dict(out=o[0], arg=o[1])
        return Case([P("graph", IN, g, fills=idx_fills(key)), P("out", OUT, shape_args(key), F32), P("value", IN, v),
                     P("arg", OUT, shape_args(key), I32, idx_fills(key)), P("stop", IN, stop, fills=(0, 1))],
                    lambda lib, p: ok(getattr(lib, "soil_upstream_extreme" + batch_suffix(key))(
                        p("out"), p("arg"), p("graph"), p("value"), p("stop"), *shape_args(key), D8, op, None)), want)

    @row("soil_stream_order" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "stream_order_ref.by_levels: all five outputs; channel, area and stop planes")
    def _(key, oracle):
        g, stop = gs(key, D8), ms(key, 5, 0.03)
        chan, area = ms(key, 6, 0.9), rs(key, 23, hi=10.0)
        thr = 1.0

        def want(lib, oracle):
            o = per_model(key, lambda m, G, Ch, A, S: {n: v for n, v in soref.by_levels(G, D8, Ch, A, thr, S).items() if n != "levels"},
                          g, chan, area, stop)
            return {n: np.asarray(o[n], I32) for n in soref.OUTPUTS}
        outs = [P(n, OUT, shape_args(key), I32, idx_fills(key) if n == "channel_graph" else (0, 1)) for n in soref.OUTPUTS]
        return Case([outs[0], P("graph", IN, g, fills=idx_fills(key)), outs[1], P("channel", IN, chan, fills=(0, 1)), outs[2],
                     P("area", IN, area), outs[3], P("stop", IN, stop, fills=(0, 1)), outs[4]],
                    lambda lib, p: ok(getattr(lib, "soil_stream_order" + batch_suffix(key))(
                        *[p(n) for n in soref.OUTPUTS], p("graph"), p("channel"), p("area"), thr, p("stop"), *shape_args(key),
                        D8, None)), want)

    # ---- the iterated stream-power steps (csrc/downstream.hip)
    @row("soil_stream_power_deposit" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "deposit_ref.solve_iterated: out, out64, flux and residual, 3 iterations, an uplift plane")
    def _(key, oracle):
        return _deposit_case(key, oracle, None)

    @row("soil_stream_power_deposit_n" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "deposit_n_ref.solve_iterated at n = 2 (no power function): out, out64, flux and residual, 3 iterations")
    def _(key, oracle):
        return _deposit_case(key, oracle, 2.0)

    @row("soil_stream_power_n" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "power_n_ref.solve_iterated at n = 2 (no power function): out, out64 and residual, 3 iterations; uplift and stop")
    def _(key, oracle):
        g, stop = gs(key, D8), ms(key, 7, 0.05)
        h, k, u = hs(key, 6), rs(key, 24, hi=0.5), rs(key, 25, hi=0.1)
        args, pairs = scales_of(key)
        dt, B = 0.75, dims(key)[0]

        def want(lib, oracle):
            o = per_model(key, lambda m, G, Hh, K, U, S: {n: v for n, v in pnref.solve_iterated(
                G, D8, Hh, K, pairs[m], dt, 2.0, U, S, iters=3, pow=None).items() if n in ("out", "out64", "residual")},
                g, h, k, u, stop)
            return dict(out=o["out"], out64=o["out64"], residual=np.asarray(o["residual"], F64).reshape(B or 1))
        return Case([P("out", OUT, shape_args(key), F32), P("height", IN, h), P("residual", OUT, (B or 1,), F64),
                     P("graph", IN, g, fills=idx_fills(key)), P("erosivity", IN, k), P("out64", OUT, shape_args(key), F64),
                     P("uplift", IN, u), P("stop", IN, stop, fills=(0, 1))],
                    lambda lib, p: ok(getattr(lib, "soil_stream_power_n" + batch_suffix(key))(
                        p("out"), p("out64"), p("residual"), p("height"), p("graph"), p("erosivity"), p("uplift"), p("stop"),
                        *shape_args(key), D8, *args, dt, 2.0, 3, None)), want)

    # ---- hillslope diffusion (csrc/diffuse.hip)
    @row("soil_diffuse" + ("_batch" if _batch else ""), BATCH if _batch else GRID,
         "diffuse_ref.solve_sweeps: out and out64; diffusivity, uplift and fixed planes, first_axis 0")
    def _(key, oracle):
        h, kd, u, fixed = hs(key, 7), rs(key, 26, lo=0.1, hi=2.0), rs(key, 27, hi=0.1), ms(key, 8, 0.05)
        args, pairs = scales_of(key)
        dt = 0.5

        def want(lib, oracle):
            o = per_model(key, lambda m, Hh, K, U, Fx: difref.solve_sweeps(Hh, pairs[m], dt, diffusivity=K, uplift=U, fixed=Fx,
                                                                          border=1, first_axis=0), h, kd, u, fixed)
            return dict(out=o[0], out64=o[1])
        return Case([P("height", IN, h), P("out", OUT, shape_args(key), F32), P("diffusivity", IN, kd),
                     P("out64", OUT, shape_args(key), F64), P("uplift", IN, u), P("fixed", IN, fixed, fills=(0, 1))],
                    lambda lib, p: ok(getattr(lib, "soil_diffuse" + batch_suffix(key))(
                        p("out"), p("out64"), p("height"), p("diffusivity"), p("uplift"), p("fixed"), *shape_args(key), *args,
                        0.0, dt, 1, 0, None)), want)


def _deposit_case(key, oracle, n):
    g = stacked(key, lambda b: _clean_graph(dims(key)[1], dims(key)[2], 2 + b))
    h, k, dpo, u = hs(key, 8), rs(key, 28, hi=0.5), rs(key, 29, hi=0.8), rs(key, 30, hi=0.1)
    args, pairs = scales_of(key)
    dt, B = 0.75, dims(key)[0]
    entry = "soil_stream_power_deposit" + ("" if n is None else "_n") + batch_suffix(key)

    def one(m, G, Hh, K, Dp, U):
        if n is None:
            o = depref.solve_iterated(oracle, G, D8, Hh, K, Dp, pairs[m], dt, U, iters=3)
        else:
            o = dnref.solve_iterated(oracle, G, D8, Hh, K, Dp, pairs[m], dt, n, U, iters=3, pow=None)
        return {name: o[name] for name in ("out", "out64", "flux", "residual")}

    def want(lib, oracle):
        o = per_model(key, one, g, h, k, dpo, u)
        return dict(out=o["out"], out64=o["out64"], flux=(o["flux"], "naneq"), residual=np.asarray(o["residual"], F64).reshape(B or 1))
    exponent = () if n is None else (n,)
    return Case([P("out", OUT, shape_args(key), F32), P("height", IN, h), P("flux", OUT, shape_args(key), F32),
                 P("graph", IN, g, fills=idx_fills(key)), P("residual", OUT, (B or 1,), F64), P("erosivity", IN, k),
                 P("out64", OUT, shape_args(key), F64), P("deposition", IN, dpo), P("uplift", IN, u)],
                lambda lib, p: ok(getattr(lib, entry)(
                    p("out"), p("out64"), p("flux"), p("residual"), p("height"), p("graph"), p("erosivity"), p("deposition"),
                    p("uplift"), *shape_args(key), D8, *args, dt, *exponent, 3, None)), want)


@memo
def _clean_graph(H, W, seed):
    """A downhill receiver graph and -1s: what oracle.accumulate, the upstream sum of the deposit steps, takes."""
    return fref.descent(fref.terrain(H, W, seed), D8)


# ------------------------------------------------------------------ the tests

@pytest.mark.gpu
@pytest.mark.parametrize("placement", ga.PLACEMENTS)
@pytest.mark.parametrize("entry,key", case_list(ROWS))
def test_guard_bands(hip, oracle, entry, key, placement):
    run_row(hip, oracle, ROWS, entry, key, placement)


# ------------------------------------------------------------------ the pointer-doubling rows on 64-bit offsets

# SOIL_PATHS_IDX64=1 (docs/KNOBS.md) is read once per process: the rows of the pointer-doubling engine and of the
# steps built on it run again in a child process that has it set, as the ops' own tests run it
PATHS_ROWS = [e + b for e in ("soil_flow_paths", "soil_downstream", "soil_stream_power", "soil_upstream_extreme",
                              "soil_stream_order", "soil_stream_power_deposit", "soil_stream_power_n",
                              "soil_stream_power_deposit_n") for b in ("", "_batch")]
def child_main():
    from oracle import pyoracle
    from soillib_amd import _abi
    lib = _abi.lib()
    assert lib.soil_device_count() > 0
    done = 0
    for entry in PATHS_ROWS:
        for key in ROWS[entry].cases:
            for placement in ga.PLACEMENTS:
                run_row(lib, pyoracle, ROWS, entry, key, placement)
                done += 1
        # the info records that count chunks on 64-bit offsets say that the knob took (soil_stream_order_info has five
        # words; those of the iterated steps — launches, chunks, iterations, scratch bytes — do not tell the offset width)
        info = {"soil_flow_paths": "soil_flow_paths_info", "soil_downstream": "soil_downstream_info",
                "soil_stream_power": "soil_downstream_info", "soil_upstream_extreme": "soil_upstream_extreme_info",
                "soil_stream_order": "soil_stream_order_info"}
        name = entry[:-len("_batch")] if entry.endswith("_batch") else entry
        if name in info:
            words = (C.c_int64 * 5)()
            _abi.check(getattr(lib, info[name])(words))
            chunks, idx64 = int(words[0]), int(words[2])
            assert idx64 == chunks >= 1, (entry, list(words))
    print("%d cases on 64-bit offsets" % done)


@pytest.mark.gpu
def test_the_pointer_doubling_rows_on_64_bit_offsets(hip):
    env = dict(os.environ, SOIL_PATHS_IDX64="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--idx64"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    want = sum(len(ROWS[e].cases) for e in PATHS_ROWS) * len(ga.PLACEMENTS)
    assert "%d cases on 64-bit offsets" % want in r.stdout, r.stdout[-1000:]


# ------------------------------------------------------------------ completeness

# entry points without a device plane argument, by the kinds the row-free test admits
EXEMPT = {
    "version, error and device plumbing": ["soil_abi_version", "soil_last_error", "soil_device_count", "soil_set_device",
                                           "soil_device_name"],
    "memory, copies, synchronisation and events": ["soil_malloc", "soil_free", "soil_memcpy_h2d", "soil_memcpy_d2h",
                                                   "soil_memcpy_d2d", "soil_stream_synchronize", "soil_device_synchronize",
                                                   "soil_event_create", "soil_event_destroy", "soil_event_record",
                                                   "soil_event_elapsed_ms"],
    "defaults, info records, modes": ["soil_param_default", "soil_noise_param_default", "soil_fill_depressions_info",
                                      "soil_flow_paths_info", "soil_downstream_info", "soil_upstream_extreme_info",
                                      "soil_stream_order_info", "soil_stream_power_deposit_info", "soil_stream_power_n_info",
                                      "soil_stream_power_deposit_n_info", "soil_diffuse_info", "soil_flat_distance_info",
                                      "soil_slope_limit_info", "soil_mfd_info", "soil_set_particle_mode",
                                      "soil_set_particle_arith", "soil_get_particle_arith", "soil_set_debris_retire",
                                      "soil_get_debris_retire", "soil_ghost_rows", "soil_workspace_release",
                                      "soil_host_objects_info"],
    "host memory": ["soil_normal_host", "soil_noise_host", "soil_tiff_peek", "soil_tiff_tag", "soil_tiff_read", "soil_tiff_write"],
    "counters returned through a host pointer": ["soil_debris_retire_violations", "soil_particle_steps"],
}


def all_rows():
    import test_gpu_guard_bands_erosion as erosion
    both = dict(ROWS)
    assert not set(both) & set(erosion.ROWS)
    both.update(erosion.ROWS)
    return both


def test_every_entry_point_with_a_device_plane_has_a_row():
    """No GPU needed: the rows and the exemptions partition _abi.SIGNATURES, and an exempt entry point is of one of
    the admitted kinds by its very name."""
    from soillib_amd import _abi
    rows = set(all_rows())
    exempt = [e for names in EXEMPT.values() for e in names]
    assert len(exempt) == len(set(exempt))
    assert not rows & set(exempt), sorted(rows & set(exempt))
    missing = sorted(set(_abi.SIGNATURES) - rows - set(exempt))
    assert not missing, "entry points that are neither a row nor exempt: %s" % missing
    unknown = sorted((rows | set(exempt)) - set(_abi.SIGNATURES))
    assert not unknown, "rows or exemptions that name no entry point: %s" % unknown
    admitted = ("_default", "_info", "_host", "soil_tiff_", "soil_memcpy_", "soil_event_", "_synchronize", "soil_set_", "soil_get_")
    plumbing = set(EXEMPT["version, error and device plumbing"]) | {"soil_malloc", "soil_free", "soil_ghost_rows",
                                                                    "soil_workspace_release", "soil_set_device"}
    counters = set(EXEMPT["counters returned through a host pointer"])
    for e in exempt:
        assert e in plumbing or e in counters or any(a in e for a in admitted), "%s is of no exempt kind" % e
    # ... and none of them takes a pointer the header documents as a device plane: the only void* of an exempt
    # entry are streams, events, host buffers and soil_malloc / soil_free / memcpy's own addresses
    for e in EXEMPT["defaults, info records, modes"] + EXEMPT["counters returned through a host pointer"]:
        assert sum(a is C.c_void_p for a in _abi.SIGNATURES[e][1]) <= 1, e      # (at most the stream)


def table():
    """The table of profiles/guard_bands/checks.txt: entry point, planes by role, shapes, reference."""
    from oracle import pyoracle
    lines = []
    for entry, r in sorted(all_rows().items()):
        case = r.build(r.cases[0], pyoracle)
        roles = {}
        for name, role, data, dtype, fills in case.planes:
            roles.setdefault(role, []).append(name)
        planes = "; ".join("%s: %s" % (role, ", ".join(roles[role])) for role in (IN, OUT, INOUT, SCRATCH) if role in roles)
        lines.append("%s%s\n    planes  %s\n    shapes  %s\n    ref     %s" % (
            entry, "  [composed]" if r.composed else "", planes, " ".join(key_id(k) for k in r.cases), r.ref))
    return "\n".join(lines)


if __name__ == "__main__":
    import test_gpu_guard_bands as this          # the one copy the erosion table imports too, not __main__'s
    if "--idx64" in sys.argv:
        this.child_main()
    else:
        print(this.table())
