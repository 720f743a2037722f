"""Upstream extrema along a receiver graph on the device (include/soil_hip.h: soil_upstream_extreme,
soil_upstream_extreme_batch; soillib_amd.soil.upstream_min / upstream_max / breach / condition_breached /
upstream_length and their _batch forms, ErosionBatch.upstream_min / upstream_max / breached / upstream_length), bit for
bit against the reference of tests/upstream_ref.py, which restates the definition and not the rounds: every comparison
is of int32 values or of float bit patterns; there is no tolerance anywhere.

  shapes     (1, 1), (1, 7); (13, 21) the scalar init; (12, 20) the 16-byte init; (5, 1028), (3, 261) two work-groups
             along a row; (64, 64); (256, 256) for the funnel; (1027, 2051) above the work-group cap
  graphs     a chain through every cell (every round is needed), a comb, a funnel in which every cell points straight
             at one outlet in the late rounds, cells with all K donors, two-cell cycles, a ring of four and a cycle
             round the border with tributaries, INT32_MIN / the cell itself / non-neighbours / diagonals under D4, the
             CPU oracle's steepest graphs of an oracle terrain, numpy's steepest graph of a terrain with plateaus, the
             library's conditioned graphs
  values     random, a plateau of equal values (arg: the smallest index, across work-group boundaries), +0 and -0 side
             by side, denormals, infinities, NaNs with payloads on a third of the cells, nothing but NaNs
  calls      min and max, every subset of {arg, out, stop}, planes 4 bytes off their alignment, a second stream with a
             call of another size in between
  batches    3 x 12 x 20 with a hostile and an all-NaN model between benign ones, slice for slice against single calls;
             more models than a launch's grid.z; chunks, work-group counts, 64-bit offsets and dense rounds in child
             processes, with the info record
  breaching  condition_breached, breach(cut=True) and upstream_length on a conditioned 96^2 terrain, the four properties
             of a breached surface, a lake cell that is cut; the batch's methods against the module's calls
"""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_paths_ref as fref
import upstream_ref as ref
from upstream_ref import D4, D8, MAX, MIN
from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 7), (13, 21), (12, 20), (5, 1028), (3, 261), (64, 64)]
OPS = {MIN: "min", MAX: "max"}


def _info():
    from soillib_amd import soil
    return soil.upstream_info()


def _rounds(H, W):
    return len(bin(H * W - 1)) - 2 if H * W > 1 else 0


def _opt(a):
    return None if a is None else to_gpu(a)


def _single(graph, value, edge, op, stop=None, arg=True):
    from soillib_amd import soil
    got = (soil.upstream_min if op == MIN else soil.upstream_max)(to_gpu(graph), to_gpu(value), edge, _opt(stop), arg)
    return (to_np(got[0]), to_np(got[1])) if arg else (to_np(got), None)


def _batch(graph, value, edge, op, stop=None, arg=True):
    from soillib_amd import soil
    fn = soil.upstream_min_batch if op == MIN else soil.upstream_max_batch
    got = fn(to_gpu(graph), to_gpu(value), edge, _opt(stop), arg)
    return (to_np(got[0]), to_np(got[1])) if arg else (to_np(got), None)


# ------------------------------------------------------------------ inputs and references, made once

@functools.lru_cache(maxsize=None)
def _graphs(H, W, edge):
    out = ref.graphs(H, W, edge)
    for g in out.values():
        g.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _values(H, W, kind):
    v = ref.values(H, W, kind, 7)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _stop(H, W):
    s = ref.stop_plane(H, W, 2)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _want(H, W, edge, gname, kind, op, with_stop):
    out = ref.extreme(_graphs(H, W, edge)[gname], _values(H, W, kind), edge, op, _stop(H, W) if with_stop else None)
    for o in out:
        o.setflags(write=False)
    return out


def _cases(H, W, edge):
    """(graph name, value kind, op, with a stop plane): every graph under every kind of value at the two small
    shapes, under three kinds that turn with the graph at the others; min and max, with and without stops, in turn."""
    names = sorted(_graphs(H, W, edge))
    every = H * W <= 13 * 21
    i = 0
    for gi, gname in enumerate(names):
        kinds = ref.VALUES if every else ("plateau", "nan_third", ref.VALUES[(gi + edge) % len(ref.VALUES)])
        for kind in kinds:
            for op in (MIN, MAX):
                yield gname, kind, op, i % 3 == 2
                i += 1


# ------------------------------------------------------------------ against the reference

@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
def test_single_grid_against_the_reference(hip, H, W, edge):
    for gname, kind, op, with_stop in _cases(H, W, edge):
        got = _single(_graphs(H, W, edge)[gname], _values(H, W, kind), edge, op, _stop(H, W) if with_stop else None)
        ref.same(got, _want(H, W, edge, gname, kind, op, with_stop),
                 "%s of %s on %s, stop %s, %dx%d edge %d" % (OPS[op], kind, gname, with_stop, H, W, edge))
        assert _info() == dict(chunks=1, vec_chunks=int(W % 4 == 0), idx64_chunks=0, rounds=_rounds(H, W))


@pytest.mark.parametrize("H,W", [(13, 21), (12, 20), (3, 261), (64, 64)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_oracles_steepest_graphs(hip, oracle, H, W, edge):
    """The CPU oracle's steepest graph of an oracle terrain (noise x 100): random values, a plateau and NaNs on a
    third of the cells, min and max, with and without stops, against the reference; and the terrain's own heights,
    which a strictly downhill graph leaves as they are."""
    h = np.ascontiguousarray(oracle.noise(H, W, seed=3.0, ext=(float(H), float(W))) * np.float32(100.0), np.float32)
    g = oracle.steepest(h, edge)
    assert g.dtype == np.int32 and (g >= 0).sum() > H * W // 2 and (g == -1).any()
    for kind in ("random", "plateau", "nan_third"):
        v = _values(H, W, kind)
        for op in (MIN, MAX):
            for stop in (None, _stop(H, W)):
                ref.same(_single(g, v, edge, op, stop), ref.extreme(g, v, edge, op, stop),
                         "oracle.steepest %dx%d edge %d, %s of %s, stop %s" % (H, W, edge, OPS[op], kind, stop is not None))
    out, arg = _single(g, h, edge, MIN)
    ref.same((out, arg), ref.extreme(g, h, edge, MIN), "the terrain's own heights")
    assert (out.view(np.uint32) == h.view(np.uint32)).all() and (arg == np.arange(H * W).reshape(H, W)).all()


@pytest.mark.parametrize("H,W", [(1, 2), (1, 3), (1, 1023), (1, 1024), (1, 1025), (32, 32), (31, 33), (4, 256)])
def test_a_chain_through_every_cell_needs_every_round(hip, H, W):
    """The least value at the head of a chain through every cell, the greatest at its foot: the head's value arrives
    at the foot only in the last of the ceil(log2(H W)) rounds, at H W = 2^k - 1, 2^k and 2^k + 1; the same chain closed
    to a cycle gives every cell the chain's extreme."""
    N = H * W
    g = fref.serpentine(H, W)
    pos = np.argsort(ref.cap.Chains("serpentine", H, W, D8).order)           # a cell's place on the chain
    v = pos.astype(np.float32).reshape(H, W)
    for op, value in ((MIN, v), (MAX, -v)):
        graph, out, arg = ref.chain_extreme(H, W, value, op)
        assert (graph == g).all() and (arg == 0).all()
        ref.same(_single(g, value, D4, op), (out, arg), "serpentine %dx%d %s" % (H, W, OPS[op]))
    v = (N - pos).astype(np.float32).reshape(H, W)                # falling along the chain: every cell keeps its own
    got = _single(g, v, D4, MIN)
    assert (got[0] == v).all() and (got[1] == np.arange(N).reshape(H, W)).all()
    closed = g.copy()
    foot = int(np.flatnonzero(g.reshape(-1) == -1)[0])
    closed.reshape(-1)[foot] = int(np.flatnonzero(g.reshape(-1) == foot)[0])   # the foot back to its donor: a 2-cycle
    ref.same(_single(closed, v, D4, MIN), ref.extreme(closed, v, D4, MIN), "a chain into a 2-cycle")


@pytest.mark.parametrize("kind", ["random", "plateau", "nan_third"])
def test_the_funnel_where_every_cell_points_at_one_outlet(hip, kind):
    """256^2 cells, none further than 510 edges from cell 0: in rounds 8 and 9 tens of thousands of cells push into
    the one word of the outlet."""
    H = W = 256
    g, v = ref.funnel(H, W), ref.values(H, W, kind, 11)
    for op in (MIN, MAX):
        want = ref.extreme(g, v, D4, op)
        ref.same(_single(g, v, D4, op), want, "funnel, %s of %s" % (OPS[op], kind))
        whole = ref.unpack(ref.words(v, op).min(keepdims=True), op, (1,))
        assert want[0][0, 0].view(np.uint32) == whole[0].view(np.uint32)[0] and want[1][0, 0] == whole[1][0]


def test_above_the_work_group_cap(hip):
    """(1027, 2051): more blocks of 256 cells than work-groups of a round, on the serpentine with a permuted value
    plane; the reference is a running minimum along the chain."""
    H, W = 1027, 2051
    assert ref.cap.above(H * W)
    v = np.random.default_rng(5).permutation(H * W).astype(np.float32).reshape(H, W) - np.float32(1e6)
    v[7, 11] = np.nan
    g, out, arg = ref.chain_extreme(H, W, v, MIN)
    ref.same(_single(g, v, D8, MIN), (out, arg), "serpentine above the cap, min")
    assert _info() == dict(chunks=1, vec_chunks=0, idx64_chunks=0, rounds=22)
    g, out, arg = ref.chain_extreme(H, W, v, MAX)
    ref.same(_single(g, v, D8, MAX, arg=False), (out, None), "serpentine above the cap, max")


# ------------------------------------------------------------------ call variants

def _planes_of_three():
    """Three models of (12, 20): a hostile graph and an all-NaN model between benign ones."""
    H, W = 12, 20
    G = _graphs(H, W, D8)
    graph = np.stack([G["descent"], G["hostile"], G["ring"]])
    value = np.stack([_values(H, W, "random"), _values(H, W, "all_nan"), _values(H, W, "nan_third")])
    stop = np.stack([_stop(H, W), np.zeros((H, W), np.int32), _stop(H, W)[::-1].copy()])
    return graph, value, stop


def test_every_subset_of_out_arg_and_stop(hip):
    from soillib_amd import _abi, silt
    graph, value, stop = _planes_of_three()
    B, H, W = graph.shape
    gg, gv, gs = to_gpu(graph), to_gpu(value), to_gpu(stop)
    ptr = lambda t: None if t is None else t.c_ptr
    for op in (MIN, MAX):
        for with_out, with_arg, with_stop in itertools.product((False, True), repeat=3):
            if not (with_out or with_arg):
                continue
            want = ref.extreme_batch(graph, value, D8, op, stop if with_stop else None)
            o = silt.tensor(silt.float32, silt.shape(B, H, W), silt.gpu) if with_out else None
            a = silt.tensor(silt.int32, silt.shape(B, H, W), silt.gpu) if with_arg else None
            _abi.check(hip.soil_upstream_extreme_batch(ptr(o), ptr(a), gg.c_ptr, gv.c_ptr, ptr(gs) if with_stop else None,
                                                       B, H, W, D8, op, _abi.stream()))
            ref.same((None if o is None else to_np(o), None if a is None else to_np(a)), want,
                     "batch %s, out %r arg %r stop %r" % (OPS[op], with_out, with_arg, with_stop))
            assert _info() == dict(chunks=1, vec_chunks=1, idx64_chunks=0, rounds=8)
            b = 1 + int(with_arg)                                 # the single grid on one model's slices
            o = silt.tensor(silt.float32, silt.shape(H, W), silt.gpu) if with_out else None
            a = silt.tensor(silt.int32, silt.shape(H, W), silt.gpu) if with_arg else None
            at = lambda t: C.c_void_p(t.ptr + 4 * b * H * W)
            _abi.check(hip.soil_upstream_extreme(ptr(o), ptr(a), at(gg), at(gv), at(gs) if with_stop else None, H, W, D8,
                                                 op, _abi.stream()))
            ref.same((None if o is None else to_np(o), None if a is None else to_np(a)), (want[0][b], want[1][b]),
                     "single %s, out %r arg %r stop %r" % (OPS[op], with_out, with_arg, with_stop))


def test_planes_off_their_16_bytes(hip):
    """Every plane 4 bytes past a 16-byte boundary, W % 4 == 0: the scalar init takes the call and gives what the
    16-byte form gives; so does one input plane off alone."""
    from soillib_amd import _abi, silt
    graph, value, stop = _planes_of_three()
    B, H, W = graph.shape
    want = ref.extreme_batch(graph, value, D8, MIN, stop)

    def shifted(arr, dtype):
        buf = silt.tensor(dtype, silt.shape(B * H * W + 4), silt.gpu)
        assert buf.ptr % 16 == 0
        view = silt.tensor.from_device(buf.ptr + 4, dtype, silt.shape(B, H, W), keepalive=buf)
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            _abi.check(hip.soil_memcpy_h2d(view.c_ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, _abi.stream()))
            _abi.check(hip.soil_stream_synchronize(_abi.stream()))
        return view

    off = [shifted(graph, silt.int32), shifted(value, silt.float32), shifted(stop, silt.int32)]
    on = [to_gpu(graph), to_gpu(value), to_gpu(stop)]
    o, a = shifted(None, silt.float32), shifted(None, silt.int32)
    for which, vec in (((0, 1, 2), 0), ((0,), 0), ((1,), 0), ((2,), 0), ((), 1)):
        g, v, s = [off[i] if i in which else on[i] for i in range(3)]
        _abi.check(hip.soil_upstream_extreme_batch(o.c_ptr, a.c_ptr, g.c_ptr, v.c_ptr, s.c_ptr, B, H, W, D8, MIN, _abi.stream()))
        ref.same((to_np(o), to_np(a)), want, "planes %r off their 16 bytes" % (which,))
        assert _info()["chunks"] == 1 and _info()["vec_chunks"] == vec, which


def test_on_another_stream_twice_and_with_another_size_in_between(hip):
    import torch
    from soillib_amd import _abi
    graph, value, stop = _planes_of_three()
    small = (graph, value, stop, ref.extreme_batch(graph, value, D8, MAX, stop))
    H, W = 64, 64
    g, v = _graphs(H, W, D8)["serpentine"], _values(H, W, "random")
    large = (g[None], v[None], None, tuple(o[None] for o in ref.extreme(g, v, D8, MAX)))
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        for graph, value, stop, want in (small, large, small, small, large):
            ref.same(_batch(graph, value, D8, MAX, stop), want, "on a second stream")
        ref.same(_single(g, v, D8, MAX), (large[3][0][0], large[3][1][0]), "single, second stream")
    finally:
        _abi.set_stream(0)


# ------------------------------------------------------------------ batches

def test_a_batch_is_its_single_calls_slice_for_slice(hip):
    for graph, value, stop in (_planes_of_three(), _five(12, 20), _five(13, 21)):
        for edge in (D4, D8):
            for op in (MIN, MAX):
                got = _batch(graph, value, edge, op, stop)
                ref.same(got, ref.extreme_batch(graph, value, edge, op, stop), "batch, edge %d %s" % (edge, OPS[op]))
                assert got[1].max() < graph[0].size, "arg is an index within its model"
                nan = 1 if len(graph) == 3 else 2
                assert (got[0][nan].view(np.uint32) == ref.NAN_WORD).all() and (got[1][nan] == -1).all(), "all NaN"
                for b in range(len(graph)):
                    one = _single(graph[b], value[b], edge, op, stop[b])
                    ref.same((got[0][b], got[1][b]), one, "model %d against the single call" % b)


def test_more_models_than_a_launch_takes(hip):
    """B = 65537 at (1, 4): two chunks (65535 models to a launch); every model against the reference of the
    different rows there are."""
    B, H, W = 65537, 1, 4
    r = np.random.default_rng(8)
    rows = np.array([[1, 2, 3, -1], [-1, 0, 1, 2], [1, 0, 3, 2], [3, 2, 1, 0], [4, 5, 6, 7], [1, 2, 1, 2],
                     [-1, -1, -1, -1], [1, 2, 3, fref.INT32_MAX]], np.int32)
    vals = np.array([[3, 1, 2, 1], [-0.0, 0.0, np.nan, -1], [np.nan] * 4, [np.inf, 5, -np.inf, 5]], np.float32)
    gi, vi = r.integers(0, len(rows), B), r.integers(0, len(vals), B)
    gi[[0, 65534, 65535, 65536]], vi[[0, 65534, 65535, 65536]] = [0, 1, 0, 1], [0, 0, 0, 0]
    graph, value = rows[gi].reshape(B, H, W), vals[vi].reshape(B, H, W)
    for op in (MIN, MAX):
        table = {(g, v): ref.extreme(rows[g].reshape(H, W), vals[v].reshape(H, W), D8, op)
                 for g in range(len(rows)) for v in range(len(vals))}
        want = tuple(np.stack([table[g, v][i] for g, v in zip(gi, vi)]) for i in range(2))
        got = _batch(graph, value, D8, op)
        ref.same(got, want, "65537 models, %s" % OPS[op])
        assert _info() == dict(chunks=2, vec_chunks=2, idx64_chunks=0, rounds=2)
        assert got[1].max() < H * W, "arg is an index within its model, in the second chunk too"


CHILD_SHAPES = [(12, 20), (13, 21)]
CHILD_ENVS = {
    "cells": {},                                                  # SOIL_FLOW_BATCH_CELLS: set per shape by the child
    "groups1": {"SOIL_PATHS_GROUPS": "1"},
    "groups3": {"SOIL_PATHS_GROUPS": "3"},
    "idx64": {"SOIL_PATHS_IDX64": "1"},
    "dense": {"SOIL_PATHS_LIST_FROM": "0"},
}


def _five(H, W):
    G = _graphs(H, W, D8)
    graph = np.stack([G["descent"], G["hostile"], G["cycles"], G["serpentine"], G["ring"]])
    value = np.stack([_values(H, W, k) for k in ("random", "nan_third", "all_nan", "plateau", "zeros")])
    return graph, value, np.stack([_stop(H, W)] * 5)


def _child_main(path, chunked):
    """The child of test_chunks_and_launch_shapes: B = 5 at both shapes, min and max; with `chunked` as 2 + 2 + 1."""
    out = {}
    for H, W in CHILD_SHAPES:
        if chunked:
            os.environ["SOIL_FLOW_BATCH_CELLS"] = str(2 * H * W + H * W // 2)
        graph, value, stop = _five(H, W)
        for op in (MIN, MAX):
            o, a = _batch(graph, value, D8, op, stop)
            i = _info()
            out["%dx%d_%s_out" % (H, W, OPS[op])], out["%dx%d_%s_arg" % (H, W, OPS[op])] = o, a
            out["%dx%d_%s_info" % (H, W, OPS[op])] = np.array([i["chunks"], i["vec_chunks"], i["idx64_chunks"], i["rounds"]])
    np.savez(path, **out)


@pytest.mark.parametrize("name", sorted(CHILD_ENVS))
def test_chunks_and_launch_shapes(hip, tmp_path, name):
    """A child process under SOIL_FLOW_BATCH_CELLS (chunks of 2 + 2 + 1 models), SOIL_PATHS_GROUPS = 1 and 3 (one
    work-group and three stride over every cell), SOIL_PATHS_IDX64 = 1 and SOIL_PATHS_LIST_FROM = 0 (dense rounds
    throughout): the reference's words whatever the path, and the info record of each call."""
    path = str(tmp_path / "upstream.npz")
    env = dict(os.environ)
    for k in ("SOIL_FLOW_BATCH_CELLS", "SOIL_PATHS_LIST_FROM", "SOIL_PATHS_IDX64", "SOIL_PATHS_GROUPS"):
        env.pop(k, None)
    env.update(CHILD_ENVS[name])
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path, name], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    chunks = 3 if name == "cells" else 1
    for H, W in CHILD_SHAPES:
        graph, value, stop = _five(H, W)
        for op in (MIN, MAX):
            key = "%dx%d_%s_" % (H, W, OPS[op])
            ref.same((got[key + "out"], got[key + "arg"]), ref.extreme_batch(graph, value, D8, op, stop),
                     "%dx%d %s under %s" % (H, W, OPS[op], name))
            assert got[key + "info"].tolist() == [chunks, chunks if W % 4 == 0 else 0, chunks if name == "idx64" else 0,
                                                  _rounds(H, W)]
    assert len(got.files) == 12


# ------------------------------------------------------------------ breaching

def _bench_height(H, seed=5.0):
    from soillib_amd import silt, soil
    p = soil.noise_t()
    p.seed = float(seed)
    p.ext = [H, H]
    h = soil.noise(silt.shape(H, H), p, host=silt.gpu)
    silt.multiply(h, 100.0)
    return h


@pytest.mark.parametrize("edge", [D4, D8])
def test_breaching_a_conditioned_terrain(hip, edge):
    from soillib_amd import soil
    H = 96
    h = _bench_height(H)
    filled, graph = soil.condition(h, edge)
    breached, graph2 = soil.condition_breached(h, edge)
    hn, fn, gn, bn = to_np(h), to_np(filled), to_np(graph), to_np(breached)
    assert (to_np(graph2) == gn).all(), "the graph is condition()'s"
    want, _ = ref.extreme(gn, hn, edge, MIN)
    ref.same((bn, None), (want, None), "condition_breached")
    b2, cut = soil.breach(h, graph, edge, cut=True)
    ref.same((to_np(b2), None), (want, None), "breach")
    ref.same((to_np(cut), None), (hn - want, None), "cut = height - breached, one fp32 subtraction")
    # the four properties, on the device's own output
    ref.check_breached(hn, bn, gn, edge)
    again = to_np(soil.breach(breached, graph, edge))
    assert (again.view(np.uint32) == bn.view(np.uint32)).all(), "breach is idempotent"
    downhill = soil.steepest(h, edge)
    same = to_np(soil.breach(h, downhill, edge))
    assert (same.view(np.uint32) == hn.view(np.uint32)).all(), "a strictly downhill graph leaves the heights as they are"
    # not vacuous: the terrain has lakes, and carving lowers cells where filling raised them
    lake = fn > hn
    assert lake.any() and ((bn < hn) & lake).any() and (to_np(cut)[lake] > 0).any(), "no lake cell is cut"
    assert (bn <= fn).all() and (bn[lake] < fn[lake]).all(), "a filled lake stands above the breached surface"
    # the longest flow path: upstream_max of the flow length less the cell's own
    scale = (20.0 / H, 30.0 / H)
    L = to_np(soil.flow_length(graph, edge, scale))
    assert not np.isnan(L).any()
    longest, _ = ref.extreme(gn, L, edge, MAX)
    got = to_np(soil.upstream_length(graph, edge, scale))
    ref.same((got, None), (longest + (-L), None), "upstream_length")
    assert (got >= 0).all() and (got[to_np(soil.accumulate(graph, to_gpu(np.ones((H, H), np.float32)), edge)) == 1] == 0).all()


def test_breaching_keeps_a_nan_height_and_passes_it_by(hip):
    from soillib_amd import soil
    H, W = 12, 20
    g = _graphs(H, W, D8)["funnel"]
    v = _values(H, W, "nan_third")
    b, cut = soil.breach(to_gpu(v), to_gpu(g), D8, cut=True)
    want, _ = ref.extreme(g, v, D8, MIN)
    ref.same((to_np(b), None), (want, None), "breach over NaNs")
    assert (np.isnan(to_np(cut)) == np.isnan(v)).all(), "the cut is NaN exactly where the height is"
    ok = ~np.isnan(v)
    assert (to_np(cut)[ok].view(np.uint32) == (v[ok] - want[ok]).view(np.uint32)).all()


def test_the_batch_methods_are_the_module_calls(hip, oracle):
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    B, H, W = 2, 96, 96
    p = product_param(script_param(oracle.default_param()))
    p.maxage = 64
    scales = [(20.0 / H * (1 + b), 20.0 / W, 4.0) for b in range(B)]
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    for scale in ((20.0 / H, 20.0 / W, 4.0), scales):
        bt = ErosionBatch(B, H, W, scale, p, 1024, [11 + 7 * b for b in range(B)])
        bt.set_layers(to_gpu(layers))
        silt.set(bt.rainfall, 1.0)
        bt.step()
        s2 = [s[:2] for s in scales] if scale is scales else scale[:2]
        for edge in (D4, D8):
            surface, graph = bt.breached(edge=edge)
            filled, g2 = soil.condition_batch(bt.height, edge)
            assert (to_np(graph) == to_np(g2)).all()
            want = to_np(soil.breach_batch(bt.height, g2, edge))
            assert (to_np(surface).view(np.uint32) == want.view(np.uint32)).all()
            hn, gn = to_np(bt.height), to_np(graph)
            for b in range(B):
                ref.same((want[b], None), (ref.extreme(gn[b], hn[b], edge, MIN)[0], None), "model %d" % b)
                ref.check_breached(hn[b], want[b], gn[b], edge)
            assert (want < to_np(filled)).any(), "some lake is cut"
            got = to_np(bt.upstream_length(graph=graph, edge=edge))
            assert (got.view(np.uint32) == to_np(soil.upstream_length_batch(graph, edge, s2)).view(np.uint32)).all()
            own = to_np(bt.upstream_length(edge=edge))            # the default graph: flow(edge)
            raw = soil.steepest_batch(bt.height, edge)
            assert (own.view(np.uint32) == to_np(soil.upstream_length_batch(raw, edge, s2)).view(np.uint32)).all()
            lo, where = bt.upstream_min(bt.height, graph=graph, edge=edge, arg=True)
            assert (to_np(lo).view(np.uint32) == want.view(np.uint32)).all()
            at = to_np(where)
            assert (np.take_along_axis(hn.reshape(B, -1), at.reshape(B, -1), 1).reshape(B, H, W) == want).all()
            hi = to_np(bt.upstream_max(bt.height, graph=graph, edge=edge))
            assert (hi.view(np.uint32) == to_np(soil.upstream_max_batch(graph, bt.height, edge)).view(np.uint32)).all()
            assert (hi >= hn).all()


# ------------------------------------------------------------------ refusals

def test_refusals_leave_the_planes_untouched(hip):
    from soillib_amd import _abi
    B, H, W = 2, 5, 8
    o = to_gpu(np.full((B, H, W), -7.5, np.float32))
    a = to_gpu(np.full((B, H, W), -77, np.int32))
    g = to_gpu(np.full((B, H, W), -1, np.int32))
    v = to_gpu(np.zeros((B, H, W), np.float32))
    st = _abi.stream()
    one, many = hip.soil_upstream_extreme, hip.soil_upstream_extreme_batch

    def refused(name, rc):
        assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, name
        assert _abi.last_error().startswith(name + ": "), (name, _abi.last_error())

    refused("upstream_extreme", one(o.c_ptr, a.c_ptr, None, v.c_ptr, None, H, W, D8, 0, st))
    refused("upstream_extreme", one(o.c_ptr, a.c_ptr, g.c_ptr, None, None, H, W, D8, 0, st))
    refused("upstream_extreme", one(None, None, g.c_ptr, v.c_ptr, None, H, W, D8, 0, st))
    refused("upstream_extreme", one(o.c_ptr, a.c_ptr, g.c_ptr, v.c_ptr, None, H, W, D8, 2, st))
    refused("upstream_extreme", one(o.c_ptr, a.c_ptr, g.c_ptr, v.c_ptr, None, H, W, 2, 0, st))
    refused("upstream_extreme", one(o.c_ptr, o.c_ptr, g.c_ptr, v.c_ptr, None, H, W, D8, 0, st))
    refused("upstream_extreme", one(v.c_ptr, a.c_ptr, g.c_ptr, v.c_ptr, None, H, W, D8, 0, st))
    for b, h, w in ((0, H, W), (B, 0, W), (B, H, -3), (B, 1 << 16, 1 << 16)):
        refused("upstream_extreme_batch", many(o.c_ptr, a.c_ptr, g.c_ptr, v.c_ptr, None, b, h, w, D8, 1, st))
    refused("upstream_extreme_batch", many(o.c_ptr, a.c_ptr, g.c_ptr, v.c_ptr, None, B, H, W, D8, -1, st))
    refused("upstream_extreme_batch", many(o.c_ptr, g.c_ptr, g.c_ptr, v.c_ptr, None, B, H, W, D8, 0, st))
    _abi.check(hip.soil_stream_synchronize(st))
    assert (to_np(o) == np.float32(-7.5)).all() and (to_np(a) == -77).all()
    assert (to_np(g) == -1).all() and (to_np(v) == 0).all()


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2] == "cells")
