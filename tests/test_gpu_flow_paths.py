"""Downstream walks along a receiver graph on the device (include/soil_hip.h: soil_flow_paths, soil_flow_paths_batch;
soillib_amd.soil.flow_paths / basins / flow_length / watershed and their _batch forms, ErosionBatch.basins /
flow_length), bit for bit against the numpy restatements of tests/flow_paths_ref.py: every comparison is of int32
values or of float bit patterns, the NaN word 0x7fc00000 included; there is no tolerance anywhere.

  shapes        the scalar form (1, 1), (1, 5), (5, 1), (2, 2), (37, 53); the 16-byte form (3, 4), (33, 260),
                (9, 1028), (256, 256); B in {1, 2, 3, 7, 64}; B = 65537 at (1, 4): more models than a launch takes
  graphs        different per model: a chain through every cell (H W - 1 edges: every round is needed — at
                H W = 2^k - 1, 2^k, 2^k + 1 too), cells with all K donors, all -1, the cell itself, non-neighbours,
                diagonals under D4, INT32_MIN / INT32_MAX, the neighbouring model's numbering, a two-cell cycle and a
                ring with trees feeding them next to parts that resolve, and the library's steepest and
                random_weighted graphs of a random terrain and of one with plateaus
  stop planes   none, one pour point, every cell, a stop cell on a cycle
  outputs       every subset of the three; anisotropic scales, per model
  plumbing      planes 4 bytes off their alignment, a second stream, repeated calls, chunks and the listed rounds in
                child processes, refusals that leave the planes untouched
  isolation     a model's slices do not change by a bit when the others are replaced
  single grid   the batch entry against the single-grid device call at 256^2 x 8 and 1024^2 x 2
  what exists   basin sizes against soil_accumulate of ones on steepest graphs at 256^2
"""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_paths_ref as ref
from flow_paths_ref import D4, D8
from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR = [(1, 1), (1, 5), (5, 1), (2, 2), (37, 53)]
VECTOR = [(3, 4), (33, 260), (9, 1028), (256, 256)]
BS = [1, 2, 3, 7, 64]
SCALES = [(1.0, 1.0), (0.25, 3.0), (1e-3, 1e3)]
NAMES = ref.NAMES
_same_words = ref.same_words              # (shared with tests/test_gpu_cpp_ops.py)


def _info():
    from soillib_amd import soil
    return soil.flow_paths_info()


def _np3(outs):
    return tuple(None if o is None else to_np(o) for o in outs)


def _single(graph, edge, scale=None, stop=None):
    from soillib_amd import soil
    return _np3(soil.flow_paths(to_gpu(graph), edge, scale, None if stop is None else to_gpu(stop)))


def _batch(graph, edge, scale=None, stop=None):
    from soillib_amd import soil
    return _np3(soil.flow_paths_batch(to_gpu(graph), edge, scale, None if stop is None else to_gpu(stop)))


# ------------------------------------------------------------------ inputs and references, made once

@functools.lru_cache(maxsize=None)
def _graphs(H, W, edge):
    """name -> graph of every kind a (H, W) grid takes: the built ones and numpy's downhill graphs of two terrains."""
    out = dict(ref.built_graphs(H, W, edge))
    if H * W <= 37 * 53:
        out["descent"] = ref.descent(ref.terrain(H, W, 2), edge)
        out["descent_plateaus"] = ref.descent(ref.terrain(H, W, 4, True), edge, seed=7)
    for g in out.values():
        g.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _stops(H, W):
    out = dict(ref.stop_planes(H, W))
    for s in out.values():
        if s is not None:
            s.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(H, W, edge, gname, sname, scale):
    """The reference of one model, made once and left as it is."""
    out = ref.walk_doubling(_graphs(H, W, edge)[gname], edge, scale, _stops(H, W)[sname])
    for o in out:
        if o is not None:
            o.setflags(write=False)
    return out


def _models(H, W, B, edge):
    """(graph name, stop name, scale) of each of B models: neighbours differ in all three."""
    gn, sn = sorted(_graphs(H, W, edge)), sorted(_stops(H, W))
    return [(gn[b % len(gn)], sn[(b // 2) % len(sn)], SCALES[b % 3]) for b in range(B)]


def _stack(H, W, B, edge):
    cfg = _models(H, W, B, edge)
    graph = np.stack([_graphs(H, W, edge)[g] for g, _, _ in cfg])
    stop = np.stack([np.zeros((H, W), np.int32) if _stops(H, W)[s] is None else _stops(H, W)[s] for _, s, _ in cfg])
    scales = [sc for _, _, sc in cfg]
    want = [_want(H, W, edge, *c) for c in cfg]
    return graph, stop, scales, tuple(np.stack([w[i] for w in want]) for i in range(3))


# ------------------------------------------------------------------ against the restatement

@pytest.mark.parametrize("H,W", SCALAR + VECTOR)
@pytest.mark.parametrize("edge", [D4, D8])
def test_single_grid_against_the_restatement(hip, H, W, edge):
    """Every graph under every stop plane (at 256^2: every graph without one, and the cycles and a hostile graph
    under each)."""
    for gname in sorted(_graphs(H, W, edge)):
        for i, sname in enumerate(sorted(_stops(H, W))):
            if H * W > 10000 and sname != "none" and gname not in ("cycles", "hostile"):
                continue
            scale = SCALES[i % 3]
            got = _single(_graphs(H, W, edge)[gname], edge, scale, _stops(H, W)[sname])
            _same_words(got, _want(H, W, edge, gname, sname, scale), "%s, stop %s, %dx%d edge %d" % (gname, sname, H, W, edge))


@pytest.mark.parametrize("H,W", [(1, 2), (1, 3), (1, 4), (1, 5), (1, 1023), (1, 1024), (1, 1025), (32, 32), (31, 33),
                                 (3, 341), (341, 3), (1025, 1), (4, 256), (5, 205)])
def test_a_chain_through_every_cell_needs_every_round(hip, H, W):
    """H W - 1 edges from the first cell: resolved by the last of the ceil(log2(H W)) rounds, at H W = 2^k - 1, 2^k and
    2^k + 1 in both forms; an implementation one round short leaves the head of the chain unresolved."""
    g = ref.serpentine(H, W)
    got = _single(g, D4, (0.25, 3.0))
    assert got[1][0, 0] == H * W - 1 and got[0][0, 0] >= 0
    _same_words(got, ref.walk_doubling(g, D4, (0.25, 3.0)), "serpentine %dx%d" % (H, W))
    # the same chain with a cycle at its end: nothing resolves, and the rounds still end
    g = g.copy()
    last = int(got[0][0, 0])
    before = int(np.flatnonzero(g.reshape(-1) == last)[0])
    g.reshape(-1)[last] = before
    t, s, l = _single(g, D4, (1.0, 1.0))
    assert (t == -1).all() and (s == -1).all() and (l.view(np.uint32) == ref.NAN_WORD).all()


@pytest.mark.parametrize("H,W,B", [(H, W, B) for H, W in SCALAR + VECTOR for B in BS])
def test_batches_against_the_restatement(hip, H, W, B):
    for edge in (D4, D8):
        graph, stop, scales, want = _stack(H, W, B, edge)
        _same_words(_batch(graph, edge, scales, stop), want, "%dx%d x %d edge %d, own scales" % (H, W, B, edge))
    one = _batch(graph, D8, SCALES[1])                            # one pair, no stop plane
    for b in (0, B - 1):
        _same_words([o[b] for o in one], ref.walk_doubling(graph[b], D8, SCALES[1]), "one pair, model %d" % b)


def test_more_models_than_a_launch_takes(hip):
    """B = 65537 at (1, 4): two chunks (65535 models to a launch).  Every model against the restatement of the
    different rows there are."""
    B, H, W = 65537, 1, 4
    r = np.random.default_rng(8)
    rows = np.array([[1, 2, 3, -1], [-1, 0, 1, 2], [1, 0, 3, 2], [3, 2, 1, 0], [4, 5, 6, 7], [1, 2, 1, 2],
                     [-1, -1, -1, -1], [1, 2, 3, ref.INT32_MAX]], np.int32)
    stops = np.array([[0, 0, 0, 0], [0, 0, 1, 0], [1, 1, 1, 1]], np.int32)
    gi, si, ci = r.integers(0, len(rows), B), r.integers(0, len(stops), B), np.arange(B) % 3
    graph, stop = rows[gi].reshape(B, H, W), stops[si].reshape(B, H, W)
    scales = [SCALES[c] for c in ci]
    got = _batch(graph, D8, scales, stop)
    table = {(g, s, c): ref.walk_serial(rows[g].reshape(H, W), D8, SCALES[c], stops[s].reshape(H, W))
             for g in range(len(rows)) for s in range(len(stops)) for c in range(3)}
    want = tuple(np.stack([table[g, s, c][i] for g, s, c in zip(gi, si, ci)]) for i in range(3))
    _same_words(got, want, "65537 models")
    assert _info() == dict(chunks=2, vec_chunks=2, idx64_chunks=0, rounds=2)
    assert (got[0][[0, 65534, 65535, 65536]] < H * W).all(), "a terminal is an index within its model"


@pytest.mark.parametrize("H,W", [(37, 53), (33, 260), (256, 256)])
@pytest.mark.parametrize("plateaus", [False, True])
def test_the_librarys_own_graphs(hip, H, W, plateaus):
    """`steepest` and `random_weighted` graphs of a random terrain and of one with plateaus."""
    from soillib_amd import soil
    h = to_gpu(ref.terrain(H, W, 5, plateaus) * np.float32(10.0))
    for edge in (D4, D8):
        for graph in (soil.steepest(h, edge), soil.random_weighted(h, edge, 11, 3, 10.0)):
            got = _np3(soil.flow_paths(graph, edge, (0.25, 3.0)))
            g = to_np(graph)
            _same_words(got, ref.walk_doubling(g, edge, (0.25, 3.0)), "%dx%d edge %d" % (H, W, edge))
            assert (got[0] >= 0).all() and (g.reshape(-1)[got[0].reshape(-1)] == -1).all()


# ------------------------------------------------------------------ outputs

def test_every_subset_of_the_outputs(hip):
    from soillib_amd import _abi, silt
    H, W, B = 33, 260, 3
    graph, stop, scales, want = _stack(H, W, B, D8)
    gg, gs = to_gpu(graph), to_gpu(stop)
    pairs = (C.c_float * (2 * B))(*[v for s in scales for v in s])
    dts = (silt.int32, silt.int32, silt.float32)
    for ask in itertools.product((False, True), repeat=3):
        if not any(ask):
            continue
        outs = [silt.tensor(dt, silt.shape(B, H, W), silt.gpu) if a else None for a, dt in zip(ask, dts)]
        _abi.check(hip.soil_flow_paths_batch(*[o.c_ptr if o is not None else None for o in outs], gg.c_ptr, gs.c_ptr,
                                             B, H, W, D8, pairs if ask[2] else None, B if ask[2] else 1, _abi.stream()))
        _same_words(_np3(outs), [w if a else None for a, w in zip(ask, want)], "batch, outputs %r" % (ask,))
        b = 1                                                    # the single grid on model 1's slices
        outs = [silt.tensor(dt, silt.shape(H, W), silt.gpu) if a else None for a, dt in zip(ask, dts)]
        one = (C.c_float * 2)(*scales[b])
        _abi.check(hip.soil_flow_paths(*[o.c_ptr if o is not None else None for o in outs],
                                       C.c_void_p(gg.ptr + 4 * b * H * W), C.c_void_p(gs.ptr + 4 * b * H * W), H, W, D8,
                                       one if ask[2] else None, _abi.stream()))
        _same_words(_np3(outs), [w[b] if a else None for a, w in zip(ask, want)], "single, outputs %r" % (ask,))


def test_the_thin_forms(hip):
    from soillib_amd import soil
    H, W, B = 37, 53, 3
    graph, stop, scales, want = _stack(H, W, B, D8)
    gg, gs = to_gpu(graph), to_gpu(stop)
    assert (to_np(soil.basins_batch(gg, D8, gs)) == want[0]).all()
    _same_words((None, None, to_np(soil.flow_length_batch(gg, D8, scales, gs))), (None, None, want[2]), "flow_length_batch")
    g1, s1 = to_gpu(graph[1]), to_gpu(stop[1])
    assert (to_np(soil.basins(g1, D8, s1)) == want[0][1]).all()
    _same_words((None, None, to_np(soil.flow_length(g1, D8, scales[1], s1))), (None, None, want[2][1]), "flow_length")
    t, s, l = soil.flow_paths(g1, D8)
    assert l is None and (to_np(s) == ref.walk_doubling(graph[1], D8)[1]).all()


def test_watershed_with_two_nested_pour_points(hip):
    from soillib_amd import soil
    g = to_gpu(np.array([[1, 2, 3, 4, 5, 6, 7, -1]], np.int32))   # a chain 0 -> ... -> 7
    assert to_np(soil.watershed(g, D8, [(0, 5)])).tolist() == [[1, 1, 1, 1, 1, 1, 0, 0]]
    assert to_np(soil.watershed(g, D8, [(0, 2), (0, 5)])).tolist() == [[1, 1, 1, 1, 1, 1, 0, 0]]   # nested: the union
    assert to_np(soil.watershed(g, D8, [(0, 7)])).tolist() == [[1] * 8]
    # the inner gauge alone catches its own part; what stops at the outer one is the difference
    inner = to_np(soil.watershed(g, D8, [(0, 2)]))
    assert inner.tolist() == [[1, 1, 1, 0, 0, 0, 0, 0]] and inner.dtype == np.int32
    stop = np.array([[0, 0, 1, 0, 0, 1, 0, 0]], np.int32)
    assert to_np(soil.basins(g, D8, to_gpu(stop))).tolist() == [[2, 2, 2, 5, 5, 5, 7, 7]]
    # on a serpentine with a cycle elsewhere: cells that never arrive are outside
    H, W = 6, 7
    c = ref.cycles(H, W)
    mask = to_np(soil.watershed(to_gpu(c), D8, [(2, 3)]))
    want = np.zeros((H, W), np.int32)
    want[2, 3:] = 1
    assert (mask == want).all()


# ------------------------------------------------------------------ plumbing

def test_planes_off_their_16_bytes(hip):
    """Every plane 4 bytes past a 16-byte boundary, W % 4 == 0: the scalar form takes the call and gives what the
    16-byte form gives."""
    from soillib_amd import _abi, silt
    H, W, B = 33, 260, 3
    graph, stop, scales, want = _stack(H, W, B, D4)

    def shifted(arr, dtype):
        buf = silt.tensor(dtype, silt.shape(B * H * W + 4), silt.gpu)
        assert buf.ptr % 16 == 0
        view = silt.tensor.from_device(buf.ptr + 4, dtype, silt.shape(B, H, W), keepalive=buf)
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            _abi.check(hip.soil_memcpy_h2d(view.c_ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, _abi.stream()))
            _abi.check(hip.soil_stream_synchronize(_abi.stream()))
        return view

    pairs = (C.c_float * (2 * B))(*[v for s in scales for v in s])
    gg, gs = shifted(graph, silt.int32), shifted(stop, silt.int32)
    outs = [shifted(None, silt.int32), shifted(None, silt.int32), shifted(None, silt.float32)]
    _abi.check(hip.soil_flow_paths_batch(*[o.c_ptr for o in outs], gg.c_ptr, gs.c_ptr, B, H, W, D4, pairs, B, _abi.stream()))
    _same_words(_np3(outs), want, "planes off their 16 bytes")
    assert _info()["chunks"] == 1 and _info()["vec_chunks"] == 0, "the scalar form takes planes off their 16 bytes"
    # only the stop plane off: the scalar form as well
    al = to_gpu(graph)
    _abi.check(hip.soil_flow_paths_batch(*[o.c_ptr for o in outs], al.c_ptr, gs.c_ptr, B, H, W, D4, pairs, B, _abi.stream()))
    _same_words(_np3(outs), want, "the stop plane off its 16 bytes")
    assert _info()["vec_chunks"] == 0
    _abi.check(hip.soil_flow_paths_batch(*[o.c_ptr for o in outs], al.c_ptr, to_gpu(stop).c_ptr, B, H, W, D4, pairs, B, _abi.stream()))
    _same_words(_np3(outs), want, "aligned inputs, outputs off their 16 bytes")
    assert _info()["vec_chunks"] == 1, "aligned inputs take the 16-byte form"


def test_on_another_stream_twice_and_with_another_size_in_between(hip):
    import torch
    from soillib_amd import _abi
    small, large = _stack(37, 53, 7, D8), _stack(33, 260, 64, D8)
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        for graph, stop, scales, want in (small, large, small, small, large):
            got = _batch(graph, D8, scales, stop)
            _same_words(got, want, "on a second stream")
        a = _single(small[0][2], D8, (1.0, 1.0))                  # the single entry through the same scratch
        _same_words(a, ref.walk_doubling(small[0][2], D8, (1.0, 1.0)), "single, second stream")
    finally:
        _abi.set_stream(0)


CHUNK_SHAPES = [(37, 53), (33, 260)]


def _child_main(path):
    """The child of test_chunks: B = 5 as chunks of 2 + 2 + 1 models and as five chunks of one."""
    out = {}
    for H, W in CHUNK_SHAPES:
        for models in (2, 1):
            os.environ["SOIL_FLOW_BATCH_CELLS"] = str(models * H * W + (H * W // 2 if models == 2 else 0))
            for edge in (D4, D8):
                graph, stop, scales, _ = _stack(H, W, 5, edge)
                for name, plane in zip(NAMES, _batch(graph, edge, scales, stop)):
                    out["%dx%d_m%d_e%d_%s" % (H, W, models, edge, name)] = plane
                i = _info()
                out["%dx%d_m%d_e%d_info" % (H, W, models, edge)] = np.array([i["chunks"], i["vec_chunks"], i["idx64_chunks"]])
    _child_optional()
    np.savez(path, **out)


# (H, W, SOIL_FLOW_BATCH_CELLS): B = 5 as 2 + 2 + 1 models, the 16-byte init and the scalar one
OPTIONAL_SHAPES = [(8, 12, 192), (8, 10, 160)]
OPTIONAL_ASKS = [((True, True, True), True), ((True, False, False), False), ((False, True, False), True),
                 ((False, False, True), False)]                  # (terminal, steps, length), the stop plane


def _child_optional():
    """The stop plane and each output given and NULL over three chunks: from the second chunk on a plane is the
    chunk's part of it, and one that is not given must stay not given.  The words of the five single-grid calls;
    raises."""
    from soillib_amd import _abi, silt
    lib = _abi.lib()
    dts = (silt.int32, silt.int32, silt.float32)
    ptr = lambda t: None if t is None else t.c_ptr
    for H, W, cells in OPTIONAL_SHAPES:
        graph, stop, scales, _ = _stack(H, W, 5, D8)
        for ask, with_stop in OPTIONAL_ASKS:
            gg, gs = to_gpu(graph), to_gpu(stop) if with_stop else None
            pairs = (C.c_float * 10)(*[v for s in scales for v in s]) if ask[2] else None
            outs = [silt.tensor(dt, silt.shape(5, H, W), silt.gpu) if a else None for a, dt in zip(ask, dts)]
            os.environ["SOIL_FLOW_BATCH_CELLS"] = str(cells)
            _abi.check(lib.soil_flow_paths_batch(*[ptr(o) for o in outs], gg.c_ptr, ptr(gs), 5, H, W, D8, pairs,
                                                 5 if ask[2] else 1, _abi.stream()))
            i = _info()
            assert (i["chunks"], i["vec_chunks"]) == (3, 3 if W % 4 == 0 else 0), (H, W, ask, with_stop, i)
            del os.environ["SOIL_FLOW_BATCH_CELLS"]
            got = _np3(outs)
            for b in range(5):
                one = _single(graph[b], D8, scales[b], stop[b] if with_stop else None)
                _same_words([None if g is None else g[b] for g in got], [w if a else None for a, w in zip(ask, one)],
                            "%dx%d outputs %r, stop %r, model %d" % (H, W, ask, with_stop, b))


@pytest.mark.parametrize("list_from", [None, "0", "1", "idx64"])
def test_chunks(hip, tmp_path, list_from):
    """Chunks of 2 + 2 + 1 models and of one model (SOIL_FLOW_BATCH_CELLS) in a child process, by default and with the
    listed rounds off (SOIL_PATHS_LIST_FROM = 0) and forced on from round 1: the restatement's results, whatever the
    chunking.  (Later first rounds: test_the_rounds_in_this_process_with_the_lists_off_and_late.)  "idx64": the
    same under SOIL_PATHS_IDX64 = 1, the 64-bit offsets of a model of 2^28 cells or more.  The child reports what each
    call did (soil_flow_paths_info): 3 and 5 chunks, the 16-byte form at (33, 260) alone, the offsets asked for.  The
    child also holds the stop plane and each output, given and NULL over three chunks, to the single-grid calls
    (_child_optional)."""
    path = str(tmp_path / "chunks.npz")
    env = dict(os.environ)
    env.pop("SOIL_FLOW_BATCH_CELLS", None)
    env.pop("SOIL_PATHS_LIST_FROM", None)
    env.pop("SOIL_PATHS_IDX64", None)
    if list_from == "idx64":
        env["SOIL_PATHS_IDX64"] = "1"
    elif list_from is not None:
        env["SOIL_PATHS_LIST_FROM"] = list_from
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    seen = 0
    for H, W in CHUNK_SHAPES:
        for edge in (D4, D8):
            want = _stack(H, W, 5, edge)[3]
            for models in (2, 1):
                planes = [got["%dx%d_m%d_e%d_%s" % (H, W, models, edge, name)] for name in NAMES]
                _same_words(planes, want, "%dx%d edge %d in chunks of %d, SOIL_PATHS_LIST_FROM %s" % (H, W, edge, models, list_from))
                seen += 4
                chunks = 3 if models == 2 else 5
                assert got["%dx%d_m%d_e%d_info" % (H, W, models, edge)].tolist() == [
                    chunks, chunks if W % 4 == 0 else 0, chunks if list_from == "idx64" else 0]
    assert seen == len(got.files)


def test_the_rounds_in_this_process_with_the_lists_off_and_late(hip, monkeypatch):
    """SOIL_PATHS_LIST_FROM is read per call: dense rounds throughout, and the lists from a late round, on the chain
    that needs every round and on cycles."""
    for H, W in ((32, 32), (33, 260)):
        for name in ("serpentine", "cycles", "hostile"):
            g = _graphs(H, W, D8)[name]
            want = _want(H, W, D8, name, "none", SCALES[1])
            for v in ("0", "1", "3", "9", "99"):
                monkeypatch.setenv("SOIL_PATHS_LIST_FROM", v)
                for idx64 in ("0", "1"):
                    monkeypatch.setenv("SOIL_PATHS_IDX64", idx64)
                    _same_words(_single(g, D8, SCALES[1]), want, "%s %dx%d, lists from %s, idx64 %s" % (name, H, W, v, idx64))
                    assert _info() == dict(chunks=1, vec_chunks=int(W % 4 == 0), idx64_chunks=int(idx64), rounds=len(bin(H * W - 1)) - 2)


# ------------------------------------------------------------------ isolation

def test_a_model_is_unchanged_when_the_others_are_replaced(hip):
    H, W, B = 33, 260, 5
    graph, stop, scales, want = _stack(H, W, B, D8)
    r = np.random.default_rng(4)
    for keep in (0, 2, 4):
        g2 = np.stack([ref.hostile(H, W, 50 + b, model=keep) for b in range(B)])
        # entries of the other models point into `keep` in the stacked numbering: no edges
        g2[(keep + 1) % B] = np.arange(H * W, dtype=np.int64).reshape(H, W) % (H * W) + (keep - (keep + 1) % B) * H * W
        s2 = (r.random((B, H, W)) < 0.1).astype(np.int32)
        sc2 = [SCALES[(b + 1) % 3] for b in range(B)]
        g2[keep], s2[keep], sc2[keep] = graph[keep], stop[keep], scales[keep]
        got = _batch(g2, D8, sc2, s2)
        _same_words([o[keep] for o in got], [w[keep] for w in want], "model %d among replaced ones" % keep)
        for b in range(B):
            assert got[0][b].max() < H * W and got[0][b].min() >= -1


def test_an_index_of_the_neighbouring_models_numbering_is_no_edge(hip):
    H, W, B = 9, 1028, 3
    g = np.stack([ref.serpentine(H, W)] * B).astype(np.int64)
    stacked = g.copy()
    stacked[1] = np.where(g[1] >= 0, g[1] + H * W, -1)            # model 1 in the stacked numbering: drains nowhere
    stacked[0, -1, :] = H * W + np.arange(W)                      # "the cell below", were the models one grid
    stacked[2, 0, :] = np.arange(W) - W                           # "the cell above": negative
    t, s, _ = _batch(stacked.astype(np.int32), D8)
    own = np.arange(H * W, dtype=np.int32).reshape(H, W)
    assert (t[1] == own).all() and (s[1] == 0).all()
    for b in (0, 2):
        wt, ws, _ = ref.walk_doubling(stacked[b].astype(np.int32), D8)
        assert (t[b] == wt).all() and (s[b] == ws).all()


# ------------------------------------------------------------------ against the single-grid device call

def _device_graphs(B, H, W, edge):
    from soillib_amd import silt, soil
    h = silt.tensor(silt.float32, silt.shape(B, H, W), silt.gpu)
    for b in range(B):
        p = soil.noise_t()
        p.seed = float(5 + b)
        p.ext = [H, W]
        one = soil.noise(silt.shape(H, W), p, host=silt.gpu)
        silt.multiply(one, 100.0)
        per = h.nbytes() // B
        from soillib_amd import _abi
        _abi.check(_abi.lib().soil_memcpy_d2d(C.c_void_p(h.ptr + b * per), one.c_ptr, per, _abi.stream()))
    return soil.steepest_batch(h, edge), soil.random_weighted_batch(h, edge, [3 + b for b in range(B)], 1, 10.0)


def _model(t, b):
    from soillib_amd import silt
    per = t.nbytes() // t.shape[0]
    return silt.tensor.from_device(t.ptr + b * per, t.type, silt.shape(*tuple(t.shape)[1:]), keepalive=t)


@pytest.mark.parametrize("H,W,B", [(256, 256, 8), (1024, 1024, 2)])
def test_the_batch_entry_against_the_single_grid_call(hip, H, W, B):
    from soillib_amd import soil
    scales = [(1.0 + b, 2.0 + 0.5 * b) for b in range(B)]
    r = np.random.default_rng(H)
    stop = to_gpu((r.random((B, H, W)) < 0.001).astype(np.int32))
    for edge in (D4, D8):
        for graph in _device_graphs(B, H, W, edge):
            for st in (None, stop):
                got = _np3(soil.flow_paths_batch(graph, edge, scales, st))
                for b in range(B):
                    one = _np3(soil.flow_paths(_model(graph, b), edge, scales[b], None if st is None else _model(st, b)))
                    _same_words([o[b] for o in got], one, "model %d of %d at %dx%d, edge %d" % (b, B, H, W, edge))
        assert (got[0] >= 0).all(), "a downhill graph has no cycle"
    # and one model against the restatement
    _same_words(one, ref.walk_doubling(to_np(_model(graph, B - 1)), D8, scales[B - 1], to_np(_model(stop, B - 1))),
                "the last model against the restatement")


def test_basin_sizes_are_what_accumulate_counts(hip):
    """On acyclic `steepest` graphs at 256^2 without a stop plane, the number of cells with terminal == t is
    accumulate(graph, ones)[t], exactly, for every terminal t (counts far below 2^24): the edge rule is the donor
    pass's."""
    from soillib_amd import soil
    H = W = 256
    ones = to_gpu(np.ones((H, W), np.float32))
    for seed, plateaus in ((1, False), (2, True)):
        h = to_gpu(ref.terrain(H, W, seed, plateaus) * np.float32(20.0))
        for edge in (D4, D8):
            graph = soil.steepest(h, edge)
            t = to_np(soil.basins(graph, edge)).reshape(-1)
            acc = to_np(soil.accumulate(graph, ones, edge)).reshape(-1)
            assert (t >= 0).all()
            sizes = np.bincount(t, minlength=H * W)
            terminals = np.flatnonzero(to_np(graph).reshape(-1) == -1)
            assert (np.flatnonzero(sizes) == terminals).all()
            assert sizes.max() < 2 ** 24 and (sizes[terminals] == acc[terminals].astype(np.int64)).all()
            assert (acc[terminals] == np.floor(acc[terminals])).all()


# ------------------------------------------------------------------ after real steps

def test_basins_and_flow_length_of_stepped_models(hip, oracle):
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    B, H, W = 3, 128, 128
    p = product_param(script_param(oracle.default_param()))
    p.maxage = 64
    scales = [(20.0 / H * (1 + b), 20.0 / W, 4.0) for b in range(B)]
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    for scale in ((20.0 / H, 20.0 / W, 4.0), scales):
        bt = ErosionBatch(B, H, W, scale, p, 1024, [11 + 7 * b for b in range(B)])
        bt.set_layers(to_gpu(layers))
        silt.set(bt.rainfall, 1.0)
        for _ in range(2):
            bt.step()
        basins, length = to_np(bt.basins()), to_np(bt.flow_length())
        stop = to_gpu((np.random.default_rng(3).random((B, H, W)) < 0.01).astype(np.int32))
        d4 = bt.flow(edge=D4)
        basins_d4, length_d4 = to_np(bt.basins(graph=d4, stop=stop)), to_np(bt.flow_length(graph=d4, stop=stop))
        own_d4, own_length_d4 = to_np(bt.basins(edge=D4)), to_np(bt.flow_length(stop=stop, edge=D4))
        for b, m in enumerate(bt.to_models()):
            s2 = (scale if scale is not scales else scales[b])[:2]
            t, _, l = _np3(soil.flow_paths(soil.steepest(m.height, D8), D8, s2))
            _same_words((basins[b], None, length[b]), (t, None, l), "model %d" % b)
            t, _, l = _np3(soil.flow_paths(soil.steepest(m.height, D4), D8, s2, _model(stop, b)))
            _same_words((basins_d4[b], None, length_d4[b]), (t, None, l), "model %d, d4 graph and pour points" % b)
            t4 = to_np(soil.basins(soil.steepest(m.height, D4), D4))
            l4 = to_np(soil.flow_length(soil.steepest(m.height, D4), D4, s2, _model(stop, b)))
            _same_words((own_d4[b], None, own_length_d4[b]), (t4, None, l4), "model %d, edge=d4" % b)
            host = ref.walk_doubling(to_np(soil.steepest(m.height, D8)), D8, s2)
            _same_words((basins[b], None, length[b]), (host[0], None, host[2]), "model %d against the restatement" % b)


# ------------------------------------------------------------------ refusals

def test_refusals_leave_the_planes_untouched(hip):
    from soillib_amd import _abi
    B, H, W = 2, 5, 8
    mark_f, mark_i = np.float32(-7.5), np.int32(-77)
    t, s = (to_gpu(np.full((B, H, W), mark_i, np.int32)) for _ in range(2))
    l = to_gpu(np.full((B, H, W), mark_f, np.float32))
    g = to_gpu(np.full((B, H, W), -1, np.int32))
    sc = (C.c_float * (2 * B))(1, 1, 1, 1)
    st = _abi.stream()
    big = 1 << 16
    one, many = hip.soil_flow_paths, hip.soil_flow_paths_batch

    def refused(name, rc):
        assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, name
        assert _abi.last_error().startswith(name + ": "), (name, _abi.last_error())

    refused("flow_paths", one(t.c_ptr, s.c_ptr, l.c_ptr, None, None, H, W, D8, sc, st))
    refused("flow_paths", one(None, None, None, g.c_ptr, None, H, W, D8, sc, st))
    refused("flow_paths", one(t.c_ptr, s.c_ptr, l.c_ptr, g.c_ptr, None, H, W, D8, None, st))
    for h, w in ((0, W), (H, 0), (-1, W), (big, big)):
        refused("flow_paths", one(t.c_ptr, s.c_ptr, l.c_ptr, g.c_ptr, None, h, w, D8, sc, st))
    for e in (2, -1, 8):
        refused("flow_paths", one(t.c_ptr, s.c_ptr, l.c_ptr, g.c_ptr, None, H, W, e, sc, st))
    refused("flow_paths_batch", many(t.c_ptr, s.c_ptr, l.c_ptr, None, None, B, H, W, D8, sc, B, st))
    refused("flow_paths_batch", many(None, None, None, g.c_ptr, None, B, H, W, D8, sc, B, st))
    refused("flow_paths_batch", many(t.c_ptr, s.c_ptr, l.c_ptr, g.c_ptr, None, B, H, W, D8, None, 1, st))
    for b, h, w in ((0, H, W), (-1, H, W), (B, 0, W), (B, H, 0), (B, H, -3), (B, big, big)):
        refused("flow_paths_batch", many(t.c_ptr, s.c_ptr, l.c_ptr, g.c_ptr, None, b, h, w, D8, sc, 1, st))
    for n in (0, B + 1, -1, 3):
        refused("flow_paths_batch", many(t.c_ptr, s.c_ptr, l.c_ptr, g.c_ptr, None, B, H, W, D8, sc, n, st))
    for e in (2, -1):
        refused("flow_paths_batch", many(t.c_ptr, s.c_ptr, l.c_ptr, g.c_ptr, None, B, H, W, e, sc, B, st))
    _abi.check(hip.soil_stream_synchronize(st))
    assert (to_np(t) == mark_i).all() and (to_np(s) == mark_i).all() and (to_np(l) == mark_f).all()


if __name__ == "__main__":
    _child_main(sys.argv[1])
