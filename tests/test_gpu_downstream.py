"""Downstream sums and the implicit stream-power step on the device (include/soil_hip.h: soil_downstream,
soil_stream_power and their _batch forms; soillib_amd.soil.downstream / stream_power / chi / erosivity,
ErosionBatch.downstream / stream_power), bit for bit against solve_doubling of tests/downstream_ref.py: every
comparison with it is of float32 and float64 bit patterns, the NaN words included; there is no tolerance in them.

  shapes        the scalar form (1, 1), (1, 5), (5, 1), (2, 2), (37, 53); the 16-byte form (3, 4), (33, 260),
                (9, 1028), (256, 256); B in {1, 2, 3, 7, 64}; B = 65537 at (1, 4): more models than a launch takes;
                a chain through every cell at H W = 2^k - 1, 2^k, 2^k + 1: every round is needed
  graphs        every built graph of flow_paths_ref (hostile entries, cycles next to parts that resolve) and numpy's
                downhill graphs; per model another graph, stop plane, scale pair and coefficient draw
  inputs        every subset of a, b, t, stop, scale NULL; both outputs and each alone
  coefficients  signed draws whose results are finite — each case asserts that its reference holds NaN only where the
                graph leaves a cell unresolved —, and hostile ones: +-0, float32 denormals, +-3e38, b > 1 along a
                chain until it overflows, one +inf, one -inf and one NaN cell: NaN only upstream of those, as the
                restatement spreads them
  plumbing      planes 4 bytes off their alignment, a second stream, repeated calls, chunks, the lists off and late
                and 64-bit offsets in child processes, refusals that leave the outputs untouched
  isolation     a hostile model between two benign ones
  single grid   the batch entries against the single calls at 256^2 x 8
  stream power  on condition()ed bench terrains at 96^2 and 256^2, D4 and D8: the restatement's bits, within 1 float32
                ulp of the serial solver, monotone along every edge, terminals unchanged, dt = 0 the heights,
                ErosionBatch.stream_power after real steps, three steps with re-conditioning
"""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import downstream_ref as dref
import flow_paths_ref as ref
from flow_paths_ref import D4, D8
from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR = [(1, 1), (1, 5), (5, 1), (2, 2), (37, 53)]
VECTOR = [(3, 4), (33, 260), (9, 1028), (256, 256)]
BS = [1, 2, 3, 7, 64]
SCALES = [(1.0, 1.0), (0.25, 3.0), (1e-3, 1e3)]
DT = 3.5
MODES = ("sum", "sum_no_b", "power")


_same_words = dref.same_words             # (shared with tests/test_gpu_cpp_ops.py)


def _info():
    from soillib_amd import soil
    return soil.downstream_info()


def _ptr(t):
    return None if t is None else t.c_ptr


def _run(graph, edge, a=None, b=None, t=None, scale=None, stop=None, power=None, outs=(True, True)):
    """One call of the C ABI on numpy planes, (H, W) or (B, H, W) by the graph's rank: (out, out64) as numpy, None
    for an output not asked for.  `scale`: None, one pair or B pairs.  `power`: (height, erosivity, uplift, dt)."""
    from soillib_amd import _abi, silt
    lib = _abi.lib()
    graph = np.asarray(graph)
    shape = graph.shape
    dev = lambda p: None if p is None else to_gpu(np.ascontiguousarray(p))
    gg, gs = dev(graph), dev(stop)
    o32 = silt.tensor(silt.float32, silt.shape(*shape), silt.gpu) if outs[0] else None
    o64 = silt.tensor(silt.float64, silt.shape(*shape), silt.gpu) if outs[1] else None
    pairs = None if scale is None else np.asarray(scale, np.float32).reshape(-1)
    sc = None if pairs is None else (C.c_float * len(pairs))(*pairs.tolist())
    tail = (sc,) if len(shape) == 2 else (sc, 1 if pairs is None else len(pairs) // 2)
    if power is None:
        planes = [dev(a), dev(b), dev(t)]
        fn = lib.soil_downstream if len(shape) == 2 else lib.soil_downstream_batch
        rc = fn(_ptr(o32), _ptr(o64), gg.c_ptr, *[_ptr(p) for p in planes], _ptr(gs), *shape, edge, *tail, _abi.stream())
    else:
        planes = [dev(power[0]), dev(power[1]), dev(power[2])]
        fn = lib.soil_stream_power if len(shape) == 2 else lib.soil_stream_power_batch
        rc = fn(_ptr(o32), _ptr(o64), _ptr(planes[0]), gg.c_ptr, _ptr(planes[1]), _ptr(planes[2]), _ptr(gs), *shape, edge,
                *tail, float(power[3]), _abi.stream())
    _abi.check(rc)
    return (None if o32 is None else to_np(o32), None if o64 is None else to_np(o64))


# ------------------------------------------------------------------ inputs and references, made once

@functools.lru_cache(maxsize=None)
def _graphs(H, W, edge):
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
def _coeffs(H, W, draw):
    """a, b in [-1, 1] and t in [-10, 10], signed; a height in [0, 100], an erosivity over 1e-6 .. 1e3 and an uplift
    in [0, 0.01].  |b| <= 1: every result is finite."""
    r = np.random.default_rng([draw, H, W])
    a, b = (r.uniform(-1.0, 1.0, (H, W)).astype(np.float32) for _ in range(2))
    t = r.uniform(-10.0, 10.0, (H, W)).astype(np.float32)
    height = (r.random((H, W)) * 100.0).astype(np.float32)
    erosivity = np.exp(r.uniform(np.log(1e-6), np.log(1e3), (H, W))).astype(np.float32)
    uplift = (r.random((H, W)) * 0.01).astype(np.float32)
    out = dict(a=a, b=b, t=t, height=height, erosivity=erosivity, uplift=uplift)
    for p in out.values():
        p.setflags(write=False)
    return out


def _solve(solve, graph, edge, c, mode, scale, stop):
    if mode == "power":
        return solve(graph, edge, scale=scale, stop=stop, power=(c["height"], c["erosivity"], c["uplift"], DT))
    return solve(graph, edge, c["a"], c["b"] if mode == "sum" else None, c["t"], scale, stop)


@functools.lru_cache(maxsize=None)
def _want(H, W, edge, gname, sname, scale, draw, mode):
    """The reference of one model, made once and left as it is; its NaN words are the unresolved cells, no others."""
    out = _solve(dref.solve_doubling, _graphs(H, W, edge)[gname], edge, _coeffs(H, W, draw), mode, scale, _stops(H, W)[sname])
    assert (np.isnan(out[1]) == ~out[2]).all() and (np.isnan(out[0]) == ~out[2]).all(), "a draw made a NaN of its own"
    for o in out:
        o.setflags(write=False)
    return out


def _models(H, W, B, edge):
    """(graph name, stop name, scale, draw) of each of B models: neighbours differ in all four."""
    gn, sn = sorted(_graphs(H, W, edge)), sorted(_stops(H, W))
    return [(gn[b % len(gn)], sn[(b // 2) % len(sn)], SCALES[b % 3], b % 2) for b in range(B)]


def _stack(H, W, B, edge, mode):
    """graph, stop, scales, the float planes (a dict) and the reference (out, out64) of B models."""
    cfg = _models(H, W, B, edge)
    graph = np.stack([_graphs(H, W, edge)[g] for g, _, _, _ in cfg])
    stop = np.stack([np.zeros((H, W), np.int32) if _stops(H, W)[s] is None else _stops(H, W)[s] for _, s, _, _ in cfg])
    planes = {k: np.stack([_coeffs(H, W, d)[k] for _, _, _, d in cfg]) for k in _coeffs(H, W, 0)}
    want = [_want(H, W, edge, *c, mode) for c in cfg]
    return graph, stop, [c[2] for c in cfg], planes, tuple(np.stack([w[i] for w in want]) for i in range(2))


def _run_mode(graph, edge, planes, mode, scale, stop, outs=(True, True)):
    if mode == "power":
        return _run(graph, edge, scale=scale, stop=stop, power=(planes["height"], planes["erosivity"], planes["uplift"], DT), outs=outs)
    return _run(graph, edge, planes["a"], planes["b"] if mode == "sum" else None, planes["t"], scale, stop, outs=outs)


# ------------------------------------------------------------------ against the restatement

@pytest.mark.parametrize("H,W", SCALAR + VECTOR)
@pytest.mark.parametrize("edge", [D4, D8])
def test_single_grid_against_the_restatement(hip, H, W, edge):
    """Every graph under every stop plane (at 256^2: every graph without one, and the cycles and a hostile graph under
    each), the mode and the draw changing from case to case."""
    k = 0
    for gname in sorted(_graphs(H, W, edge)):
        for i, sname in enumerate(sorted(_stops(H, W))):
            if H * W > 10000 and sname != "none" and gname not in ("cycles", "hostile"):
                continue
            for mode in MODES if H * W <= 10000 else (MODES[k % 3],):
                scale, draw = SCALES[(i + k) % 3], k % 2
                c = _coeffs(H, W, draw)
                got = _run_mode(_graphs(H, W, edge)[gname], edge, c, mode, scale, _stops(H, W)[sname])
                _same_words(got, _want(H, W, edge, gname, sname, scale, draw, mode),
                            "%s, stop %s, %s, %dx%d edge %d" % (gname, sname, mode, H, W, edge))
            k += 1
    assert _info()["chunks"] == 1 and _info()["vec_chunks"] == int(W % 4 == 0)


@pytest.mark.parametrize("H,W", [(1, 2), (1, 3), (1, 4), (1, 5), (1, 1023), (1, 1024), (1, 1025), (32, 32), (31, 33),
                                 (3, 341), (341, 3), (1025, 1), (4, 256), (5, 205)])
def test_a_chain_through_every_cell_needs_every_round(hip, H, W):
    """H W - 1 edges from the first cell: resolved by the last of the ceil(log2(H W)) rounds, at H W = 2^k - 1, 2^k and
    2^k + 1 in both init forms; one round short leaves the head of the chain NaN."""
    g = ref.serpentine(H, W)
    c = _coeffs(H, W, 3)
    for b in (c["b"], None):
        want = dref.solve_doubling(g, D4, c["a"], b, c["t"], (0.25, 3.0))
        assert want[2].all() and not np.isnan(want[1]).any()
        _same_words(_run(g, D4, c["a"], b, c["t"], (0.25, 3.0)), want, "serpentine %dx%d" % (H, W))
        assert _info()["rounds"] == len(bin(H * W - 1)) - 2
    steps = _run(g, D4)[0]
    assert steps[0, 0] == H * W - 1
    # the same chain with a cycle at its end: nothing resolves, and the rounds still end
    g = g.copy()
    last = int(np.flatnonzero(g.reshape(-1) == -1)[0])
    g.reshape(-1)[last] = int(np.flatnonzero(g.reshape(-1) == last)[0])
    out, out64 = _run(g, D4, c["a"], c["b"], c["t"])
    assert (dref.words(out) == dref.NAN32).all() and (dref.words(out64) == dref.NAN64).all()


@pytest.mark.parametrize("H,W,B", [(H, W, B) for H, W in SCALAR + VECTOR for B in BS])
def test_batches_against_the_restatement(hip, H, W, B):
    for edge, mode in ((D4, "sum"), (D8, "sum_no_b"), (D8, "power"), (D4, "power"), (D8, "sum")):
        if H * W > 10000 and B > 7 and (edge, mode) not in ((D8, "sum"), (D4, "power")):
            continue
        graph, stop, scales, planes, want = _stack(H, W, B, edge, mode)
        _same_words(_run_mode(graph, edge, planes, mode, scales, stop), want, "%dx%d x %d edge %d %s, own scales" % (H, W, B, edge, mode))
    one = _run_mode(graph, D8, planes, "sum", SCALES[1], None)      # one pair, no stop plane
    for b in (0, B - 1):
        c = {k: v[b] for k, v in planes.items()}
        _same_words([o[b] for o in one], _solve(dref.solve_doubling, graph[b], D8, c, "sum", SCALES[1], None), "one pair, model %d" % b)


def test_more_models_than_a_launch_takes(hip):
    """B = 65537 at (1, 4): two chunks (65535 models to a launch).  Every model against the restatement of the
    different rows there are."""
    B, H, W = 65537, 1, 4
    r = np.random.default_rng(8)
    rows = np.array([[1, 2, 3, -1], [-1, 0, 1, 2], [1, 0, 3, 2], [3, 2, 1, 0], [4, 5, 6, 7], [1, 2, 1, 2],
                     [-1, -1, -1, -1], [1, 2, 3, ref.INT32_MAX]], np.int32)
    stops = np.array([[0, 0, 0, 0], [0, 0, 1, 0], [1, 1, 1, 1]], np.int32)
    draws = r.uniform(-1.0, 1.0, (4, 3, 4)).astype(np.float32)                       # a, b, t of four draws
    gi, si, di, ci = r.integers(0, len(rows), B), r.integers(0, len(stops), B), r.integers(0, 4, B), np.arange(B) % 3
    graph, stop = rows[gi].reshape(B, H, W), stops[si].reshape(B, H, W)
    a, b, t = (draws[di, k].reshape(B, H, W) for k in range(3))
    got = _run(graph, D8, a, b, t, [SCALES[c] for c in ci], stop)
    table = [dref.solve_doubling(rows[g].reshape(H, W), D8, *[draws[d, k].reshape(H, W) for k in range(3)], SCALES[c],
                                 stops[s].reshape(H, W))
             for g in range(len(rows)) for s in range(len(stops)) for d in range(4) for c in range(3)]
    assert all((np.isnan(v[1]) == ~v[2]).all() for v in table)
    which = ((gi * len(stops) + si) * 4 + di) * 3 + ci
    want = tuple(np.stack([v[i] for v in table])[which] for i in range(2))
    _same_words(got, want, "65537 models")
    assert _info() == dict(chunks=2, vec_chunks=2, idx64_chunks=0, rounds=2)


# ------------------------------------------------------------------ inputs and outputs

def test_every_subset_of_null_inputs(hip):
    H, W, B = 33, 260, 3
    graph, stop, scales, planes, _ = _stack(H, W, B, D8, "sum")
    for k, (na, nb, nt, ns, nsc) in enumerate(itertools.product((False, True), repeat=5)):
        a, b, t = (None if n else planes[key] for n, key in ((na, "a"), (nb, "b"), (nt, "t")))
        st, sc = None if ns else stop, None if nsc else scales
        outs = ((True, True), (True, False), (False, True))[k % 3]
        want = dref.solve_batch(dref.solve_doubling, graph, D8, a, b, t, sc, st)
        assert (np.isnan(want[1]) == ~want[2]).all()
        got = _run(graph, D8, a, b, t, sc, st, outs=outs)
        assert [g is not None for g in got] == list(outs)
        _same_words(got, want, "batch, null %r, outputs %r" % ((na, nb, nt, ns, nsc), outs))
        m = k % B                                                    # the single grid on model m's slices
        at = lambda p: None if p is None else p[m]
        got = _run(graph[m], D8, at(a), at(b), at(t), None if sc is None else sc[m], at(st), outs=outs)
        _same_words(got, [w[m] for w in want], "single, null %r, outputs %r" % ((na, nb, nt, ns, nsc), outs))
    for outs in ((True, False), (False, True)):                      # the stream-power step, each output alone and no uplift
        pw = (planes["height"], planes["erosivity"], None, DT)
        want = dref.solve_batch(dref.solve_doubling, graph, D8, scale=scales, power=pw)
        _same_words(_run(graph, D8, scale=scales, power=pw, outs=outs), want, "stream power without uplift, outputs %r" % (outs,))


def test_b_null_gives_the_bits_of_b_one(hip):
    H, W = 37, 53
    c = _coeffs(H, W, 1)
    ones = np.ones((H, W), np.float32)
    for gname in ("serpentine", "hostile", "cycles"):
        g = _graphs(H, W, D8)[gname]
        _same_words(_run(g, D8, c["a"], None, c["t"], SCALES[2]), _run(g, D8, c["a"], ones, c["t"], SCALES[2]), gname)


def _hostile_planes(H, W, graph, edge):
    """Coefficients a benign draw never holds, on `graph`, and the plane of cells that may turn NaN: those whose way
    down passes a cell made non-finite on purpose (an inf, a NaN, a run of b = 3e38 that overflows fp64)."""
    N = H * W
    c = _coeffs(H, W, 5)
    a, b, t = (c[k].copy().reshape(-1) for k in ("a", "b", "t"))
    at = lambda k: (k * 7919 + 13) % N
    specials = [0.0, -0.0, 1e-44, -1e-40, 3e38, -3e38]
    for i, v in enumerate(specials):
        a[at(3 * i)], b[at(3 * i + 1)], t[at(3 * i + 2)] = v, v, v
    t[np.flatnonzero(np.arange(N) % 11 == 0)] = 3e38                 # (float)A overflows to inf on many cells: no NaN
    marked = np.zeros(N, np.float32)
    if N >= 64:
        a[N // 4:N // 4 + 2], b[N // 4:N // 4 + 2] = 3e38, 1.0          # 6e38 on a chain: inf as a float, not as a double
        run = np.arange(N // 2, N // 2 + 12)                         # twelve cells in index order: on a chain, a run of it
        b[run], marked[run] = 3e38, 1
        for k, v in ((40, np.inf), (41, -np.inf), (42, np.nan)):
            a[at(k)], marked[at(k)] = v, 1
        t[at(43)], marked[at(43)] = np.inf, 1
    a, b, t, marked = (p.reshape(H, W) for p in (a, b, t, marked))
    # cells upstream of a marked one: the sum of the marks along the way, the terminal's included, is not zero
    reach = dref.solve_doubling(graph, edge, a=marked, t=marked)
    return a.astype(np.float32), b.astype(np.float32), t.astype(np.float32), (reach[1] != 0) | ~reach[2]


@pytest.mark.parametrize("H,W", [(1, 5), (37, 53), (33, 260)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_hostile_coefficients(hip, H, W, edge):
    """+-0, denormals, +-3e38, b = 3e38 along a run of cells until B overflows, +-inf and a NaN: the restatement's
    bits, NaN only where the graph does not resolve or upstream of a cell made non-finite on purpose, and most of
    the grid still finite."""
    seen = dict(inf=False, nan=False, float_overflow=False)
    for gname, graph in sorted(_graphs(H, W, edge).items()):
        a, b, t, may = _hostile_planes(H, W, graph, edge)
        for scale in (None, SCALES[1]):
            want = dref.solve_doubling(graph, edge, a, b, t, scale)
            assert not (np.isnan(want[1]) & ~may).any(), "%s: a NaN outside the cells it was put in" % gname
            if gname not in ("serpentine", "hostile", "hostile2") and H * W >= 64:
                assert np.isfinite(want[1]).mean() > 0.5, gname
            seen["inf"] |= bool(np.isinf(want[1]).any())
            seen["nan"] |= bool((np.isnan(want[1]) & want[2]).any())
            seen["float_overflow"] |= bool((np.isinf(want[0]) & np.isfinite(want[1])).any())
            _same_words(_run(graph, edge, a, b, t, scale), want, "%s %dx%d edge %d" % (gname, H, W, edge))
    if H * W >= 64:
        assert all(seen.values()), seen
        g = _graphs(H, W, edge)["serpentine"]
        den = dref.solve_doubling(g, edge, a=np.full((H, W), 1e-45, np.float32), b=np.full((H, W), 0.5, np.float32))
        tiny = np.abs(den[0][den[0] != 0]).min()
        assert tiny < 2.0 ** -126, "a float32 denormal among the results"
        _same_words(_run(g, edge, a=np.full((H, W), 1e-45, np.float32), b=np.full((H, W), 0.5, np.float32)), den, "denormal results")


# ------------------------------------------------------------------ plumbing

def test_planes_off_their_16_bytes(hip):
    """Each input plane in turn 4 bytes past a 16-byte boundary, W % 4 == 0: the scalar form takes the call (seen in
    soil_downstream_info) and gives what the 16-byte form gives; outputs off their alignment do not matter."""
    from soillib_amd import _abi, silt
    H, W, B = 33, 260, 3
    graph, stop, scales, planes, want = _stack(H, W, B, D4, "sum")
    want_p = _stack(H, W, B, D4, "power")[4]

    def placed(arr, dtype, off):
        buf = silt.tensor(dtype, silt.shape(B * H * W + 4), silt.gpu)
        assert buf.ptr % 16 == 0
        view = silt.tensor.from_device(buf.ptr + off, dtype, silt.shape(B, H, W), keepalive=buf)
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            _abi.check(hip.soil_memcpy_h2d(view.c_ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, _abi.stream()))
            _abi.check(hip.soil_stream_synchronize(_abi.stream()))
        return view

    pairs = (C.c_float * (2 * B))(*[v for s in scales for v in s])
    names = ("graph", "a", "b", "t", "stop")
    host = dict(graph=graph, a=planes["a"], b=planes["b"], t=planes["t"], stop=stop)
    host_p = dict(graph=graph, a=planes["height"], b=planes["erosivity"], t=planes["uplift"], stop=stop)
    for off_name in names + (None,):
        for out_off in (0, 4):
            o32, o64 = placed(None, silt.float32, out_off), placed(None, silt.float64, 2 * out_off)
            for src, power, ref_words in ((host, False, want), (host_p, True, want_p)):
                d = {k: placed(src[k], silt.int32 if k in ("graph", "stop") else silt.float32, 4 if k == off_name else 0) for k in names}
                if power:
                    _abi.check(hip.soil_stream_power_batch(o32.c_ptr, o64.c_ptr, d["a"].c_ptr, d["graph"].c_ptr, d["b"].c_ptr, d["t"].c_ptr,
                                                           d["stop"].c_ptr, B, H, W, D4, pairs, B, DT, _abi.stream()))
                else:
                    _abi.check(hip.soil_downstream_batch(o32.c_ptr, o64.c_ptr, d["graph"].c_ptr, d["a"].c_ptr, d["b"].c_ptr, d["t"].c_ptr,
                                                         d["stop"].c_ptr, B, H, W, D4, pairs, B, _abi.stream()))
                _same_words((to_np(o32), to_np(o64)), ref_words, "%s off its 16 bytes, outputs %d, power %r" % (off_name, out_off, power))
                assert _info()["chunks"] == 1 and _info()["vec_chunks"] == int(off_name is None), (off_name, out_off, power)


def test_on_another_stream_twice_and_with_another_size_in_between(hip):
    import torch
    from soillib_amd import _abi
    small, large = _stack(37, 53, 7, D8, "sum"), _stack(33, 260, 64, D8, "power")
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        for (graph, stop, scales, planes, want), mode in ((small, "sum"), (large, "power"), (small, "sum"), (small, "sum"), (large, "power")):
            _same_words(_run_mode(graph, D8, planes, mode, scales, stop), want, "on a second stream")
        c = {k: v[2] for k, v in small[3].items()}
        _same_words(_run_mode(small[0][2], D8, c, "sum_no_b", (1.0, 1.0), None),
                    _solve(dref.solve_doubling, small[0][2], D8, c, "sum_no_b", (1.0, 1.0), None), "single, second stream")
    finally:
        _abi.set_stream(0)


CHUNK_SHAPES = [(37, 53), (33, 260)]


def _child_main(path):
    """The child of test_chunks: B = 5 as chunks of 2 + 2 + 1 models and as five chunks of one, every mode."""
    out = {}
    for H, W in CHUNK_SHAPES:
        for models in (2, 1):
            os.environ["SOIL_FLOW_BATCH_CELLS"] = str(models * H * W + (H * W // 2 if models == 2 else 0))
            for edge in (D4, D8):
                for mode in MODES:
                    graph, stop, scales, planes, _ = _stack(H, W, 5, edge, mode)
                    key = "%dx%d_m%d_e%d_%s" % (H, W, models, edge, mode)
                    out[key + "_out"], out[key + "_out64"] = _run_mode(graph, edge, planes, mode, scales, stop)
                    i = _info()
                    out[key + "_info"] = np.array([i["chunks"], i["vec_chunks"], i["idx64_chunks"]])
    _child_optional()
    np.savez(path, **out)


# (H, W, SOIL_FLOW_BATCH_CELLS): B = 5 as 2 + 2 + 1 models, the 16-byte init and the scalar one
OPTIONAL_SHAPES = [(8, 12, 192), (8, 10, 160)]
OPTIONAL_NULLS = {"sum": [(), ("a", "t", "stop", "out64"), ("b", "out")],
                  "power": [(), ("uplift", "stop", "out64"), ("out",)]}


def _child_optional():
    """Every optional argument given and NULL over three chunks: from the second chunk on a plane is the chunk's part
    of it, and a plane that is not given must stay not given.  The words of the five single-grid calls; raises."""
    for H, W, cells in OPTIONAL_SHAPES:
        for mode, nulls in OPTIONAL_NULLS.items():
            graph, stop, scales, planes, _ = _stack(H, W, 5, D8, mode)
            shrink = np.float32([1.0, 0.9, 0.8, 0.7, 0.6])[:, None, None]          # no two models share a plane
            planes = {k: v * shrink for k, v in planes.items()}
            for null in nulls:
                p = {k: None if k in null else v for k, v in planes.items()}
                s = None if "stop" in null else stop
                outs = ("out" not in null, "out64" not in null)
                os.environ["SOIL_FLOW_BATCH_CELLS"] = str(cells)
                got = _run_mode(graph, D8, p, mode, scales, s, outs)
                i = _info()
                assert (i["chunks"], i["vec_chunks"]) == (3, 3 if W % 4 == 0 else 0), (H, W, mode, null, i)
                del os.environ["SOIL_FLOW_BATCH_CELLS"]
                for b in range(5):
                    one = _run_mode(graph[b], D8, {k: None if v is None else v[b] for k, v in p.items()}, mode,
                                    scales[b], None if s is None else s[b], outs)
                    assert [g is None for g in got] == [o is None for o in one] == [not o for o in outs]
                    _same_words([None if g is None else g[b] for g in got], one,
                                "%dx%d %s without %s, model %d" % (H, W, mode, null, b))


@pytest.mark.parametrize("knob", [None, "0", "1", "3", "idx64"])
def test_chunks(hip, tmp_path, knob):
    """Chunks of 2 + 2 + 1 models and of one model (SOIL_FLOW_BATCH_CELLS) in a child process: by default, with the
    listed rounds off (SOIL_PATHS_LIST_FROM = 0), from round 1 and from the later round 3, and ("idx64") under
    SOIL_PATHS_IDX64 = 1, the 64-bit offsets of a model of 2^28 cells or more.  The restatement's bits whatever the
    chunking; the child reports what each call did (soil_downstream_info).  The child also holds a, b, t, stop, uplift
    and either output, given and NULL over three chunks, to the single-grid calls (_child_optional)."""
    path = str(tmp_path / "chunks.npz")
    env = dict(os.environ)
    for name in ("SOIL_FLOW_BATCH_CELLS", "SOIL_PATHS_LIST_FROM", "SOIL_PATHS_IDX64"):
        env.pop(name, None)
    if knob == "idx64":
        env["SOIL_PATHS_IDX64"] = "1"
    elif knob is not None:
        env["SOIL_PATHS_LIST_FROM"] = knob
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    seen = 0
    for H, W in CHUNK_SHAPES:
        for edge in (D4, D8):
            for mode in MODES:
                want = _stack(H, W, 5, edge, mode)[4]
                for models in (2, 1):
                    key = "%dx%d_m%d_e%d_%s" % (H, W, models, edge, mode)
                    _same_words((got[key + "_out"], got[key + "_out64"]), want, "%s, knob %s" % (key, knob))
                    seen += 3
                    chunks = 3 if models == 2 else 5
                    assert got[key + "_info"].tolist() == [chunks, chunks if W % 4 == 0 else 0, chunks if knob == "idx64" else 0]
    assert seen == len(got.files)


def test_the_rounds_in_this_process_with_the_lists_off_and_late(hip, monkeypatch):
    """The knobs are read per call: dense rounds throughout, the lists from a late round and 64-bit offsets, on the
    chain that needs every round and on cycles."""
    for H, W in ((32, 32), (33, 260)):
        for name in ("serpentine", "cycles", "hostile"):
            g = _graphs(H, W, D8)[name]
            for mode in MODES:
                want = _want(H, W, D8, name, "none", SCALES[1], 0, mode)
                for v in ("0", "1", "3", "9", "99"):
                    monkeypatch.setenv("SOIL_PATHS_LIST_FROM", v)
                    for idx64 in ("0", "1"):
                        monkeypatch.setenv("SOIL_PATHS_IDX64", idx64)
                        _same_words(_run_mode(g, D8, _coeffs(H, W, 0), mode, SCALES[1], None), want,
                                    "%s %dx%d %s, lists from %s, idx64 %s" % (name, H, W, mode, v, idx64))
                        assert _info() == dict(chunks=1, vec_chunks=int(W % 4 == 0), idx64_chunks=int(idx64), rounds=len(bin(H * W - 1)) - 2)


def test_the_two_call_infos_stay_each_entry_s_own(hip, monkeypatch):
    """One driver fills both records (csrc/flow_paths.hpp ptr_run): a flow_paths_batch call of 2 + 2 + 1 models and a
    single-grid downstream call, in either order, leave each entry's info what its own call made it, and both calls
    give the restatements' bits."""
    import test_gpu_flow_paths as fp
    graph, stop, scales, paths_want = fp._stack(5, 8, 5, D8)
    g = _graphs(3, 5, D8)["hostile"]
    down_want = _want(3, 5, D8, "hostile", "none", SCALES[1], 0, "sum")
    paths_info = dict(chunks=3, vec_chunks=3, idx64_chunks=0, rounds=6)        # 80 cells a chunk; ceil(log2 40)
    down_info = dict(chunks=1, vec_chunks=0, idx64_chunks=0, rounds=4)         # W = 5: scalar init; ceil(log2 15)

    def paths():
        monkeypatch.setenv("SOIL_FLOW_BATCH_CELLS", "80")
        fp._same_words(fp._batch(graph, D8, scales, stop), paths_want, "5x8 x 5 in chunks of 80 cells")
        monkeypatch.delenv("SOIL_FLOW_BATCH_CELLS")

    def down():
        _same_words(_run_mode(g, D8, _coeffs(3, 5, 0), "sum", SCALES[1], None), down_want, "hostile 3x5")

    for first, second in ((paths, down), (down, paths)):
        first()
        second()
        assert fp._info() == paths_info and _info() == down_info, (first.__name__, fp._info(), _info())


# ------------------------------------------------------------------ isolation

def test_a_hostile_model_between_two_benign_ones(hip):
    """Model 1: a hostile graph with entries in its neighbours' numbering and non-finite coefficients.  Models 0 and
    2 keep the bits they have alone, model 1 the restatement's."""
    H, W = 33, 260
    for edge in (D4, D8):
        g1 = ref.hostile(H, W, 60, model=1)
        a1, b1, t1, _ = _hostile_planes(H, W, g1, edge)
        benign = [_coeffs(H, W, d) for d in (0, 1)]
        graph = np.stack([_graphs(H, W, edge)["serpentine"], g1, _graphs(H, W, edge)["all_donors"]])
        a, b, t = (np.stack([benign[0][k], p, benign[1][k]]) for k, p in (("a", a1), ("b", b1), ("t", t1)))
        got = _run(graph, edge, a, b, t, SCALES)
        want = dref.solve_batch(dref.solve_doubling, graph, edge, a, b, t, SCALES)
        _same_words(got, want, "edge %d" % edge)
        for m in (0, 2):
            assert not np.isnan(got[1][m]).any(), "model %d took a NaN from its neighbour" % m
            _same_words([o[m] for o in got], _run(graph[m], edge, a[m], b[m], t[m], SCALES[m]), "model %d alone" % m)
        pw = (np.stack([benign[0]["height"], t1, benign[1]["height"]]), np.abs(a), np.stack([benign[0]["uplift"], a1, benign[1]["uplift"]]), DT)
        got = _run(graph, edge, scale=SCALES, power=pw)
        _same_words(got, dref.solve_batch(dref.solve_doubling, graph, edge, scale=SCALES, power=pw), "stream power, edge %d" % edge)
        assert not np.isnan(got[1][0]).any() and not np.isnan(got[1][2]).any()


# ------------------------------------------------------------------ against the single-grid device call

def _bench_heights(B, H, W):
    """B bench terrains (noise x 100, another seed per model) as one (B, H, W) GPU tensor."""
    from soillib_amd import _abi, silt, soil
    h = silt.tensor(silt.float32, silt.shape(B, H, W), silt.gpu)
    per = h.nbytes() // B
    for b in range(B):
        p = soil.noise_t()
        p.seed = float(5 + b)
        p.ext = [H, W]
        one = soil.noise(silt.shape(H, W), p, host=silt.gpu)
        silt.multiply(one, 100.0)
        _abi.check(_abi.lib().soil_memcpy_d2d(C.c_void_p(h.ptr + b * per), one.c_ptr, per, _abi.stream()))
    return h


def _model(t, b):
    from soillib_amd import silt
    per = t.nbytes() // t.shape[0]
    return silt.tensor.from_device(t.ptr + b * per, t.type, silt.shape(*tuple(t.shape)[1:]), keepalive=t)


def test_the_batch_entries_against_the_single_grid_calls(hip):
    from soillib_amd import soil
    B, H, W = 8, 256, 256
    scales = [(1.0 + b, 2.0 + 0.5 * b) for b in range(B)]
    r = np.random.default_rng(H)
    stop = to_gpu((r.random((B, H, W)) < 0.001).astype(np.int32))
    a, b_, t = (to_gpu(r.uniform(-1.0, 1.0, (B, H, W)).astype(np.float32)) for _ in range(3))
    k = to_gpu(np.exp(r.uniform(np.log(1e-6), np.log(1e3), (B, H, W))).astype(np.float32))
    h = _bench_heights(B, H, W)
    for edge in (D4, D8):
        graph = soil.random_weighted_batch(h, edge, [3 + i for i in range(B)], 1, 10.0)
        for st in (None, stop):
            sm = lambda p, i: None if p is None else _model(p, i)
            for dbl in (False, True):
                got = to_np(soil.downstream_batch(graph, edge, a, b_, t, scales, st, double=dbl))
                got_p = to_np(soil.stream_power_batch(h, graph, k, edge, scales, DT, a, st, double=dbl))
                for i in range(B):
                    one = to_np(soil.downstream(_model(graph, i), edge, sm(a, i), sm(b_, i), sm(t, i), scales[i], sm(st, i), double=dbl))
                    assert (dref.words(got[i]) == dref.words(one)).all(), (edge, i, dbl)
                    one = to_np(soil.stream_power(_model(h, i), _model(graph, i), _model(k, i), edge, scales[i], DT, sm(a, i), sm(st, i), double=dbl))
                    assert (dref.words(got_p[i]) == dref.words(one)).all(), (edge, i, dbl)
                assert np.isfinite(got).all() and np.isfinite(got_p).all(), "a downhill graph has no cycle"
    i = B - 1                                                        # and one model against the restatement
    want = dref.solve_doubling(to_np(_model(graph, i)), D8, to_np(_model(a, i)), to_np(_model(b_, i)), to_np(_model(t, i)),
                               scales[i], to_np(_model(stop, i)))
    _same_words((None, got[i]), want, "the last model against the restatement")


def test_the_thin_forms_and_what_exists(hip):
    """downstream with everything NULL is flow_paths' steps, with a scale its length (D4, dyadic scales: every sum is
    exact), with t = the cell's index and a = 0 its terminal; chi is downstream of its weights."""
    from soillib_amd import soil
    H, W = 96, 96
    h = _model(_bench_heights(1, H, W), 0)
    for edge in (D4, D8):
        filled, graph = soil.condition(h, edge)
        terminal, steps, length = (to_np(p) for p in soil.flow_paths(graph, edge, (0.25, 8.0)))
        assert (terminal >= 0).all()
        assert (to_np(soil.downstream(graph, edge)) == steps).all()
        assert (to_np(soil.downstream(graph, edge, double=True)) == steps).all()
        if edge == D4:
            assert (ref.words(to_np(soil.downstream(graph, edge, scale=(0.25, 8.0)))) == ref.words(length)).all()
        cells = to_gpu(np.arange(H * W, dtype=np.float32).reshape(H, W))
        zeros = to_gpu(np.zeros((H, W), np.float32))
        assert (to_np(soil.downstream(graph, edge, a=zeros, terminal=cells)) == terminal).all()
        outlet = to_np(soil.downstream(graph, edge, a=zeros, terminal=filled))      # the height of a cell's outlet
        assert (outlet == to_np(filled).reshape(-1)[terminal]).all()
        area = soil.accumulate(graph, to_gpu(np.ones((H, W), np.float32)), edge)
        chi = to_np(soil.chi(graph, area, edge, (0.5, 2.0), theta=0.45, A0=1.0))
        w = (np.float32(1.0) / to_np(area)) ** np.float32(0.45)
        host = dref.solve_doubling(to_np(graph), edge, a=w.astype(np.float32), scale=(0.5, 2.0))[0]
        assert np.isfinite(chi).all() and (chi[terminal == np.arange(H * W).reshape(H, W)] == 0).all()
        # the weights are torch's float32 powers, a few ulps from numpy's and not bit-pinned; a sum of non-negative
        # terms keeps their relative error, and the float32 result adds half an ulp: 2^-20 covers four ulps of both
        assert (np.abs(chi - host) <= 2.0 ** -20 * host).all()


# ------------------------------------------------------------------ the stream-power step

@functools.lru_cache(maxsize=None)
def _conditioned(H, edge):
    """A conditioned bench terrain and the planes of a step on it, as numpy: filled, graph, erosivity, uplift."""
    from soillib_amd import soil
    h = _model(_bench_heights(1, H, H), 0)
    filled, graph = soil.condition(h, edge)
    area = soil.accumulate(graph, to_gpu(np.ones((H, H), np.float32)), edge)
    k = soil.erosivity(area, 2e-3, 0.5)
    uplift = np.full((H, H), 0.01, np.float32)      # uniform: the lifted surface still falls along every edge
    out = tuple(np.ascontiguousarray(p) for p in (to_np(filled), to_np(graph), to_np(k), uplift))
    assert np.allclose(out[2], 2e-3 * np.sqrt(to_np(area).astype(np.float64)), rtol=1e-5, atol=0), "erosivity = K area^m"
    for p in out:
        p.setflags(write=False)
    return out


@pytest.mark.parametrize("H", [96, 256])
@pytest.mark.parametrize("edge", [D4, D8])
def test_stream_power_on_a_conditioned_terrain(hip, H, edge):
    filled, graph, k, uplift = _conditioned(H, edge)
    scale, dt = (20.0 / H, 30.0 / H), 40.0
    for u in (uplift, None):
        pw = (filled, k, u, dt)
        want = dref.solve_doubling(graph, edge, scale=scale, power=pw)
        assert want[2].all() and np.isfinite(want[1]).all(), "a conditioned graph resolves every cell"
        got = _run(graph, edge, scale=scale, power=pw)
        _same_words(got, want, "%d^2 edge %d" % (H, edge))
        serial = dref.solve_serial(graph, edge, scale=scale, power=pw)
        d = dref.ulps32(got[0], serial[0])
        print("stream power %d^2 edge %d uplift %r: %d float32 ulps at most from the serial solver, %d cells differ" % (
            H, edge, u is not None, d.max(), (d > 0).sum()))
        assert d.max() <= 1
        r = graph.reshape(-1)
        has = np.flatnonzero(r >= 0)                                 # (a conditioned graph: an entry >= 0 is an edge)
        out = got[0].reshape(-1)
        below = out[r[has]]
        assert (out[has] >= np.nextafter(below, np.float32(-np.inf))).all(), "out[n] >= out[r(n)] to within 1 ulp"
        if u is None:
            assert (out <= filled.reshape(-1)).all() and (out < filled.reshape(-1)).any(), "incision lowers, never raises"
        terminals = graph.reshape(-1) < 0
        assert terminals.any() and (dref.words(got[0].reshape(-1)[terminals]) == dref.words(filled.reshape(-1)[terminals])).all()
    same = _run(graph, edge, scale=scale, power=(filled, k, None, 0.0))
    _same_words(same, (filled, filled.astype(np.float64)), "dt = 0 returns the heights")
    same = _run(graph, edge, scale=scale, power=(filled, k, uplift, 0.0))
    assert (same[0] == filled).all()


def test_stream_power_of_stepped_models(hip, oracle):
    """ErosionBatch.stream_power after real steps is the chain done by hand, model by model, with one scale and with
    a scale per model; the batch's planes stay as they are."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    B, H, W = 3, 128, 128
    p = product_param(script_param(oracle.default_param()))
    p.maxage = 64
    scales = [(20.0 / H * (1 + b), 20.0 / W, 4.0) for b in range(B)]
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    uplift = to_gpu((np.random.default_rng(2).random((B, H, W)) * 1e-3).astype(np.float32))
    for scale in ((20.0 / H, 20.0 / W, 4.0), scales):
        bt = ErosionBatch(B, H, W, scale, p, 1024, [11 + 7 * b for b in range(B)])
        bt.set_layers(to_gpu(layers))
        silt.set(bt.rainfall, 1.0)
        for _ in range(2):
            bt.step()
        before = to_np(bt.height).copy()
        got = to_np(bt.stream_power(25.0, 1e-3, m=0.4, uplift=uplift))
        got_d4 = to_np(bt.stream_power(25.0, 1e-3, edge=D4))
        assert (to_np(bt.height) == before).all(), "the batch's own state is not touched"
        pairs = [s[:2] for s in scales] if scale is scales else [scale[:2]]
        flow = to_np(bt.flow())
        for kw, want in ((dict(), dref.solve_batch(dref.solve_doubling, flow, D8, scale=pairs)),
                         (dict(scaled=False, terminal=bt.height, double=True),
                          dref.solve_batch(dref.solve_doubling, flow, D8, t=before))):
            sums = to_np(bt.downstream(**kw))
            assert (dref.words(sums) == dref.words(want[1 if kw else 0])).all(), "ErosionBatch.downstream(%r)" % sorted(kw)
        for b, m in enumerate(bt.to_models()):
            s2 = (scale if scale is not scales else scales[b])[:2]
            for edge, out, u, mm in ((D8, got, _model(uplift, b), 0.4), (D4, got_d4, None, 0.5)):
                filled, graph = soil.condition(m.height, edge)
                area = soil.accumulate(graph, to_gpu(np.ones((H, W), np.float32)), edge)
                one = to_np(soil.stream_power(filled, graph, soil.erosivity(area, 1e-3, mm), edge, s2, 25.0, u))
                assert (dref.words(out[b]) == dref.words(one)).all(), "model %d edge %d" % (b, edge)
                assert np.isfinite(one).all()


def test_three_steps_with_re_conditioning_stay_finite(hip):
    """After a step a strictly downhill graph may hold float32 ties — two fp64 heights in the right order round to one
    float — so each step starts again from condition(); the surface stays finite and keeps falling."""
    from soillib_amd import soil
    H = 96
    h = _model(_bench_heights(1, H, H), 0)
    ones = to_gpu(np.ones((H, H), np.float32))
    first, ties = to_np(h), 0
    for _ in range(3):
        filled, graph = soil.condition(h, D8)
        k = soil.erosivity(soil.accumulate(graph, ones, D8), 5e-3, 0.5)
        h = soil.stream_power(filled, graph, k, D8, (0.2, 0.2), 100.0)
        out, g = to_np(h).reshape(-1), to_np(graph).reshape(-1)
        assert np.isfinite(out).all()
        has = np.flatnonzero(g >= 0)
        ties += int((out[has] == out[g[has]]).sum())
        assert (out[has] >= np.nextafter(out[g[has]], np.float32(-np.inf))).all()
    print("float32 ties along the edges after the three steps: %d" % ties)
    # (the fill is monotone and a step without uplift never raises a cell: nothing lies above the first fill)
    assert (to_np(h) <= to_np(soil.fill_depressions(to_gpu(first), D8))).all()


# ------------------------------------------------------------------ refusals

def test_refusals_leave_the_outputs_untouched(hip):
    from soillib_amd import _abi, silt
    B, H, W = 2, 5, 8
    mark = np.float32(-7.5)
    o32 = to_gpu(np.full((B, H, W), mark, np.float32))
    o64 = to_gpu(np.full((B, H, W), np.float64(mark), np.float64))
    g = to_gpu(np.full((B, H, W), -1, np.int32))
    f = [to_gpu(np.ones((B, H, W), np.float32)) for _ in range(3)]
    sc = (C.c_float * (2 * B))(1, 1, 1, 1)
    bad_sc = (C.c_float * (2 * B))(1, 1, 0, 1)
    st = _abi.stream()
    big = 1 << 16
    P = lambda t: t.c_ptr

    def sums(name, out=o32, out64=o64, graph=g, a=f[0], Bn=B, h=H, w=W, e=D8, s=sc, n=B):
        fn = getattr(hip, "soil_" + name)
        dims = (h, w, e, s) if name == "downstream" else (Bn, h, w, e, s, n)
        return fn(_ptr(out), _ptr(out64), _ptr(graph), _ptr(a), P(f[1]), P(f[2]), None, *dims, st)

    def power(name, out=o32, out64=o64, graph=g, height=f[0], k=f[1], Bn=B, h=H, w=W, e=D8, s=sc, n=B, dt=1.0):
        fn = getattr(hip, "soil_" + name)
        dims = (h, w, e, s, dt) if name == "stream_power" else (Bn, h, w, e, s, n, dt)
        return fn(_ptr(out), _ptr(out64), _ptr(height), _ptr(graph), _ptr(k), P(f[2]), None, *dims, st)

    def refused(name, rc):
        assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, name
        assert _abi.last_error().startswith(name + ": "), (name, _abi.last_error())

    for call, names in ((sums, ("downstream", "downstream_batch")), (power, ("stream_power", "stream_power_batch"))):
        for name in names:
            refused(name, call(name, graph=None))
            refused(name, call(name, out=None, out64=None))
            refused(name, call(name, out=f[1]))                      # an output that is an input plane
            refused(name, call(name, out64=g))
            for h, w in ((0, W), (H, 0), (-1, W), (big, big)):
                refused(name, call(name, h=h, w=w))
            for e in (2, -1, 8):
                refused(name, call(name, e=e))
            if name.endswith("_batch"):
                for b in (0, -1):
                    refused(name, call(name, Bn=b))
                for n in (0, B + 1, -1, 3):
                    refused(name, call(name, n=n))
    for name in ("stream_power", "stream_power_batch"):
        refused(name, power(name, height=None))
        refused(name, power(name, k=None))
        refused(name, power(name, s=None))
        for dt in (-1.0, float("inf"), float("nan")):
            refused(name, power(name, dt=dt))
    refused("stream_power_batch", power("stream_power_batch", s=bad_sc))
    _abi.check(hip.soil_stream_synchronize(st))
    assert (to_np(o32) == mark).all() and (to_np(o64) == mark).all()
    assert isinstance(o64, silt.tensor)


if __name__ == "__main__":
    _child_main(sys.argv[1])
