"""The stream-power step with sediment deposition on the device (include/soil_hip.h: soil_stream_power_deposit and its
_batch form; soillib_amd.soil.stream_power_deposit / _batch / deposition, ErosionBatch.stream_power_deposit and
evolve(G=...)), bit for bit against solve_iterated of tests/deposit_ref.py: every comparison with it is of the words of
out (float32), out64 (float64), flux (float32) and residual (float64), the NaN words included; there is no tolerance.

  shapes     1x17, 17x1, 12x20 (the 16-byte init and q passes), 13x21 (the scalar ones), 48x64 (several work-groups
             of a round), 5x1028 and 3x261 (two work-groups along a row in the init and q passes: 257 threads a row in
             the 16-byte form, 261 in the scalar one); D4 and D8
  graphs     every built graph of flow_paths_ref (a chain through every cell, cells with all donors, no edge at all,
             hostile entries, cycles: NaN words on a cycle and upstream of it) and downhill graphs
  inputs     with and without uplift, iters 1, 2 and 6, NaN heights as voids, dt = 0, erosivity 0
  batches    3 x 12x20 with one pair and with a pair per model against the single calls, a hostile model between two
             benign ones, in child processes chunks of 2 + 2 + 1 and of one model, 64-bit offsets, and the lists of
             both engines off and from their first round
  identities a zero deposition plane against soil.stream_power of the library itself
  plumbing   planes 4 bytes off their alignment, a second stream, the call info
  methods    ErosionBatch.stream_power_deposit and evolve with and without G against the module calls chained by hand
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import deposit_ref as dep
import downstream_ref as dref
import flow_paths_ref as ref
from flow_paths_ref import D4, D8
from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 17), (17, 1), (12, 20), (13, 21), (48, 64), (5, 1028), (3, 261)]
SCALES = [(0.3, 0.7), (1.0, 1.0), (2.5, 0.125)]
DT = 10.0
ALL = ("out", "out64", "flux", "residual")


def _oracle():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


def _ptr(t):
    return None if t is None else t.c_ptr


def _run(graph, edge, height, erosivity, deposition, scale, dt=DT, uplift=None, iters=6, want=ALL):
    """One call of the C ABI on numpy planes, (H, W) or (B, H, W) by the graph's rank: a dict of the outputs asked for
    (`want`) as numpy.  `scale`: one pair or B pairs."""
    from soillib_amd import _abi, silt
    lib = _abi.lib()
    graph = np.asarray(graph)
    shape = graph.shape
    B = 1 if len(shape) == 2 else shape[0]
    dev = lambda p: None if p is None else to_gpu(np.ascontiguousarray(p))
    planes = [dev(height), dev(graph), dev(erosivity), dev(deposition), dev(uplift)]
    outs = dict(out=silt.tensor(silt.float32, silt.shape(*shape), silt.gpu) if "out" in want else None,
                out64=silt.tensor(silt.float64, silt.shape(*shape), silt.gpu) if "out64" in want else None,
                flux=silt.tensor(silt.float32, silt.shape(*shape), silt.gpu) if "flux" in want else None,
                residual=to_gpu(np.full(B, -1.0, np.float64)) if "residual" in want else None)
    pairs = np.asarray(scale, np.float32).reshape(-1)
    sc = (C.c_float * len(pairs))(*pairs.tolist())
    tail = (sc,) if len(shape) == 2 else (sc, len(pairs) // 2)
    fn = lib.soil_stream_power_deposit if len(shape) == 2 else lib.soil_stream_power_deposit_batch
    _abi.check(fn(*[_ptr(outs[k]) for k in ALL], *[_ptr(p) for p in planes], *shape, edge, *tail, float(dt), int(iters),
                  _abi.stream()))
    return {k: to_np(v) for k, v in outs.items() if v is not None}


def _info():
    from soillib_amd import soil
    return soil.stream_power_deposit_info()


# ------------------------------------------------------------------ inputs and references, made once

@functools.lru_cache(maxsize=None)
def _graphs(H, W, edge):
    out = dict(ref.built_graphs(H, W, edge))
    out["descent"] = ref.descent((ref.terrain(H, W, 2) * 10).astype(np.float32), edge)
    out["descent_random"] = ref.descent((ref.terrain(H, W, 4) * 10).astype(np.float32), edge, seed=7)
    for g in out.values():
        g.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _planes(H, W, draw):
    """A height of terrain * 10, an erosivity over 1e-3 .. 10, a deposition in [0, 2] and an uplift in [0, 0.01]."""
    r = np.random.default_rng([draw, H, W])
    out = dict(height=(ref.terrain(H, W, 2 + draw) * 10).astype(np.float32),
               erosivity=np.exp(r.uniform(np.log(1e-3), np.log(10.0), (H, W))).astype(np.float32),
               deposition=r.uniform(0.0, 2.0, (H, W)).astype(np.float32),
               uplift=(r.random((H, W)) * 0.01).astype(np.float32))
    for p in out.values():
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(H, W, edge, gname, scale, draw, uplift, iters, dt=DT):
    p = _planes(H, W, draw)
    out = dep.solve_iterated(_oracle(), _graphs(H, W, edge)[gname], edge, p["height"], p["erosivity"], p["deposition"],
                             scale, dt, p["uplift"] if uplift else None, iters)
    assert (np.isnan(out["out64"]) == ~out["final"]).all(), "a draw made a NaN of its own"
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _got(H, W, edge, gname, scale, draw, uplift, iters, dt=DT, **kw):
    p = _planes(H, W, draw)
    return _run(_graphs(H, W, edge)[gname], edge, p["height"], p["erosivity"], p["deposition"], scale, dt,
                p["uplift"] if uplift else None, iters, **kw)


# ------------------------------------------------------------------ against the restatement

@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
def test_single_grid_against_the_restatement(hip, H, W, edge):
    """Every graph, iters 1, 2 and 6, with and without uplift, the scale and the draw changing from case to case."""
    k = 0
    for gname in sorted(_graphs(H, W, edge)):
        for iters in (1, 2, 6):
            case = (H, W, edge, gname, SCALES[k % 3], k % 2, k % 2 == 0, iters)
            want = _want(*case)
            dep.same_words(_got(*case), want, "%s iters %d, %dx%d edge %d" % (gname, iters, H, W, edge))
            i = _info()
            assert i["iters"] == iters and i["chunks"] == 1
            if gname == "cycles":
                assert np.isnan(want["out64"]).any() and np.isfinite(want["out64"]).any()
            if gname.startswith("descent"):
                assert want["final"].all() and (want["flux"] != 0).any() and want["residual"] > 0
            k += 1


def test_each_output_alone(hip):
    case = (13, 21, D8, "descent", SCALES[0], 0, True, 3)
    want = _want(*case)
    for outs in (("out",), ("out64",), ("out", "flux"), ("out64", "residual")):
        got = _got(*case, want=outs)
        assert sorted(got) == sorted(outs)
        dep.same_words(got, want, "outputs %r" % (outs,))


@pytest.mark.parametrize("H,W", [(12, 20), (13, 21)])
def test_voids_dt_zero_and_erosivity_zero(hip, H, W):
    o = _oracle()
    p = _planes(H, W, 0)
    for edge in (D4, D8):
        g = _graphs(H, W, edge)["descent"]
        area = o.accumulate(g, np.ones((H, W), np.float32), edge)
        # NaN heights: a cell in mid-stream and a head
        h = p["height"].copy()
        at = int(np.argmax(np.where((area > 4) & (g >= 0), area, 0)))
        h.reshape(-1)[[at, int(np.argmin(area))]] = np.nan
        want = dep.solve_iterated(o, g, edge, h, p["erosivity"], p["deposition"], SCALES[0], DT, p["uplift"], 4)
        marks = np.isnan(h).astype(np.float32)
        way = dref.solve_doubling(g, edge, a=marks, t=marks)[1] != 0
        assert (np.isnan(want["out64"]) == way).all() and way.sum() > 5, "the void and everything upstream of it"
        assert np.isfinite(want["flux"]).all() and np.isfinite(want["residual"])
        dep.same_words(_run(g, edge, h, p["erosivity"], p["deposition"], SCALES[0], DT, p["uplift"], 4), want, "voids")
        # dt = 0: the heights, nothing moves
        want = dep.solve_iterated(o, g, edge, p["height"], p["erosivity"], p["deposition"], SCALES[0], 0.0, p["uplift"], 3)
        assert (want["out"] == p["height"]).all() and want["residual"] == 0 and not want["flux"].any()
        dep.same_words(_run(g, edge, p["height"], p["erosivity"], p["deposition"], SCALES[0], 0.0, p["uplift"], 3), want, "dt = 0")
        # erosivity 0: nothing is eroded, so nothing is deposited; the uplift stays.  ((1 + g) b) / (1 + g) is b to
        # within two roundings, 2^-51 |b| a cell, and the flux sums at most H W of those
        zero = np.zeros((H, W), np.float32)
        want = dep.solve_iterated(o, g, edge, p["height"], zero, p["deposition"], SCALES[0], DT, p["uplift"], 3)
        assert np.abs(want["flux"]).max() <= H * W * 2.0 ** -51 * (np.abs(p["height"]).max() + 1.0)
        dep.same_words(_run(g, edge, p["height"], zero, p["deposition"], SCALES[0], DT, p["uplift"], 3), want, "erosivity 0")


# ------------------------------------------------------------------ batches

def _stack(H, W, B, edge, iters, uplift=True):
    """graph, planes (a dict), the scales and the reference of B models: neighbours differ in graph, scale and draw."""
    names = sorted(_graphs(H, W, edge))
    cfg = [(names[(2 * b + 1) % len(names)], SCALES[b % 3], b % 2) for b in range(B)]
    graph = np.stack([_graphs(H, W, edge)[g] for g, _, _ in cfg])
    planes = {k: np.stack([_planes(H, W, d)[k] for _, _, d in cfg]) for k in _planes(H, W, 0)}
    wants = [_want(H, W, edge, g, s, d, uplift, iters) for g, s, d in cfg]
    want = {k: np.stack([np.asarray(w[k]) for w in wants]) for k in ALL}
    return graph, planes, [s for _, s, _ in cfg], want


def _run_stack(graph, planes, scales, edge, iters, uplift=True, **kw):
    return _run(graph, edge, planes["height"], planes["erosivity"], planes["deposition"], scales, DT,
                planes["uplift"] if uplift else None, iters, **kw)


@pytest.mark.parametrize("edge", [D4, D8])
def test_a_batch_equals_the_single_calls(hip, edge):
    B, H, W, iters = 3, 12, 20, 4
    graph, planes, scales, want = _stack(H, W, B, edge, iters)
    got = _run_stack(graph, planes, scales, edge, iters)
    dep.same_words(got, want, "a pair per model")
    for b in range(B):
        one = _run(graph[b], edge, *[planes[k][b] for k in ("height", "erosivity", "deposition")], scales[b], DT,
                   planes["uplift"][b], iters)
        dep.same_words({k: got[k][b] for k in ALL}, {k: one[k].reshape(got[k][b].shape) for k in ALL}, "model %d alone" % b)
    got = _run_stack(graph, planes, SCALES[1], edge, iters, uplift=False)
    o = _oracle()
    for b in range(B):
        w = dep.solve_iterated(o, graph[b], edge, planes["height"][b], planes["erosivity"][b], planes["deposition"][b],
                               SCALES[1], DT, None, iters)
        dep.same_words({k: got[k][b] for k in ALL}, w, "one pair, model %d" % b)


def test_a_hostile_model_between_two_benign_ones(hip):
    H, W, iters = 12, 20, 3
    o = _oracle()
    for edge in (D4, D8):
        graph = np.stack([_graphs(H, W, edge)["descent"], ref.hostile(H, W, 60, model=1), _graphs(H, W, edge)["descent_random"]])
        planes = {k: np.stack([_planes(H, W, d)[k] for d in (0, 1, 0)]).copy() for k in _planes(H, W, 0)}
        bad = planes["height"][1].reshape(-1)
        bad[3], bad[40], bad[77] = np.nan, np.inf, -np.inf
        planes["erosivity"][1].reshape(-1)[[5, 50]] = np.inf, 3e38
        planes["deposition"][1].reshape(-1)[[9, 90]] = 3e38, np.nan
        got = _run_stack(graph, planes, SCALES, edge, iters)
        for b in range(3):
            w = dep.solve_iterated(o, graph[b], edge, *[planes[k][b] for k in ("height", "erosivity", "deposition")],
                                   SCALES[b], DT, planes["uplift"][b], iters)
            dep.same_words({k: got[k][b] for k in ALL}, w, "model %d edge %d" % (b, edge))
        for b in (0, 2):
            assert np.isfinite(got["out64"][b]).all() and np.isfinite(got["flux"][b]).all(), "model %d took something from its neighbour" % b


CHUNK_SHAPES = [(12, 20), (13, 21)]


def _child_main(path):
    """The child of test_chunks_and_knobs: B = 5 as chunks of 2 + 2 + 1 models, as five chunks of one and whole."""
    out = {}
    for H, W in CHUNK_SHAPES:
        for models in (2, 1, 0):
            if models:
                os.environ["SOIL_FLOW_BATCH_CELLS"] = str(models * H * W + (H * W // 2 if models == 2 else 0))
            else:
                os.environ.pop("SOIL_FLOW_BATCH_CELLS", None)
            for edge in (D4, D8):
                graph, planes, scales, _ = _stack(H, W, 5, edge, 3)
                key = "%dx%d_m%d_e%d_" % (H, W, models, edge)
                for k, v in _run_stack(graph, planes, scales, edge, 3).items():
                    out[key + k] = v
                i = _info()
                out[key + "info"] = np.array([i["chunks"], i["iters"], i["launches"]])
    _child_optional()
    np.savez(path, **out)


# (H, W, SOIL_FLOW_BATCH_CELLS): B = 5 as 2 + 2 + 1 models, the 16-byte passes and the scalar ones
OPTIONAL_SHAPES = [(8, 12, 192), (8, 10, 160)]
OPTIONAL_NULLS = [(), ("uplift", "out64", "flux"), ("out", "residual")]


def _child_optional():
    """The uplift and every output given and NULL over three chunks: from the second chunk on a plane is the chunk's
    part of it, and one that is not given must stay not given.  The words of the five single-grid calls; raises."""
    for H, W, cells in OPTIONAL_SHAPES:
        graph, planes, scales, _ = _stack(H, W, 5, D8, 2)
        shrink = np.float32([1.0, 0.9, 0.8, 0.7, 0.6])[:, None, None]              # no two models share a plane
        planes = {k: v * shrink for k, v in planes.items()}
        for null in OPTIONAL_NULLS:
            kw = dict(uplift="uplift" not in null, want=tuple(k for k in ALL if k not in null))
            os.environ["SOIL_FLOW_BATCH_CELLS"] = str(cells)
            got = _run_stack(graph, planes, scales, D8, 2, **kw)
            assert _info()["chunks"] == 3 and sorted(got) == sorted(kw["want"]), (H, W, null, _info(), sorted(got))
            del os.environ["SOIL_FLOW_BATCH_CELLS"]
            for b in range(5):
                one = _run_stack(graph[b], {k: v[b] for k, v in planes.items()}, scales[b], D8, 2, **kw)
                dep.same_words({k: v[b] for k, v in got.items()}, one, "%dx%d without %s, model %d" % (H, W, null, b))


@pytest.mark.parametrize("knob", [None, "idx64", "paths_0", "paths_1", "rake_0", "rake_1"])
def test_chunks_and_knobs(hip, tmp_path, knob):
    """A 5-model batch in a child process, whole and in chunks of 2 + 2 + 1 and of one model (SOIL_FLOW_BATCH_CELLS):
    by default, under SOIL_PATHS_IDX64 = 1, and with the listed rounds of either engine off (0) and from the first
    round they can start at (1): SOIL_PATHS_LIST_FROM, SOIL_RAKE_LIST_FROM.  The restatement's words every time.  The
    child also holds the uplift and each output, given and NULL over three chunks, to the single-grid calls
    (_child_optional)."""
    path = str(tmp_path / "chunks.npz")
    env = dict(os.environ)
    for name in ("SOIL_FLOW_BATCH_CELLS", "SOIL_PATHS_LIST_FROM", "SOIL_PATHS_IDX64", "SOIL_RAKE_LIST_FROM"):
        env.pop(name, None)
    if knob == "idx64":
        env["SOIL_PATHS_IDX64"] = "1"
    elif knob is not None:
        env["SOIL_PATHS_LIST_FROM" if knob.startswith("paths") else "SOIL_RAKE_LIST_FROM"] = knob[-1]
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    for H, W in CHUNK_SHAPES:
        for edge in (D4, D8):
            want = _stack(H, W, 5, edge, 3)[3]
            launches = {}
            for models in (2, 1, 0):
                key = "%dx%d_m%d_e%d_" % (H, W, models, edge)
                dep.same_words({k: got[key + k] for k in ALL}, want, "%s, knob %s" % (key, knob))
                chunks, iters, launches[models] = got[key + "info"].tolist()
                assert (chunks, iters) == ({2: 3, 1: 5, 0: 1}[models], 3)
            assert launches[2] == 3 * launches[0] and launches[1] == 5 * launches[0], "a chunk's launches do not depend on its models"


# ------------------------------------------------------------------ identities and plumbing

@pytest.mark.parametrize("H,W", [(12, 20), (13, 21), (48, 64), (5, 1028), (3, 261)])
def test_a_zero_deposition_plane_gives_the_library_s_stream_power(hip, H, W):
    from soillib_amd import soil
    p = _planes(H, W, 1)
    zero = to_gpu(np.zeros((H, W), np.float32))
    h, k, u = to_gpu(p["height"]), to_gpu(p["erosivity"]), to_gpu(p["uplift"])
    for edge in (D4, D8):
        for gname, g in sorted(_graphs(H, W, edge).items()):
            graph = to_gpu(g)
            for uplift, iters, dbl in ((None, 1, False), (u, 2, True), (u, 5, False)):
                want = to_np(soil.stream_power(h, graph, k, edge, SCALES[0], DT, uplift, double=dbl))
                got = to_np(soil.stream_power_deposit(h, graph, k, zero, edge, SCALES[0], DT, uplift, iters, dbl))
                assert got.dtype == want.dtype and (dref.words(got) == dref.words(want)).all(), (gname, edge, iters, dbl)


def test_planes_off_their_16_bytes(hip):
    """Each input plane in turn 4 bytes past a 16-byte boundary, W % 4 == 0: the scalar passes take the call and give
    what the 16-byte ones give; outputs off their alignment do not matter."""
    from soillib_amd import _abi, silt
    B, H, W, iters = 3, 12, 20, 3
    graph, planes, scales, want = _stack(H, W, B, D8, iters)

    def placed(arr, dtype, off, count=B * H * W, shape=(B, H, W)):
        buf = silt.tensor(dtype, silt.shape(count + 4), silt.gpu)
        assert buf.ptr % 16 == 0
        view = silt.tensor.from_device(buf.ptr + off, dtype, silt.shape(*shape), keepalive=buf)
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            _abi.check(hip.soil_memcpy_h2d(view.c_ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, _abi.stream()))
            _abi.check(hip.soil_stream_synchronize(_abi.stream()))
        return view

    pairs = (C.c_float * (2 * B))(*[v for s in scales for v in s])
    names = ("height", "graph", "erosivity", "deposition", "uplift")
    host = dict(planes, graph=graph)
    for off_name in names + (None,):
        for out_off in (0, 4):
            o32, o64 = placed(None, silt.float32, out_off), placed(None, silt.float64, 2 * out_off)
            fl, rs = placed(None, silt.float32, out_off), placed(None, silt.float64, 2 * out_off, B, (B,))
            d = {k: placed(host[k], silt.int32 if k == "graph" else silt.float32, 4 if k == off_name else 0) for k in names}
            _abi.check(hip.soil_stream_power_deposit_batch(o32.c_ptr, o64.c_ptr, fl.c_ptr, rs.c_ptr, *[d[k].c_ptr for k in names],
                                                           B, H, W, D8, pairs, B, DT, iters, _abi.stream()))
            dep.same_words(dict(out=to_np(o32), out64=to_np(o64), flux=to_np(fl), residual=to_np(rs)), want,
                           "%s off its 16 bytes, outputs %d" % (off_name, out_off))


def test_on_another_stream_twice_and_with_another_size_in_between(hip):
    import torch
    from soillib_amd import _abi
    small, large = _stack(13, 21, 3, D8, 2), _stack(48, 64, 2, D4, 3)
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        for (graph, planes, scales, want), edge, iters in ((small, D8, 2), (large, D4, 3), (small, D8, 2), (small, D8, 2), (large, D4, 3)):
            dep.same_words(_run_stack(graph, planes, scales, edge, iters), want, "on a second stream")
    finally:
        _abi.set_stream(0)


def test_the_call_info(hip):
    """iters, and a launch count that is the same at B = 1 and B = 3: per iteration an init, the rounds of one model and
    a final, from the second on a q pass and an accumulation, one q pass at the start, and one more with its
    accumulation for the flux."""
    H, W = 12, 20
    rounds = len(bin(H * W - 1)) - 2                              # ceil(log2(H W))
    rake = 2 + 2 * (int(np.ceil(np.log2(np.float32(H * W)) / np.float32(2.0))) + 1)
    for iters in (1, 4):
        counts = []
        for B in (1, 3):
            graph, planes, scales, want = _stack(H, W, B, D8, iters)
            dep.same_words(_run_stack(graph, planes, scales, D8, iters), want, "B = %d" % B)
            i = _info()
            assert i["iters"] == iters and i["chunks"] == 1 and i["scratch_bytes"] >= 56 * B * H * W
            counts.append(i["launches"])
            _run_stack(graph, planes, scales, D8, iters, want=("out",))
            assert _info()["launches"] == i["launches"] - 1 - rake, "without the flux: a q pass and an accumulation less"
        assert counts[0] == counts[1] == 1 + iters * (2 + rounds) + (iters - 1) * (1 + rake) + 1 + rake


# ------------------------------------------------------------------ the batch methods

def test_the_batch_methods_against_the_module_calls(hip, oracle):
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    B, H, W = 3, 32, 32
    p = product_param(script_param(oracle.default_param()))
    p.maxage = 64
    scales = [(20.0 / H * (1 + b), 20.0 / W, 4.0) for b in range(B)]
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    uplift = to_gpu((np.random.default_rng(2).random((B, H, W)) * 1e-3).astype(np.float32))
    ones = to_gpu(np.ones((B, H, W), np.float32))
    dt, K, m, G, iters = 25.0, 1e-2, 0.4, 1.5, 5
    for scale in ((20.0 / H, 20.0 / W, 4.0), scales):
        bt = ErosionBatch(B, H, W, scale, p, 256, [11 + 7 * b for b in range(B)])
        bt.set_layers(to_gpu(layers))
        silt.set(bt.rainfall, 1.0)
        bt.step()
        before = to_np(bt.height).copy()
        got, flux, res = bt.stream_power_deposit(dt, K, m, G, iters, uplift=uplift, flux=True, residual=True)
        got_d4 = bt.stream_power_deposit(dt, K, edge=D4)
        assert (to_np(bt.height) == before).all(), "the batch's own state is not touched"
        pairs = [list(s[:2]) for s in scales] if scale is scales else [list(scale[:2])] * B
        for edge, mm, GG, it, u, out in ((D8, m, G, iters, uplift, got), (D4, 0.5, 1.0, 8, None, got_d4)):
            filled, graph = soil.condition_batch(bt.height, edge)
            area = soil.accumulate_batch(graph, ones, edge)
            cell = to_gpu(np.array([s[0] * s[1] for s in pairs], np.float32).reshape(B, 1, 1))
            hand = soil.stream_power_deposit_batch(filled, graph, soil.erosivity(area, K, mm), soil.deposition(area, GG, cell),
                                                   edge, pairs, dt, u, it, flux=True, residual=True)
            assert (dref.words(to_np(out)) == dref.words(to_np(hand[0]))).all(), "edge %d" % edge
            if edge == D8:
                assert (dref.words(to_np(flux)) == dref.words(to_np(hand[1]))).all()
                assert (dref.words(to_np(res)) == dref.words(to_np(hand[2]))).all() and to_np(res).shape == (B,)
                assert np.isfinite(to_np(out)).all() and (to_np(flux) != 0).any()
        # evolve: with G the deposit step, without it today's stream-power step, then the diffusion either way
        path = [list(s[:2]) for s in scales] if scale is scales else list(scale[:2])
        carved = bt.stream_power_deposit(dt, K, m, G, iters, uplift=uplift)
        want = soil.diffuse_batch(carved, path, dt, 0.05, border="fixed", first_axis=1)
        assert (dref.words(to_np(bt.evolve(dt, K, m, 0.05, uplift, first_axis=1, G=G, iters=iters))) == dref.words(to_np(want))).all()
        plain = soil.diffuse_batch(bt.stream_power(dt, K, m, uplift=uplift), path, dt, 0.05, border="fixed")
        assert (dref.words(to_np(bt.evolve(dt, K, m, 0.05, uplift))) == dref.words(to_np(plain))).all()
        assert (to_np(want) != to_np(soil.diffuse_batch(bt.stream_power(dt, K, m, uplift=uplift), path, dt, 0.05, first_axis=1))).any()


if __name__ == "__main__":
    _child_main(sys.argv[1])
