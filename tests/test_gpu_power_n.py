"""The stream-power step with a slope exponent above 1 on the device (include/soil_hip.h: soil_stream_power_n and its
_batch form, soil_selftest_math64; soillib_amd.soil.stream_power_n / _batch, ErosionBatch.stream_power(n=...) and
evolve(n=...)), bit for bit against solve_iterated of tests/power_n_ref.py with the power taken from the device's own
function (soil_selftest_math64 op 0): every comparison with it is of the words of out (float32), out64 (float64) and
residual (float64), the NaN words included; there is no tolerance.  The power function itself is held to np.power.

  shapes     12x20 (the 16-byte init pass), 13x21 (the scalar one), 5x1028 and 3x261 (two work-groups along a row in the
             new init pass: 257 threads a row in the 16-byte form, 261 in the scalar one); D4 and D8
  graphs     a chain through every cell (under heights that put many a receiver above its donor), the oracle's
             steepest graph of a conditioned terrain with a filled lake, cycles, entries that are no edge
  settings   n 1.5, 2 and 2.5, iters 1, 3 and 8, with and without uplift and stop, out, out64 and both
  inputs     a NaN height on a terminal and in mid-chain, erosivity 0, planes 4 bytes off their alignment
  identities n == 2 without any power, n == 1 against soil.stream_power of the library itself
  batches    3 x 12x20 with one pair and with a pair per model against the single calls; in a child process under
             SOIL_PATHS_GROUPS = 3, whole and in chunks of 2 + 2 + 1; a second stream
  plumbing   the residual where the largest change lies in another work-group than the first, the call info
  methods    ErosionBatch.stream_power(n=2) and evolve(n=2) against the module calls chained by hand
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import downstream_ref as dref
import flats_ref
import flow_paths_ref as ref
import power_n_ref as pn
from flow_paths_ref import D4, D8
from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(12, 20), (13, 21), (5, 1028), (3, 261)]
SCALES = [(0.3, 0.7), (1.0, 1.0), (2.5, 0.125)]
EXPONENTS = (1.5, 2.0, 2.5)
COUNTS = (1, 3, 8)
DT = 10.0
ALL = ("out", "out64", "residual")


def _oracle():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


def _ptr(t):
    return None if t is None else t.c_ptr


def device_pow(S, e):
    """soil_selftest_math64 op 0 on two float64 arrays of one shape: the power as the init pass evaluates it."""
    from soillib_amd import _abi, silt
    S, e = np.ascontiguousarray(S, np.float64), np.ascontiguousarray(e, np.float64)
    assert S.shape == e.shape
    out = silt.tensor(silt.float64, silt.shape(S.size), silt.gpu)
    a, b = to_gpu(S.reshape(-1)), to_gpu(e.reshape(-1))
    _abi.check(_abi.lib().soil_selftest_math64(out.c_ptr, a.c_ptr, b.c_ptr, S.size, 0, _abi.stream()))
    return to_np(out).reshape(S.shape)


def _run(graph, edge, height, erosivity, scale, n, dt=DT, uplift=None, stop=None, iters=3, want=ALL):
    """One call of the C ABI on numpy planes, (H, W) or (B, H, W) by the graph's rank: a dict of the outputs asked for
    (`want`) as numpy.  `scale`: one pair or B pairs."""
    from soillib_amd import _abi, silt
    lib = _abi.lib()
    graph = np.asarray(graph)
    shape = graph.shape
    B = 1 if len(shape) == 2 else shape[0]
    dev = lambda p: None if p is None else to_gpu(np.ascontiguousarray(p))
    planes = [dev(height), dev(graph), dev(erosivity), dev(uplift), dev(stop)]
    outs = dict(out=silt.tensor(silt.float32, silt.shape(*shape), silt.gpu) if "out" in want else None,
                out64=silt.tensor(silt.float64, silt.shape(*shape), silt.gpu) if "out64" in want else None,
                residual=to_gpu(np.full(B, -1.0, np.float64)) if "residual" in want else None)
    pairs = np.asarray(scale, np.float32).reshape(-1)
    sc = (C.c_float * len(pairs))(*pairs.tolist())
    tail = (sc,) if len(shape) == 2 else (sc, len(pairs) // 2)
    fn = lib.soil_stream_power_n if len(shape) == 2 else lib.soil_stream_power_n_batch
    _abi.check(fn(*[_ptr(outs[k]) for k in ALL], *[_ptr(p) for p in planes], *shape, edge, *tail, float(dt), float(n),
                  int(iters), _abi.stream()))
    return {k: to_np(v) for k, v in outs.items() if v is not None}


def _info():
    from soillib_amd import soil
    return soil.stream_power_n_info()


# ------------------------------------------------------------------ inputs and references, made once

@functools.lru_cache(maxsize=None)
def _conditioned(H, W, edge):
    """A noise terrain x 100 with a basin pressed into it, conditioned on the CPU: the filled surface and its steepest
    graph (the oracle's) with the flats routed (flats_ref)."""
    o = _oracle()
    dem = (o.noise(H, W, seed=5.0, ext=(float(H), float(W))) * 100).astype(np.float32)
    dem[max(1, H // 3):min(H - 1, 2 * H // 3 + 1), W // 4:3 * W // 4] -= np.float32(40.0)   # inside the border
    filled = o.fill_depressions(dem, edge)
    g = o.steepest(filled, edge)
    g = flats_ref.receivers(g, filled, flats_ref.distance_bfs(filled, edge), edge)
    r = g.reshape(-1)
    level = (r >= 0) & (filled.reshape(-1) == filled.reshape(-1)[np.where(r >= 0, r, 0)])
    assert level.sum() >= 8, "the terrain has a filled lake"
    filled.setflags(write=False)
    g.setflags(write=False)
    return filled, g


@functools.lru_cache(maxsize=None)
def _graphs(H, W, edge):
    built = dict(ref.built_graphs(H, W, edge))
    out = dict(serpentine=built["serpentine"], hostile=built["hostile"], conditioned=_conditioned(H, W, edge)[1])
    if "cycles" in built:
        out["cycles"] = built["cycles"]
    for g in out.values():
        g.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _planes(H, W, edge, gname, draw):
    """The conditioned graph takes its own filled surface; any other a height of terrain * 10, under which about
    half the receivers lie above their donors.  An erosivity over 1e-3 .. 10, an uplift in [0, 0.01], a stop plane
    with a few pour points."""
    r = np.random.default_rng([draw, H, W])
    height = _conditioned(H, W, edge)[0] if gname == "conditioned" else (ref.terrain(H, W, 2 + draw) * 10).astype(np.float32)
    stop = (r.random((H, W)) < 0.04).astype(np.int32) * 3
    out = dict(height=height, erosivity=np.exp(r.uniform(np.log(1e-3), np.log(10.0), (H, W))).astype(np.float32),
               uplift=(r.random((H, W)) * 0.01).astype(np.float32), stop=stop)
    for p in out.values():
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(H, W, edge, gname, scale, draw, uplift, stop, n, iters, power="device"):
    """The restatement with the device's own power, every iteration count from one run.  power None: no power."""
    p = _planes(H, W, edge, gname, draw)
    out = pn.solve_iterated(_graphs(H, W, edge)[gname], edge, p["height"], p["erosivity"], scale, DT, n,
                            p["uplift"] if uplift else None, p["stop"] if stop else None, iters,
                            device_pow if power == "device" else None, every=True)
    return out


def _got(H, W, edge, gname, scale, draw, uplift, stop, n, iters, **kw):
    p = _planes(H, W, edge, gname, draw)
    return _run(_graphs(H, W, edge)[gname], edge, p["height"], p["erosivity"], scale, n, DT,
                p["uplift"] if uplift else None, p["stop"] if stop else None, iters, **kw)


# ------------------------------------------------------------------ the power

def test_the_power_function_against_numpy(hip):
    """sp_pow within a relative 2^-50 of np.power for S from the denormals to 1e6 and e from 0.25 to 15 — where the
    result is itself a denormal, whose spacing 2^-1074 no relative bound can go below, within one such step —, exact
    at S = 0 and S = 1, NaN for a NaN, and any other op refused."""
    from soillib_amd import _abi
    S = np.concatenate([[5e-324, 1e-320, 2.2e-308, 2.3e-308], np.exp(np.linspace(np.log(1e-300), np.log(1e6), 4001)),
                        [0.5, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, 2.0, 1e6]])
    for e in (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.0, 7.3, 15.0):
        got, want = device_pow(S, np.full_like(S, e)), np.power(S, e)
        err = np.abs(got - want)
        ok = err <= np.maximum(2.0 ** -50 * want, np.where(want < 2.0 ** -1022, 2.0 ** -1074, 0.0))
        rel = np.where(want >= 2.0 ** -1022, err / np.maximum(want, 2.0 ** -1022), 0.0).max()
        print("e = %g: %.3g relative at most (2^-50 = %.3g)" % (e, rel, 2.0 ** -50))
        assert ok.all(), (e, S[~ok][:4], got[~ok][:4], want[~ok][:4])
    e = np.array([0.25, 0.5, 1.0, 1.5, 2.5, 15.0])
    assert (dref.words(device_pow(np.zeros(6), e)) == dref.words(np.zeros(6))).all(), "S = 0: +0"
    assert (device_pow(np.ones(6), e) == 1.0).all(), "S = 1"
    assert np.isnan(device_pow(np.full(6, np.nan), e)).all(), "a NaN in is a NaN out"
    a = to_gpu(np.ones(4))
    for op in (1, 2, 12, -1):
        assert hip.soil_selftest_math64(a.c_ptr, a.c_ptr, a.c_ptr, 4, op, _abi.stream()) == _abi.SOIL_ERR_INVALID_ARGUMENT
        assert _abi.last_error().startswith("selftest_math64: ")


# ------------------------------------------------------------------ against the restatement

@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
def test_single_grid_against_the_restatement(hip, H, W, edge):
    """Every graph with every exponent, the iteration counts 1, 3 and 8 from one run of the restatement; scale, draw,
    uplift, stop and the outputs asked for change from case to case."""
    k = 0
    for gname in sorted(_graphs(H, W, edge)):
        for n in EXPONENTS:
            scale, draw, uplift, stop = SCALES[k % 3], k % 2, k % 2 == 0, k % 3 == 1
            steps = _want(H, W, edge, gname, scale, draw, uplift, stop, n, max(COUNTS))["steps"]
            for j, iters in enumerate(COUNTS):
                outs = (("out", "out64", "residual"), ("out", "residual"), ("out64",))[(k + j) % 3]
                got = _got(H, W, edge, gname, scale, draw, uplift, stop, n, iters, want=outs)
                assert sorted(got) == sorted(outs)
                pn.same_words(got, steps[iters - 1], "%s n %g iters %d, %dx%d edge %d" % (gname, n, iters, H, W, edge))
                i = _info()
                assert i["iters"] == iters and i["chunks"] == 1
            last = steps[-1]
            if gname == "cycles":
                assert np.isnan(last["out64"]).any() and np.isfinite(last["out64"]).any()
            if gname == "conditioned" and not stop:
                assert last["final"].all() and np.isfinite(last["out64"]).all() and steps[0]["residual"] > 0
            k += 1


def test_the_cases_are_what_they_say(hip):
    """A receiver above its donor, entries that are no edge, the lake: in the inputs of the test above."""
    for H, W in SHAPES:
        p = _planes(H, W, D8, "serpentine", 0)
        g = _graphs(H, W, D8)["serpentine"].reshape(-1)
        h = p["height"].reshape(-1)
        has = g >= 0
        assert (h[g[has]] > h[has]).sum() > has.sum() // 4, "receivers above their donors"
        is_edge = pn.planes(_graphs(H, W, D8)["hostile"], D8, p["height"], p["erosivity"], (1, 1), DT)[0]
        assert (~is_edge).sum() > H * W // 4 and is_edge.sum() > H * W // 10
        assert p["stop"].any()


@pytest.mark.parametrize("H,W", [(12, 20), (13, 21)])
def test_n_equal_two_needs_no_power(hip, H, W):
    for edge in (D4, D8):
        for gname in ("conditioned", "serpentine"):
            case = (H, W, edge, gname, SCALES[0], 1, True, False, 2.0, 3)
            want = _want(*case, power=None)
            pn.same_words(_got(*case), want, "P = S, %s %dx%d edge %d" % (gname, H, W, edge))
            pn.same_words(want, _want(*case), "the device's pow(S, 1) is S")


@pytest.mark.parametrize("H,W", [(12, 20), (13, 21)])
def test_voids_and_erosivity_zero(hip, H, W):
    o = _oracle()
    for edge in (D4, D8):
        filled, g = _conditioned(H, W, edge)
        p = _planes(H, W, edge, "conditioned", 0)
        area = o.accumulate(g, np.ones((H, W), np.float32), edge)
        terminal = ref.walk_serial(g, edge)[0].reshape(-1)
        # a NaN height in mid-chain: the cell and everything upstream of it
        h = filled.copy()
        mid = int(np.argmax(np.where((area > 4) & (g >= 0) & (area < area.max()), area, 0)))
        h.reshape(-1)[mid] = np.nan
        want = pn.solve_iterated(g, edge, h, p["erosivity"], SCALES[0], DT, 2.5, p["uplift"], None, 3, device_pow)
        marks = np.isnan(h).astype(np.float32)
        way = dref.solve_doubling(g, edge, a=marks, t=marks)[1] != 0
        assert (np.isnan(want["out64"]) == way).all() and 4 < way.sum() < H * W and np.isfinite(want["residual"])
        pn.same_words(_run(g, edge, h, p["erosivity"], SCALES[0], 2.5, DT, p["uplift"], None, 3), want, "a void in mid-chain")
        # on a terminal: its whole basin
        h = filled.copy()
        t = int(terminal[mid])
        h.reshape(-1)[t] = np.nan
        want = pn.solve_iterated(g, edge, h, p["erosivity"], SCALES[0], DT, 1.5, None, None, 3, device_pow)
        assert (np.isnan(want["out64"]).reshape(-1) == (terminal == t)).all() and (terminal == t).sum() > 4
        pn.same_words(_run(g, edge, h, p["erosivity"], SCALES[0], 1.5, DT, None, None, 3), want, "a void on a terminal")
        # erosivity 0: the lifted heights, the terminals their own; nothing moves between the iterates
        zero = np.zeros((H, W), np.float32)
        want = pn.solve_iterated(g, edge, filled, zero, SCALES[0], DT, 2.5, p["uplift"], None, 3, device_pow)
        lifted = np.where(g >= 0, filled.astype(np.float64) + DT * p["uplift"].astype(np.float64), filled)
        assert (want["out64"] == lifted).all() and want["residual"] == 0
        pn.same_words(_run(g, edge, filled, zero, SCALES[0], 2.5, DT, p["uplift"], None, 3), want, "erosivity 0")


@pytest.mark.parametrize("H,W", [(12, 20), (13, 21), (5, 1028)])
def test_n_equal_one_is_the_library_s_stream_power(hip, H, W):
    from soillib_amd import soil
    for edge in (D4, D8):
        for gname, g in sorted(_graphs(H, W, edge).items()):
            p = _planes(H, W, edge, gname, 1)
            h, k, u, s, graph = (to_gpu(p["height"]), to_gpu(p["erosivity"]), to_gpu(p["uplift"]), to_gpu(p["stop"]), to_gpu(g))
            for uplift, stop, iters, dbl in ((None, None, 1, False), (u, s, 2, True), (u, None, 8, False)):
                want = to_np(soil.stream_power(h, graph, k, edge, SCALES[0], DT, uplift, stop, double=dbl))
                got, res = soil.stream_power_n(h, graph, k, edge, SCALES[0], DT, 1.0, uplift, stop, iters, dbl, True)
                got = to_np(got)
                assert got.dtype == want.dtype and (dref.words(got) == dref.words(want)).all(), (gname, edge, iters, dbl)
                assert dref.words(to_np(res)).tolist() == [0], "the residual of n = 1 is +0"
                assert _info()["iters"] == 0


def test_the_residual_of_a_change_in_another_work_group(hip):
    """48 x 64: twelve work-groups of the final pass.  Without erosivity in the first four rows — the first
    work-group's 256 cells — nothing changes there between the iterates, so the maximum comes from another one."""
    H, W, edge = 48, 64, D8
    filled, g = _conditioned(H, W, edge)
    p = _planes(H, W, edge, "conditioned", 0)
    k = p["erosivity"].copy()
    k[:4] = 0
    for n, iters in ((1.5, 1), (2.0, 2), (2.5, 3)):
        steps = pn.solve_iterated(g, edge, filled, k, SCALES[1], DT, n, p["uplift"], None, iters, device_pow, every=True)["steps"]
        before = dref.solve_doubling(g, edge, scale=SCALES[1], power=(filled, k, p["uplift"], DT))[1] if iters == 1 else steps[-2]["out64"]
        change = np.abs(steps[-1]["out64"] - before).reshape(-1)
        assert change[:256].max() == 0 and np.argmax(change) >= 256 and change.max() == steps[-1]["residual"] > 0
        pn.same_words(_run(g, edge, filled, k, SCALES[1], n, DT, p["uplift"], None, iters), steps[-1], "n %g iters %d" % (n, iters))


# ------------------------------------------------------------------ batches

def _stack(H, W, B, edge, n, iters, uplift=True, stop=True):
    """graph, planes (a dict), the scales and the reference of B models: neighbours differ in graph, scale and draw."""
    names = sorted(_graphs(H, W, edge))
    cfg = [(names[(b + 1) % len(names)], SCALES[b % 3], b % 2) for b in range(B)]
    graph = np.stack([_graphs(H, W, edge)[g] for g, _, _ in cfg])
    planes = {k: np.stack([_planes(H, W, edge, g, d)[k] for g, _, d in cfg]) for k in ("height", "erosivity", "uplift", "stop")}
    wants = [_want(H, W, edge, g, s, d, uplift, stop, n, iters)["steps"][iters - 1] for g, s, d in cfg]
    want = {k: np.stack([np.asarray(w[k]) for w in wants]) for k in ALL}
    return graph, planes, [s for _, s, _ in cfg], want


def _run_stack(graph, planes, scales, edge, n, iters, uplift=True, stop=True, **kw):
    return _run(graph, edge, planes["height"], planes["erosivity"], scales, n, DT, planes["uplift"] if uplift else None,
                planes["stop"] if stop else None, iters, **kw)


@pytest.mark.parametrize("edge", [D4, D8])
def test_a_batch_equals_the_single_calls(hip, edge):
    B, H, W, n, iters = 3, 12, 20, 2.5, 3
    graph, planes, scales, want = _stack(H, W, B, edge, n, iters)
    got = _run_stack(graph, planes, scales, edge, n, iters)
    pn.same_words(got, want, "a pair per model")
    for b in range(B):
        one = _run(graph[b], edge, planes["height"][b], planes["erosivity"][b], scales[b], n, DT, planes["uplift"][b],
                   planes["stop"][b], iters)
        pn.same_words({k: got[k][b] for k in ALL}, {k: one[k].reshape(got[k][b].shape) for k in ALL}, "model %d alone" % b)
    got = _run_stack(graph, planes, SCALES[1], edge, n, iters, uplift=False, stop=False)
    for b in range(B):
        w = pn.solve_iterated(graph[b], edge, planes["height"][b], planes["erosivity"][b], SCALES[1], DT, n, None, None,
                              iters, device_pow)
        pn.same_words({k: got[k][b] for k in ALL}, w, "one pair, model %d" % b)
        one = _run(graph[b], edge, planes["height"][b], planes["erosivity"][b], SCALES[1], n, DT, None, None, iters)
        pn.same_words({k: got[k][b] for k in ALL}, {k: one[k].reshape(got[k][b].shape) for k in ALL}, "one pair, model %d alone" % b)


CHUNK_SHAPES = [(12, 20), (13, 21)]
CHILD = (2.5, 3)                                              # n, iters


def _child_main(path):
    """The child of test_chunking_does_not_show: B = 5 whole and as chunks of 2 + 2 + 1 models."""
    out = {}
    for H, W in CHUNK_SHAPES:
        for models in (2, 0):
            if models:
                os.environ["SOIL_FLOW_BATCH_CELLS"] = str(2 * H * W + H * W // 2)
            else:
                os.environ.pop("SOIL_FLOW_BATCH_CELLS", None)
            for edge in (D4, D8):
                graph, planes, scales, want = _stack(H, W, 5, edge, *CHILD)
                key = "%dx%d_m%d_e%d_" % (H, W, models, edge)
                for k, v in _run_stack(graph, planes, scales, edge, *CHILD).items():
                    out[key + k] = v
                for k in ALL:                                     # (the device's power is the child's to ask for)
                    out[key + "want_" + k] = want[k]
                i = _info()
                out[key + "info"] = np.array([i["chunks"], i["iters"], i["launches"]])
    _child_optional()
    np.savez(path, **out)


# (H, W, SOIL_FLOW_BATCH_CELLS): B = 5 as 2 + 2 + 1 models, the 16-byte init passes and the scalar ones
OPTIONAL_SHAPES = [(8, 12, 192), (8, 10, 160)]
OPTIONAL_NULLS = [(), ("uplift", "stop", "out64"), ("out", "residual")]


def _child_optional():
    """The uplift, the stop plane and every output given and NULL over three chunks: from the second chunk on a plane
    is the chunk's part of it, and one that is not given must stay not given.  Five models that differ in every plane;
    the words of the five single-grid calls; raises."""
    n, iters = 2.5, 2
    for H, W, cells in OPTIONAL_SHAPES:
        built = dict(ref.built_graphs(H, W, D8))
        cfg = [(("serpentine", "hostile")[b % 2], b) for b in range(5)]
        graph = np.stack([built[g] for g, _ in cfg])
        planes = {k: np.stack([_planes(H, W, D8, g, d)[k] for g, d in cfg]) for k in ("height", "erosivity", "uplift", "stop")}
        scales = [SCALES[b % 3] for b in range(5)]
        for null in OPTIONAL_NULLS:
            kw = dict(uplift="uplift" not in null, stop="stop" not in null, want=tuple(k for k in ALL if k not in null))
            os.environ["SOIL_FLOW_BATCH_CELLS"] = str(cells)
            got = _run_stack(graph, planes, scales, D8, n, iters, **kw)
            assert _info()["chunks"] == 3 and sorted(got) == sorted(kw["want"]), (H, W, null, _info(), sorted(got))
            del os.environ["SOIL_FLOW_BATCH_CELLS"]
            for b in range(5):
                one = _run_stack(graph[b], {k: v[b] for k, v in planes.items()}, scales[b], D8, n, iters, **kw)
                pn.same_words({k: v[b] for k, v in got.items()}, one, "%dx%d without %s, model %d" % (H, W, null, b))


def test_chunking_does_not_show(hip, tmp_path):
    """A 5-model batch in one child process under SOIL_PATHS_GROUPS = 3 (read once per process: three work-groups a
    round, several trips each), whole and in chunks of 2 + 2 + 1 models (SOIL_FLOW_BATCH_CELLS): the restatement's
    words every time, and a chunk's launches do not depend on its models.  The child also holds the uplift, the stop
    plane and each output, given and NULL over three chunks, to the single-grid calls (_child_optional)."""
    path = str(tmp_path / "chunks.npz")
    env = dict(os.environ)
    for name in ("SOIL_FLOW_BATCH_CELLS", "SOIL_PATHS_LIST_FROM", "SOIL_PATHS_IDX64"):
        env.pop(name, None)
    env["SOIL_PATHS_GROUPS"] = "3"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    for H, W in CHUNK_SHAPES:
        for edge in (D4, D8):
            launches = {}
            for models in (2, 0):
                key = "%dx%d_m%d_e%d_" % (H, W, models, edge)
                pn.same_words({k: got[key + k] for k in ALL}, {k: got[key + "want_" + k] for k in ALL}, key)
                chunks, iters, launches[models] = got[key + "info"].tolist()
                assert (chunks, iters) == ({2: 3, 0: 1}[models], CHILD[1])
            assert launches[2] == 3 * launches[0]
            # and the restatement the child compared with is this process's own
            pn.same_words({k: got[key + "want_" + k] for k in ALL}, _stack(H, W, 5, edge, *CHILD)[3], "the child's reference")


def test_planes_off_their_16_bytes(hip):
    """Each input plane in turn 4 bytes past a 16-byte boundary, W % 4 == 0: the scalar init passes take the call and
    give what the 16-byte ones give; outputs off their alignment do not matter."""
    from soillib_amd import _abi, silt
    B, H, W, n, iters = 3, 12, 20, 1.5, 3
    graph, planes, scales, want = _stack(H, W, B, D8, n, iters)

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
    names = ("height", "graph", "erosivity", "uplift", "stop")
    host = dict(planes, graph=graph)
    for off_name in names + (None,):
        for out_off in (0, 4):
            o32, o64 = placed(None, silt.float32, out_off), placed(None, silt.float64, 2 * out_off)
            rs = placed(None, silt.float64, 2 * out_off, B, (B,))
            d = {k: placed(host[k], silt.int32 if k in ("graph", "stop") else silt.float32, 4 if k == off_name else 0)
                 for k in names}
            _abi.check(hip.soil_stream_power_n_batch(o32.c_ptr, o64.c_ptr, rs.c_ptr, *[d[k].c_ptr for k in names],
                                                     B, H, W, D8, pairs, B, DT, n, iters, _abi.stream()))
            pn.same_words(dict(out=to_np(o32), out64=to_np(o64), residual=to_np(rs)), want,
                          "%s off its 16 bytes, outputs %d" % (off_name, out_off))


def test_on_another_stream_twice_and_with_another_size_in_between(hip):
    import torch
    from soillib_amd import _abi
    small, large = _stack(13, 21, 3, D8, 2.0, 2), _stack(5, 1028, 2, D4, 2.5, 3)
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        for (graph, planes, scales, want), edge, n, iters in ((small, D8, 2.0, 2), (large, D4, 2.5, 3), (small, D8, 2.0, 2),
                                                              (small, D8, 2.0, 2), (large, D4, 2.5, 3)):
            pn.same_words(_run_stack(graph, planes, scales, edge, n, iters), want, "on a second stream")
    finally:
        _abi.set_stream(0)


def test_the_call_info(hip):
    """(iters + 1) solves' worth of launches — an init, the rounds of one model and a final each, the rounds as
    soil.downstream_info() reports them for soil.stream_power on the same shape — the same at B = 1 and B = 3; the
    scratch is the layout's: the scale records of a batch with a pair per model, two record buffers, two B planes, the
    lists of min(ceil(cells / 256), 8192) work-groups, their fills, 256 bytes of control words, and 8 bytes a cell for
    the iterate."""
    from soillib_amd import soil
    H, W, n = 12, 20, 2.5
    up = lambda v: (v + 255) // 256 * 256
    for iters in (1, 4):
        for B in (1, 3):
            graph, planes, scales, want = _stack(H, W, B, D8, n, iters)
            pn.same_words(_run_stack(graph, planes, scales, D8, n, iters), want, "B = %d" % B)
            i = _info()
            soil.stream_power_batch(to_gpu(planes["height"]), to_gpu(graph), to_gpu(planes["erosivity"]), D8, scales, DT)
            rounds = soil.downstream_info()["rounds"]
            assert rounds == len(bin(H * W - 1)) - 2
            assert (i["iters"], i["chunks"], i["launches"]) == (iters, 1, (iters + 1) * (2 + rounds))
            cells = B * H * W
            groups = min((cells + 255) // 256, 8192)
            seg = ((cells + groups - 1) // groups + 255) // 256 * 256
            layout = 2 * up(16 * cells) + 2 * up(8 * cells) + 2 * up(4 * seg * groups) + 2 * up(4 * groups) + 256
            assert i["scratch_bytes"] == up(8 * cells) + (up(24 * B) if B > 1 else 0) + layout


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
    dt, K, m, iters = 25.0, 1e-2, 0.4, 5
    for scale in ((20.0 / H, 20.0 / W, 4.0), scales):
        bt = ErosionBatch(B, H, W, scale, p, 256, [11 + 7 * b for b in range(B)])
        bt.set_layers(to_gpu(layers))
        silt.set(bt.rainfall, 1.0)
        bt.step()
        before = to_np(bt.height).copy()
        got, res = bt.stream_power(dt, K, m, uplift=uplift, n=2, iters=iters, residual=True)
        got_d4 = bt.stream_power(dt, K, edge=D4, n=1.5)
        plain = bt.stream_power(dt, K, m, uplift=uplift)
        assert (to_np(bt.height) == before).all(), "the batch's own state is not touched"
        pairs = [list(s[:2]) for s in scales] if scale is scales else [list(scale[:2])] * B
        for edge, mm, nn, it, u, out in ((D8, m, 2.0, iters, uplift, got), (D4, 0.5, 1.5, 8, None, got_d4)):
            filled, graph = soil.condition_batch(bt.height, edge)
            k = soil.erosivity(soil.accumulate_batch(graph, ones, edge), K, mm)
            hand = soil.stream_power_n_batch(filled, graph, k, edge, pairs, dt, nn, u, None, it, residual=True)
            assert (dref.words(to_np(out)) == dref.words(to_np(hand[0]))).all(), "edge %d" % edge
            if edge == D8:
                assert (dref.words(to_np(res)) == dref.words(to_np(hand[1]))).all() and to_np(res).shape == (B,)
                assert np.isfinite(to_np(out)).all() and (to_np(out) != to_np(plain)).any()
                same = soil.stream_power_batch(filled, graph, k, edge, pairs, dt, u)
                assert (dref.words(to_np(plain)) == dref.words(to_np(same))).all(), "n = 1 runs what it ran"
        # evolve: with n the Newton step, without it today's stream-power step, then the diffusion either way
        path = [list(s[:2]) for s in scales] if scale is scales else list(scale[:2])
        want = soil.diffuse_batch(got, path, dt, 0.05, border="fixed", first_axis=1)
        assert (dref.words(to_np(bt.evolve(dt, K, m, 0.05, uplift, first_axis=1, iters=iters, n=2))) == dref.words(to_np(want))).all()
        want = soil.diffuse_batch(plain, path, dt, 0.05, border="fixed")
        assert (dref.words(to_np(bt.evolve(dt, K, m, 0.05, uplift))) == dref.words(to_np(want))).all()
        with pytest.raises(ValueError, match=r"ErosionBatch\.evolve: G \(deposition\) takes the slope exponent n = 1 only"):
            bt.evolve(dt, K, m, 0.05, uplift, G=1, n=2)


if __name__ == "__main__":
    _child_main(sys.argv[1])
