"""The erosion-deposition step at a slope exponent above 1 on the device (include/soil_hip.h: soil_stream_power_deposit_n
and its _batch form; soillib_amd.soil.stream_power_deposit_n / _batch, ErosionBatch.stream_power_deposit_n and
evolve_deposit), bit for bit against solve_iterated of tests/deposit_n_ref.py with the power taken from the device's own
function (soil_selftest_math64 op 0): every comparison is of the words of out (float32), out64 (float64), flux
(float32) and residual (float64), the NaN words included; there is no tolerance.

  shapes     12x20 (the 16-byte q and init passes), 13x21 (the scalar ones), 5x1028 and 3x261 (two work-groups along a
             row in both passes); D4 and D8
  graphs     a chain through every cell, the oracle's steepest graph of a conditioned terrain with a filled lake,
             cycles, entries that are no edge
  settings   n 1.5, 2, 2.5 and 3, iters 1, 3 and 8, with and without uplift, each output alone and all together
  inputs     a G / A deposition plane, a plane of zeros and one with a single huge entry; a NaN height on a terminal and
             in mid-chain, erosivity 0, planes 4 bytes off their alignment
  identities zero deposition against soil.stream_power_n, n == 1 against soil.stream_power_deposit, n == 2 without any
             power
  batches    3 x 12x20 with one pair and with a pair per model against the single calls; in a child process under
             SOIL_PATHS_GROUPS = 3, whole and in chunks of 2 + 1; a second stream
  plumbing   the residual where the largest change lies in another work-group than the first, the call info
  methods    ErosionBatch.stream_power_deposit_n and evolve_deposit against the module calls chained by hand
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import deposit_n_ref as dn
import downstream_ref as dref
import flats_ref
import flow_paths_ref as ref
from flow_paths_ref import D4, D8
from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(12, 20), (13, 21), (5, 1028), (3, 261)]
SCALES = [(0.3, 0.7), (1.0, 1.0), (2.5, 0.125)]
EXPONENTS = (1.5, 2.0, 2.5, 3.0)
COUNTS = (1, 3, 8)
DEPOSITS = ("area", "zero", "huge")
DT = 10.0
ALL = ("out", "out64", "flux", "residual")


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


def _run(graph, edge, height, erosivity, deposition, scale, n, dt=DT, uplift=None, iters=3, want=ALL):
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
    fn = lib.soil_stream_power_deposit_n if len(shape) == 2 else lib.soil_stream_power_deposit_n_batch
    _abi.check(fn(*[_ptr(outs[k]) for k in ALL], *[_ptr(p) for p in planes], *shape, edge, *tail, float(dt), float(n),
                  int(iters), _abi.stream()))
    return {k: to_np(v) for k, v in outs.items() if v is not None}


def _info():
    from soillib_amd import soil
    return soil.stream_power_deposit_n_info()


# ------------------------------------------------------------------ inputs and references, made once

@functools.lru_cache(maxsize=None)
def _conditioned(H, W, edge):
    """A noise terrain x 100 with a basin pressed into it, conditioned on the CPU: the filled surface, its steepest
    graph (the oracle's) with the flats routed (flats_ref), and the drainage area."""
    o = _oracle()
    dem = (o.noise(H, W, seed=5.0, ext=(float(H), float(W))) * 100).astype(np.float32)
    dem[max(1, H // 3):min(H - 1, 2 * H // 3 + 1), W // 4:3 * W // 4] -= np.float32(40.0)   # inside the border
    filled = o.fill_depressions(dem, edge)
    g = o.steepest(filled, edge)
    g = flats_ref.receivers(g, filled, flats_ref.distance_bfs(filled, edge), edge)
    r = g.reshape(-1)
    level = (r >= 0) & (filled.reshape(-1) == filled.reshape(-1)[np.where(r >= 0, r, 0)])
    assert level.sum() >= 8, "the terrain has a filled lake"
    area = o.accumulate(g, np.ones((H, W), np.float32), edge)
    for p in (filled, g, area):
        p.setflags(write=False)
    return filled, g, area


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
    """The conditioned graph takes its own filled surface; any other a height of terrain * 10, under which about half
    the receivers lie above their donors.  An erosivity over 1e-3 .. 10, an uplift in [0, 0.01], and the three
    deposition planes: (1 + draw) / A of the conditioned graph's area, zeros, and G / A with one entry of 3e38."""
    r = np.random.default_rng([draw, H, W])
    height = _conditioned(H, W, edge)[0] if gname == "conditioned" else (ref.terrain(H, W, 2 + draw) * 10).astype(np.float32)
    area = (np.float32(1.0 + draw) / _conditioned(H, W, edge)[2]).astype(np.float32)
    huge = area.copy()
    huge.reshape(-1)[(H * W) // 2 + 1] = np.float32(3e38)
    out = dict(height=height, erosivity=np.exp(r.uniform(np.log(1e-3), np.log(10.0), (H, W))).astype(np.float32),
               uplift=(r.random((H, W)) * 0.01).astype(np.float32), area=area, zero=np.zeros((H, W), np.float32), huge=huge)
    for p in out.values():
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(H, W, edge, gname, scale, draw, uplift, dname, n, iters, power="device"):
    """The restatement with the device's own power, every iteration count from one run.  power None: no power."""
    p = _planes(H, W, edge, gname, draw)
    return dn.solve_iterated(_oracle(), _graphs(H, W, edge)[gname], edge, p["height"], p["erosivity"], p[dname], scale, DT,
                             n, p["uplift"] if uplift else None, iters, device_pow if power == "device" else None,
                             every=True)


def _got(H, W, edge, gname, scale, draw, uplift, dname, n, iters, **kw):
    p = _planes(H, W, edge, gname, draw)
    return _run(_graphs(H, W, edge)[gname], edge, p["height"], p["erosivity"], p[dname], scale, n, DT,
                p["uplift"] if uplift else None, iters, **kw)


# ------------------------------------------------------------------ against the restatement

OUTPUTS = (ALL, ("out",), ("out64",), ("out", "flux"), ("out64", "residual"), ("out", "out64"))


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
def test_single_grid_against_the_restatement(hip, H, W, edge):
    """Every graph with every exponent, the iteration counts 1, 3 and 8 from one run of the restatement; the scale, the
    draw, the uplift, the deposition plane and the outputs asked for change from case to case."""
    k = 0
    for gname in sorted(_graphs(H, W, edge)):
        for n in EXPONENTS:
            scale, draw, uplift, dname = SCALES[k % 3], k % 2, k % 2 == 0, DEPOSITS[(k + k // 4) % 3]
            steps = _want(H, W, edge, gname, scale, draw, uplift, dname, n, max(COUNTS))["steps"]
            for j, iters in enumerate(COUNTS):
                outs = OUTPUTS[(k + 2 * j) % len(OUTPUTS)]
                got = _got(H, W, edge, gname, scale, draw, uplift, dname, n, iters, want=outs)
                assert sorted(got) == sorted(outs)
                dn.same_words(got, steps[iters - 1], "%s %s n %g iters %d, %dx%d edge %d" % (gname, dname, n, iters, H, W, edge))
                i = _info()
                assert i["iters"] == iters and i["chunks"] == 1
            last = steps[-1]
            if gname == "cycles":
                assert np.isnan(last["out64"]).any() and np.isfinite(last["out64"]).any()
            if gname == "conditioned":
                assert last["final"].all() and np.isfinite(last["out64"]).all() and steps[0]["residual"] > 0
                assert (last["flux"] != 0).any()
            k += 1


def test_the_cases_are_what_they_say(hip):
    """Every deposition plane meets the conditioned graph and another one; the huge entry sits on a cell with an edge;
    the G / A plane moves the result away from the zero plane's."""
    seen = set()
    for H, W in SHAPES[:2]:
        k = 0
        for gname in sorted(_graphs(H, W, D8)):
            for n in EXPONENTS:
                seen.add((gname == "conditioned", DEPOSITS[(k + k // 4) % 3]))
                k += 1
        p = _planes(H, W, D8, "conditioned", 0)
        g = _graphs(H, W, D8)["conditioned"]
        assert g.reshape(-1)[int(np.argmax(p["huge"]))] >= 0
        a = _want(H, W, D8, "conditioned", SCALES[1], 0, True, "area", 2.0, 3)["steps"][-1]
        z = _want(H, W, D8, "conditioned", SCALES[1], 0, True, "zero", 2.0, 3)["steps"][-1]
        assert np.abs(a["out64"] - z["out64"]).max() > 1e-3
    assert seen == {(c, d) for c in (True, False) for d in DEPOSITS}


@pytest.mark.parametrize("H,W", [(12, 20), (13, 21)])
def test_n_equal_two_needs_no_power(hip, H, W):
    """P = S: the restatement without any power gives the device's words, so no power — the device's own or one that
    would differ from it — is consulted at n == 2."""
    for edge in (D4, D8):
        for gname in ("conditioned", "serpentine"):
            case = (H, W, edge, gname, SCALES[0], 1, True, "area", 2.0, 3)
            want = _want(*case, power=None)
            dn.same_words(_got(*case), want, "P = S, %s %dx%d edge %d" % (gname, H, W, edge))
            p = _planes(H, W, edge, gname, 1)
            other = dn.solve_iterated(_oracle(), _graphs(H, W, edge)[gname], edge, p["height"], p["erosivity"], p["area"],
                                      SCALES[0], DT, 2.0, p["uplift"], 3, pow=lambda S, e: S * 1.5)
            dn.same_words(other, want, "a power that differs is not consulted")


@pytest.mark.parametrize("H,W", [(12, 20), (13, 21)])
def test_voids_and_erosivity_zero(hip, H, W):
    o = _oracle()
    for edge in (D4, D8):
        filled, g, area = _conditioned(H, W, edge)
        p = _planes(H, W, edge, "conditioned", 0)
        terminal = ref.walk_serial(g, edge)[0].reshape(-1)
        # a NaN height in mid-chain: the cell and everything upstream of it; the flux stays finite
        h = filled.copy()
        mid = int(np.argmax(np.where((area > 4) & (g >= 0) & (area < area.max()), area, 0)))
        h.reshape(-1)[mid] = np.nan
        want = dn.solve_iterated(o, g, edge, h, p["erosivity"], p["area"], SCALES[0], DT, 2.5, p["uplift"], 3, device_pow)
        marks = np.isnan(h).astype(np.float32)
        way = dref.solve_doubling(g, edge, a=marks, t=marks)[1] != 0
        assert (np.isnan(want["out64"]) == way).all() and 4 < way.sum() < H * W
        assert np.isfinite(want["residual"]) and np.isfinite(want["flux"]).all()
        dn.same_words(_run(g, edge, h, p["erosivity"], p["area"], SCALES[0], 2.5, DT, p["uplift"], 3), want, "a void in mid-chain")
        # on a terminal: its whole basin
        h = filled.copy()
        t = int(terminal[mid])
        h.reshape(-1)[t] = np.nan
        want = dn.solve_iterated(o, g, edge, h, p["erosivity"], p["area"], SCALES[0], DT, 1.5, None, 3, device_pow)
        assert (np.isnan(want["out64"]).reshape(-1) == (terminal == t)).all() and (terminal == t).sum() > 4
        dn.same_words(_run(g, edge, h, p["erosivity"], p["area"], SCALES[0], 1.5, DT, None, 3), want, "a void on a terminal")
        # erosivity 0: the lifted heights, the terminals their own — to the rounding of ((1 + g) b) / (1 + g), and to
        # the bit without deposition; nothing is removed, so next to nothing flows
        zero = np.zeros((H, W), np.float32)
        lifted = np.where(g >= 0, filled.astype(np.float64) + DT * p["uplift"].astype(np.float64), filled)
        for dname in ("area", "zero"):
            want = dn.solve_iterated(o, g, edge, filled, zero, p[dname], SCALES[0], DT, 2.5, p["uplift"], 3, device_pow)
            bound = 0.0 if dname == "zero" else 2.0 ** -51 * np.abs(lifted).max()
            assert np.abs(want["out64"] - lifted).max() <= bound and want["residual"] <= bound
            assert np.abs(want["flux"]).max() <= H * W * bound
            dn.same_words(_run(g, edge, filled, zero, p[dname], SCALES[0], 2.5, DT, p["uplift"], 3), want, "erosivity 0, " + dname)


# ------------------------------------------------------------------ the identities, on the device

@pytest.mark.parametrize("H,W", [(12, 20), (13, 21), (5, 1028)])
def test_zero_deposition_is_the_library_s_stream_power_n(hip, H, W):
    from soillib_amd import soil
    for edge in (D4, D8):
        for gname, g in sorted(_graphs(H, W, edge).items()):
            p = _planes(H, W, edge, gname, 1)
            assert not ((p["height"] == 0) & np.signbit(p["height"])).any(), "no b == -0.0, the identity's one exception"
            h, k, u, z, graph = (to_gpu(p["height"]), to_gpu(p["erosivity"]), to_gpu(p["uplift"]), to_gpu(p["zero"]), to_gpu(g))
            for uplift, n, iters, dbl in ((None, 1.5, 1, False), (u, 2.0, 3, True), (u, 2.5, 8, False)):
                want, wres = soil.stream_power_n(h, graph, k, edge, SCALES[0], DT, n, uplift, None, iters, dbl, True)
                got, gres = soil.stream_power_deposit_n(h, graph, k, z, edge, SCALES[0], DT, n, uplift, iters, dbl, residual=True)
                got, want = to_np(got), to_np(want)
                assert got.dtype == want.dtype and (dref.words(got) == dref.words(want)).all(), (gname, edge, n, iters, dbl)
                assert (dref.words(to_np(gres)) == dref.words(to_np(wres))).all()


@pytest.mark.parametrize("H,W", [(12, 20), (13, 21), (5, 1028)])
def test_n_equal_one_is_the_library_s_deposit_step(hip, H, W):
    from soillib_amd import soil
    for edge in (D4, D8):
        for gname, g in sorted(_graphs(H, W, edge).items()):
            p = _planes(H, W, edge, gname, 1)
            h, k, u, d, graph = (to_gpu(p["height"]), to_gpu(p["erosivity"]), to_gpu(p["uplift"]), to_gpu(p["area"]), to_gpu(g))
            for uplift, iters, dbl in ((None, 1, False), (u, 3, True)):
                want = soil.stream_power_deposit(h, graph, k, d, edge, SCALES[0], DT, uplift, iters, dbl, True, True)
                launches = soil.stream_power_deposit_info()["launches"]
                got = soil.stream_power_deposit_n(h, graph, k, d, edge, SCALES[0], DT, 1.0, uplift, iters, dbl, True, True)
                for a, b in zip(got, want):
                    a, b = to_np(a), to_np(b)
                    assert a.dtype == b.dtype and (dref.words(a) == dref.words(b)).all(), (gname, edge, iters, dbl)
                assert _info()["iters"] == iters and _info()["launches"] == launches, "its iterations and nothing else"


def test_the_residual_of_a_change_in_another_work_group(hip):
    """48 x 64: twelve work-groups of the final pass.  Without erosivity in the first four rows — the first
    work-group's 256 cells — nothing is removed there, and nothing drains into a row of heads: the maximum comes from
    another work-group."""
    H, W, edge = 48, 64, D8
    filled, g, area = _conditioned(H, W, edge)
    p = _planes(H, W, edge, "conditioned", 0)
    k = p["erosivity"].copy()
    k[:4] = 0
    d = p["area"].copy()
    d[:4] = 0                                                 # (what drains in from rows below would be deposited)
    o = _oracle()
    for n, iters in ((1.5, 1), (2.0, 2), (2.5, 3)):
        steps = dn.solve_iterated(o, g, edge, filled, k, d, SCALES[1], DT, n, p["uplift"], iters, device_pow, every=True)["steps"]
        before = dref.solve_doubling(g, edge, scale=SCALES[1], power=(filled, k, p["uplift"], DT))[1] if iters == 1 else steps[-2]["out64"]
        change = np.abs(steps[-1]["out64"] - before).reshape(-1)
        assert change[:256].max() == 0 and np.argmax(change) >= 256 and change.max() == steps[-1]["residual"] > 0
        dn.same_words(_run(g, edge, filled, k, d, SCALES[1], n, DT, p["uplift"], iters), steps[-1], "n %g iters %d" % (n, iters))


# ------------------------------------------------------------------ batches

def _stack(H, W, B, edge, n, iters, uplift=True):
    """graph, planes (a dict), the scales and the reference of B models: neighbours differ in graph, scale, draw and
    deposition plane."""
    names = sorted(_graphs(H, W, edge))
    cfg = [(names[(b + 1) % len(names)], SCALES[b % 3], b % 2, DEPOSITS[b % 3]) for b in range(B)]
    graph = np.stack([_graphs(H, W, edge)[g] for g, _, _, _ in cfg])
    planes = {k: np.stack([_planes(H, W, edge, g, d)[k] for g, _, d, _ in cfg]) for k in ("height", "erosivity", "uplift")}
    planes["deposition"] = np.stack([_planes(H, W, edge, g, d)[dname] for g, _, d, dname in cfg])
    wants = [_want(H, W, edge, g, s, d, uplift, dname, n, iters)["steps"][iters - 1] for g, s, d, dname in cfg]
    want = {k: np.stack([np.asarray(w[k]) for w in wants]) for k in ALL}
    return graph, planes, [s for _, s, _, _ in cfg], want


def _run_stack(graph, planes, scales, edge, n, iters, uplift=True, **kw):
    return _run(graph, edge, planes["height"], planes["erosivity"], planes["deposition"], scales, n, DT,
                planes["uplift"] if uplift else None, iters, **kw)


@pytest.mark.parametrize("edge", [D4, D8])
def test_a_batch_equals_the_single_calls(hip, edge):
    B, H, W, n, iters = 3, 12, 20, 2.5, 3
    graph, planes, scales, want = _stack(H, W, B, edge, n, iters)
    got = _run_stack(graph, planes, scales, edge, n, iters)
    dn.same_words(got, want, "a pair per model")
    for b in range(B):
        one = _run(graph[b], edge, planes["height"][b], planes["erosivity"][b], planes["deposition"][b], scales[b], n, DT,
                   planes["uplift"][b], iters)
        dn.same_words({k: got[k][b] for k in ALL}, {k: one[k].reshape(got[k][b].shape) for k in ALL}, "model %d alone" % b)
    got = _run_stack(graph, planes, SCALES[1], edge, n, iters, uplift=False)
    for b in range(B):
        w = dn.solve_iterated(_oracle(), graph[b], edge, planes["height"][b], planes["erosivity"][b], planes["deposition"][b],
                              SCALES[1], DT, n, None, iters, device_pow)
        dn.same_words({k: got[k][b] for k in ALL}, w, "one pair, model %d" % b)


CHUNK_SHAPES = [(12, 20), (13, 21)]
CHILD = (2.5, 3)                                              # n, iters


def _child_main(path):
    """The child of test_chunking_does_not_show: B = 3 whole and as chunks of 2 + 1 models, every output given; then
    the uplift and the side outputs NULL over the two chunks against the single calls."""
    out = {}
    for H, W in CHUNK_SHAPES:
        for models in (2, 0):
            if models:
                os.environ["SOIL_FLOW_BATCH_CELLS"] = str(2 * H * W + H * W // 2)
            else:
                os.environ.pop("SOIL_FLOW_BATCH_CELLS", None)
            for edge in (D4, D8):
                graph, planes, scales, want = _stack(H, W, 3, edge, *CHILD)
                key = "%dx%d_m%d_e%d_" % (H, W, models, edge)
                for k, v in _run_stack(graph, planes, scales, edge, *CHILD).items():
                    out[key + k] = v
                for k in ALL:                                     # (the device's power is the child's to ask for)
                    out[key + "want_" + k] = want[k]
                i = _info()
                out[key + "info"] = np.array([i["chunks"], i["iters"], i["launches"]])
    H, W = CHUNK_SHAPES[0]
    graph, planes, scales, _ = _stack(H, W, 3, D8, *CHILD)
    for null in (("uplift", "out64", "flux"), ("out", "residual")):
        kw = dict(uplift="uplift" not in null, want=tuple(k for k in ALL if k not in null))
        os.environ["SOIL_FLOW_BATCH_CELLS"] = str(2 * H * W + H * W // 2)
        got = _run_stack(graph, planes, scales, D8, *CHILD, **kw)
        assert _info()["chunks"] == 2 and sorted(got) == sorted(kw["want"])
        del os.environ["SOIL_FLOW_BATCH_CELLS"]
        for b in range(3):
            one = _run_stack(graph[b], {k: v[b] for k, v in planes.items()}, scales[b], D8, *CHILD, **kw)
            dn.same_words({k: v[b] for k, v in got.items()}, {k: v.reshape(got[k][b].shape) for k, v in one.items()},
                          "without %s, model %d" % (null, b))
    np.savez(path, **out)


def test_chunking_does_not_show(hip, tmp_path):
    """A 3-model batch in one fresh child process under SOIL_PATHS_GROUPS = 3 (read once per process), whole and in
    chunks of 2 + 1 models (SOIL_FLOW_BATCH_CELLS): the restatement's words every time, the second chunk's planes are
    its own part of each, and what is not given stays not given."""
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
            for models in (2, 0):
                key = "%dx%d_m%d_e%d_" % (H, W, models, edge)
                dn.same_words({k: got[key + k] for k in ALL}, {k: got[key + "want_" + k] for k in ALL}, key)
                chunks, iters, _ = got[key + "info"].tolist()
                assert (chunks, iters) == ({2: 2, 0: 1}[models], CHILD[1])
            # and the restatement the child compared with is this process's own
            dn.same_words({k: got[key + "want_" + k] for k in ALL}, _stack(H, W, 3, edge, *CHILD)[3], "the child's reference")


def test_planes_off_their_16_bytes(hip):
    """Each input plane in turn 4 bytes past a 16-byte boundary, W % 4 == 0: the scalar q and init passes take the call
    and give what the 16-byte ones give; outputs off their alignment do not matter."""
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
    names = ("height", "graph", "erosivity", "deposition", "uplift")
    host = dict(planes, graph=graph)
    for off_name in names + (None,):
        out_off = 4 if off_name in ("graph", "deposition") else 0
        o32, o64 = placed(None, silt.float32, out_off), placed(None, silt.float64, 2 * out_off)
        fl, rs = placed(None, silt.float32, out_off), placed(None, silt.float64, 2 * out_off, B, (B,))
        d = {k: placed(host[k], silt.int32 if k == "graph" else silt.float32, 4 if k == off_name else 0) for k in names}
        _abi.check(hip.soil_stream_power_deposit_n_batch(o32.c_ptr, o64.c_ptr, fl.c_ptr, rs.c_ptr, *[d[k].c_ptr for k in names],
                                                         B, H, W, D8, pairs, B, DT, n, iters, _abi.stream()))
        dn.same_words(dict(out=to_np(o32), out64=to_np(o64), flux=to_np(fl), residual=to_np(rs)), want,
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
            dn.same_words(_run_stack(graph, planes, scales, edge, n, iters), want, "on a second stream")
    finally:
        _abi.set_stream(0)


def test_the_call_info(hip):
    """The launches are the start's solve (an init, the rounds of one model, a final), `iters` times a q pass, an
    accumulation and a solve, and with the flux a q pass and an accumulation more.  The deposit step at iters + 1
    iterations launches iters + 1 solves, iters + 1 accumulations (the flux's among them) and one q pass more, the one
    that makes its x^0: this call's launches are its launches less one — the same at B = 1 and B = 3.  Without the
    flux, a q pass and an accumulation less.  The scratch is the deposit step's own: the entries share their slots."""
    from soillib_amd import soil
    H, W, n = 12, 20, 2.5
    for iters in (1, 4):
        for B in (1, 3):
            graph, planes, scales, want = _stack(H, W, B, D8, n, iters)
            dn.same_words(_run_stack(graph, planes, scales, D8, n, iters), want, "B = %d" % B)
            i = _info()
            dev = {k: to_gpu(v) for k, v in planes.items()}
            soil.stream_power_deposit_batch(dev["height"], to_gpu(graph), dev["erosivity"], dev["deposition"], D8, scales,
                                            DT, dev["uplift"], iters + 1, False, True, True)
            more = soil.stream_power_deposit_info()
            soil.stream_power_deposit_batch(dev["height"], to_gpu(graph), dev["erosivity"], dev["deposition"], D8, scales,
                                            DT, dev["uplift"], iters + 2, False, True, True)
            rake = soil.stream_power_deposit_info()["launches"] - more["launches"] - (3 + _rounds(H, W))
            assert rake > 0, "an iteration more is a q pass, an accumulation and a solve of 2 + rounds launches"
            assert (i["iters"], i["chunks"]) == (iters, 1)
            assert i["launches"] == more["launches"] - 1
            assert i["scratch_bytes"] == more["scratch_bytes"]
            without = _run_stack(graph, planes, scales, D8, n, iters, want=("out",))
            assert sorted(without) == ["out"] and _info()["launches"] == i["launches"] - 1 - rake


def _rounds(H, W):
    """The rounds of one model: ceil(log2(H W))."""
    return len(bin(H * W - 1)) - 2


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
    dt, K, m, G, n, iters = 25.0, 1e-2, 0.4, 0.8, 2.0, 5
    same = lambda a, b: (dref.words(to_np(a)) == dref.words(to_np(b))).all()
    for scale in ((20.0 / H, 20.0 / W, 4.0), scales):
        bt = ErosionBatch(B, H, W, scale, p, 256, [11 + 7 * b for b in range(B)])
        bt.set_layers(to_gpu(layers))
        silt.set(bt.rainfall, 1.0)
        bt.step()
        before = to_np(bt.height).copy()
        got, flux, res = bt.stream_power_deposit_n(dt, K, m, G, n, iters, uplift=uplift, flux=True, residual=True)
        got_d4 = bt.stream_power_deposit_n(dt, K, edge=D4, n=1.5)
        assert (to_np(bt.height) == before).all(), "the batch's own state is not touched"
        pairs = [list(s[:2]) for s in scales] if scale is scales else [list(scale[:2])] * B
        cell = to_gpu(np.array([s[0] * s[1] for s in pairs], np.float32).reshape(B, 1, 1))
        for edge, mm, GG, nn, it, u, out in ((D8, m, G, n, iters, uplift, got), (D4, 0.5, 1.0, 1.5, soil.DEPOSIT_N_ITERS, None, got_d4)):
            filled, graph = soil.condition_batch(bt.height, edge)
            area = soil.accumulate_batch(graph, ones, edge)
            hand = soil.stream_power_deposit_n_batch(filled, graph, soil.erosivity(area, K, mm), soil.deposition(area, GG, cell),
                                                     edge, pairs, dt, nn, u, it, flux=True, residual=True)
            assert same(out, hand[0]), "edge %d" % edge
            if edge == D8:
                assert same(flux, hand[1]) and same(res, hand[2]) and to_np(res).shape == (B,)
                assert np.isfinite(to_np(out)).all()
                plain = bt.stream_power(dt, K, m, uplift=uplift, n=n, iters=iters)
                assert (to_np(out) != to_np(plain)).any(), "the deposition shows"
        # evolve_deposit: the step, the collapse where asked for, the diffusion
        path = [list(s[:2]) for s in scales] if scale is scales else list(scale[:2])
        carved = bt.stream_power_deposit_n(dt, K, m, G, n, iters, uplift=uplift)
        want = soil.diffuse_batch(carved, path, dt, 0.05, border="fixed", first_axis=1)
        assert same(bt.evolve_deposit(dt, K, G, n, m, 0.05, None, uplift, iters, first_axis=1), want)
        want = soil.diffuse_batch(soil.slope_limit_batch(carved, path, 0.6, D8), path, dt, 0.05, border="fixed")
        assert same(bt.evolve_deposit(dt, K, G, n, m, 0.05, 0.6, uplift, iters), want)
        with pytest.raises(ValueError, match=r"ErosionBatch\.evolve: G \(deposition\) takes the slope exponent n = 1 only"):
            bt.evolve(dt, K, m, 0.05, uplift, G=1, n=2)


if __name__ == "__main__":
    _child_main(sys.argv[1])
