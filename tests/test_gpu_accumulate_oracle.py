"""Flow accumulation (csrc/graph.hip: soil_accumulate, soil_multiflow) against the CPU oracle at the sizes it is
used at, bit for bit (util.assert_bit_equal, NaN for NaN), no tolerance and no exempted cell.

The rake rounds promise the reference's floats added in the reference's order.  The small parity grids never reach
the machinery that could break that promise, so this file goes where it runs:

  small grids      every graph builder of util.py (a chain through every cell, cells with all K donors, no edge at
                   all, cycles, entries that are no edge), hostile sources and decays, planes off their 16 bytes
  knobs            SOIL_RAKE_LIST_FROM / SOIL_RAKE_GROUPS are read once per process: child processes
  strided          grids above 8192 * 256 cells, where a thread of a dense round takes several cells and a list
                   segment takes several batches of appends; cells above 2^23; the band-walk donor kernel (8192^2)
  offsets          both sides of the 32-bit byte-offset threshold (K * elem * 4 = 2^32), from stacked tiles
  multiflow        the two lanes really side by side, against the script's loop; workspaces growing and reused

The oracle is always fed the graph the test built or the graph the device made, never its own random_weighted: the
counted CDF-edge receivers of util.assert_receivers_close do not enter.  orc_accumulate is serial; independent
calls run on up to 16 threads (ctypes releases the GIL)."""
import concurrent.futures
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from util import (assert_bit_equal, built_graphs, graph_cycles, graph_fan_chain, graph_snake, graph_wild,
                  stack_graphs, terrain, to_gpu, to_np)

pytestmark = pytest.mark.gpu

D4, D8 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(64, 64), (37, 53), (128, 96), (1, 1), (1, 300), (300, 1), (2, 40), (5, 1028)]
KNOB_CASE = (1537, 2051)


# ------------------------------------------------------------------ helpers

def _oracle_many(oracle, jobs):
    """[(graph, source, edge, decay or None)] -> the oracle's planes, independent calls on up to 16 threads."""
    if not jobs:
        return []
    with concurrent.futures.ThreadPoolExecutor(min(16, len(jobs))) as ex:
        return list(ex.map(lambda j: oracle.accumulate(j[0], j[1], j[2], decay=j[3]), jobs))


def _upload(arr):
    """A device copy of `arr` without a second host copy on the way."""
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.ascontiguousarray(arr)).gpu()


def _device_accumulate(graph, source, edge, decay=None):
    from soillib_amd import soil
    g, s = _upload(graph), _upload(source)
    if decay is None:
        return to_np(soil.accumulate(g, s, edge))
    return to_np(soil.accumulate_decay(g, s, _upload(decay), edge))


def _planes(H, W, seed):
    """Sources in [0.5, 1.5) (sums that round) and decays in [0.8, 1)."""
    r = np.random.default_rng(seed)
    return (0.5 + r.random((H, W))).astype(np.float32), (0.8 + 0.2 * r.random((H, W))).astype(np.float32)


def _device_dem(H, W, seed):
    """Device noise x 100: heights of ~100 m, the DEM of the multiple-flow script (tests/test_gpu_fullsize.py)."""
    from soillib_amd import silt, soil
    p = soil.noise_t()
    p.seed = float(seed)
    p.ext = [H, W]
    h = soil.noise(silt.shape(H, W), p, host=silt.gpu)
    silt.multiply(h, 100.0)
    return h


def _check(oracle, cases):
    """cases: [(what, graph, source, edge, decay)].  The device's planes, then the oracle's (threaded), bit for bit."""
    got = [_device_accumulate(g, s, e, d) for _, g, s, e, d in cases]
    want = _oracle_many(oracle, [(g, s, e, d) for _, g, s, e, d in cases])
    for (what, *_), a, b in zip(cases, got, want):
        assert_bit_equal(a, b, what)


def _small_graphs(oracle, H, W, edge):
    from soillib_amd import soil
    gh = to_gpu(terrain(oracle, H, W)[..., 0].copy())
    graphs = built_graphs(H, W, edge)
    graphs["steepest"] = to_np(soil.steepest(gh, edge))
    graphs["random_weighted"] = to_np(soil.random_weighted(gh, edge, 0, 1, 10.0))
    graphs["cycles"] = graph_cycles(graphs["random_weighted"])
    graphs["wild"] = graph_wild(graphs["random_weighted"])
    return graphs


# ------------------------------------------------------------------ 2. small and ragged grids, every builder

@pytest.mark.parametrize("H,W", SMALL)
@pytest.mark.parametrize("edge", [D4, D8])
def test_small_grids_every_builder(hip, oracle, H, W, edge):
    src, decay = _planes(H, W, 1)
    cases = []
    for name, g in _small_graphs(oracle, H, W, edge).items():
        cases.append(("%s %dx%d accumulate" % (name, H, W), g, src, edge, None))
        cases.append(("%s %dx%d accumulate_decay" % (name, H, W), g, src, edge, decay))
    _check(oracle, cases)


@pytest.mark.parametrize("H,W", SMALL)
def test_small_grids_hostile_values(hip, oracle, H, W):
    """NaN, +inf, -0.0, a denormal and 3e38 (sums overflow) among the sources; 0, -0.5 (powf of a negative base on
    the diagonal slots), 1, 2, NaN and 1e-30 among the decays; on legal graphs.  NaN for NaN, every other cell
    bit for bit."""
    r = np.random.default_rng(7)
    src, decay = _planes(H, W, 2)
    n = H * W
    for arr, values in ((src, [np.nan, np.inf, -0.0, 1e-42, 3e38]), (decay, [0.0, -0.5, 1.0, 2.0, np.nan, 1e-30])):
        flat = arr.reshape(-1)
        for v in values:
            flat[r.choice(n, size=min(n, n // 24 + 1), replace=False)] = np.float32(v)
    assert n < 6 or (np.isnan(src).any() and np.isinf(src).any() and (decay < 0).any())
    cases = []
    for edge in (D4, D8):
        graphs = _small_graphs(oracle, H, W, edge)
        for name in ("random_weighted", "steepest", "fan", "fan_chain", "one_sink"):
            cases.append(("hostile source, %s %dx%d edge %d" % (name, H, W, edge), graphs[name], src, edge, None))
            cases.append(("hostile source and decay, %s %dx%d edge %d" % (name, H, W, edge), graphs[name], src, edge, decay))
    _check(oracle, cases)


@pytest.mark.parametrize("H,W", [(64, 64), (128, 96), (1, 300), (2, 40), (5, 1028)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_small_grids_planes_off_their_16_bytes(hip, oracle, H, W, edge):
    """graph, source and out 4 bytes past a 16-byte boundary with W % 4 == 0: the one-cell-per-thread k_donors takes
    the call instead of k_donors4, and must agree with it (and with the oracle)."""
    from soillib_amd import _abi, silt
    assert W % 4 == 0

    def shifted(arr, dtype):
        buf = silt.tensor(dtype, silt.shape(H * W + 4), silt.gpu)
        assert buf.ptr % 16 == 0
        view = silt.tensor.from_device(buf.ptr + 4, dtype, silt.shape(H, W), keepalive=buf)
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            _abi.check(hip.soil_memcpy_h2d(view.c_ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, _abi.stream()))
            _abi.check(hip.soil_stream_synchronize(_abi.stream()))
        return view

    src, decay = _planes(H, W, 3)
    graphs = _small_graphs(oracle, H, W, edge)
    for name in ("random_weighted", "fan_chain", "wild"):
        g = graphs[name]
        for d in (None, decay):
            gv, sv, ov = shifted(g, silt.int32), shifted(src, silt.float32), shifted(None, silt.float32)
            dv = None if d is None else _upload(d)
            _abi.check(hip.soil_accumulate(ov.c_ptr, gv.c_ptr, sv.c_ptr, None if dv is None else dv.c_ptr,
                                           H, W, edge, _abi.stream()))
            narrow = to_np(ov)
            assert_bit_equal(narrow, _device_accumulate(g, src, edge, d), "k_donors against k_donors4, %s" % name)
            assert_bit_equal(narrow, oracle.accumulate(g, src, edge, decay=d), "k_donors against the oracle, %s" % name)


# ------------------------------------------------------------------ 3a. above the strided threshold

def _sized_cases(H, W, edges, graphs=("random_weighted", "steepest"), decays=(False, True)):
    from soillib_amd import soil
    assert H * W > 8192 * 256
    h = _device_dem(H, W, 5)
    src, decay = _planes(H, W, 11)
    cases = []
    for edge in edges:
        for name in graphs:
            if name == "random_weighted":
                g = to_np(soil.random_weighted(h, edge, 0, 7, 10.0))
            elif name == "steepest":
                g = to_np(soil.steepest(h, edge))
            elif name == "snake":
                g = graph_snake(H, W)
            else:
                g = graph_fan_chain(H, W, edge)
            for with_decay in decays:
                cases.append(("%s %dx%d edge %d decay %s" % (name, H, W, edge, with_decay), g, src, edge,
                              decay if with_decay else None))
    return cases


def test_knob_case_strided_1537x2051(hip, oracle):
    """W % 4 != 0, elem % 256 != 0, the narrow donor kernel; D8, random_weighted, a decay tensor.  (The one sized
    case the child processes of test_rake_knobs run as well.)"""
    _check(oracle, _sized_cases(*KNOB_CASE, edges=(D8,), graphs=("random_weighted",), decays=(True,)))


@pytest.mark.parametrize("H,W", [(1537, 2051), (2048, 2048), (1100, 4100), (4096, 4096)])
def test_strided_rounds_against_the_oracle(hip, oracle, H, W):
    """Above 8192 * 256 cells a thread of a dense round takes several cells and a list segment several batches of
    appends.  (1537, 2051): ragged; (2048, 2048): a power of two; (1100, 4100): wide, W % 4 == 0; (4096, 4096):
    BASELINE config 3's grid, cell indices above 2^23.  Both edges, both graph makers, with and without a decay."""
    _check(oracle, _sized_cases(H, W, edges=(D4, D8)))


def test_strided_rounds_on_a_4m_cell_chain(hip, oracle):
    """snake and fan_chain at 2048^2: a chain through 4 M cells stays on the lists to the last round."""
    _check(oracle, _sized_cases(2048, 2048, edges=(D4, D8), graphs=("snake", "fan_chain")))


def test_strided_rounds_at_8192(hip, oracle):
    """8192^2, D8, no decay: the band-walk donor kernel (win_shape_for(0, 5, H, W) from 2048 band groups on)."""
    from soillib_amd import silt
    _check(oracle, _sized_cases(8192, 8192, edges=(D8,), graphs=("random_weighted",), decays=(False,)))
    silt.empty_cache()


# ------------------------------------------------------------------ 3. the knobs, in child processes

KNOBS = ([{"SOIL_RAKE_LIST_FROM": str(v)} for v in (0, 1, 3, 7)] +
         [{"SOIL_RAKE_GROUPS": str(v)} for v in (1, 3, 64, 1000000)] +
         [{"SOIL_RAKE_GROUPS": "3", "SOIL_RAKE_LIST_FROM": "1"}])


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join("%s=%s" % kv for kv in sorted(k.items())))
def test_rake_knobs(hip, knobs):
    """Every setting of the two knobs of the rake rounds (docs/KNOBS.md) must give the oracle's bits.  Few groups on
    a small grid is the cheap way into the strided loop with many batches of appends per segment."""
    env = dict(os.environ, **knobs)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", "test_small_grids or test_knob_case"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, "%s:\n%s\n%s" % (knobs, r.stdout[-3000:], r.stderr[-1000:])
    assert " passed" in r.stdout and "failed" not in r.stdout


# ------------------------------------------------------------------ 4. both sides of the 32-bit offset threshold

TILE_H, TILE_W = 256, 16384


def _workspace_bytes(elem, K):
    """What accumulate_impl asks of the library's workspace (graph.hip), plus graph, source, decay and out."""
    al = lambda b: (b + 255) & ~255
    nb = min((elem + 255) // 256, 8192)
    seg = ((elem + nb - 1) // nb + 255) // 256 * 256
    return 3 * al(4 * elem) + 4 * al(4 * elem * K) + 2 * al(4 * seg * nb) + 2 * al(4 * nb) + 256 + 4 * 4 * elem


def _stacked_tiles_against_the_oracle(hip, oracle, edge, counts):
    import torch
    from soillib_amd import _abi, silt, soil
    K = 4 if edge == D4 else 8
    h, W = TILE_H, TILE_W
    T = max(counts)
    graphs, srcs, decays = [], [], []
    for t in range(T):                                   # tiles that all differ: own DEM, own draws, own planes
        graphs.append(to_np(soil.random_weighted(_device_dem(h, W, 20 + t), edge, 2, t, 10.0)))
        s, d = _planes(h, W, 1000 + t)
        srcs.append(s), decays.append(d)
    assert all((graphs[0] != g).any() for g in graphs[1:])
    ones = np.ones((h, W), np.float32)
    t0 = time.time()
    planes = _oracle_many(oracle, [job for g, s, d in zip(graphs, srcs, decays)
                                   for job in ((g, ones, edge, None), (g, s, edge, None), (g, s, edge, d))])
    print("oracle, %d tiles of %d x %d, edge %d: %.1f s" % (T, h, W, edge, time.time() - t0))
    for t, g in enumerate(graphs):                       # every tile finishes within its own round count
        assert planes[3 * t][g < 0].astype(np.float64).sum() == h * W, "tile %d has not finished" % t
    silt.empty_cache()                                   # what earlier tests left cached would hide what a case takes
    _abi.check(hip.soil_workspace_release())
    try:
        for n in counts:
            elem = n * h * W
            G = stack_graphs(graphs[:n])
            S = np.concatenate(srcs[:n])
            assert G.shape == (n * h, W) and int(G.max()) >= (n - 1) * h * W
            for with_decay in (False, True):
                what = "%d tiles, edge %d, decay %s, K * elem * 4 = %.3f * 2^32" % (n, edge, with_decay, K * elem / 2.0 ** 30)
                hip.soil_device_synchronize()
                free0 = torch.cuda.mem_get_info(0)[0]
                need = _workspace_bytes(elem, K)
                assert free0 >= need, "%s: the device has %.1f GB free, the case needs %.1f GB" % (what, free0 / 1e9, need / 1e9)
                want = np.concatenate(planes[2 if with_decay else 1:3 * n:3])
                dv = _upload(np.concatenate(decays[:n])) if with_decay else None
                gv, sv = _upload(G), _upload(S)
                out = soil.accumulate_decay(gv, sv, dv, edge) if with_decay else soil.accumulate(gv, sv, edge)
                hip.soil_device_synchronize()
                print("%s: %.2f GB of device memory in use on top of what was" % (what, (free0 - torch.cuda.mem_get_info(0)[0]) / 1e9))
                got = to_np(out)
                del out, gv, sv, dv
                silt.empty_cache()
                _abi.check(hip.soil_workspace_release())
                assert_bit_equal(got, want, what)
                del got, want
    finally:
        silt.empty_cache()
        hip.soil_workspace_release()


def test_stacked_tiles_across_the_offset_threshold_d8(hip, oracle):
    """D8, tiles of 256 x 16384 (4.2 M cells) stacked: 31 tiles (130 M cells: 32-bit byte offsets, up to 4.16 G —
    above 2^31, where a signed offset would go wrong) and 33 tiles (138 M > 2^27 cells: the int64_t kernels), with
    a decay tensor and without.  The expected plane is the tiles' own accumulations stacked (the stacking rule,
    tests/test_oracle_kat.py).  A truncated index would be caught: the tiles all differ (own DEM, own draws, own
    sources and decays), and at 33 tiles K * elem exceeds 2^30 words, so a byte offset cut to 32 bits lands in
    another tile's slots — other donors, other values."""
    _stacked_tiles_against_the_oracle(hip, oracle, D8, (31, 33))


def test_stacked_tiles_across_the_offset_threshold_d4(hip, oracle):
    """D4, 65 tiles (273 M > 2^28 cells: the int64_t kernels with K = 4), with a decay tensor and without; see the
    D8 test for why a truncated index cannot hide."""
    _stacked_tiles_against_the_oracle(hip, oracle, D4, (65,))


# ------------------------------------------------------------------ 5. soil_multiflow at size

def _multiflow_terms(oracle, height, src, edge, seed, ks, T=10.0):
    """k -> accumulate(random_weighted(height, edge, seed, k, T), source) by the oracle, on the device's graphs."""
    from soillib_amd import soil
    graphs = [to_np(soil.random_weighted(height, edge, seed, k, T)) for k in ks]
    return dict(zip(ks, _oracle_many(oracle, [(g, src, edge, None) for g in graphs])))


def _mean(terms, order, K, shape):
    mean = np.zeros(shape, np.float64)
    for k in order:                                      # the loop of the multiple-flow script, term by term
        mean += (terms[k] / np.float32(K)).astype(np.float64)
    return mean


@pytest.mark.parametrize("H,W", [(1537, 2052), (2048, 2048)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_multiflow_at_size(hip, oracle, H, W, edge):
    """K in {1, 4, 5, 9} with kRwBatch = 4: one batch, a full batch, a graph set reused, both sets reused twice; odd
    and even counts on the two lanes.  Whole, and in three shards added into one plane."""
    from soillib_amd import soil
    height = _device_dem(H, W, 5)
    src, _ = _planes(H, W, 13)
    gs = _upload(src)
    terms = _multiflow_terms(oracle, height, src, edge, 11, list(range(9)))
    for K in (1, 4, 5, 9):
        got = to_np(soil.multiflow(height, gs, K, 10.0, edge, seed=11))
        assert got.dtype == np.float64
        assert_bit_equal(got, _mean(terms, range(K), K, (H, W)), "multiflow K = %d" % K)
        shards = soil.multiflow(height, gs, K, 10.0, edge, seed=11, first=0, stride=3)
        for first in (1, 2):
            soil.multiflow(height, gs, K, 10.0, edge, seed=11, first=first, stride=3, out=shards)
        order = [k for first in (0, 1, 2) for k in range(first, K, 3)]
        assert_bit_equal(to_np(shards), _mean(terms, order, K, (H, W)), "multiflow in shards, K = %d" % K)


def test_multiflow_lanes_grow_and_are_reused(hip, oracle):
    """Small, large, small again in one process: a lane's workspace grows and is reused; then soil.accumulate on
    the same thread, in lane 0's workspace."""
    from soillib_amd import soil
    K = 5
    for H, W in ((88, 120), (2048, 2048), (88, 120)):
        height = _device_dem(H, W, 9)
        src, decay = _planes(H, W, H)
        terms = _multiflow_terms(oracle, height, src, D8, 3, list(range(K)))
        got = to_np(soil.multiflow(height, _upload(src), K, 10.0, D8, seed=3))
        assert_bit_equal(got, _mean(terms, range(K), K, (H, W)), "multiflow %dx%d" % (H, W))
        g = to_np(soil.random_weighted(height, D8, 3, 1, 10.0))
        _check(oracle, [("accumulate after multiflow %dx%d" % (H, W), g, src, D8, None),
                        ("accumulate_decay after multiflow %dx%d" % (H, W), g, src, D8, decay)])
