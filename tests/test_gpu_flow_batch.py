"""Flow routing over a batch of models (include/soil_hip.h: soil_direction_batch, soil_steepest_batch,
soil_random_weighted_batch, soil_slope_batch, soil_accumulate_batch; soillib_amd.soil.*_batch and
ErosionBatch.flow / drainage / flow_slope), bit for bit: every comparison is of int32 values or of float bit
patterns (util.assert_bit_equal: NaN for NaN), there is no tolerance anywhere.

  oracle        model by model against the CPU oracle the single-grid kernels are held to: graphs and directions
                on random heights with plateaus and exact ties, slopes with one and with per-model scales,
                accumulation on steepest and on built graphs (a chain through every cell, cells with all K donors,
                no edge, cycles, entries that are no edge), signed sources and a NaN that stays in its model
  shapes        the scalar form (1, 1), (5, 1), (1, 8), (37, 53); the window form (3, 4), (33, 260) — a second
                256-column wave strip —, (9, 1028) — a second 1024-column work-group piece —, (256, 256);
                B in {1, 2, 3, 7, 64}; B = 65537 at (1, 4): the split of the models over launches
  isolation     nothing a model holds reaches another one
  single grid   all five entries against the single-grid device calls at (256, 256) x 8 and (1024, 1024) x 2;
                random_weighted only so (the oracle's exact exponentials differ on counted CDF-edge draws)
  chunking      SOIL_FLOW_BATCH_CELLS in child processes, also under SOIL_RAKE_LIST_FROM = 0 and 1
  plumbing      planes off their 16 bytes, a second stream, the call twice, another size in between, refusals
  after steps   ErosionBatch.flow / drainage / flow_slope on stepped models against the oracle
"""
import concurrent.futures
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from util import (assert_bit_equal, built_graphs, graph_cycles, graph_wild, product_param, script_param, terrain,
                  to_gpu, to_np)

pytestmark = pytest.mark.gpu

D4, D8 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR = [(1, 1), (5, 1), (1, 8), (37, 53)]
WINDOW = [(3, 4), (33, 260), (9, 1028), (256, 256)]
BS = [1, 2, 3, 7, 64]
CASES = [(H, W, B) for H, W in SCALAR + WINDOW for B in BS]
CHUNK_SHAPES = [(37, 53), (33, 260)]


# ------------------------------------------------------------------ inputs and references, made once

def _heights(B, H, W, seed=0):
    """Random heights on a grid of eighths (exact ties between neighbours), a plateau in every model (none of its
    inner cells has a receiver) and a different terrain per model."""
    r = np.random.default_rng(1000003 * seed + 10007 * B + 101 * H + W)
    h = (r.integers(0, 64, size=(B, H, W)) / 8.0).astype(np.float32)
    smooth = np.add.outer(np.arange(H), np.arange(W)).astype(np.float32)
    for b in range(B):
        if b % 3 == 1:
            h[b] += np.float32(0.25 * (b + 1)) * smooth          # a ramp under the noise: long paths
        x0, y0 = int(r.integers(0, H)), int(r.integers(0, W))
        h[b, x0:x0 + max(1, H // 3), y0:y0 + max(1, W // 3)] = np.float32(3.0 + b)   # a plateau
    return h


@functools.lru_cache(maxsize=None)
def _case(H, W, B):
    """Heights, the oracle's graphs and directions, sources, decays and scales of a case, made once: the tests
    leave them as they are."""
    from oracle import pyoracle
    h = _heights(B, H, W)
    r = np.random.default_rng(7 * B + H * W)
    src = (r.random((B, H, W)) - 0.25).astype(np.float32)        # signed
    decay = (0.8 + 0.2 * r.random((B, H, W))).astype(np.float32)
    scales = [(0.5 + 0.25 * b, 2.0 - 0.125 * (b % 9)) for b in range(B)]
    ref = {}
    for edge in (D4, D8):
        ref["steepest", edge] = np.stack([pyoracle.steepest(h[b], edge) for b in range(B)])
        ref["direction", edge] = np.stack([pyoracle.direction(h[b], edge) for b in range(B)])
    ref.update(h=h, src=src, decay=decay, scales=scales)
    return ref


def _built(B, H, W, edge, base):
    """A different built graph per model, in the manner of test_gpu_accumulate_oracle.py: a chain through every
    cell, cells with all K donors, the same on a chain, no edge at all, one sink, cycles, entries that are no edge
    (among them indices of the next model's numbering, H W and above)."""
    names = ["snake", "fan", "fan_chain", "no_edges", "one_sink", "cycles", "wild"]
    fixed = built_graphs(H, W, edge)
    out = []
    for b in range(B):
        name = names[b % len(names)]
        if name == "cycles":
            out.append(graph_cycles(base[b], seed=5 + b))
        elif name == "wild":
            out.append(graph_wild(base[b], seed=9 + b))
        else:
            out.append(fixed[name])
    return np.stack(out).astype(np.int32)


def _oracle_accumulate(graph, src, edge, decay=None):
    """Model by model; orc_accumulate is serial and ctypes releases the GIL: up to 16 threads."""
    from oracle import pyoracle
    one = lambda b: pyoracle.accumulate(graph[b], src[b], edge, decay=None if decay is None else decay[b])
    with concurrent.futures.ThreadPoolExecutor(min(16, graph.shape[0])) as ex:
        return np.stack(list(ex.map(one, range(graph.shape[0]))))


def _acc(graph, src, edge, decay=None):
    from soillib_amd import soil
    return to_np(soil.accumulate_batch(to_gpu(graph), to_gpu(src), edge, None if decay is None else to_gpu(decay)))


# ------------------------------------------------------------------ against the oracle, model by model

@pytest.mark.parametrize("H,W,B", CASES)
def test_graphs_against_the_oracle(hip, H, W, B):
    from soillib_amd import soil
    c = _case(H, W, B)
    gh = to_gpu(c["h"])
    for edge in (D4, D8):
        assert_bit_equal(to_np(soil.steepest_batch(gh, edge)), c["steepest", edge], "steepest_batch edge %d" % edge)
        assert_bit_equal(to_np(soil.direction_batch(gh, edge)), c["direction", edge], "direction_batch edge %d" % edge)
    g = c["steepest", D8]
    assert (g == -1).any() and g.max() < H * W, "a receiver is an index within its model"


@pytest.mark.parametrize("H,W,B", CASES)
def test_slope_against_the_oracle(hip, oracle, H, W, B):
    from soillib_amd import soil
    c = _case(H, W, B)
    gh = to_gpu(c["h"])
    for edge in (D4, D8):
        flow = c["steepest", edge]
        gf = to_gpu(flow)
        one = to_np(soil.slope_batch(gh, gf, [0.7, 1.9]))
        per = to_np(soil.slope_batch(gh, gf, c["scales"]))
        for b in range(B):
            assert_bit_equal(one[b], oracle.slope(c["h"][b], flow[b], (0.7, 1.9)), "slope_batch, one scale, model %d" % b)
            assert_bit_equal(per[b], oracle.slope(c["h"][b], flow[b], c["scales"][b]), "slope_batch, own scale, model %d" % b)


@pytest.mark.parametrize("H,W,B", CASES)
def test_accumulate_against_the_oracle(hip, H, W, B):
    c = _case(H, W, B)
    for edge in (D4, D8):
        for what, graph in (("steepest", c["steepest", edge]), ("built", _built(B, H, W, edge, c["steepest", edge]))):
            for decay in (None, c["decay"]):
                got = _acc(graph, c["src"], edge, decay)
                assert_bit_equal(got, _oracle_accumulate(graph, c["src"], edge, decay),
                                 "accumulate_batch %s edge %d decay %s" % (what, edge, decay is not None))


@pytest.mark.parametrize("H,W,B", [(37, 53, 7), (33, 260, 3), (256, 256, 2), (1, 8, 64)])
def test_a_nan_stays_in_its_model(hip, H, W, B):
    """A NaN source in every cell of the LAST row of one model, on graphs that drain every model towards its first
    row: the whole of that model's drainage may go NaN, no cell of any other model does."""
    c = _case(H, W, B)
    bad = B // 2
    src = c["src"].copy()
    src[bad, -1, :] = np.nan
    h = np.broadcast_to(np.arange(H, dtype=np.float32)[:, None] + 1.0, (B, H, W)).copy()   # drains upwards
    from soillib_amd import soil
    for edge in (D4, D8):
        graph = to_np(soil.steepest_batch(to_gpu(h), edge))
        got = _acc(graph, src, edge, c["decay"])
        assert np.isnan(got[bad]).any()
        for b in range(B):
            if b != bad:
                assert not np.isnan(got[b]).any(), "model %d caught model %d's NaN" % (b, bad)
        assert_bit_equal(got, _oracle_accumulate(graph, src, edge, c["decay"]), "NaN source, edge %d" % edge)


def test_the_split_of_the_models_over_launches(hip, oracle):
    """B = 65537 at (1, 4): more models than a launch takes (65535).  Every entry on every model: graphs, slopes and
    accumulations against the oracle of the different models there are (3^4 height rows, 3 sources, 2 decays), the
    random graphs against the single-grid call for the models around the split."""
    from soillib_amd import soil
    B, H, W = 65537, 1, 4
    r = np.random.default_rng(5)
    h = r.integers(0, 3, size=(B, H, W)).astype(np.float32)
    src = np.array([[0.5, 1.0, -1.5, 2.0], [1.0, 1.0, 1.0, 1.0], [3.0, -0.25, 0.75, 1.25]], np.float32)[
        r.integers(0, 3, size=B)].reshape(B, H, W)
    decay = np.array([[0.5, 0.75, 1.0, 0.25], [0.9, 0.8, 0.7, 0.6]], np.float32)[r.integers(0, 2, size=B)].reshape(B, H, W)
    gh = to_gpu(h)
    # the oracle once per different (height, source, decay) row, spread back over the models
    key = np.concatenate([h.reshape(B, -1), src.reshape(B, -1), decay.reshape(B, -1)], axis=1)
    uniq, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    for edge in (D4, D8):
        g = to_np(soil.steepest_batch(gh, edge))
        d = to_np(soil.direction_batch(gh, edge))
        s = to_np(soil.slope_batch(gh, to_gpu(g), [1.5, 0.5]))
        a = to_np(soil.accumulate_batch(to_gpu(g), to_gpu(src), edge))
        ad = to_np(soil.accumulate_batch(to_gpu(g), to_gpu(src), edge, to_gpu(decay)))
        want = [(oracle.steepest(h[b], edge), oracle.direction(h[b], edge)) for b in first]
        assert_bit_equal(g, np.stack([w[0] for w in want])[inverse], "steepest_batch")
        assert_bit_equal(d, np.stack([w[1] for w in want])[inverse], "direction_batch")
        assert_bit_equal(s, np.stack([oracle.slope(h[b], g[b], (1.5, 0.5)) for b in first])[inverse], "slope_batch")
        assert_bit_equal(a, np.stack([oracle.accumulate(g[b], src[b], edge) for b in first])[inverse], "accumulate_batch")
        assert_bit_equal(ad, np.stack([oracle.accumulate(g[b], src[b], edge, decay=decay[b]) for b in first])[inverse],
                         "accumulate_batch with decay")
        seeds = [(977 * b + 3) % (1 << 40) for b in range(B)]
        rw = to_np(soil.random_weighted_batch(gh, edge, seeds, 3, 2.0))
        for b in (0, 1, 65533, 65534, 65535, 65536):
            assert_bit_equal(rw[b], to_np(soil.random_weighted(to_gpu(h[b]), edge, seeds[b], 3, 2.0)),
                             "random_weighted_batch, model %d" % b)
        # per-model scales past the split
        scales = [(1.0 + (b % 7), 0.5 + (b % 3)) for b in range(B)]
        sp = to_np(soil.slope_batch(gh, to_gpu(g), scales))
        for b in (0, 65534, 65535, 65536):
            assert_bit_equal(sp[b], oracle.slope(h[b], g[b], scales[b]), "slope_batch, own scale, model %d" % b)


# ------------------------------------------------------------------ isolation

@pytest.mark.parametrize("H,W", [(37, 53), (33, 260)])
@pytest.mark.parametrize("top", [True, False])
def test_no_receiver_outside_the_model(hip, oracle, H, W, top):
    """Every model holds the same ramp, draining across its top (or bottom) edge row: a cell of that row would find
    a lower cell in the last (first) row of the model before (after) it if a neighbour off the edge existed."""
    from soillib_amd import soil
    B = 5
    ramp = np.arange(H, dtype=np.float32)[:, None] + np.zeros((1, W), np.float32)
    h = np.broadcast_to(ramp if top else ramp[::-1], (B, H, W)).copy()
    for edge in (D4, D8):
        g = to_np(soil.steepest_batch(to_gpu(h), edge))
        d = to_np(soil.direction_batch(to_gpu(h), edge))
        rw = to_np(soil.random_weighted_batch(to_gpu(h), edge, list(range(B)), 1, 0.5))
        edge_row = 0 if top else H - 1
        for b in range(B):
            assert (g[b, edge_row] == -1).all() and (d[b, edge_row] == -1).all() and (rw[b, edge_row] == -1).all()
            assert_bit_equal(g[b], oracle.steepest(h[b], edge), "steepest, model %d" % b)
        assert g.min() >= -1 and g.max() < H * W and rw.min() >= -1 and rw.max() < H * W
        up = to_np(soil.accumulate_batch(to_gpu(g), to_gpu(np.ones((B, H, W), np.float32)), edge))
        assert_bit_equal(up[:, edge_row], np.full((B, W), float(H), np.float32), "upstream cells of the edge row")


def test_a_model_is_unchanged_when_the_others_are_replaced(hip):
    from soillib_amd import soil
    H, W, B = 33, 260, 5
    a, other = _case(H, W, B), _heights(B, H, W, seed=1)
    r = np.random.default_rng(3)
    for keep in (0, 2, 4):
        h2, s2, d2 = other.copy(), r.standard_normal((B, H, W)).astype(np.float32), a["decay"][::-1].copy()
        h2[keep], s2[keep], d2[keep] = a["h"][keep], a["src"][keep], a["decay"][keep]
        s2[(keep + 1) % B, 0, 0] = np.nan
        for edge in (D4, D8):
            def run(h, s, d):
                g = soil.steepest_batch(to_gpu(h), edge)
                return (to_np(g), to_np(soil.accumulate_batch(g, to_gpu(s), edge, to_gpu(d))),
                        to_np(soil.slope_batch(to_gpu(h), g, a["scales"])))
            for x, y, what in zip(run(a["h"], a["src"], a["decay"]), run(h2, s2, d2), ("graph", "drainage", "slope")):
                assert_bit_equal(x[keep], y[keep], "%s of model %d, edge %d" % (what, keep, edge))


@pytest.mark.parametrize("H,W", [(37, 53), (33, 260)])
def test_an_index_of_the_neighbouring_models_numbering_is_no_edge(hip, oracle, H, W):
    """Model 1's graph with receivers written in the STACKED numbering (H W + index: what a stacked single grid
    would hold) drains nowhere; in its own numbering it drains as the oracle says; model 0, whose last row points
    at model 1's first row in stacked numbering, keeps those cells as outlets."""
    from soillib_amd import soil
    B = 3
    c = _case(H, W, B)
    g = c["steepest", D8].copy()
    stacked = g.copy()
    stacked[1] = np.where(g[1] >= 0, g[1] + H * W, -1)
    stacked[0, -1, :] = H * W + np.arange(W)                     # "the cell below", were the models one grid
    stacked[2, 0, :] = np.arange(W) - W                          # "the cell above": negative, no edge either
    got = _acc(stacked, c["src"], D8)
    assert_bit_equal(got[1], c["src"][1], "a model whose entries are all of another numbering accumulates nothing")
    for b in (0, 2):
        assert_bit_equal(got[b], oracle.accumulate(stacked[b], c["src"][b], D8), "model %d" % b)
    assert_bit_equal(_acc(g, c["src"], D8)[1], oracle.accumulate(g[1], c["src"][1], D8), "model 1 in its own numbering")


# ------------------------------------------------------------------ against the single-grid device calls

def _device_heights(B, H, W):
    from soillib_amd import silt, soil
    out = silt.tensor(silt.float32, silt.shape(B, H, W), silt.gpu)
    for b in range(B):
        p = soil.noise_t()
        p.seed = float(5 + b)
        p.ext = [H, W]
        one = soil.noise(silt.shape(H, W), p, host=silt.gpu)
        silt.multiply(one, 100.0)
        _d2d(out, b, one)
    return out


def _d2d(batch, b, single):
    from soillib_amd import _abi
    per = batch.nbytes() // batch.shape[0]
    _abi.check(_abi.lib().soil_memcpy_d2d(C.c_void_p(batch.ptr + b * per), single.c_ptr, per, _abi.stream()))


def _model(t, b):
    from soillib_amd import silt
    dims = tuple(t.shape)[1:]
    per = t.nbytes() // t.shape[0]
    return silt.tensor.from_device(t.ptr + b * per, t.type, silt.shape(*dims), keepalive=t)


@pytest.mark.parametrize("H,W,B", [(256, 256, 8), (1024, 1024, 2)])
def test_all_five_entries_against_the_single_grid_calls(hip, H, W, B):
    from soillib_amd import soil
    gh = _device_heights(B, H, W)
    r = np.random.default_rng(H + B)
    src = to_gpu((0.5 + r.random((B, H, W))).astype(np.float32))
    decay = to_gpu((0.8 + 0.2 * r.random((B, H, W))).astype(np.float32))
    seeds = [1 << 33 | (17 * b + 1) for b in range(B)]
    scales = [(1.0 + b, 2.0 + 0.5 * b) for b in range(B)]
    host_h = to_np(gh)
    for edge in (D4, D8):
        K = 4 if edge == D4 else 8
        steep, direc = soil.steepest_batch(gh, edge), soil.direction_batch(gh, edge)
        rw = {off: soil.random_weighted_batch(gh, edge, seeds, off, 10.0) for off in (0, 5)}
        slope_one, slope_per = soil.slope_batch(gh, steep, [3.0, 0.5]), soil.slope_batch(gh, rw[5], scales)
        acc = soil.accumulate_batch(rw[0], src, edge)
        acc_d = soil.accumulate_batch(steep, src, edge, decay)
        for b in range(B):
            hb = _model(gh, b)
            assert_bit_equal(to_np(_model(steep, b)), to_np(soil.steepest(hb, edge)), "steepest %d" % b)
            assert_bit_equal(to_np(_model(direc, b)), to_np(soil.direction(hb, edge)), "direction %d" % b)
            for off in (0, 5):
                assert_bit_equal(to_np(_model(rw[off], b)), to_np(soil.random_weighted(hb, edge, seeds[b], off, 10.0)),
                                 "random_weighted %d offset %d" % (b, off))
            assert_bit_equal(to_np(_model(slope_one, b)), to_np(soil.slope(hb, _model(steep, b), [3.0, 0.5])), "slope %d" % b)
            assert_bit_equal(to_np(_model(slope_per, b)), to_np(soil.slope(hb, _model(rw[5], b), scales[b])), "slope, own scale %d" % b)
            assert_bit_equal(to_np(_model(acc, b)), to_np(soil.accumulate(_model(rw[0], b), _model(src, b), edge)), "accumulate %d" % b)
            assert_bit_equal(to_np(_model(acc_d, b)),
                             to_np(soil.accumulate_decay(_model(steep, b), _model(src, b), _model(decay, b), edge)),
                             "accumulate_decay %d" % b)
        # every receiver is -1 or a strictly lower neighbour inside the model
        dx = np.array([-1, 0, 0, 1, -1, -1, 1, 1])[:K]
        dy = np.array([0, -1, 1, 0, -1, 1, -1, 1])[:K]
        x, y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        for name, graph in (("steepest", to_np(steep)), ("random_weighted", to_np(rw[0]))):
            for b in range(B):
                g = graph[b]
                has = g >= 0
                assert g.min() >= -1 and g.max() < H * W
                rx, ry = g // W, g % W
                near = np.zeros((H, W), bool)
                for k in range(K):
                    near |= (rx == x + dx[k]) & (ry == y + dy[k])
                assert (near | ~has).all(), "%s: a receiver of model %d is no neighbour" % (name, b)
                lower = host_h[b].reshape(-1)[np.where(has, g, 0)] < host_h[b]
                assert (lower | ~has).all(), "%s: a receiver of model %d is not strictly lower" % (name, b)


# ------------------------------------------------------------------ chunking, in child processes

def _chunk_inputs(H, W):
    B = 5
    c = _case(H, W, B)
    graphs = {edge: (c["steepest", edge], _built(B, H, W, edge, c["steepest", edge])) for edge in (D4, D8)}
    return c, graphs


def _chunk_results(H, W):
    """name -> plane, for every graph, edge and decay of the chunking case (the caller has set the knob)."""
    c, graphs = _chunk_inputs(H, W)
    out = {}
    for edge in (D4, D8):
        for i, graph in enumerate(graphs[edge]):
            for decay in (None, c["decay"]):
                out["e%d_g%d_d%d" % (edge, i, decay is not None)] = _acc(graph, c["src"], edge, decay)
    return out


def _child_main(path):
    """The child of test_chunks: both shapes as 2 + 2 + 1 models and as five chunks of one, saved for the parent."""
    out = {}
    for H, W in CHUNK_SHAPES:
        for models in (2, 1):
            os.environ["SOIL_FLOW_BATCH_CELLS"] = str(models * H * W + (H * W // 2 if models == 2 else 0))
            for name, plane in _chunk_results(H, W).items():
                out["%dx%d_m%d_%s" % (H, W, models, name)] = plane
    np.savez(path, **out)


@functools.lru_cache(maxsize=None)
def _unchunked(H, W):
    assert "SOIL_FLOW_BATCH_CELLS" not in os.environ
    c, graphs = _chunk_inputs(H, W)
    got = _chunk_results(H, W)
    for edge in (D4, D8):                                        # and the unchunked results are the oracle's
        for i, graph in enumerate(graphs[edge]):
            for decay in (None, c["decay"]):
                assert_bit_equal(got["e%d_g%d_d%d" % (edge, i, decay is not None)],
                                 _oracle_accumulate(graph, c["src"], edge, decay), "unchunked")
    return got


@pytest.mark.parametrize("list_from", [None, "0", "1"])
def test_chunks(hip, tmp_path, list_from):
    """B = 5 at (37, 53) and at (33, 260) as chunks of 2 + 2 + 1 models and as five chunks of one
    (SOIL_FLOW_BATCH_CELLS), by default and under SOIL_RAKE_LIST_FROM = 0 and 1 (read once per process: a child):
    identical to the unchunked results of this process."""
    path = str(tmp_path / "chunks.npz")
    env = dict(os.environ)
    env.pop("SOIL_FLOW_BATCH_CELLS", None)
    if list_from is not None:
        env["SOIL_RAKE_LIST_FROM"] = list_from
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    seen = 0
    for H, W in CHUNK_SHAPES:
        want = _unchunked(H, W)
        for models in (2, 1):
            for name, plane in want.items():
                assert_bit_equal(got["%dx%d_m%d_%s" % (H, W, models, name)], plane,
                                 "%dx%d in chunks of %d, %s, SOIL_RAKE_LIST_FROM %s" % (H, W, models, name, list_from))
                seen += 1
    assert seen == 2 * 2 * 8 == len(got.files)


# ------------------------------------------------------------------ plumbing

def test_planes_off_their_16_bytes(hip, oracle):
    """Every plane 4 bytes past a 16-byte boundary inside a larger allocation, W % 4 == 0: the scalar forms take the
    calls, and give what the window forms give."""
    from soillib_amd import _abi, silt, soil
    H, W, B = 33, 260, 3
    c = _case(H, W, B)

    def shifted(arr, dtype):
        buf = silt.tensor(dtype, silt.shape(B * H * W + 4), silt.gpu)
        assert buf.ptr % 16 == 0
        view = silt.tensor.from_device(buf.ptr + 4, dtype, silt.shape(B, H, W), keepalive=buf)
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            _abi.check(hip.soil_memcpy_h2d(view.c_ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, _abi.stream()))
            _abi.check(hip.soil_stream_synchronize(_abi.stream()))
        return view

    seeds = (C.c_uint64 * B)(5, 6, 7)
    scales = (C.c_float * (2 * B))(*[v for s in c["scales"] for v in s])
    hv, sv, dv = shifted(c["h"], silt.float32), shifted(c["src"], silt.float32), shifted(c["decay"], silt.float32)
    gh = to_gpu(c["h"])
    for edge in (D4, D8):
        g, d, rw = shifted(None, silt.int32), shifted(None, silt.int32), shifted(None, silt.int32)
        sl, acc = shifted(None, silt.float32), shifted(None, silt.float32)
        st = _abi.stream()
        _abi.check(hip.soil_steepest_batch(g.c_ptr, hv.c_ptr, B, H, W, edge, st))
        _abi.check(hip.soil_direction_batch(d.c_ptr, hv.c_ptr, B, H, W, edge, st))
        _abi.check(hip.soil_random_weighted_batch(rw.c_ptr, hv.c_ptr, B, H, W, edge, seeds, 2, 10.0, st))
        _abi.check(hip.soil_slope_batch(sl.c_ptr, hv.c_ptr, g.c_ptr, B, H, W, scales, B, st))
        _abi.check(hip.soil_accumulate_batch(acc.c_ptr, g.c_ptr, sv.c_ptr, dv.c_ptr, B, H, W, edge, st))
        assert_bit_equal(to_np(g), c["steepest", edge], "steepest_batch, scalar form")
        assert_bit_equal(to_np(d), c["direction", edge], "direction_batch, scalar form")
        assert_bit_equal(to_np(rw), to_np(soil.random_weighted_batch(gh, edge, [5, 6, 7], 2, 10.0)), "random_weighted_batch")
        assert_bit_equal(to_np(sl), to_np(soil.slope_batch(gh, to_gpu(c["steepest", edge]), c["scales"])), "slope_batch")
        assert_bit_equal(to_np(acc), _oracle_accumulate(c["steepest", edge], c["src"], edge, c["decay"]), "accumulate_batch")


def test_on_another_stream_twice_and_with_another_size_in_between(hip):
    """A second stream; the call made twice (the workspace and the staging reused); a call of another size — more
    models, a larger grid, then a smaller one — in between."""
    import torch
    from soillib_amd import _abi, soil
    small, large = _case(37, 53, 7), _case(33, 260, 64)

    def run(c, edge):
        gh = to_gpu(c["h"])
        g = soil.steepest_batch(gh, edge)
        B = c["h"].shape[0]
        return (g, soil.accumulate_batch(g, to_gpu(c["src"]), edge, to_gpu(c["decay"])),
                soil.slope_batch(gh, g, c["scales"]), soil.random_weighted_batch(gh, edge, list(range(B)), 1, 5.0))

    def check(c, edge, got, rw_first):
        assert_bit_equal(to_np(got[0]), c["steepest", edge], "steepest_batch")
        assert_bit_equal(to_np(got[1]), _oracle_accumulate(c["steepest", edge], c["src"], edge, c["decay"]), "accumulate_batch")
        assert_bit_equal(to_np(got[3]), rw_first, "random_weighted_batch, the same call again")

    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        first_small, first_large = run(small, D8), run(large, D8)
        s.synchronize()
        rw_small, rw_large = to_np(first_small[3]), to_np(first_large[3])
        slope_small = to_np(first_small[2])
        for c, rw in ((small, rw_small), (large, rw_large), (small, rw_small), (small, rw_small)):
            got = run(c, D8)
            s.synchronize()
            check(c, D8, got, rw)
        assert_bit_equal(to_np(got[2]), slope_small, "slope_batch, the same call again")
    finally:
        _abi.set_stream(0)


# ------------------------------------------------------------------ after real steps

def test_flow_drainage_and_slope_of_stepped_models(hip, oracle):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionBatch
    B, H, W = 4, 256, 256
    p = product_param(script_param(oracle.default_param()))
    p.maxage = 64
    scales = [(20.0 / H * (1 + b), 20.0 / W, 4.0) for b in range(B)]
    r = np.random.default_rng(12)
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    for scale in ((20.0 / H, 20.0 / W, 4.0), scales):
        bt = ErosionBatch(B, H, W, scale, p, 2048, [11 + 7 * b for b in range(B)])
        bt.set_layers(to_gpu(layers))
        silt.set(bt.rainfall, to_gpu((0.5 + r.random((B, H, W))).astype(np.float32)))
        silt.set(bt.uplift, to_gpu((0.5 * r.random((B, H, W))).astype(np.float32)))
        for _ in range(3):
            bt.step()
        flow, direc = to_np(bt.flow()), to_np(bt.flow(kind="direction", edge=D4))
        rw = to_np(bt.flow(kind="random_weighted", T=10.0, offset=2))
        area, slope = to_np(bt.drainage()), to_np(bt.flow_slope())
        discharge = to_np(bt.drainage(source=bt.rainfall))
        d4 = to_np(bt.drainage(graph=bt.flow(edge=D4), source=bt.rainfall, decay=bt.uplift, edge=D4))
        ones = np.ones((H, W), np.float32)
        for b in range(B):
            pl = bt.model_planes(b)
            h, s2 = pl["height"], (scale if scale is not scales else scales[b])[:2]
            assert np.isfinite(h).all() and h.std() > 0
            assert_bit_equal(flow[b], oracle.steepest(h, D8), "flow() of model %d" % b)
            assert_bit_equal(direc[b], oracle.direction(h, D4), "flow(direction, d4) of model %d" % b)
            assert_bit_equal(area[b], oracle.accumulate(flow[b], ones, D8), "drainage() of model %d" % b)
            assert_bit_equal(slope[b], oracle.slope(h, flow[b], s2), "flow_slope() of model %d" % b)
            assert_bit_equal(discharge[b], oracle.accumulate(flow[b], pl["rainfall"], D8), "drainage(rainfall) of model %d" % b)
            assert_bit_equal(d4[b], oracle.accumulate(oracle.steepest(h, D4), pl["rainfall"], D4, decay=pl["uplift"]),
                             "drainage(d4, decay) of model %d" % b)
            from soillib_amd import soil
            assert_bit_equal(rw[b], to_np(soil.random_weighted(to_gpu(h), D8, bt.seeds[b], 2, 10.0)), "flow(random_weighted)")


# ------------------------------------------------------------------ refusals

def test_refusals_leave_the_planes_untouched(hip):
    from soillib_amd import _abi
    B, H, W = 2, 5, 8
    mark_f, mark_i = np.float32(-7.5), np.int32(-77)
    f = [to_gpu(np.full((B, H, W), mark_f, np.float32)) for _ in range(4)]
    g = [to_gpu(np.full((B, H, W), mark_i, np.int32)) for _ in range(2)]
    seeds = (C.c_uint64 * B)(1, 2)
    scales = (C.c_float * (2 * B))(1, 1, 1, 1)
    st = _abi.stream()
    big = 1 << 16                                                # H * W = 2^32 > INT32_MAX
    sizes = [(0, H, W), (-1, H, W), (B, 0, W), (B, H, 0), (B, H, -3), (B, big, big)]

    def refused(name, rc):
        assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, name
        assert name[len("soil_"):] + ":" in _abi.last_error(), (name, _abi.last_error())

    for name in ("soil_direction_batch", "soil_steepest_batch"):
        fn = getattr(hip, name)
        refused(name, fn(None, f[0].c_ptr, B, H, W, D8, st))
        refused(name, fn(g[0].c_ptr, None, B, H, W, D8, st))
        refused(name, fn(g[0].c_ptr, f[0].c_ptr, B, H, W, 2, st))
        refused(name, fn(g[0].c_ptr, f[0].c_ptr, B, H, W, -1, st))
        for b, h, w in sizes:
            refused(name, fn(g[0].c_ptr, f[0].c_ptr, b, h, w, D8, st))
    name, fn = "soil_random_weighted_batch", hip.soil_random_weighted_batch
    refused(name, fn(None, f[0].c_ptr, B, H, W, D8, seeds, 0, 1.0, st))
    refused(name, fn(g[0].c_ptr, None, B, H, W, D8, seeds, 0, 1.0, st))
    refused(name, fn(g[0].c_ptr, f[0].c_ptr, B, H, W, D8, None, 0, 1.0, st))
    refused(name, fn(g[0].c_ptr, f[0].c_ptr, B, H, W, 5, seeds, 0, 1.0, st))
    for b, h, w in sizes:
        refused(name, fn(g[0].c_ptr, f[0].c_ptr, b, h, w, D8, seeds, 0, 1.0, st))
    name, fn = "soil_slope_batch", hip.soil_slope_batch
    refused(name, fn(None, f[1].c_ptr, g[0].c_ptr, B, H, W, scales, B, st))
    refused(name, fn(f[0].c_ptr, None, g[0].c_ptr, B, H, W, scales, B, st))
    refused(name, fn(f[0].c_ptr, f[1].c_ptr, None, B, H, W, scales, B, st))
    refused(name, fn(f[0].c_ptr, f[1].c_ptr, g[0].c_ptr, B, H, W, None, B, st))
    for n in (0, B + 1, -1, 3):
        refused(name, fn(f[0].c_ptr, f[1].c_ptr, g[0].c_ptr, B, H, W, scales, n, st))
    for b, h, w in sizes:
        refused(name, fn(f[0].c_ptr, f[1].c_ptr, g[0].c_ptr, b, h, w, scales, 1, st))
    name, fn = "soil_accumulate_batch", hip.soil_accumulate_batch
    refused(name, fn(None, g[0].c_ptr, f[1].c_ptr, None, B, H, W, D8, st))
    refused(name, fn(f[0].c_ptr, None, f[1].c_ptr, None, B, H, W, D8, st))
    refused(name, fn(f[0].c_ptr, g[0].c_ptr, None, f[2].c_ptr, B, H, W, D8, st))
    refused(name, fn(f[0].c_ptr, g[0].c_ptr, f[1].c_ptr, f[2].c_ptr, B, H, W, 9, st))
    for b, h, w in sizes:
        refused(name, fn(f[0].c_ptr, g[0].c_ptr, f[1].c_ptr, None, b, h, w, D4, st))
    _abi.check(hip.soil_stream_synchronize(st))
    for t in f:
        assert (to_np(t) == mark_f).all()
    for t in g:
        assert (to_np(t) == mark_i).all()


if __name__ == "__main__":
    _child_main(sys.argv[1])
