"""The pointer-doubling engine (csrc/flow_paths.hpp) above its work-group cap, under its four entries: soil_flow_paths,
soil_downstream, soil_stream_power and soil_stream_power_deposit and their _batch forms.  A round runs on
min(ceil(elem / 256), 8192) work-groups; above 8192 * 256 = 2 097 152 cells a chunk a work-group strides over several
blocks of cells, its list segment holds several work-groups' worth of entries, the listed rounds walk lists longer
than a work-group and the final passes make several trips.  Every comparison is word for word (int32 and float bit
patterns, the NaN words included); there is no tolerance.

  true sizes   1027 x 2051 (the scalar init; a second trip that only the first 37 work-groups make, the last of them
               with 9 cells), 1100 x 2052 (the 16-byte init), 9 x 512^2 in one chunk (every final pass strided: 1024
               blocks a model against 911 work-groups), 4096^2 (eight trips, segments of 2048 entries, which the
               serpentine fills to the last entry in the first listed round)
  references   at the 2 M shapes the numpy restatements (ref.walk_doubling, dref.solve_doubling, dep.solve_iterated)
               on a chain through every cell, hostile entries, cycles and the oracle's steepest graph of a terrain;
               at 4096^2 the closed forms of tests/paths_cap_ref.py (held to the restatements, without a GPU, by
               tests/test_paths_above_cap.py).  Each is made once and left as it is.
  deposit      the residual is a maximum over strided trips: the cell whose change is largest placed outside its
               work-group's first trip, and inside it, the placement asserted from the reference
  small grids  the same code in child processes under SOIL_PATHS_GROUPS = 1, 3, 7 and 64 (read once per process), with
               the lists off and with 64-bit offsets: every graph, all four entries, a batch whole and in chunks
  not vacuous  every case asserts from its shape that its chunk is above the cap, and what the entry's info call says;
               the deposit cases and every child hold the scratch bytes to a restatement of ptr_layout
"""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import deposit_ref as dep
import downstream_ref as dref
import flow_paths_ref as ref
import paths_cap_ref as cap
from flow_paths_ref import D4, D8
from util import to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR_2M, VECTOR_2M = (1027, 2051), (1100, 2052)
SHAPES_2M = [SCALAR_2M, VECTOR_2M]
BATCH = (9, 512, 512)
BIG = (4096, 4096)
SCALE = (0.25, 3.0)
EXACT_SCALE, EXACT_UNIT = (0.25, 2.0), 0.25
BATCH_SCALES = [(0.25 * (1 + b), 3.0 / (1 + b % 4)) for b in range(BATCH[0])]
DT = 10.0
ALL = ("out", "out64", "flux", "residual")

SECONDS = {}                                                      # CPU seconds of each reference, by name
CACHES = []


def _clocked(fn):
    """The seconds of every call added up under the function's name."""
    @functools.wraps(fn)
    def inner(*args):
        t0 = time.perf_counter()
        out = fn(*args)
        SECONDS[fn.__name__] = SECONDS.get(fn.__name__, 0.0) + time.perf_counter() - t0
        return out
    return inner


def _timed(fn):
    """A reference made once: lru_cache around _clocked."""
    CACHES.append(functools.lru_cache(maxsize=None)(_clocked(fn)))
    return CACHES[-1]


@pytest.fixture(scope="module", autouse=True)
def _reference_seconds():
    """After the module: the seconds each reference took, and the references themselves let go."""
    yield
    print("\nCPU seconds of the references: " + ", ".join("%s %.1f" % kv for kv in sorted(SECONDS.items())))
    for c in CACHES:
        c.cache_clear()


def _frozen(out):
    for o in out.values() if isinstance(out, dict) else out:
        if isinstance(o, np.ndarray):
            o.setflags(write=False)
    return out


def _oracle():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


# ------------------------------------------------------------------ the device calls

def _np3(outs):
    return tuple(None if o is None else to_np(o) for o in outs)


def _flow_paths(graph, edge, scale=None, stop=None):
    from soillib_amd import soil
    fn = soil.flow_paths if np.ndim(graph) == 2 else soil.flow_paths_batch
    got = _np3(fn(to_gpu(graph), edge, scale, None if stop is None else to_gpu(stop)))
    return got, soil.flow_paths_info()


def _downstream(*args, **kw):
    from soillib_amd import soil
    from test_gpu_downstream import _run
    return _run(*args, **kw), soil.downstream_info()


def _deposit(*args, **kw):
    from soillib_amd import soil
    from test_gpu_deposit import _run
    return _run(*args, **kw), soil.stream_power_deposit_info()


def _expect_info(info, H, W, vec=None):
    """One chunk, the init form W takes (aligned planes), 32-bit offsets, the rounds of one model."""
    vec = int(W % 4 == 0) if vec is None else vec
    assert info == dict(chunks=1, vec_chunks=vec, idx64_chunks=0, rounds=cap.ceil_log2(H * W)), info


def _deposit_layout_holds(graph, edge, planes, scales, groups=cap.CAP):
    """The scratch of the shape under `groups`: a call that accumulates nothing (iters 1, out alone), so that the bytes
    it reports are the engine's and the planes', restated."""
    _, info = _deposit(graph, edge, planes["height"], planes["erosivity"], planes["deposition"], scales, DT, None, 1, want=("out",))
    B = 1 if np.ndim(graph) == 2 else graph.shape[0]
    assert info["chunks"] == 1 and info["iters"] == 1
    assert info["scratch_bytes"] == cap.deposit_bytes(graph.size, B, np.size(scales) > 2, groups), (info, groups)


# ------------------------------------------------------------------ inputs and references, made once

def graph_2m(H, W, edge, name):
    return _graph_2m(H, W, edge if name == "steepest" else D8, name)        # (the built graphs do not depend on the edge)


@_timed
def _graph_2m(H, W, edge, name):
    if name == "serpentine":
        g = cap.graph_of("serpentine", H, W)[0].copy()
    elif name == "hostile":
        g = ref.hostile(H, W, 21)
    elif name == "cycles":
        g = ref.cycles(H, W)
    else:
        g = _oracle().steepest((ref.terrain(H, W, 2) * 10).astype(np.float32), edge)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _stop(H, W):
    s = cap.stop_plane(H, W, 4, 1e-4)
    s.setflags(write=False)
    return s


@_timed
def walk_2m(H, W, edge, name, stopped):
    return _frozen(ref.walk_doubling(graph_2m(H, W, edge, name), edge, SCALE, _stop(H, W) if stopped else None))


@functools.lru_cache(maxsize=None)
def _coeffs(H, W, draw=0):
    """The draws of tests/test_gpu_downstream.py: a, b in [-1, 1] and t in [-10, 10]; a height in [0, 100], an
    erosivity over 1e-6 .. 1e3 and an uplift in [0, 0.01]."""
    r = np.random.default_rng([draw, H, W])
    a, b = (r.uniform(-1.0, 1.0, (H, W)).astype(np.float32) for _ in range(2))
    t = r.uniform(-10.0, 10.0, (H, W)).astype(np.float32)
    height = (r.random((H, W)) * 100.0).astype(np.float32)
    erosivity = np.exp(r.uniform(np.log(1e-6), np.log(1e3), (H, W))).astype(np.float32)
    uplift = (r.random((H, W)) * 0.01).astype(np.float32)
    return _frozen(dict(a=a, b=b, t=t, height=height, erosivity=erosivity, uplift=uplift))


def _edge_of(name):
    return D8 if name == "steepest" else D4


@_timed
def sums_2m(H, W, name, with_b, stopped):
    c, edge = _coeffs(H, W), _edge_of(name)
    out = dref.solve_doubling(graph_2m(H, W, edge, name), edge, c["a"], c["b"] if with_b else None, c["t"], SCALE,
                              _stop(H, W) if stopped else None)
    assert (np.isnan(out[1]) == ~out[2]).all() and out[2].all(), "a draw made a NaN of its own"
    return _frozen(out)


@_timed
def power_2m(H, W, name, uplift):
    c, edge = _coeffs(H, W), _edge_of(name)
    out = dref.solve_doubling(graph_2m(H, W, edge, name), edge, scale=SCALE,
                              power=(c["height"], c["erosivity"], c["uplift"] if uplift else None, DT))
    assert out[2].all() and not np.isnan(out[1]).any()
    return _frozen(out)


@_timed
def chains_big(name, edge):
    return cap.Chains(name, *BIG, edge)


@_clocked
def walk_big(c, scale, stop):
    return c.walk(scale, stop)


@_clocked
def sums_big(c, a, b, t, scale):
    return c.sums(a, b, t, scale)


@_timed
def stop_big():
    s = cap.stop_plane(*BIG, 6, 1e-5)
    s.setflags(write=False)
    return s


@_timed
def planes_big():
    return _frozen(cap.exact_planes(*BIG, 9, cut=1e-5))


# ------------------------------------------------------------------ flow_paths

@pytest.mark.parametrize("H,W", SHAPES_2M)
@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("name", ["serpentine", "hostile", "cycles", "steepest"])
@pytest.mark.parametrize("stopped", [False, True])
def test_flow_paths_just_above_the_cap(hip, H, W, edge, name, stopped):
    assert cap.above(H * W) and cap.layout(H * W, 0)["seg"] == 512
    want = walk_2m(H, W, edge, name, stopped)
    if name == "serpentine" and not stopped:
        assert want[1][0, 0] == H * W - 1, "every round is needed"
    if name == "cycles":
        assert (want[0] == -1).any() and (want[0] >= 0).any()
    got, info = _flow_paths(graph_2m(H, W, edge, name), edge, SCALE, _stop(H, W) if stopped else None)
    _expect_info(info, H, W)
    ref.same_words(got, want, "%s %dx%d edge %d stop %s" % (name, H, W, edge, stopped))


@pytest.mark.parametrize("name,edge", [("serpentine", D4), ("comb", D4), ("staircase", D8)])
@pytest.mark.parametrize("stopped", [False, True])
def test_flow_paths_at_4096(hip, name, edge, stopped):
    H, W = BIG
    L = cap.layout(H * W, 0)
    assert cap.above(H * W) and (L["groups"], L["seg"], H * W // (256 * L["groups"])) == (8192, 2048, 8)
    c = chains_big(name, edge)
    stop = stop_big() if stopped else None
    scale = (3.0, 4.0) if name == "staircase" else SCALE
    want = walk_big(c, scale, stop)
    if name == "serpentine" and not stopped:
        assert want[1][0, 0] == H * W - 1 and (want[1] > 0).sum() == H * W - 1, "all but one cell are listed: full segments"
    got, info = _flow_paths(c.graph, edge, scale, stop)
    _expect_info(info, H, W)
    ref.same_words(got, want, "%s 4096^2 stop %s" % (name, stopped))


@_timed
def batch_graphs(edge):
    """Nine models, neighbours with different graphs, one of them hostile; a stop plane on every other model."""
    B, H, W = BATCH
    o = _oracle()
    makers = [lambda: cap.graph_of("serpentine", H, W)[0], lambda: ref.hostile(H, W, 31, model=1),
              lambda: o.steepest((ref.terrain(H, W, 3) * 10).astype(np.float32), edge), lambda: ref.cycles(H, W),
              lambda: cap.graph_of("comb", H, W)[0], lambda: o.steepest((ref.terrain(H, W, 5, True) * 10).astype(np.float32), edge),
              lambda: cap.graph_of("staircase", H, W)[0], lambda: ref.hostile(H, W, 32, model=7),
              lambda: ref.all_donors(H, W, edge)]
    graph = np.stack([m() for m in makers]).astype(np.int32)
    stop = np.stack([cap.stop_plane(H, W, 10 + b, 1e-3) if b % 2 else np.zeros((H, W), np.int32) for b in range(B)])
    return _frozen((graph, stop))


@_timed
def batch_walk(edge):
    graph, stop = batch_graphs(edge)
    return _frozen(ref.walk_batch(ref.walk_doubling, graph, edge, BATCH_SCALES, stop))


@pytest.mark.parametrize("edge", [D4, D8])
def test_flow_paths_batch_of_nine_in_one_chunk(hip, edge):
    B, H, W = BATCH
    assert cap.above(B * H * W) and (H * W + 255) // 256 == 1024 and (8192 + B - 1) // B == 911
    graph, stop = batch_graphs(edge)
    got, info = _flow_paths(graph, edge, BATCH_SCALES, stop)
    _expect_info(info, H, W)
    ref.same_words(got, batch_walk(edge), "9 x 512^2 edge %d" % edge)


# ------------------------------------------------------------------ downstream

@pytest.mark.parametrize("H,W", SHAPES_2M)
@pytest.mark.parametrize("name", ["serpentine", "steepest"])
@pytest.mark.parametrize("with_b", [True, False])
def test_downstream_just_above_the_cap(hip, H, W, name, with_b):
    assert cap.above(H * W)
    c, edge = _coeffs(H, W), _edge_of(name)
    got, info = _downstream(graph_2m(H, W, edge, name), edge, c["a"], c["b"] if with_b else None, c["t"], SCALE)
    _expect_info(info, H, W)
    dref.same_words(got, sums_2m(H, W, name, with_b, False), "%s %dx%d b %s" % (name, H, W, with_b))


def test_downstream_just_above_the_cap_with_pour_points(hip):
    H, W = VECTOR_2M
    assert cap.above(H * W) and (_stop(H, W) != 0).sum() > 100
    c = _coeffs(H, W)
    got, info = _downstream(graph_2m(H, W, D4, "serpentine"), D4, c["a"], c["b"], c["t"], SCALE, _stop(H, W))
    _expect_info(info, H, W)
    dref.same_words(got, sums_2m(H, W, "serpentine", True, True), "serpentine with pour points")


@pytest.mark.parametrize("name", ["serpentine", "comb"])
@pytest.mark.parametrize("with_b", [False, True])
def test_exact_downstream_sums_at_4096(hip, name, with_b):
    H, W = BIG
    assert cap.above(H * W) and cap.layout(H * W, 8)["seg"] == 2048
    c = chains_big(name, D4)
    a, b, t = planes_big()
    b = b if with_b else None
    assert cap.exact(c.weights(a, t, EXACT_SCALE), EXACT_UNIT)
    want = sums_big(c, a, b, t, EXACT_SCALE)
    if with_b:
        assert ((b.reshape(-1) == 0) & c.has_edge).sum() > 50, "chains that are cut"
    elif name == "serpentine":
        assert (want[0].astype(np.float64) != want[1]).any(), "sums that float32 rounds"
    got, info = _downstream(c.graph, D4, a, b, t, EXACT_SCALE)
    _expect_info(info, H, W)
    dref.same_words(got, want, "%s 4096^2 b %s" % (name, with_b))


# ------------------------------------------------------------------ stream_power

@pytest.mark.parametrize("H,W", SHAPES_2M)
@pytest.mark.parametrize("name", ["steepest", "serpentine"])
@pytest.mark.parametrize("uplift", [True, False])
def test_stream_power_just_above_the_cap(hip, H, W, name, uplift):
    assert cap.above(H * W)
    c, edge = _coeffs(H, W), _edge_of(name)
    got, info = _downstream(graph_2m(H, W, edge, name), edge, scale=SCALE,
                            power=(c["height"], c["erosivity"], c["uplift"] if uplift else None, DT))
    _expect_info(info, H, W)
    dref.same_words(got, power_2m(H, W, name, uplift), "%s %dx%d uplift %s" % (name, H, W, uplift))


@_timed
def batch_terrains():
    """Nine terrains, their D8 steepest graphs and the planes of the deposit step, model by model."""
    B, H, W = BATCH
    o = _oracle()
    height = np.stack([(ref.terrain(H, W, 2 + b) * 10).astype(np.float32) for b in range(B)])
    graph = np.stack([o.steepest(height[b], D8) for b in range(B)])
    r = np.random.default_rng([B, H, W])
    planes = dict(height=height, erosivity=np.exp(r.uniform(np.log(1e-3), np.log(10.0), (B, H, W))).astype(np.float32),
                  deposition=r.uniform(0.0, 2.0, (B, H, W)).astype(np.float32),
                  uplift=(r.random((B, H, W)) * 0.01).astype(np.float32))
    return _frozen((graph,)) + (_frozen(planes),)


@_timed
def batch_power():
    graph, p = batch_terrains()
    return _frozen(dref.solve_batch(dref.solve_doubling, graph, D8, scale=BATCH_SCALES,
                                    power=(p["height"], p["erosivity"], p["uplift"], DT)))


def test_stream_power_batch_of_nine_in_one_chunk(hip):
    B, H, W = BATCH
    assert cap.above(B * H * W) and (H * W + 255) // 256 > (8192 + B - 1) // B, "the final pass strides"
    graph, p = batch_terrains()
    got, info = _downstream(graph, D8, scale=BATCH_SCALES, power=(p["height"], p["erosivity"], p["uplift"], DT))
    _expect_info(info, H, W)
    want = batch_power()
    assert want[2].all()
    dref.same_words(got, want, "9 x 512^2")


# ------------------------------------------------------------------ stream_power_deposit

def _damped(deposition, keep):
    """The deposition plane, divided by 64 outside `keep`: the changes of an iteration are largest where it is kept."""
    return np.where(keep, deposition, deposition * np.float32(1.0 / 64.0)).astype(np.float32)


def _trip_of_the_largest_change(steps, k, groups):
    """(trip, work-group) in k_dep_final on `groups` work-groups a model of the cell whose iterate changed most in
    iteration k >= 2, from the reference: argmax |x^k - x^(k-1)|, which must be the residual the reference reports."""
    diff = np.abs(steps[k - 1]["out64"] - steps[k - 2]["out64"]).reshape(-1)
    assert not np.isnan(diff).any()
    at = int(np.argmax(diff))
    assert dref.words(np.float64(diff[at])) == dref.words(np.float64(steps[k - 1]["residual"])) and diff[at] > 0
    assert (diff == diff[at]).sum() == 1, "one cell alone holds the maximum"
    return at // 256 // groups, at // 256 % groups


@_timed
def deposit_2m(place):
    """The planes and what iters = 1, 2, 3 return at 1100 x 2052: `place` "late": the largest change outside the first
    trip of k_dep_final's 8192 work-groups (cells from 8192 * 256 on), "first": inside the first trip of one of the 626
    work-groups that make a second (8818 blocks): there a later trip's word could take its place."""
    H, W = VECTOR_2M
    graph = graph_2m(H, W, D8, "steepest")
    r = np.random.default_rng([7, H, W])
    n = np.arange(H * W).reshape(H, W)
    keep = n >= cap.CAP * 256 if place == "late" else n < ((H * W + 255) // 256 - cap.CAP) * 256
    planes = dict(height=(ref.terrain(H, W, 2) * 10).astype(np.float32),
                  erosivity=np.exp(r.uniform(np.log(1e-3), np.log(10.0), (H, W))).astype(np.float32),
                  deposition=_damped(r.uniform(0.0, 2.0, (H, W)).astype(np.float32), keep),
                  uplift=(r.random((H, W)) * 0.01).astype(np.float32))
    steps = dep.solve_iterated(_oracle(), graph, D8, planes["height"], planes["erosivity"], planes["deposition"], SCALE, DT,
                               planes["uplift"], 3, every=True)["steps"]
    for s in steps:
        assert s["final"].all() and not np.isnan(s["out64"]).any()
        _frozen(s)
    return graph, _frozen(planes), steps


@pytest.mark.parametrize("place,iters", [("late", 2), ("late", 3), ("first", 2)])
def test_deposit_just_above_the_cap(hip, place, iters):
    H, W = VECTOR_2M
    assert cap.above(H * W) and (H * W + 255) // 256 > cap.CAP, "k_dep_final strides"
    graph, p, steps = deposit_2m(place)
    trip, group = _trip_of_the_largest_change(steps, iters, cap.CAP)
    assert trip == (1 if place == "late" else 0) and group < (H * W + 255) // 256 - cap.CAP, "a work-group of two trips"
    _deposit_layout_holds(graph, D8, p, SCALE)
    got, info = _deposit(graph, D8, p["height"], p["erosivity"], p["deposition"], SCALE, DT, p["uplift"], iters)
    assert info["chunks"] == 1 and info["iters"] == iters
    dep.same_words(got, steps[iters - 1], "1100x2052 iters %d, the largest change in trip %d" % (iters, trip))


@_timed
def deposit_batch():
    """The batch of nine: even models keep their deposition where k_dep_final's 911 work-groups a model make their second
    trip (cells from 911 * 256 on), odd models in the first trip of the 113 work-groups that make a second."""
    B, H, W = BATCH
    graph, p = batch_terrains()
    n = np.arange(H * W).reshape(H, W)
    late, first = n >= 911 * 256, n < (1024 - 911) * 256
    planes = dict(p, deposition=np.stack([_damped(p["deposition"][b], late if b % 2 == 0 else first) for b in range(B)]))
    o = _oracle()
    runs = [dep.solve_iterated(o, graph[b], D8, planes["height"][b], planes["erosivity"][b], planes["deposition"][b],
                               BATCH_SCALES[b], DT, planes["uplift"][b], 3, every=True)["steps"] for b in range(B)]
    steps = [{k: np.stack([np.asarray(run[i][k]) for run in runs]) for k in ALL + ("final",)} for i in range(3)]
    trips = [[_trip_of_the_largest_change(run, k, 911) for run in runs] for k in (2, 3)]
    return graph, _frozen(planes), [_frozen(s) for s in steps], trips


@pytest.mark.parametrize("iters", [2, 3])
def test_deposit_batch_of_nine_in_one_chunk(hip, iters):
    B, H, W = BATCH
    assert cap.above(B * H * W) and (H * W + 255) // 256 == 1024 and (8192 + B - 1) // B == 911
    graph, p, steps, trips = deposit_batch()
    assert [t for t, _ in trips[iters - 2]] == [1 if b % 2 == 0 else 0 for b in range(B)], "where each model's largest change lies"
    assert all(g < 1024 - 911 for _, g in trips[iters - 2]), "in a work-group of two trips"
    assert steps[iters - 1]["final"].all()
    _deposit_layout_holds(graph, D8, p, BATCH_SCALES)
    got, info = _deposit(graph, D8, p["height"], p["erosivity"], p["deposition"], BATCH_SCALES, DT, p["uplift"], iters)
    assert info["chunks"] == 1 and info["iters"] == iters
    dep.same_words(got, steps[iters - 1], "9 x 512^2 iters %d" % iters)


# ------------------------------------------------------------------ the same code on small grids: SOIL_PATHS_GROUPS

KNOB_SHAPES = [(37, 53), (33, 260), (9, 1028)]
KNOB_BATCH = (5, 33, 260)
SETTINGS = {"groups_1": (1, {}), "groups_3": (3, {}), "groups_7": (7, {}), "groups_64": (64, {}),
            "groups_3_lists_off": (3, {"SOIL_PATHS_LIST_FROM": "0"}), "groups_3_idx64": (3, {"SOIL_PATHS_IDX64": "1"})}
KNOB_SCALES = [(0.3, 0.7), (1.0, 1.0), (2.5, 0.125)]


def knob_cases(groups):
    """The shapes a setting takes: those whose chunk has more blocks of 256 cells than `groups`; ("batch",) the batch."""
    B, H, W = KNOB_BATCH
    return [s for s in KNOB_SHAPES if cap.above(s[0] * s[1], groups)] + ([("batch",)] if cap.above(B * H * W, groups) else [])


@functools.lru_cache(maxsize=None)
def knob_graphs(H, W, edge):
    out = dict(ref.built_graphs(H, W, edge))
    out["descent"] = ref.descent((ref.terrain(H, W, 2) * 10).astype(np.float32), edge)
    out["descent_random"] = ref.descent((ref.terrain(H, W, 4) * 10).astype(np.float32), edge, seed=7)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def knob_planes(H, W, draw):
    """The draws of the downstream tests and, for the deposit step, a terrain's height and a deposition in [0, 2]."""
    r = np.random.default_rng([draw, H, W, 5])
    out = dict(_coeffs(H, W, draw), terrain=(ref.terrain(H, W, 2 + draw) * 10).astype(np.float32),
               kd=np.exp(r.uniform(np.log(1e-3), np.log(10.0), (H, W))).astype(np.float32),
               deposition=r.uniform(0.0, 2.0, (H, W)).astype(np.float32), stop=cap.stop_plane(H, W, 20 + draw, 0.01))
    return _frozen(out)


def knob_calls(H, W, edge):
    """(key, entry, arguments) of every call on one shape: each graph through all four entries, with and without a
    stop plane, b and the uplift; the deposit step with iters = 3."""
    for k, (gname, g) in enumerate(sorted(knob_graphs(H, W, edge).items())):
        p, scale = knob_planes(H, W, k % 2), KNOB_SCALES[k % 3]
        key = "%dx%d_e%d_%s_" % (H, W, edge, gname)
        yield key + "walk", "walk", (g, edge, scale, None)
        yield key + "walk_stop", "walk", (g, edge, scale, p["stop"])
        yield key + "sum", "sum", dict(graph=g, edge=edge, a=p["a"], b=p["b"], t=p["t"], scale=scale)
        yield key + "sum_stop", "sum", dict(graph=g, edge=edge, a=p["a"], t=p["t"], scale=scale, stop=p["stop"])
        yield key + "power", "sum", dict(graph=g, edge=edge, scale=scale, power=(p["height"], p["erosivity"], p["uplift"], DT))
        yield key + "power_stop", "sum", dict(graph=g, edge=edge, scale=scale, stop=p["stop"], power=(p["height"], p["erosivity"], None, DT))
        yield key + "deposit", "deposit", (g, edge, p["terrain"], p["kd"], p["deposition"], scale, DT, p["uplift"] if k % 2 == 0 else None, 3)


def knob_batch_calls(edge):
    """The same for the batch of five: neighbours differ in graph, scale and draw; a pair per model."""
    B, H, W = KNOB_BATCH
    names = sorted(knob_graphs(H, W, edge))
    cfg = [(names[(3 * b + 1) % len(names)], KNOB_SCALES[b % 3], b % 2) for b in range(B)]
    g = np.stack([knob_graphs(H, W, edge)[n] for n, _, _ in cfg])
    p = {k: np.stack([knob_planes(H, W, d)[k] for _, _, d in cfg]) for k in knob_planes(H, W, 0)}
    scales = [s for _, s, _ in cfg]
    key = "batch_e%d_" % edge
    yield key + "walk_stop", "walk", (g, edge, scales, p["stop"])
    yield key + "sum", "sum", dict(graph=g, edge=edge, a=p["a"], b=p["b"], t=p["t"], scale=scales)
    yield key + "power_stop", "sum", dict(graph=g, edge=edge, scale=scales, stop=p["stop"], power=(p["height"], p["erosivity"], p["uplift"], DT))
    yield key + "deposit", "deposit", (g, edge, p["terrain"], p["kd"], p["deposition"], scales, DT, p["uplift"], 3)


def _device(entry, args):
    """A call's outputs as a dict of planes."""
    if entry == "walk":
        return dict(zip(ref.NAMES, _flow_paths(*args)[0]))
    if entry == "sum":
        return dict(zip(("out", "out64"), _downstream(**args)[0]))
    return _deposit(*args)[0]


@functools.lru_cache(maxsize=None)
def knob_want(shape, edge):
    """key -> the restatement's outputs of every call on a shape (or the batch), made once for all settings."""
    out = {}
    o = _oracle()
    for key, entry, args in (knob_batch_calls(edge) if shape == ("batch",) else knob_calls(*shape, edge)):
        batch = shape == ("batch",)
        if entry == "walk":
            w = ref.walk_batch(ref.walk_doubling, *args) if batch else ref.walk_doubling(*args)
            out[key] = dict(zip(ref.NAMES, w))
        elif entry == "sum":
            w = dref.solve_batch(dref.solve_doubling, **args) if batch else dref.solve_doubling(**args)
            out[key] = dict(out=w[0], out64=w[1])
        else:
            solve = lambda *a: dep.solve_iterated(o, *a)
            out[key] = dep.solve_batch(solve, *args) if batch else dep.solve_iterated(o, *args)
    return out


def _child_main(path, groups):
    """The child of test_small_grids_under_the_groups_knob: asserts once that the knob is in force (the deposit call's
    scratch against the layout restated for `groups`), then every call of every shape the setting takes; the batch
    whole and in chunks of 2 + 2 + 1 models (SOIL_FLOW_BATCH_CELLS, read per call)."""
    B, H, W = KNOB_BATCH
    p = {k: np.stack([knob_planes(H, W, 0)[k]] * B) for k in ("height", "erosivity", "deposition")}
    assert cap.deposit_bytes(B * H * W, B, False, groups) != cap.deposit_bytes(B * H * W, B, False)
    _deposit_layout_holds(np.stack([knob_graphs(H, W, D8)["descent"]] * B), D8, p, KNOB_SCALES[0], groups)
    out = {}
    for shape in knob_cases(groups):
        for edge in (D4, D8):
            if shape == ("batch",):
                for chunked in (False, True):
                    if chunked:
                        os.environ["SOIL_FLOW_BATCH_CELLS"] = str(2 * H * W + H * W // 2)
                    for key, entry, args in knob_batch_calls(edge):
                        for name, plane in _device(entry, args).items():
                            out["%s%s/%s" % (key, "_chunked" if chunked else "", name)] = plane
                    os.environ.pop("SOIL_FLOW_BATCH_CELLS", None)
            else:
                for key, entry, args in knob_calls(*shape, edge):
                    for name, plane in _device(entry, args).items():
                        out["%s/%s" % (key, name)] = plane
    np.savez(path, **out)


def test_which_shapes_each_setting_takes():
    pairs = [(name, shape) for name, (groups, _) in SETTINGS.items() for shape in knob_cases(groups)]
    assert len(pairs) == 21 and knob_cases(64) == [("batch",)]
    for groups in (1, 3, 7):
        assert knob_cases(groups) == KNOB_SHAPES + [("batch",)]
    # the chunks of 2 + 2 + 1 models under 64 work-groups: segments of 512 entries, then of 256 for the last
    B, H, W = KNOB_BATCH
    assert [cap.layout(m * H * W, 0, 64)["seg"] for m in (5, 2, 1)] == [768, 512, 256]
    assert [cap.layout(m * H * W, 0, 3)["seg"] for m in (5, 2, 1)] == [14336, 5888, 3072]


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_small_grids_under_the_groups_knob(hip, tmp_path, setting):
    """One child per setting (SOIL_PATHS_GROUPS is read once per process), one after the other."""
    groups, more = SETTINGS[setting]
    path = str(tmp_path / "knob.npz")
    env = dict(os.environ)
    for name in ("SOIL_FLOW_BATCH_CELLS", "SOIL_PATHS_LIST_FROM", "SOIL_PATHS_IDX64", "SOIL_PATHS_GROUPS"):
        env.pop(name, None)
    env.update(more, SOIL_PATHS_GROUPS=str(groups))
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path, str(groups)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    shapes = knob_cases(groups)
    assert shapes and all(cap.above(KNOB_BATCH[0] * KNOB_BATCH[1] * KNOB_BATCH[2] if s == ("batch",) else s[0] * s[1], groups) for s in shapes)
    seen = 0
    for shape in shapes:
        for edge in (D4, D8):
            for key, want in knob_want(shape, edge).items():
                for suffix in ("", "_chunked") if shape == ("batch",) else ("",):
                    planes = {f.split("/")[1]: got[f] for f in got.files if f.startswith(key + suffix + "/")}
                    seen += len(planes)
                    what = "%s%s under %s" % (key, suffix, setting)
                    if "terminal" in planes:
                        ref.same_words([planes[n] for n in ref.NAMES], [want[n] for n in ref.NAMES], what)
                    elif "flux" in planes:
                        assert sorted(planes) == sorted(ALL)
                        dep.same_words(planes, want, what)
                    else:
                        dref.same_words((planes["out"], planes["out64"]), (want["out"], want["out64"]), what)
    assert seen == len(got.files) and seen > 0


if __name__ == "__main__":
    _child_main(sys.argv[1], int(sys.argv[2]))
