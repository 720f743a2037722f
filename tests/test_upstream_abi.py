"""Upstream extrema along a receiver graph (include/soil_hip.h: "flow graphs: upstream extrema"; soil_upstream_extreme,
soil_upstream_extreme_batch), what can be checked without a GPU: the reference of tests/upstream_ref.py against
reachability itself on small graphs with cycles, the key order and the ties of `arg` on hand-made cells, the four
properties of a breached surface on the reference, the header, the bound symbols and the surfaces, every refusal of the
two entries with the entry's name and its text, SOIL_ERR_NO_DEVICE for a well-formed call, and the ValueErrors of the
Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flow_paths_ref as fref
import upstream_ref as ref
from upstream_ref import D4, D8, MAX, MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(*words):
    return np.array(words, np.uint32).view(np.float32)


# ---- the reference against reachability ------------------------------------------------------------------------

@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("op", [MIN, MAX])
def test_the_sweep_is_reachability_on_small_graphs_with_cycles(edge, op):
    H, W = 6, 7
    r = np.random.default_rng([edge, op])
    built = ref.graphs(H, W, edge)
    for seed in range(12):                                        # random neighbours: trees, chains and cycles of any length
        n = np.arange(H * W).reshape(H, W)
        step = r.choice(np.array([-W - 1, -W, -W + 1, -1, 1, W - 1, W, W + 1, 0, 1000]), (H, W))
        built["random %d" % seed] = (n + step).astype(np.int32)
    cycles = 0
    for name, g in built.items():
        for kind in ref.VALUES:
            v = ref.values(H, W, kind, 5)
            for stop in (None, ref.stop_plane(H, W, 1)):
                ref.same(ref.extreme(g, v, edge, op, stop), ref.brute(g, v, edge, op, stop),
                         "%s, %s, stop %s" % (name, kind, stop is not None))
        cycles += int((fref.walk_serial(g, edge)[0] < 0).any())
    assert cycles >= 8, "the random graphs are meant to have cycles"


def test_the_closed_form_on_the_serpentine_is_the_sweep():
    for H, W in ((1, 9), (5, 4), (7, 9)):
        for op in (MIN, MAX):
            for kind in ("random", "nan_third", "plateau"):
                v = ref.values(H, W, kind, 2)
                g, out, arg = ref.chain_extreme(H, W, v, op)
                assert (g == fref.serpentine(H, W)).all()
                ref.same((out, arg), ref.extreme(g, v, D4, op), "serpentine %dx%d %s" % (H, W, kind))


# ---- the order and the ties, by hand ---------------------------------------------------------------------------

CHAIN = np.array([[1, 2, 3, 4, -1]], np.int32)                    # 0 -> 1 -> 2 -> 3 -> 4


def test_a_chain_by_hand():
    v = np.array([[3.0, 1.0, 2.0, 1.0, 5.0]], np.float32)
    out, arg = ref.extreme(CHAIN, v, D8, MIN)
    assert out.tolist() == [[3.0, 1.0, 1.0, 1.0, 1.0]] and arg.tolist() == [[0, 1, 1, 1, 1]]   # the tie: cell 1, not 3
    out, arg = ref.extreme(CHAIN, v, D8, MAX)
    assert out.tolist() == [[3.0, 3.0, 3.0, 3.0, 5.0]] and arg.tolist() == [[0, 0, 0, 0, 4]]
    stop = np.array([[0, 1, 0, 0, 0]], np.int32)                  # cell 1 collects and passes nothing on
    out, arg = ref.extreme(CHAIN, v, D8, MIN, stop)
    assert out.tolist() == [[3.0, 1.0, 2.0, 1.0, 1.0]] and arg.tolist() == [[0, 1, 2, 3, 3]]


def test_signed_zeros_denormals_infinities():
    pz, nz, den, nden = 0x00000000, 0x80000000, 0x00000001, 0x80000001
    v = _f32(pz, nz, den, nden, 0x7F800000).reshape(1, 5)
    out, arg = ref.extreme(CHAIN, v, D8, MIN)
    assert out.view(np.uint32).tolist() == [[pz, nz, nz, nden, nden]] and arg.tolist() == [[0, 1, 1, 3, 3]]
    out, arg = ref.extreme(CHAIN, v, D8, MAX)                     # +0 wins over -0, a denormal over both, +inf over all
    assert out.view(np.uint32).tolist() == [[pz, pz, den, den, 0x7F800000]] and arg.tolist() == [[0, 0, 2, 2, 4]]
    v = _f32(0xFF800000, 0x7F800000, nz, pz, nz).reshape(1, 5)
    out, arg = ref.extreme(CHAIN, v, D8, MIN)
    assert out.view(np.uint32).tolist() == [[0xFF800000] * 5] and arg.tolist() == [[0] * 5]


def test_nan_is_ignored_where_a_number_arrives_and_canonical_where_none_does():
    qnan, snan, nnan = 0x7FC00001, 0x7F800001, 0xFFC12345
    v = _f32(qnan, snan, 0x40000000, nnan, 0xC0000000).reshape(1, 5)          # NaN NaN 2 NaN -2
    for op, want, where in ((MIN, [0x7FC00000, 0x7FC00000, 0x40000000, 0x40000000, 0xC0000000], [-1, -1, 2, 2, 4]),
                            (MAX, [0x7FC00000, 0x7FC00000, 0x40000000, 0x40000000, 0x40000000], [-1, -1, 2, 2, 2])):
        out, arg = ref.extreme(CHAIN, v, D8, op)
        assert out.view(np.uint32).tolist() == [want] and arg.tolist() == [where], op


def test_a_cycle_takes_everything_that_drains_into_it():
    g = np.array([[1, 2, 1, -1, 3]], np.int32)                    # 0 -> 1 <-> 2; 3 a terminal; 4 -> 3
    v = np.array([[-4.0, 7.0, 6.0, 1.0, 0.5]], np.float32)
    out, arg = ref.extreme(g, v, D8, MIN)
    assert out.tolist() == [[-4.0, -4.0, -4.0, 0.5, 0.5]] and arg.tolist() == [[0, 0, 0, 4, 4]]
    out, arg = ref.extreme(g, v, D8, MAX)
    assert out.tolist() == [[-4.0, 7.0, 7.0, 1.0, 0.5]] and arg.tolist() == [[0, 1, 1, 3, 4]]


def test_the_keys_are_monotone_and_come_back():
    v = np.array([-np.inf, -3.4e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.4e38, np.inf], np.float32)
    k = ref.key_of(ref.bits(v))
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert (ref.bits_of(k) == ref.bits(v)).all()
    assert (ref.key_of(np.array([0x7FC00000, 0xFFFFFFFF, 0x7F800001], np.uint32)) == ref.NAN_KEY).all()
    assert ref.NAN_KEY > k.max()


# ---- the four properties of a breached surface, on the reference -----------------------------------------------

@pytest.mark.parametrize("edge", [D4, D8])
def test_the_properties_of_a_breached_surface(edge):
    H, W = 20, 24
    h = fref.terrain(H, W, 3, True)
    downhill = fref.descent(h, edge)
    breached, _ = ref.extreme(downhill, h, edge, MIN)
    assert (ref.bits(breached) == ref.bits(h)).all(), "a strictly downhill graph leaves the heights as they are"
    h[3, 4] = np.array([0xFFC00123], np.uint32).view(np.float32)[0]
    for name, g in ref.graphs(H, W, edge).items():
        breached, _ = ref.extreme(g, h, edge, MIN)
        ref.check_breached(h, breached, g, edge)
        again, _ = ref.extreme(g, breached, edge, MIN)
        assert (ref.bits(again) == ref.bits(breached)).all(), "breach is idempotent (%s)" % name


# ---- the header, the symbols, the surfaces ---------------------------------------------------------------------

ENTRIES = {
    "soil_upstream_extreme": "float* out, int32_t* arg, const int32_t* graph, const float* value, const int32_t* stop, "
                             "int64_t H, int64_t W, int edge, int op, void* stream",
    "soil_upstream_extreme_batch": "float* out, int32_t* arg, const int32_t* graph, const float* value, "
                                   "const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, int op, void* stream",
    "soil_upstream_extreme_info": "int64_t info[4]",
}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
    flat = _squash(re.sub(r"\n \* ?", "\n", text))
    for phrase in ("-inf < ... < -0 < +0 < ... < +inf < NaN", "key_of", "0x7fc00000", "u reaches n iff",
                   "Cycles are allowed", "+0 wins over -0", "the smallest index", "-1 where out[n] is NaN",
                   "word for word those of soil_flow_paths", "passes nothing on", "`op` not 0 or 1",
                   "SOIL_FLOW_BATCH_CELLS", "Either of `out` and `arg` may be NULL, not both"):
        assert phrase in flat, phrase


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    i64, vp, cint = C.c_int64, C.c_void_p, C.c_int
    assert _abi.SIGNATURES["soil_upstream_extreme"] == (cint, [vp, vp, vp, vp, vp, i64, i64, cint, cint, vp])
    assert _abi.SIGNATURES["soil_upstream_extreme_batch"] == (cint, [vp, vp, vp, vp, vp, i64, i64, i64, cint, cint, vp])
    assert _abi.SIGNATURES["soil_upstream_extreme_info"] == (cint, [C.POINTER(i64)])
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_upstream_extreme(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["upstream.hip"]
    source = open(os.path.join(build.CSRC, "upstream.hip")).read()
    assert "atomicMin" in source and "WS_UPSTREAM" in source
    for other in ("flow_paths.hip", "downstream.hip", "graph.hip"):
        assert "upstream_extreme" not in open(os.path.join(build.CSRC, other)).read(), other


def test_the_surfaces():
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch, ErosionModel
    for name in ("upstream_min", "upstream_max", "upstream_min_batch", "upstream_max_batch", "upstream_info", "breach",
                 "breach_batch", "condition_breached", "condition_breached_batch", "upstream_length",
                 "upstream_length_batch"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    for name in ("upstream_min", "upstream_max", "breached", "upstream_length"):
        assert callable(getattr(ErosionBatch, name)) and not hasattr(ErosionModel, name), name
    assert "adds no mass" in ErosionBatch.breached.__doc__ and "stream_power_batch" in ErosionBatch.breached.__doc__
    # nothing new is named in soil.hpp, and no knob came with the entries
    text = open(os.path.join(ROOT, "include", "soil.hpp")).read()
    for word in ("upstream_extreme", "upstream_min", "upstream_max", "upstream_length", "breach"):
        assert word not in text, word
    knobs = open(os.path.join(ROOT, "docs", "KNOBS.md")).read()
    for knob in ("SOIL_PATHS_GROUPS", "SOIL_PATHS_LIST_FROM", "SOIL_PATHS_IDX64", "SOIL_FLOW_BATCH_CELLS"):
        assert knob in knobs, knob                                # the engine's knobs, which the entries share
    assert not re.search(r"getenv", open(os.path.join(ROOT, "soillib_amd", "csrc", "upstream.hip")).read())


def test_the_call_info_needs_no_device():
    from soillib_amd import _abi, soil
    assert _abi.lib().soil_upstream_extreme_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error() == "upstream_extreme_info: null info"
    assert sorted(soil.upstream_info()) == ["chunks", "idx64_chunks", "rounds", "vec_chunks"]


# ---- refusals of the two entries, without a device -------------------------------------------------------------

def _calls():
    """(what, the text after the entry's name, single-grid call or None, batch call): each breaks one rule; the
    pointers stand for planes of 4 x 4 cells (never read)."""
    from soillib_amd import _abi
    lib = _abi.lib()
    cells = 3 * 16 * 4
    o, a, g, v, s = (C.c_void_p(1 << 20 + i) for i in range(5))   # far apart
    inside = lambda p, off: C.c_void_p(p.value + off)
    one, many = lib.soil_upstream_extreme, lib.soil_upstream_extreme_batch
    big = 1 << 16
    shape_text = "a model must have 1..2^31-1 cells (int32 graph)"
    out = [
        ("null graph", "null graph", lambda: one(o, a, None, v, s, 4, 4, D8, 0, None), lambda: many(o, a, None, v, s, 3, 4, 4, D8, 0, None)),
        ("null value", "null value", lambda: one(o, a, g, None, s, 4, 4, D8, 0, None), lambda: many(o, a, g, None, s, 3, 4, 4, D8, 1, None)),
        ("no output", "no output asked for (out and arg are both null)", lambda: one(None, None, g, v, s, 4, 4, D8, 0, None),
         lambda: many(None, None, g, v, None, 3, 4, 4, D8, 0, None)),
        ("H = 0", "empty grid", lambda: one(o, None, g, v, None, 0, 4, D8, 0, None), lambda: many(o, None, g, v, None, 3, 0, 4, D8, 0, None)),
        ("W = 0", "empty grid", lambda: one(o, None, g, v, None, 4, 0, D4, 1, None), lambda: many(o, None, g, v, None, 3, 4, 0, D4, 1, None)),
        ("W < 0", "empty grid", lambda: one(None, a, g, v, None, 4, -2, D4, 0, None), lambda: many(None, a, g, v, None, 3, 4, -2, D4, 0, None)),
        ("H W > INT32_MAX", shape_text, lambda: one(o, None, g, v, None, big, big, D8, 0, None),
         lambda: many(o, None, g, v, None, 1, big, big // 2, D8, 0, None)),
        ("edge 2", "invalid edge enumerator", lambda: one(o, a, g, v, None, 4, 4, 2, 0, None), lambda: many(o, a, g, v, None, 3, 4, 4, 2, 0, None)),
        ("edge -1", "invalid edge enumerator", lambda: one(o, a, g, v, None, 4, 4, -1, 0, None), lambda: many(o, a, g, v, None, 3, 4, 4, -1, 0, None)),
        ("op 2", "op must be 0 (min) or 1 (max)", lambda: one(o, a, g, v, None, 4, 4, D8, 2, None), lambda: many(o, a, g, v, None, 3, 4, 4, D8, 2, None)),
        ("op -1", "op must be 0 (min) or 1 (max)", lambda: one(o, a, g, v, None, 4, 4, D8, -1, None), lambda: many(o, a, g, v, None, 3, 4, 4, D8, -1, None)),
        ("B = 0", "B must be >= 1", None, lambda: many(o, a, g, v, None, 0, 4, 4, D8, 0, None)),
        ("B < 0", "B must be >= 1", None, lambda: many(o, a, g, v, None, -3, 4, 4, D8, 0, None)),
        ("out is value", "an output aliases an input plane", lambda: one(v, a, g, v, s, 4, 4, D8, 0, None), lambda: many(v, a, g, v, s, 3, 4, 4, D8, 0, None)),
        ("arg is graph", "an output aliases an input plane", lambda: one(o, g, g, v, s, 4, 4, D8, 0, None), lambda: many(o, g, g, v, s, 3, 4, 4, D8, 0, None)),
        ("arg inside stop", "an output aliases an input plane", lambda: one(None, inside(s, 60), g, v, s, 4, 4, D8, 1, None),
         lambda: many(None, inside(s, cells - 4), g, v, s, 3, 4, 4, D8, 1, None)),
        ("out ends inside graph", "an output aliases an input plane", lambda: one(inside(g, -60), a, g, v, s, 4, 4, D8, 0, None),
         lambda: many(inside(g, 4 - cells), a, g, v, s, 3, 4, 4, D8, 0, None)),
        ("out is arg", "out and arg overlap", lambda: one(o, o, g, v, s, 4, 4, D8, 0, None), lambda: many(o, inside(o, cells - 4), g, v, s, 3, 4, 4, D8, 0, None)),
    ]
    return out


def test_every_refusal_names_its_entry_and_has_its_text():
    from soillib_amd import _abi
    for what, text, single, batch in _calls():
        for name, call in (("upstream_extreme", single), ("upstream_extreme_batch", batch)):
            if call is None:
                continue
            assert call() == _abi.SOIL_ERR_INVALID_ARGUMENT, (what, name)
            assert _abi.last_error() == "%s: %s" % (name, text), (what, name, _abi.last_error())


def test_planes_side_by_side_are_not_refused_for_aliasing():
    """Planes that touch without sharing a byte pass the checks: the call gets as far as looking for a device."""
    from soillib_amd import _abi
    lib = _abi.lib()
    if lib.soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    base = 1 << 20
    p = [C.c_void_p(base + 64 * i) for i in range(5)]             # five planes of 4 x 4 cells, back to back
    assert lib.soil_upstream_extreme(p[0], p[1], p[2], p[3], p[4], 4, 4, D8, 0, None) == _abi.SOIL_ERR_NO_DEVICE


def test_a_well_formed_call_fails_loudly_without_a_device():
    from soillib_amd import _abi
    lib = _abi.lib()
    if lib.soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    o, a, g, v, s = (C.c_void_p(1 << 20 + i) for i in range(5))
    assert lib.soil_upstream_extreme(o, a, g, v, s, 4, 4, D8, 0, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_upstream_extreme(None, a, g, v, None, 4, 4, D4, 1, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_upstream_extreme_batch(o, None, g, v, s, 3, 4, 4, D8, 1, None) == _abi.SOIL_ERR_NO_DEVICE


# ---- the ValueErrors of the Python layer: before any device work -----------------------------------------------

def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def _module_refusals():
    from soillib_amd import soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    v2, v3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    return [
        (soil.upstream_min, (g3, v2, soil.d8), {}, r"upstream_min: graph: expected a \(H, W\)"),
        (soil.upstream_min, (v2, v2, soil.d8), {}, "upstream_min: graph: expected an int32"),
        (soil.upstream_min, (g2, g2, soil.d8), {}, "upstream_min: value: expected a float32"),
        (soil.upstream_min, (g2, _host(np.float32, (3, 4)), soil.d8), {}, "upstream_min: value"),
        (soil.upstream_min, (g2, v2, 2), {}, "upstream_min: edge"),
        (soil.upstream_min, (g2, v2, soil.d8), dict(stop=v2), "upstream_min: stop"),
        (soil.upstream_max, (g2, v2, soil.d4), dict(stop=_host(np.int32, (3, 4))), "upstream_max: stop"),
        (soil.upstream_max, (g2, np.zeros((4, 3), np.float32), soil.d4), {}, "upstream_max: value"),
        (soil.upstream_min_batch, (g2, v2, soil.d8), {}, r"upstream_min_batch: graph: expected a \(B, H, W\)"),
        (soil.upstream_min_batch, (g3, v2, soil.d8), {}, "upstream_min_batch: value"),
        (soil.upstream_max_batch, (g3, v3, "d8"), {}, "upstream_max_batch: edge"),
        (soil.upstream_max_batch, (g3, v3, soil.d8), dict(stop=g2), "upstream_max_batch: stop"),
        (soil.breach, (v2, g3, soil.d8), {}, "breach: graph"),
        (soil.breach, (g2, g2, soil.d8), {}, "breach: height: expected a float32"),
        (soil.breach, (v2, g2, 9), {}, "breach: edge"),
        (soil.breach_batch, (v2, g3, soil.d8), {}, "breach_batch: height: expected a tensor of shape"),
        (soil.condition_breached, (v3,), {}, "condition_breached: height"),
        (soil.condition_breached, (g2,), {}, "condition_breached: height"),
        (soil.condition_breached, (v2, 3), {}, "condition_breached: edge"),
        (soil.condition_breached_batch, (v2,), {}, "condition_breached_batch: height"),
        (soil.condition_breached_batch, (v3,), dict(graph=g2), "condition_breached_batch: graph"),
        (soil.upstream_length, (g3, soil.d8, [1.0, 1.0]), {}, "upstream_length: graph"),
        (soil.upstream_length, (g2, soil.d8, [1.0]), {}, "upstream_length: scale"),
        (soil.upstream_length, (g2, 5, [1.0, 1.0]), {}, "upstream_length: edge"),
        (soil.upstream_length_batch, (g3, soil.d8, [[1.0, 1.0]] * 4), {}, "upstream_length_batch: scale"),
        (soil.upstream_length_batch, (g3, soil.d8, [1.0, 1.0]), dict(stop=g2), "upstream_length_batch: stop"),
    ]


def test_the_module_functions_refuse():
    for fn, args, kw, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the refusal came after the planes were touched (%s)" % name)


def _batch_without_a_device(B=5, scales=None):
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch.__new__(ErosionBatch)
    bt.B, bt.H, bt.W = B, 4, 3
    bt.seeds = list(range(B))
    bt.scale, bt.scales = ([1.0, 1.0, 1.0], None) if scales is None else (None, scales)
    bt.height = _Untouchable()
    return bt


def _batch_refusals():
    """(method, the stub's scales, args, kw, match)."""
    good, value = _host(np.int32, (5, 4, 3)), _host(np.float32, (5, 4, 3))
    out = []
    for method in ("upstream_min", "upstream_max"):
        for args, kw in (((_host(np.float32, (5, 3, 4)),), {}), ((good,), {}), ((3.0,), {}),
                         ((value,), dict(graph=_host(np.int32, (5, 3, 4)))), ((value,), dict(graph=value)),
                         ((value,), dict(graph=good, stop=value)), ((value,), dict(graph=good, stop=1)),
                         ((value,), dict(graph=good, edge=2)), ((value,), dict(edge="d4"))):
            out.append((method, None, args, kw, r"ErosionBatch\.%s" % method))
    for kw in (dict(graph=value), dict(graph=good, stop=_host(np.int32, (4, 4, 3))), dict(graph=good, edge=2)):
        out.append(("upstream_length", None, (), kw, r"ErosionBatch\.upstream_length"))
    out.append(("upstream_length", [[1.0, 1.0, 1.0]] * 4, (good,), {}, r"ErosionBatch\.upstream_length"))
    for kw in (dict(edge=7), dict(kind="direction"), dict(kind="random_weighted")):
        out.append(("breached", None, (), kw, r"ErosionBatch\.(breached|conditioned)"))
    return out


def test_the_batch_methods_refuse():
    for method, scales, args, kw, match in _batch_refusals():
        with pytest.raises(ValueError, match=match):
            getattr(_batch_without_a_device(scales=scales), method)(*args, **kw)
