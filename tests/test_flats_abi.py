"""Flats and filled lakes (include/soil_hip.h: "flow graphs: conditioning"; soil_flat_distance, soil_flat_receivers and
their _batch forms), what can be checked without a GPU: the refusals of the four entries with the entry's name in the
message, the symbols and the surfaces; the two numpy restatements of the flat distance (tests/flats_ref.py) against
each other and against closed forms; and the properties the definition promises on the oracle's filled surfaces — no
cell unreached, the patched graph without an interior terminal and without a cycle."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import flats_ref as ref
import flow_paths_ref
from flats_ref import D4, D8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 9), (9, 1), (3, 3), (8, 11), (23, 31)]
ENTRIES = {
    "soil_flat_distance": "int32_t* dist, const float* height, int64_t H, int64_t W, int edge, void* stream",
    "soil_flat_distance_batch": "int32_t* dist, const float* height, int64_t B, int64_t H, int64_t W, int edge, "
                                "void* stream",
    "soil_flat_receivers": "int32_t* out, const int32_t* in, const float* height, const int32_t* dist, int64_t H, "
                           "int64_t W, int edge, void* stream",
    "soil_flat_receivers_batch": "int32_t* out, const int32_t* in, const float* height, const int32_t* dist, "
                                 "int64_t B, int64_t H, int64_t W, int edge, void* stream",
    "soil_flat_distance_info": "int64_t info[4]",
}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


# ---- the header, the symbols, the surfaces ---------------------------------------------------------------------

def test_the_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    assert "flow graphs: conditioning" in text
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
    flat = _squash(re.sub(r"\n \* ?", "\n", text))
    for phrase in ("h[nb] < h[c]", "dist[nb] == dist[n] - 1", "out == in is allowed", "is acyclic",
                   "synchronise the stream before they return", "do not synchronise", "SOIL_FLATS_PER_CHECK",
                   "-0 == +0", "not the sum"):
        assert phrase in flat, phrase


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    i64, vp, cint = C.c_int64, C.c_void_p, C.c_int
    assert _abi.SIGNATURES["soil_flat_distance"] == (cint, [vp, vp, i64, i64, cint, vp])
    assert _abi.SIGNATURES["soil_flat_distance_batch"] == (cint, [vp, vp, i64, i64, i64, cint, vp])
    assert _abi.SIGNATURES["soil_flat_receivers"] == (cint, [vp, vp, vp, vp, i64, i64, cint, vp])
    assert _abi.SIGNATURES["soil_flat_receivers_batch"] == (cint, [vp, vp, vp, vp, i64, i64, i64, cint, vp])
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_flat_distance(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["flats.hip"]


def test_the_call_info_is_all_zero_before_a_call_and_needs_no_device():
    from soillib_amd import _abi, soil
    info = (C.c_int64 * 4)(7, 7, 7, 7)
    assert _abi.lib().soil_flat_distance_info(info) == _abi.SOIL_OK
    assert list(info) == [0, 0, 0, 0]
    assert _abi.lib().soil_flat_distance_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error().startswith("flat_distance_info: ")
    assert soil.flat_distance_info() == dict(launches=0, tiles=0, models=0, looks=0)


def test_the_surfaces():
    import soillib
    from soillib_amd import soil
    for name in ("flat_distance", "flat_receivers", "resolve_flats", "flat_distance_batch", "flat_receivers_batch",
                 "resolve_flats_batch", "flat_distance_info"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    text = open(os.path.join(ROOT, "include", "soil.hpp")).read()
    for name in ("flat_distance", "flat_receivers", "resolve_flats"):
        assert re.search(r"inline [^;{]*\b%s\(" % name, text), name
    assert "soil_flat_distance(" in text and "soil_flat_receivers(" in text
    assert "SOIL_FLATS_PER_CHECK" in open(os.path.join(ROOT, "docs", "KNOBS.md")).read()


# ---- refusals, without a device --------------------------------------------------------------------------------

def _calls():
    """(what, {entry: call}): each call breaks one rule; `p` stands for a tensor (never read)."""
    from soillib_amd import _abi
    lib = _abi.lib()
    p = C.c_void_p(4096)
    d, db, r, rb = lib.soil_flat_distance, lib.soil_flat_distance_batch, lib.soil_flat_receivers, lib.soil_flat_receivers_batch
    big = 1 << 16

    def sized(B, H, W, e):
        return {"flat_distance": lambda: d(p, p, H, W, e, None), "flat_distance_batch": lambda: db(p, p, B, H, W, e, None),
                "flat_receivers": lambda: r(p, p, p, p, H, W, e, None),
                "flat_receivers_batch": lambda: rb(p, p, p, p, B, H, W, e, None)}

    out = [
        ("null dist", {"flat_distance": lambda: d(None, p, 4, 4, D8, None),
                       "flat_distance_batch": lambda: db(None, p, 3, 4, 4, D8, None),
                       "flat_receivers": lambda: r(p, p, p, None, 4, 4, D8, None),
                       "flat_receivers_batch": lambda: rb(p, p, p, None, 3, 4, 4, D8, None)}),
        ("null height", {"flat_distance": lambda: d(p, None, 4, 4, D4, None),
                         "flat_distance_batch": lambda: db(p, None, 3, 4, 4, D4, None),
                         "flat_receivers": lambda: r(p, p, None, p, 4, 4, D4, None),
                         "flat_receivers_batch": lambda: rb(p, p, None, p, 3, 4, 4, D4, None)}),
        ("null out", {"flat_receivers": lambda: r(None, p, p, p, 4, 4, D8, None),
                      "flat_receivers_batch": lambda: rb(None, p, p, p, 3, 4, 4, D8, None)}),
        ("null in", {"flat_receivers": lambda: r(p, None, p, p, 4, 4, D8, None),
                     "flat_receivers_batch": lambda: rb(p, None, p, p, 3, 4, 4, D8, None)}),
        ("H = 0", sized(3, 0, 4, D8)), ("W = 0", sized(3, 4, 0, D4)), ("H < 0", sized(3, -1, 4, D8)),
        ("W < 0", sized(3, 4, -2, D8)), ("H W > INT32_MAX", sized(1, big, big // 2, D8)),
        ("edge 2", sized(3, 4, 4, 2)), ("edge -1", sized(3, 4, 4, -1)),
    ]
    for what, B in (("B = 0", 0), ("B < 0", -3)):
        calls = sized(B, 4, 4, D8)
        out.append((what, {k: v for k, v in calls.items() if k.endswith("_batch")}))
    return out


def test_every_refusal_names_its_entry():
    from soillib_amd import _abi
    seen = 0
    for what, calls in _calls():
        for name, call in calls.items():
            assert call() == _abi.SOIL_ERR_INVALID_ARGUMENT, (what, name)
            assert _abi.last_error().startswith(name + ": "), (what, name, _abi.last_error())
            seen += 1
    assert seen == 2 * 4 + 2 * 2 + 7 * 4 + 2 * 2


def test_a_well_formed_call_fails_loudly_without_a_device():
    from soillib_amd import _abi
    lib = _abi.lib()
    if lib.soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    p = C.c_void_p(4096)
    assert lib.soil_flat_distance(p, p, 4, 4, D8, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_flat_distance_batch(p, p, 3, 4, 4, D4, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_flat_receivers(p, p, p, p, 4, 4, D8, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_flat_receivers_batch(p, p, p, p, 3, 4, 4, D4, None) == _abi.SOIL_ERR_NO_DEVICE


def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def _module_refusals():
    from soillib_amd import soil
    h2, h3, g2, g3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3)), _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    return [
        (soil.flat_distance, (h3, soil.d8), r"flat_distance: height: expected a \(H, W\)"),
        (soil.flat_distance, (g2, soil.d8), "flat_distance: height: expected a float32"),
        (soil.flat_distance, (h2, 2), "flat_distance: edge"),
        (soil.flat_distance_batch, (h2, soil.d8), r"flat_distance_batch: height: expected a \(B, H, W\)"),
        (soil.flat_distance_batch, (h3, "d8"), "flat_distance_batch: edge"),
        (soil.flat_receivers, (g3, h2, g2, soil.d8), "flat_receivers: graph"),
        (soil.flat_receivers, (h2, h2, g2, soil.d8), "flat_receivers: graph: expected an int32"),
        (soil.flat_receivers, (g2, _host(np.float32, (3, 4)), g2, soil.d8), "flat_receivers: height"),
        (soil.flat_receivers, (g2, h2, h2, soil.d8), "flat_receivers: dist"),
        (soil.flat_receivers, (g2, h2, g2, 7), "flat_receivers: edge"),
        (soil.flat_receivers_batch, (g2, h3, g3, soil.d8), "flat_receivers_batch: graph"),
        (soil.flat_receivers_batch, (g3, h3, _host(np.int32, (4, 4, 3)), soil.d4), "flat_receivers_batch: dist"),
        (soil.resolve_flats, (h3, soil.d8), "resolve_flats: height"),
        (soil.resolve_flats, (h2, True), "resolve_flats: edge"),
        (soil.resolve_flats_batch, (h2, soil.d8), "resolve_flats_batch: height"),
    ]


def test_the_module_functions_refuse():
    for fn, args, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args)


# ---- the two restatements ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SHAPES + [(65, 129)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_two_restatements_agree_on_every_construction(H, W, edge):
    for name, h in ref.constructions(H, W) + [("serpentine", ref.serpentine(H, W)), ("corridor", ref.corridor(W))]:
        a, b = ref.distance_bfs(h, edge), ref.distance_relax(h, edge)
        assert a.dtype == b.dtype == np.int32 and (a == b).all(), "%s at %dx%d edge %d" % (name, H, W, edge)
        assert ((a == 0) == ref.seeds(h, edge)).all() and (a[np.isnan(h)] == -1).all(), name


@pytest.mark.parametrize("edge", [D4, D8])
def test_closed_forms(edge):
    for H, W in SHAPES + [(64, 64), (40, 17)]:
        x, y = np.mgrid[0:H, 0:W]
        want = np.minimum(np.minimum(x, y), np.minimum(H - 1 - x, W - 1 - y))
        assert (ref.distance_bfs(ref.level(H, W), edge) == want).all(), (H, W)      # the distance to the border
    for L in (1, 2, 7, 100):
        d = ref.distance_bfs(ref.corridor(L), edge)
        assert d[1, :L].tolist() == list(range(L)), L                               # one open end: 0 .. L - 1
        assert (d[0] == 0).all() and (d[2] == 0).all() and d[1, L] == 0             # the walls are on the border
    # a closed depression and single pits: no chain reaches a seed
    h = ref.closed(20, 30)
    d = ref.distance_bfs(h, edge)
    assert (d[h == 3.0] == -1).all() and (d[h == 1.0] == -1).all() and (d[h == 9.0] >= 0).all()
    # -0 == +0 and inf == inf make one flat; NaN equals nothing, itself included
    assert (ref.distance_bfs(ref.signed_zeros(9, 9), edge) == ref.distance_bfs(ref.level(9, 9), edge)).all()
    assert (ref.distance_bfs(np.full((9, 9), np.inf, np.float32), edge) == ref.distance_bfs(ref.level(9, 9), edge)).all()
    h = ref.level(5, 5)
    h[2, 2] = np.nan
    d = ref.distance_bfs(h, edge)
    assert d[2, 2] == -1 and d[1, 2] == 0 and d[2, 1] == 0 and d[1, 1] == (1 if edge == D4 else 0)


def test_flats_that_touch_diagonally_are_one_flat_under_d8_only():
    h = ref.diagonal_flats(15, 15)
    d4, d8 = ref.distance_bfs(h, D4), ref.distance_bfs(h, D8)
    inner = np.zeros_like(h, bool)
    inner[6:9, 6:9] = True                                         # the middle block: level 2 inside level 9 under D4
    assert (h[inner] == 2.0).all() and (d4[inner] == -1).all() and (d8[inner] >= 0).all()
    # out through the corners, block by block: (1, 1) is one step from the border, (7, 7) six diagonal steps further
    assert d8[1, 1] == 1 and d8[6, 6] == 6 and d8[7, 7] == 7


def test_the_receiver_rule_by_hand():
    h = ref.corridor(5)
    for edge in (D4, D8):
        dist = ref.distance_bfs(h, edge)
        g = np.full(h.shape, -1, np.int32)
        out = ref.receivers(g, h, dist, edge)
        assert out[1, :5].tolist() == [-1, 6, 7, 8, 9] and (out[0] == -1).all() and (out[2] == -1).all()
        g[1, 3] = 2                                                # an entry >= 0 stays, whatever it is
        g[1, 2] = -7                                               # any negative entry is "no receiver"
        out = ref.receivers(g, h, dist, edge)
        assert out[1, 3] == 2 and out[1, 2] == 7
        g = ref.hostile_graph(*h.shape)                            # a dist that belongs to no height: nothing qualifies
        assert (ref.receivers(g, h, np.full(h.shape, 5, np.int32), edge) == g).all()
    # the first neighbour in table order: up before left before right before down, the diagonals last
    h = ref.level(5, 5)
    g = np.full((5, 5), -1, np.int32)
    out = ref.receivers(g, h, ref.distance_bfs(h, D8), D8)
    assert out[1, 1] == 1 and out[3, 3] == 3 * 5 + 4 and out[2, 2] == 1 * 5 + 2 and out[1, 3] == 3
    out = ref.receivers(g, h, ref.distance_bfs(h, D4), D4)
    assert out[2, 2] == 1 * 5 + 2 and out[3, 1] == 3 * 5 + 0


# ---- properties on the oracle's surfaces -----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _surface(oracle, S, edge):
    dem = oracle.noise(S, S, seed=3.0, ext=(float(S), float(S))) * np.float32(100.0)
    return dem, oracle.fill_depressions(dem, edge)


@pytest.mark.parametrize("S,edge", [(96, D4), (96, D8), (160, D8)])
def test_a_filled_surface_drains_through_its_flats(oracle, S, edge):
    dem, filled = _surface(oracle, S, edge)
    dist = ref.distance_bfs(filled, edge)
    assert (dist == ref.distance_relax(filled, edge)).all()
    assert (dist >= 0).all(), "every cell of a filled surface reaches a cell that can drain"
    graph = oracle.steepest(filled, edge)
    assert (graph >= -1).all()
    flat = ref.interior_terminals(graph)
    assert flat.any() and ((dist > 0) == flat).all(), "dist > 0 exactly on the interior terminals of steepest"
    out = ref.receivers(graph, filled, dist, edge)
    assert not ref.interior_terminals(out).any(), "the patched graph has no interior terminal"
    assert (out[~flat] == graph[~flat]).all()
    terminal, steps, _ = flow_paths_ref.walk_doubling(out, edge)
    assert (terminal >= 0).all() and (steps >= 0).all(), "no cycle"
    tx, ty = terminal // S, terminal % S
    assert ((tx == 0) | (tx == S - 1) | (ty == 0) | (ty == S - 1)).all(), "every walk ends on the border"
    raw = ref.distance_bfs(dem, edge)
    assert (raw == -1).any(), "the unfilled DEM has pits no flat drains"
    print("%d^2 edge %d: %d flat cells, largest distance %d" % (S, edge, int(flat.sum()), int(dist.max())))
