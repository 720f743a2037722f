"""Every free wrapper of include/soil.hpp (namespace silt, namespace soil) run on the device by one C++ binary,
tests/cpp/test_cpp_ops.cpp, and each plane it writes compared with the CPU reference of the operation — the oracle,
the numpy restatements of tests/*_ref.py — never with the Python binding of the same library, which builds its
argument lists on its own.  The comparisons are the ones the operations' own GPU tests apply, through the same
functions; no tolerance here is new.

The inputs are made so that a wrapper that swaps two extents, hands scale.y for scale.x, drops an optional plane or
counts its scales wrongly computes something else (test_the_inputs_tell_the_arguments_apart, on the CPU): grids of
12 x 20 (rows of whole four-cell windows) and 13 x 21, a batch of 3 x 12 x 20, scales (0.3, 0.7), a pair per model,
D4 and D8, heights with a flat patch, every optional plane once given and once not.

Without a GPU: test_every_wrapper_is_exercised holds the binary's list of wrappers against the header's, and the
binary compiles under -Wall -Wextra -Werror and refuses to run."""
import functools
import os
import re
import time

import numpy as np
import pytest

import downstream_ref as dref
import flats_ref
import flow_paths_ref as fref
from flow_paths_ref import D4, D8
from test_cpp_api import ROOT, _build, _run
from util import (assert_bit_equal, assert_debris_close, assert_fluvial_close, assert_receivers_close,
                  assert_solve_uniform_close, cell_inputs, terrain)

gpu = pytest.mark.gpu

GRIDS = {"a": (12, 20), "b": (13, 21)}
B = 3
EDGES = (("d4", D4), ("d8", D8))
SC, SC3 = (0.3, 0.7), (0.3, 0.7, 4.0)
PER, ONE = [(0.3, 0.7), (1.1, 0.4), (0.25, 3.0)], [(0.6, 0.2)]
DT = 3.5
SEEDS = [3, 5, 9]
TP = (33, 50, 700)                          # the particle launches: H, W, walkers
# wrappers of the header that another binary runs: (name, the file that runs it)
COVERED_ELSEWHERE = (("erode", "tests/cpp/test_cpp_api.cpp"),)
TYPES = {"f32": np.dtype("<f4"), "i32": np.dtype("<i4"), "u64": np.dtype("<u8")}


# ------------------------------------------------------------------ the inputs, made once and left unchanged

def _height(oracle, H, W, seed):
    h = terrain(oracle, H, W, seed=seed)[..., 0].copy()
    h[3:8, 4:10] = h[5, 6]                  # a flat patch: cells without a receiver, and some a step from its rim
    return h


def _coefficients(r, shape, height):
    """a, b in [-1, 1], t in [-10, 10], an erosivity over 1e-6 .. 1e3 and an uplift in [0, 0.01], as the downstream
    tests draw them (|b| <= 1: every result is finite), and a stop plane with a tenth of the cells marked."""
    a, b = (r.uniform(-1.0, 1.0, shape).astype(np.float32) for _ in range(2))
    t = r.uniform(-10.0, 10.0, shape).astype(np.float32)
    k = np.exp(r.uniform(np.log(1e-6), np.log(1e3), shape)).astype(np.float32)
    up = (r.random(shape) * 0.01).astype(np.float32)
    stop = (r.random(shape) < 0.1).astype(np.int32)
    return dict(ca=a, cb=b, ct=t, k=k, up=up, stop=stop, src=(0.5 + r.random(shape)).astype(np.float32),
                decay=(0.8 + 0.2 * r.random(shape)).astype(np.float32), h=height)


@functools.lru_cache(maxsize=None)
def _inputs(oracle):
    inp = {}
    for g, (H, W) in GRIDS.items():
        r = np.random.default_rng([7, H, W])
        h = _height(oracle, H, W, 3.0)
        for name, p in _coefficients(r, (H, W), h).items():
            inp["%s_%s" % (name, g)] = p
        for es, edge in EDGES:
            inp["graph_%s_%s" % (g, es)] = oracle.steepest(h, edge)
            inp["rwgraph_%s_%s" % (g, es)] = oracle.random_weighted(h, edge, 11, 2, 10.0)
            inp["dist_%s_%s" % (g, es)] = flats_ref.distance_bfs(h, edge)
        for c in (1, 2):
            inp["t%d_%s" % (c, g)] = r.standard_normal((H, W, c)).astype(np.float32)
            inp["source%d_%s" % (c, g)] = (r.random((H, W, c)) * 1e-3).astype(np.float32)
        inp["flow_" + g] = -oracle.gradient(h, SC)
        inp["sudecay_" + g] = (r.random((H, W)) * 0.01).astype(np.float32)
        cells = cell_inputs(oracle, H, W)             # as test_gpu_parity.test_mass_transfer_albedo_bit_exact
        cells["layers"][::3, ::2, 1] = 0.0
        c3 = lambda: r.random((H, W, 3)).astype(np.float32) * np.float32(1.3)
        inp.update({"layers_" + g: cells["layers"], "uplift_" + g: cells["uplift"], "mass_" + g: cells["massFlux"] * 8,
                    "momentum_" + g: cells["velocityFlux"], "debris_" + g: cells["debrisFlux"] * 30,
                    "delta_" + g: (r.standard_normal((H, W, 2)) * 0.01).astype(np.float32),
                    "albedo_bedrock_" + g: c3(), "albedo_fluvial_" + g: c3(), "albedo_debris_" + g: c3(),
                    "albedo_surface_" + g: c3()})
    H, W = GRIDS["a"]
    r = np.random.default_rng([8, B, H, W])
    hb = np.stack([_height(oracle, H, W, 3.0 + 5.0 * b) for b in range(B)])
    for name, p in _coefficients(r, (B, H, W), hb).items():
        inp[name + "b"] = p
    for es, edge in EDGES:
        inp["graphb_" + es] = np.stack([oracle.steepest(hb[b], edge) for b in range(B)])
    H, W, _ = TP
    r = np.random.default_rng(21)                     # as test_gpu_parity.test_transport_fluvial_parity draws them
    inp["tp_layers"] = terrain(oracle, H, W, sediment=0.01)
    inp["tf_rainfall"] = (0.5 + r.random((H, W))).astype(np.float32)
    inp["tf_discharge"] = (r.random((H, W)) * 0.1).astype(np.float32)
    inp["tf_momentum"] = (r.standard_normal((H, W, 2)) * 2).astype(np.float32)
    inp["tf_albedo"] = r.random((H, W, 3)).astype(np.float32)
    r = np.random.default_rng(22)
    inp["td_velocity"] = (r.standard_normal((H, W, 2)) * 0.5).astype(np.float32)
    inp["td_albedo"] = r.random((H, W, 3)).astype(np.float32)
    inp["sa"] = np.arange(1003, dtype=np.float32)
    inp["sb"] = np.random.default_rng(1).standard_normal(1003).astype(np.float32)
    for p in inp.values():
        p.setflags(write=False)
    return inp


def _write_planes(path, planes):
    with open(os.path.join(path, "inputs.txt"), "w") as manifest:
        for name, p in planes.items():
            kind = {"float32": "f32", "int32": "i32", "uint64": "u64"}[p.dtype.name]
            np.ascontiguousarray(p).astype(TYPES[kind]).tofile(os.path.join(path, name + ".bin"))
            manifest.write("%s %s %s\n" % (name, kind, " ".join(str(d) for d in p.shape)))


def _read_planes(path):
    out = {}
    with open(os.path.join(path, "outputs.txt")) as manifest:
        for line in manifest:
            name, kind, *dims = line.split()
            dims = [int(d) for d in dims]
            p = np.fromfile(os.path.join(path, name + ".bin"), TYPES[kind])
            assert p.size == int(np.prod(dims)), (name, p.size, dims)
            assert name not in out, "the binary wrote %s twice" % name
            out[name] = p.reshape(dims)
    return out


# ------------------------------------------------------------------ the binary: built once, run once

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cpp_ops_build"), "test_cpp_ops", extra=("-Wall", "-Wextra", "-Werror"))


@pytest.fixture(scope="module")
def cpp(hip, oracle, exe, tmp_path_factory):
    """name -> plane of everything the binary wrote."""
    path = str(tmp_path_factory.mktemp("cpp_ops_planes"))
    _write_planes(path, _inputs(oracle))
    t0 = time.perf_counter()
    rc, stdout = _run([exe, path], 90)       # the binary's own watchdog ends it after 60 s
    wall = time.perf_counter() - t0
    assert rc == 0 and "CPP_OPS_OK" in stdout, stdout
    print("test_cpp_ops: %.2f s wall; %s" % (wall, [l for l in stdout.splitlines() if l.startswith("CPP_OPS_WALL")][0]))
    return _read_planes(path)


# ------------------------------------------------------------------ without a GPU

def _header_wrappers():
    """name -> number of overloads of the free inline functions of namespace silt and namespace soil in
    include/soil.hpp; soil::io, the detail and error namespaces and class members (indented) are out."""
    with open(os.path.join(ROOT, "include", "soil.hpp")) as f:
        text = f.read()
    for inner in ("io", "detail", "error"):
        text, n = re.subn(r"\nnamespace %s \{.*?\n\}  // namespace %s\n" % (inner, inner), "\n", text, flags=re.S)
        assert n == 1, inner
    names = {}
    for m in re.finditer(r"^inline\s+[\w:<>, ]+?[\s&*]+(\w+)\(", text, flags=re.M):
        names[m.group(1)] = names.get(m.group(1), 0) + 1
    return names


def test_every_wrapper_is_exercised(exe):
    """A wrapper added to the header without a run in tests/cpp/test_cpp_ops.cpp fails here."""
    header = _header_wrappers()
    assert len(header) > 40 and header["set"] == 2 and header["resolve_flats"] == 2 and "tiff" not in header, header
    rc, stdout = _run([exe, "--list"], 30)
    assert rc == 0, stdout
    listed = {}
    for line in stdout.splitlines():
        kind, name = line.split()
        assert kind == "OP", line
        listed[name] = listed.get(name, 0) + 1
    for name, where in COVERED_ELSEWHERE:
        assert name in header and name not in listed, (name, where)
        with open(os.path.join(ROOT, where)) as f:
            assert re.search(r"\bsoil::%s\(" % name, f.read()), "%s does not run soil::%s" % (where, name)
        listed[name] = header[name]
    assert listed == header, "not run: %s; not in the header: %s" % (
        sorted(n for n in header if listed.get(n, 0) < header[n]), sorted(n for n in listed if listed[n] > header.get(n, 0)))


def test_cpp_ops_compiles_and_refuses_without_device(exe, oracle, tmp_path):
    """The binary builds under -Wall -Wextra -Werror (the fixture), and without a device its first allocation throws."""
    from soillib_amd import _abi
    assert os.access(exe, os.X_OK)
    if _abi.lib().soil_device_count() > 0:
        return                               # a HIP device is visible: the GPU tests below run the same binary
    _write_planes(str(tmp_path), _inputs(oracle))
    rc, out = _run([exe, str(tmp_path)], 120)
    assert rc == 0 and "NO_DEVICE_OK" in out, out


def test_the_reader_refuses_a_plane_of_another_size(exe, tmp_path):
    """The planes are read before the first device call: a file one float short of its manifest line, or one float
    long, ends the binary with the plane named, on any machine."""
    planes = {"p": np.arange(6, dtype=np.float32).reshape(2, 3), "q": np.arange(4, dtype=np.int32)}
    for size, dims in ((20, "2 3"), (28, "2 3"), (24, "2 4")):
        _write_planes(str(tmp_path), planes)
        assert open(str(tmp_path / "inputs.txt")).read() == "p f32 2 3\nq i32 4\n"
        with open(str(tmp_path / "p.bin"), "wb") as f:
            f.write(b"\0" * size)
        with open(str(tmp_path / "inputs.txt"), "w") as f:
            f.write("p f32 %s\nq i32 4\n" % dims)
        rc, out = _run([exe, str(tmp_path)], 30)
        assert rc == 1 and "p.bin holds %d bytes" % size in out and "CPP_OPS_OK" not in out and "NO_DEVICE_OK" not in out, out
    rc, out = _run([exe, str(tmp_path / "nowhere")], 30)
    assert rc == 1 and "cannot open" in out, out


def _differ(a, b):
    """Whether two int32 or float32 planes differ in a word."""
    return bool((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any())


def test_the_inputs_tell_the_arguments_apart(oracle):
    """On the CPU: each optional plane, each scale and each extent changes the reference of the call it goes to, so
    a wrapper that drops or swaps it cannot give the expected plane."""
    inp = _inputs(oracle)
    differ = _differ
    assert np.float32(20.0) / np.float32(33.0) == np.float32(20.0 / 33.0) and np.float32(20.0) / np.float32(50.0) == np.float32(20.0 / 50.0)
    for g, (H, W) in GRIDS.items():
        def at(name):                        # "stop" -> stop_<g>, "graph_d8" -> graph_<g>_d8
            base, _, es = name.rpartition("_")
            return inp["%s_%s_%s" % (base, g, es)] if es in ("d4", "d8") else inp["%s_%s" % (name, g)]

        assert (at("graph_d8") == -1).sum() > 4 and at("stop").sum() > 4
        assert differ(at("dist_d4"), at("dist_d8")) and (at("dist_d8") > 0).any() and (at("dist_d4") > 0).any()
        assert differ(oracle.slope(at("h"), at("graph_d8"), SC), oracle.slope(at("h"), at("graph_d8"), SC[::-1]))
        for es, edge in EDGES:
            graph = at("graph_" + es)
            assert differ(graph, at("rwgraph_" + es))
            assert differ(flats_ref.receivers(graph, at("h"), at("dist_" + es), edge), graph), "the flat patch is resolved"
            with_stop, without = fref.walk_doubling(graph, edge, SC, at("stop")), fref.walk_doubling(graph, edge, SC)
            assert all(differ(a, b) for a, b in zip(with_stop, without))
            assert differ(without[2], fref.walk_doubling(graph, edge, SC[::-1])[2])
            assert differ(oracle.accumulate(graph, at("src"), edge), oracle.accumulate(graph, at("src"), edge, decay=at("decay")))
            full = dref.solve_doubling(graph, edge, at("ca"), at("cb"), at("ct"), SC, at("stop"))[0]
            for other in (dref.solve_doubling(graph, edge, at("ca"), at("ct"), at("cb"), SC, at("stop")),
                          dref.solve_doubling(graph, edge, at("ca"), at("cb"), at("ct"), None, at("stop")),
                          dref.solve_doubling(graph, edge, at("ca"), at("cb"), at("ct"), SC),
                          dref.solve_doubling(graph, edge, None, at("cb"), at("ct"), SC, at("stop")),
                          dref.solve_doubling(graph, edge, at("ca"), None, at("ct"), SC, at("stop")),
                          dref.solve_doubling(graph, edge, at("ca"), at("cb"), None, SC, at("stop"))):
                assert differ(full, other[0])
            pw = lambda uplift: (at("h"), at("k"), uplift, DT)
            power = dref.solve_doubling(graph, edge, scale=SC, stop=at("stop"), power=pw(at("up")))[0]
            assert differ(power, dref.solve_doubling(graph, edge, scale=SC, stop=at("stop"), power=pw(None))[0])
            assert differ(power, dref.solve_doubling(graph, edge, scale=SC, power=pw(at("up")))[0])
    for es, edge in EDGES:
        graph = inp["graphb_" + es]
        per = fref.walk_batch(fref.walk_doubling, graph, edge, PER, inp["stopb"])
        first = fref.walk_batch(fref.walk_doubling, graph, edge, PER[:1], inp["stopb"])
        assert differ(per[2][1], first[2][1]) and differ(per[2][2], first[2][2]), "a pair per model, not the first for all"
        for b in range(B):
            assert differ(oracle.accumulate(graph[b], inp["srcb"][b], edge),
                          oracle.accumulate(graph[b], inp["srcb"][b], edge, decay=inp["decayb"][b]))
            assert differ(graph[b], graph[(b + 1) % B]), "the models differ"


# ------------------------------------------------------------------ on the device

@gpu
def test_silt_ops(cpp, oracle):
    inp = _inputs(oracle)
    assert cpp["set_f"].dtype == np.float32 and cpp["set_f"].shape == (7, 9) and (cpp["set_f"] == np.float32(3.5)).all()
    assert cpp["set_i"].dtype == np.int32 and cpp["set_i"].shape == (7, 9) and (cpp["set_i"] == -4).all()
    np.testing.assert_array_equal(cpp["add"], inp["sa"] + inp["sb"])
    np.testing.assert_array_equal(cpp["multiply"], inp["sa"] * np.float32(0.5))
    assert cpp["seed"].shape == (100, 2) and (cpp["seed"][:, 0] == 42).all() and (cpp["seed"][:, 1] == 1000).all()


@gpu
def test_flow_maps(cpp, oracle):
    """direction, steepest, random_weighted, slope and their batch forms."""
    inp = _inputs(oracle)
    for g in GRIDS:
        h = inp["h_" + g]
        for es, edge in EDGES:
            tag = "_%s_%s" % (g, es)
            assert_bit_equal(cpp["steepest" + tag], oracle.steepest(h, edge), "steepest" + tag)
            assert_bit_equal(cpp["direction" + tag], oracle.direction(h, edge), "direction" + tag)
            assert_receivers_close(oracle, cpp["random_weighted" + tag], oracle.random_weighted(h, edge, 3, 7, 10.0), h,
                                   4 if edge == D4 else 8, 3, 7, 10.0)
        assert_bit_equal(cpp["slope_" + g], oracle.slope(h, inp["graph_%s_d8" % g], SC), "slope_" + g)
    hb = inp["hb"]
    for es, edge in EDGES:
        for b in range(B):
            what = "_batch_%s, model %d" % (es, b)
            assert_bit_equal(cpp["steepest_batch_" + es][b], oracle.steepest(hb[b], edge), "steepest" + what)
            assert_bit_equal(cpp["direction_batch_" + es][b], oracle.direction(hb[b], edge), "direction" + what)
            assert_receivers_close(oracle, cpp["random_weighted_batch_" + es][b], oracle.random_weighted(hb[b], edge, SEEDS[b], 7, 10.0),
                                   hb[b], 4 if edge == D4 else 8, SEEDS[b], 7, 10.0)
    for name, scales in (("per", PER), ("one", ONE)):
        for b in range(B):
            assert_bit_equal(cpp["slope_batch_" + name][b], oracle.slope(hb[b], inp["graphb_d8"][b], scales[b % len(scales)]),
                             "slope_batch_%s, model %d" % (name, b))


@gpu
def test_accumulate_and_fill(cpp, oracle):
    """accumulate, accumulate_decay, fill_depressions and their batch forms."""
    inp = _inputs(oracle)
    for g in GRIDS:
        for es, edge in EDGES:
            tag = "_%s_%s" % (g, es)
            graph, src = inp["graph" + tag], inp["src_" + g]
            assert_bit_equal(cpp["accumulate" + tag], oracle.accumulate(graph, src, edge), "accumulate" + tag)
            assert_bit_equal(cpp["accumulate_decay" + tag], oracle.accumulate(graph, src, edge, decay=inp["decay_" + g]),
                             "accumulate_decay" + tag)
            assert_bit_equal(cpp["fill_depressions" + tag], oracle.fill_depressions(inp["h_" + g], edge), "fill_depressions" + tag)
    for es, edge in EDGES:
        for b in range(B):
            graph, src = inp["graphb_" + es][b], inp["srcb"][b]
            what = "_batch_%s, model %d" % (es, b)
            assert_bit_equal(cpp["accumulate_batch_" + es][b], oracle.accumulate(graph, src, edge), "accumulate" + what)
            assert_bit_equal(cpp["accumulate_batch_decay_" + es][b], oracle.accumulate(graph, src, edge, decay=inp["decayb"][b]),
                             "accumulate with a decay" + what)
            assert_bit_equal(cpp["fill_depressions_batch_" + es][b], oracle.fill_depressions(inp["hb"][b], edge), "fill_depressions" + what)


@gpu
def test_flats(cpp, oracle):
    """flat_distance, flat_receivers and both resolve_flats."""
    inp = _inputs(oracle)
    for g in GRIDS:
        h = inp["h_" + g]
        for es, edge in EDGES:
            tag = "_%s_%s" % (g, es)
            dist = inp["dist" + tag]
            flats_ref.same(cpp["flat_distance" + tag], dist, "flat_distance" + tag)
            flats_ref.same(cpp["flat_receivers" + tag], flats_ref.receivers(inp["graph" + tag], h, dist, edge), "flat_receivers" + tag)
            flats_ref.same(cpp["resolve_flats_graph" + tag], flats_ref.receivers(inp["rwgraph" + tag], h, dist, edge),
                           "resolve_flats with a graph" + tag)
            flats_ref.same(cpp["resolve_flats" + tag], flats_ref.receivers(oracle.steepest(h, edge), h, dist, edge), "resolve_flats" + tag)


def _paths(cpp, name):
    return tuple(cpp["%s_%s" % (name, part)] for part in fref.NAMES)


@gpu
def test_flow_paths(cpp, oracle):
    """flow_paths, basins, flow_length and their batch forms, with and without pour points."""
    inp = _inputs(oracle)
    for g in GRIDS:
        for es, edge in EDGES:
            tag = "_%s_%s" % (g, es)
            graph = inp["graph" + tag]
            for suffix, stop in (("_stop", inp["stop_" + g]), ("", None)):
                want = fref.walk_doubling(graph, edge, SC, stop)
                fref.same_words(_paths(cpp, "flow_paths" + suffix + tag), want, "flow_paths" + suffix + tag)
                fref.same_words((cpp["basins" + suffix + tag], None, cpp["flow_length" + suffix + tag]), (want[0], None, want[2]),
                                "basins, flow_length" + suffix + tag)
    for es, edge in EDGES:
        graph = inp["graphb_" + es]
        for suffix, scales, stop in (("_stop_", PER, inp["stopb"]), ("_", ONE, None)):
            want = fref.walk_batch(fref.walk_doubling, graph, edge, scales, stop)
            fref.same_words(_paths(cpp, "flow_paths_batch" + suffix + es), want, "flow_paths_batch" + suffix + es)
            fref.same_words((cpp["basins_batch" + suffix + es], None, cpp["flow_length_batch" + suffix + es]), (want[0], None, want[2]),
                            "basins_batch, flow_length_batch" + suffix + es)


@gpu
def test_downstream_and_stream_power(cpp, oracle):
    """downstream, stream_power and their batch forms: every optional argument given, and none."""
    inp = _inputs(oracle)
    solve = dref.solve_doubling
    for g in GRIDS:
        at = lambda name: inp["%s_%s" % (name, g)]
        for es, edge in EDGES:
            tag = "_%s_%s" % (g, es)
            graph = inp["graph" + tag]
            dref.same_words((cpp["downstream_all" + tag], None), solve(graph, edge, at("ca"), at("cb"), at("ct"), SC, at("stop")),
                            "downstream_all" + tag)
            dref.same_words((cpp["downstream" + tag], None), solve(graph, edge), "downstream" + tag)
            dref.same_words((cpp["stream_power_all" + tag], None),
                            solve(graph, edge, scale=SC, stop=at("stop"), power=(at("h"), at("k"), at("up"), DT)), "stream_power_all" + tag)
            dref.same_words((cpp["stream_power" + tag], None), solve(graph, edge, scale=SC, power=(at("h"), at("k"), None, DT)),
                            "stream_power" + tag)
    many = functools.partial(dref.solve_batch, solve)
    ca, cb, ct, stop = (inp[k] for k in ("cab", "cbb", "ctb", "stopb"))
    for es, edge in EDGES:
        graph = inp["graphb_" + es]
        dref.same_words((cpp["downstream_batch_all_" + es], None), many(graph, edge, ca, cb, ct, PER, stop), "downstream_batch_all_" + es)
        dref.same_words((cpp["downstream_batch_one_" + es], None), many(graph, edge, ca, cb, ct, ONE), "downstream_batch_one_" + es)
        dref.same_words((cpp["downstream_batch_" + es], None), many(graph, edge), "downstream_batch_" + es)
        dref.same_words((cpp["stream_power_batch_all_" + es], None),
                        many(graph, edge, scale=PER, stop=stop, power=(inp["hb"], inp["kb"], inp["upb"], DT)), "stream_power_batch_all_" + es)
        dref.same_words((cpp["stream_power_batch_" + es], None), many(graph, edge, scale=ONE, power=(inp["hb"], inp["kb"], None, DT)),
                        "stream_power_batch_" + es)


@gpu
def test_stencils_and_noise(cpp, oracle):
    """gradient, negslope, laplacian and gaussian_blur at 1 and 2 channels, noise."""
    inp = _inputs(oracle)
    for g, (H, W) in GRIDS.items():
        h = inp["h_" + g]
        assert_bit_equal(cpp["gradient_" + g], oracle.gradient(h, SC), "gradient_" + g)
        assert_bit_equal(cpp["negslope_" + g], oracle.negslope(h, SC), "negslope_" + g)
        for c in (1, 2):
            t = inp["t%d_%s" % (c, g)]
            assert_bit_equal(cpp["laplacian%d_%s" % (c, g)], oracle.laplacian(t, SC), "laplacian%d_%s" % (c, g))
            assert_bit_equal(cpp["gaussian_blur%d_%s" % (c, g)], oracle.gaussian_blur(t, 3.0), "gaussian_blur%d_%s" % (c, g))
        assert_bit_equal(cpp["noise_" + g], oracle.noise(H, W, seed=3.0, ext=(float(H), float(W))), "noise_" + g)


@gpu
def test_cell_ops(cpp, oracle):
    """mass_transfer with the colour planes, mass_creep, layer_merge, under the default parameters."""
    inp = _inputs(oracle)
    op = oracle.default_param()
    for g in GRIDS:
        at = lambda name: inp["%s_%s" % (name, g)]
        delta, surface = at("delta").copy(), at("albedo_surface").copy()
        oracle.mass_transfer(delta, at("layers"), at("uplift"), at("mass"), at("momentum"), at("debris"), at("albedo_bedrock"),
                             at("albedo_fluvial"), at("albedo_debris"), surface, SC3, op)
        assert_bit_equal(cpp["mass_transfer_delta_" + g], delta, "mass_transfer: delta, " + g)
        assert_bit_equal(cpp["mass_transfer_surface_" + g], surface, "mass_transfer: albedo_surface, " + g)
        assert (surface != at("albedo_surface")).any() and (delta != at("delta")).any()
        creep = at("delta").copy()
        oracle.mass_creep(creep, at("layers"), SC3, op)
        assert_bit_equal(cpp["mass_creep_" + g], creep, "mass_creep_" + g)
        assert (creep != at("delta")).any()
        assert_bit_equal(cpp["layer_merge_" + g], oracle.layer_merge(at("layers")), "layer_merge_" + g)


@gpu
def test_solve_uniform(cpp, oracle):
    """K = 1, 2; the generators seeded in C++ with silt::seed(r, 5, 100)."""
    inp = _inputs(oracle)
    for g in GRIDS:
        for c in (1, 2):
            want = oracle.solve_uniform(inp["flow_" + g], inp["source%d_%s" % (c, g)], inp["sudecay_" + g], oracle.rng_seed(700, 5, 100), SC, 700)
            assert np.isfinite(want).any() and (want[np.isfinite(want)] != 0).any()
            assert_solve_uniform_close(cpp["solve_uniform%d_%s" % (c, g)], want)


@functools.lru_cache(maxsize=None)
def _transport_want(oracle):
    """The oracle's planes of the two particle launches, under the default parameters."""
    inp = _inputs(oracle)
    H, W, N = TP
    scale = (20.0 / H, 20.0 / W, 4.0)
    op = oracle.default_param()
    z = lambda *c: np.zeros((H, W) + c, np.float32)
    f = dict(wh=inp["tf_discharge"].copy(), wf=z(), m=z(), mf=z(), v=inp["tf_momentum"].copy(), vf=z(2), af=z(3), rng=oracle.rng_seed(N, 5, 100))
    f["steps"] = oracle.transport_fluvial(inp["tp_layers"], inp["tf_rainfall"], f["wh"], f["wf"], f["m"], f["mf"], f["v"], f["vf"], f["af"],
                                          inp["tf_albedo"], f["rng"], scale, op)
    d = dict(v=inp["td_velocity"].copy(), vf=z(2), m=z(), mf=z(), af=z(3), rng=oracle.rng_seed(N, 6, 9))
    d["steps"] = oracle.transport_debris(inp["tp_layers"], d["v"], d["vf"], d["m"], d["mf"], d["af"], inp["td_albedo"], d["rng"], scale, op)
    return f, d


@gpu
def test_transport_fluvial(cpp, oracle):
    want = _transport_want(oracle)[0]
    assert want["steps"] > TP[2]                    # the particles really move
    got = dict(wh=cpp["tf_discharge"], wf=cpp["tf_discharge_track"], m=cpp["tf_mass"], mf=cpp["tf_mass_track"], v=cpp["tf_momentum"],
               vf=cpp["tf_momentum_track"], af=cpp["tf_albedo_track"])
    assert (cpp["tf_rng"][:, 0] == 5).all() and (cpp["tf_rng"][:, 1] == want["rng"]["offset"]).all()   # the same draws, walker for walker
    assert_fluvial_close(got, want)


@gpu
def test_transport_debris(cpp, oracle):
    want = _transport_want(oracle)[1]
    got = dict(v=cpp["td_velocity"], vf=cpp["td_velocity_track"], m=cpp["td_mass"], mf=cpp["td_mass_track"], af=cpp["td_albedo_track"])
    assert (cpp["td_rng"][:, 0] == 6).all() and (cpp["td_rng"][:, 1] == want["rng"]["offset"]).all()
    assert_debris_close(got, want)


class _Seen(dict):
    """The planes, and which of them were looked at."""

    def __init__(self, planes):
        super().__init__(planes)
        self.seen = set()

    def __getitem__(self, name):
        self.seen.add(name)
        return super().__getitem__(name)


@gpu
def test_every_plane_the_binary_writes_is_compared(cpp, oracle):
    """A wrapper run in the binary whose result no test above reads would pass whatever it computed: the comparisons
    once more, on a dict that notes what they read."""
    planes = _Seen(cpp)
    for compare in (test_silt_ops, test_flow_maps, test_accumulate_and_fill, test_flats, test_flow_paths,
                    test_downstream_and_stream_power, test_stencils_and_noise, test_cell_ops, test_solve_uniform,
                    test_transport_fluvial, test_transport_debris):
        compare(planes, oracle)
    assert sorted(planes.seen) == sorted(planes), sorted(set(planes) - planes.seen)
    assert len(planes) == 187
