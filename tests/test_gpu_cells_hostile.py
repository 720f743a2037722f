"""The fused cell phase (csrc/erosion_cells.hip: k_erode_cells_fused, its scalar twin, k_zero_flux) and the
stand-alone cell ops against the oracle, bit for bit, on hostile planes and in every launch shape.

The planes are util.hostile_cell_inputs / hostile_colour_inputs: fluxes of exactly 0, NaN in cell (0, 0), plateaus
across group, wave and row boundaries, ties split differently between bedrock and sediment, bare rock, cliffs, both
clamps of `transfer`, signed zeros, denormals, the ends of the fp32 range and +-inf / NaN at every kind of place.
tests/test_cells_hostile.py asserts without a GPU that they reach every branch and stay mostly finite, and that each
shape below is in the launch class it stands for.  Every comparison here is assert_bit_equal (NaN matches NaN, every
other value by its bits); every case runs under the default parameters, the script's and two drawn at random.

  * soil_erode_cells_fused, _ex and _colour on twelve shapes, with and without SOIL_CELLS_KEEP_FLUX: every output
    plane; the flux planes zero inside the row range, or kept; `layers` untouched;
  * row ranges: rows outside the range hold what they held; a range of (252, 260) that stays in the remap class;
  * a remap-sized slab with x0 > 0 and ghost rows, stitched into the whole grid;
  * the four batch entries with B = 3, the hostile model between two benign ones: every model's slice equal to its
    own single-model call and to the oracle;
  * mass_transfer (with and without colour, from a delta that holds -0), mass_creep, layer_merge, and both
    normalise kernels through transport_fluvial / transport_debris with no walkers;
  * one plane 4 bytes off its 16-byte alignment (an input, an output, a colour plane): the scalar kernel;
  * SOIL_CELLS_VARIANT 1 to 6 (the 512- and 128-thread kernels, DIRECT, the one-kernel re-zero under remap), and
    SOIL_CELLS_NT=1 / SOIL_CELLS_SPLIT=0 in a child process each (they are read once per process).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from util import (CELL_FLUX, CELL_IN, CELL_OUT, COLOUR_IN, COLOUR_OUT, HOSTILE_SHAPES, assert_bit_equal, bits,
                  cell_inputs, cell_param_sets, colour_inputs, copy_param, hostile_cell_inputs, hostile_colour_inputs,
                  oracle_colour_cells, product_param, to_gpu, to_np)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTOR_SHAPES = [s for s in HOSTILE_SHAPES if s[1] % 4 == 0]
PARAM_SETS = ("default", "script", "random0", "random1")
OUT_SHAPE = dict(layers_next=(2,), height=(), waterHeight=(), mass=(), velocity=(2,), debris=(), debrisVelocity=(2,))

_REF = {}


def reference(oracle, H, W, pname, benign=False):
    """(inp, col, oracle param, scale, the oracle's planes with colour) of one case; computed once and shared."""
    key = (H, W, pname, benign)
    if key not in _REF:
        seed = H * 1000 + W
        if benign:
            inp, col = cell_inputs(oracle, H, W, seed + 5), colour_inputs(H, W, seed + 6)
        else:
            inp = hostile_cell_inputs(oracle, H, W, seed=seed)
            col = hostile_colour_inputs(inp, seed=seed)
        op, scale = {n: (o, s) for n, o, s in cell_param_sets(oracle, H, W)}[pname]
        want = oracle_colour_cells(oracle, inp, col, scale, op)
        for a in list(inp.values()) + list(col.values()) + list(want.values()):
            a.setflags(write=False)
        _REF[key] = (inp, col, op, scale, want)
    return _REF[key]


def prefill(H, W, seed=1):
    """What the output planes hold before a call: numbers (not NaN, which would match any NaN) no kernel writes."""
    r = np.random.default_rng(seed)
    return {k: (r.random((H, W) + c) + 2.0).astype(np.float32) for k, c in OUT_SHAPE.items()}


def upload(inp, col, before):
    g = {k: to_gpu(v) for k, v in inp.items()}
    g.update({k: to_gpu(v) for k, v in before.items()})
    if col is not None:
        g.update({k: to_gpu(v) for k, v in col.items()})
    return g


def plane_structs(g, colour):
    from soillib_amd import _abi
    planes = _abi.ErosionPlanes()
    for name in _abi._PLANES:
        setattr(planes, name, g[name].ptr)
    if not colour:
        return planes, None
    cp = _abi.ColourPlanes()
    for field, name in zip(_abi.COLOUR_PLANES, COLOUR_IN):
        setattr(cp, field, g[name].ptr)
    return planes, cp


def launch(hip, g, entry, dom, scale, pp, keep):
    """entry: "plain" (soil_erode_cells_fused; no flags), "ex", "colour"."""
    from soillib_amd import _abi
    planes, cp = plane_structs(g, entry == "colour")
    flags = _abi.SOIL_CELLS_KEEP_FLUX if keep else 0
    sc = _abi.vec(scale, 3)
    if entry == "plain":
        assert not keep
        rc = hip.soil_erode_cells_fused(C.byref(planes), C.byref(dom), sc, pp._ref(), None)
    elif entry == "ex":
        rc = hip.soil_erode_cells_fused_ex(C.byref(planes), C.byref(dom), sc, pp._ref(), flags, None)
    else:
        rc = hip.soil_erode_cells_fused_colour(C.byref(planes), C.byref(cp), C.byref(dom), sc, pp._ref(), flags, None)
    _abi.check(rc)


def check(g, inp, col, want, before, rows, keep, colour, what):
    """Every plane of the device case `g` after a call on rows [r0, r1) against the oracle's planes `want`."""
    H = inp["layers"].shape[0]
    r0, r1 = rows
    inside = slice(r0, r1)
    outside = np.ones(H, bool)
    outside[inside] = False
    for name in CELL_OUT + (COLOUR_OUT if colour else ()):
        got = to_np(g[name])
        assert_bit_equal(got[inside], want[name][inside], "%s: %s" % (what, name))
        held = before[name] if name in before else col[name]
        assert_bit_equal(got[outside], held[outside], "%s: %s outside the rows" % (what, name))
    for name in CELL_FLUX:
        got = to_np(g[name])
        if keep:
            assert_bit_equal(got, inp[name], "%s: %s kept" % (what, name))
        else:
            assert (bits(got[inside]) == 0).all(), "%s: %s not re-zeroed" % (what, name)
            assert_bit_equal(got[outside], inp[name][outside], "%s: %s outside the rows" % (what, name))
    for name in ("layers", "uplift", "rainfall"):
        assert_bit_equal(to_np(g[name]), inp[name], "%s: %s is input only" % (what, name))
    if colour:
        assert_bit_equal(to_np(g["albedoBedrock"]), col["albedoBedrock"], what + ": albedoBedrock is input only")


def run_case(hip, oracle, H, W, pname, entry, keep, rows=None, what=""):
    from soillib_amd import _abi
    inp, col, op, scale, want = reference(oracle, H, W, pname)
    colour = entry == "colour"
    before = prefill(H, W)
    g = upload(inp, col if colour else None, before)
    rows = rows or (0, H)
    launch(hip, g, entry, _abi.Domain(H, W, 0, H, rows[0], rows[1]), scale, product_param(op), keep)
    check(g, inp, col, want, before, rows, keep, colour,
          "%s %s %dx%d rows %s keep %d %s" % (entry, pname, H, W, rows, keep, what))


# ---------------------------------------------------------------- every entry point in every launch shape

@pytest.mark.parametrize("pname", PARAM_SETS)
@pytest.mark.parametrize("H,W", HOSTILE_SHAPES)
def test_fused_cells_on_hostile_planes(hip, oracle, H, W, pname):
    for entry, keep in (("plain", False), ("ex", False), ("ex", True), ("colour", False), ("colour", True)):
        run_case(hip, oracle, H, W, pname, entry, keep)


def row_ranges(H):
    out = [(1, H - 1)] if H >= 3 else []
    if H >= 72:
        out.append((17, 70))
    if H >= 8:
        out.append((H // 2, H // 2 + 1))
    return out


@pytest.mark.parametrize("H,W", VECTOR_SHAPES + [(37, 53)])
def test_row_ranges_leave_the_other_rows_alone(hip, oracle, H, W):
    """(252, 260) rows (1, 251): 16250 groups in 64 blocks, the remap class with idle lanes; (17, 70) and a single
    row fall out of it."""
    for rows in row_ranges(H):
        for pname in ("script", "random1"):
            for entry, keep in (("ex", False), ("ex", True), ("colour", False), ("colour", True)):
                run_case(hip, oracle, H, W, pname, entry, keep, rows)


@pytest.mark.parametrize("entry", ["ex", "colour"])
def test_a_remap_sized_slab_with_ghost_rows(hip, oracle, entry):
    """A 300 x 260 grid in three slabs with one ghost row; the middle one owns global rows 20 .. 271 (x0 = 19): 252
    rows, 16380 groups, 64 blocks — remap with idle lanes, on a domain that does not start at the grid's top."""
    from soillib_amd import _abi
    H, W = 300, 260
    colour = entry == "colour"
    for pname in ("script", "random1"):
        inp, col, op, scale, want = reference(oracle, H, W, pname)
        pp = product_param(op)
        names = CELL_OUT + (COLOUR_OUT if colour else ())
        got = {k: np.zeros_like(want[k]) for k in names}
        for o0, o1 in ((0, 20), (20, 272), (272, 300)):
            x0, x1 = max(0, o0 - 1), min(H, o1 + 1)
            rows = x1 - x0
            sl = slice(x0, x1)
            before = prefill(rows, W)
            g = upload({k: v[sl] for k, v in inp.items()}, {k: v[sl] for k, v in col.items()} if colour else None, before)
            launch(hip, g, entry, _abi.Domain(H, W, x0, rows, o0 - x0, o1 - x0), scale, pp, False)
            for k in names:
                a = to_np(g[k])
                got[k][o0:o1] = a[o0 - x0:o1 - x0]
                ghost = np.ones(rows, bool)
                ghost[o0 - x0:o1 - x0] = False
                held = before[k] if k in before else col[k][sl]
                assert_bit_equal(a[ghost], held[ghost], "slab %d: ghost rows of %s" % (o0, k))
            for k in CELL_FLUX:
                a = to_np(g[k])
                assert (bits(a[o0 - x0:o1 - x0]) == 0).all(), k
                assert_bit_equal(a[ghost], inp[k][sl][ghost], "slab %d: ghost rows of %s" % (o0, k))
        for k in names:
            assert_bit_equal(got[k], want[k], "%s slabs, %s: %s" % (entry, pname, k))


# ---------------------------------------------------------------- batches: nothing crosses a model boundary

@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("form", ["uniform", "colour", "params", "params_colour", "models", "models_colour"])
@pytest.mark.parametrize("H,W", [(9, 260), (252, 260), (37, 53)])
def test_batches_with_a_hostile_model_in_the_middle(hip, oracle, H, W, form, keep):
    """B = 3, the hostile model between two benign ones.  The sweep gives every model its own parameters, the batch
    of models its own scale as well.  Every model's slice: the oracle's planes for that model alone, and the bits of
    its own single-model call."""
    from soillib_amd import _abi
    colour = form.endswith("colour")
    per_model = form.startswith(("params", "models"))
    names = ("script", "random0", "random1") if per_model else ("script",) * 3
    if form.startswith("params"):               # one scale for the whole sweep: every model's reference under it
        scale = reference(oracle, H, W, "script")[3]
    B = 3
    cases = []
    for b in range(B):
        inp, col, op, sc, want = reference(oracle, H, W, names[b], benign=b != 1)
        if form.startswith("params") and names[b] != "script":
            sc = scale
            want = oracle_colour_cells(oracle, inp, col, sc, op)
        cases.append((inp, col, op, sc, want))
    before = [prefill(H, W, seed=10 + b) for b in range(B)]
    stack = lambda arrays: np.ascontiguousarray(np.stack(arrays))
    g = {k: to_gpu(stack([c[0][k] for c in cases])) for k in CELL_IN}
    g.update({k: to_gpu(stack([bf[k] for bf in before])) for k in OUT_SHAPE})
    if colour:
        g.update({k: to_gpu(stack([c[1][k] for c in cases])) for k in COLOUR_IN})
    planes, cp = plane_structs(g, colour)
    cref = C.byref(cp) if colour else None
    flags = _abi.SOIL_CELLS_KEEP_FLUX if keep else 0
    if form == "uniform":
        rc = hip.soil_erode_cells_fused_batch(C.byref(planes), B, H, W, _abi.vec(cases[0][3], 3),
                                              product_param(cases[0][2])._ref(), flags, None)
    elif form == "colour":
        rc = hip.soil_erode_cells_fused_batch_colour(C.byref(planes), cref, B, H, W, _abi.vec(cases[0][3], 3),
                                                     product_param(cases[0][2])._ref(), flags, None)
    elif form.startswith("params"):
        params = (_abi.Param * B)()
        for b in range(B):
            copy_param(cases[b][2], params[b])
        rc = hip.soil_erode_cells_fused_batch_params(C.byref(planes), cref, B, H, W, _abi.vec(scale, 3), params, flags, None)
    else:
        models = (_abi.BatchModel * B)()
        for b in range(B):
            copy_param(cases[b][2], models[b].param)
            for i in range(3):
                models[b].scale[i] = cases[b][3][i]
        rc = hip.soil_erode_cells_fused_batch_models(C.byref(planes), cref, B, H, W, models, flags, None)
    _abi.check(rc)
    got = {k: to_np(v) for k, v in g.items()}
    for b in range(B):
        inp, col, op, sc, want = cases[b]
        gb = {k: v[b] for k, v in got.items()}
        what = "%s batch, model %d" % (form, b)
        check_host(gb, inp, col, want, keep, colour, what)
        # ... and its own single-model call
        single = upload(inp, col if colour else None, before[b])
        launch(hip, single, "colour" if colour else "ex", _abi.Domain(H, W, 0, H, 0, H), sc, product_param(op), keep)
        for k in CELL_OUT + CELL_FLUX + (COLOUR_OUT if colour else ()):
            assert_bit_equal(gb[k], to_np(single[k]), "%s against the single model: %s" % (what, k))


def check_host(got, inp, col, want, keep, colour, what):
    """check() for planes already on the host, all rows."""
    for name in CELL_OUT + (COLOUR_OUT if colour else ()):
        assert_bit_equal(got[name], want[name], "%s: %s" % (what, name))
    for name in CELL_FLUX:
        if keep:
            assert_bit_equal(got[name], inp[name], "%s: %s kept" % (what, name))
        else:
            assert (bits(got[name]) == 0).all(), "%s: %s not re-zeroed" % (what, name)
    for name in ("layers", "uplift", "rainfall"):
        assert_bit_equal(got[name], inp[name], "%s: %s is input only" % (what, name))
    if colour:
        assert_bit_equal(got["albedoBedrock"], col["albedoBedrock"], what + ": albedoBedrock is input only")


# ---------------------------------------------------------------- the stand-alone ops on the same planes

@pytest.mark.parametrize("pname", PARAM_SETS)
@pytest.mark.parametrize("H,W", [(12, 40), (37, 53), (252, 260), (5, 1), (1, 1)])
def test_stand_alone_cell_ops_on_hostile_planes(hip, oracle, H, W, pname):
    """normalise (transport_* with no walkers: the particle launch returns at once, the normalise runs), mass_transfer
    with and without the colour planes, mass_creep, layer_merge: each against the oracle's op on the same planes.
    The delta mass_transfer adds to holds -0, +0 and numbers: on a flat cell nothing visited it adds fmaxf(0, +0),
    and a -0 becomes +0 (tests/test_cells_hostile.py: the order of the zeros)."""
    from soillib_amd import _abi, soil
    inp, col, op, scale, want = reference(oracle, H, W, pname)
    pp = product_param(op)
    sc = _abi.vec(scale, 3)
    ptr = lambda t: t.c_ptr
    z = lambda *c: np.zeros((H, W) + c, np.float32)
    layers = to_gpu(inp["layers"])
    for with_colour in (False, True):
        # --- normalize_fluvial / normalize_debris
        o = dict(wh=z(), m=z(), v=z(2), d=z(), dv=z(2), af=col["albedoFluvial"].copy(), ad=col["albedoDebris"].copy())
        src = col["albedoSurface"]
        oracle.normalize_fluvial(inp["waterFlux"], inp["massFlux"], inp["velocityFlux"], o["af"] if with_colour else None,
                                 inp["layers"], inp["rainfall"], o["wh"], o["m"], o["v"], src if with_colour else None,
                                 scale, op)
        oracle.normalize_debris(inp["debrisFlux"], inp["debrisVelocityFlux"], o["ad"] if with_colour else None,
                                inp["layers"], o["d"], o["dv"], src if with_colour else None, scale, op)
        r = np.random.default_rng(3)
        g = {k: to_gpu((r.random(v.shape) + 2).astype(np.float32)) for k, v in o.items() if k not in ("af", "ad")}
        g.update(af=to_gpu(col["albedoFluvial"]), ad=to_gpu(col["albedoDebris"]), src=to_gpu(src))
        f = {k: to_gpu(inp[k]) for k in CELL_FLUX}
        none = C.c_void_p(None)
        rain = to_gpu(inp["rainfall"])
        _abi.check(hip.soil_transport_fluvial(
            ptr(layers), ptr(rain), ptr(g["wh"]), ptr(f["waterFlux"]), ptr(g["m"]), ptr(f["massFlux"]),
            ptr(g["v"]), ptr(f["velocityFlux"]), none, ptr(g["af"]) if with_colour else none,
            ptr(g["src"]) if with_colour else none, none, 0, H, W, sc, pp._ref(), None))
        _abi.check(hip.soil_transport_debris(
            ptr(layers), ptr(g["dv"]), ptr(f["debrisVelocityFlux"]), ptr(g["d"]), ptr(f["debrisFlux"]), none,
            ptr(g["ad"]) if with_colour else none, ptr(g["src"]) if with_colour else none, none, 0, H, W, sc,
            pp._ref(), None))
        for k in ("wh", "m", "v", "d", "dv") + (("af", "ad") if with_colour else ()):
            assert_bit_equal(to_np(g[k]), o[k], "normalise (colour %d): %s" % (with_colour, k))
        for k in CELL_FLUX:
            assert_bit_equal(to_np(f[k]), inp[k], "normalise leaves %s" % k)
        for k, name in (("wh", "waterHeight"), ("m", "mass"), ("v", "velocity"), ("d", "debris"), ("dv", "debrisVelocity")):
            assert_bit_equal(o[k], want[name], "the oracle's normalise is the fused reference's: " + name)

        # --- mass_transfer (+ colour), then mass_creep on the same delta
        delta0 = (r.standard_normal((H, W, 2)) * 0.01).astype(np.float32)
        delta0[r.random((H, W)) < 0.4] = -0.0
        delta0[r.random((H, W)) < 0.2] = 0.0
        want_d, want_s = delta0.copy(), col["albedoSurface"].copy()
        c3 = (col["albedoBedrock"], o["af"], o["ad"], want_s) if with_colour else (None,) * 4
        oracle.mass_transfer(want_d, inp["layers"], inp["uplift"], o["m"], o["v"], o["d"], *c3, scale, op)
        g_d, g_s = to_gpu(delta0), to_gpu(col["albedoSurface"])
        gc = (to_gpu(col["albedoBedrock"]), to_gpu(o["af"]), to_gpu(o["ad"]), g_s) if with_colour else (None,) * 4
        soil.mass_transfer(g_d, layers, to_gpu(inp["uplift"]), to_gpu(z()), to_gpu(o["m"]), to_gpu(o["v"]),
                           to_gpu(o["d"]), to_gpu(z(2)), *gc, scale, pp)
        assert_bit_equal(to_np(g_d), want_d, "mass_transfer (colour %d): delta" % with_colour)
        if with_colour:
            assert_bit_equal(to_np(g_s), want_s, "mass_transfer: albedo_surface")
            assert_bit_equal(want_s, want["albedoSurface"], "the oracle's transfer is the fused reference's")
        oracle.mass_creep(want_d, inp["layers"], scale, op)
        soil.mass_creep(g_d, layers, scale, pp)
        assert_bit_equal(to_np(g_d), want_d, "mass_creep after mass_transfer")
    # --- creep alone, from zero; layer_merge
    want_d, g_d = z(2), to_gpu(z(2))
    oracle.mass_creep(want_d, inp["layers"], scale, op)
    soil.mass_creep(g_d, layers, scale, pp)
    assert_bit_equal(to_np(g_d), want_d, "mass_creep")
    g_h = to_gpu(np.full((H, W), 7.0, np.float32))
    soil.layer_merge(g_h, layers)
    assert_bit_equal(to_np(g_h), oracle.layer_merge(inp["layers"]), "layer_merge")
    assert_bit_equal(to_np(layers), inp["layers"], "layers are input only")


# ---------------------------------------------------------------- planes off their 16 bytes

@pytest.mark.parametrize("which", ["massFlux", "uplift", "waterHeight", "height", "albedoSurface", "albedoBedrock"])
@pytest.mark.parametrize("H,W", [(12, 40), (252, 260)])
def test_one_plane_four_bytes_off_its_alignment(hip, oracle, H, W, which):
    """W % 4 == 0, but one plane starts 4 bytes past a 16-byte boundary: vec_path sends the call to the scalar
    kernel.  Input planes, output planes and colour planes, one at a time (one-channel and colour planes: every
    float is still on its own 4 bytes).  The same bits as the aligned call's and the oracle's; the float in front
    of the plane and the one behind it are left alone."""
    from soillib_amd import _abi, silt
    colour = which.startswith("albedo")
    entry = "colour" if colour else "ex"
    for pname, keep in (("script", False), ("random0", True)):
        inp, col, op, scale, want = reference(oracle, H, W, pname)
        before = prefill(H, W)
        g = upload(inp, col if colour else None, before)
        host = dict(inp, **before, **(col if colour else {}))[which]
        guard = np.float32(-7.5)
        block = to_gpu(np.concatenate([[guard], host.ravel(), [guard]]).astype(np.float32))
        assert block.ptr % 16 == 0
        g[which] = silt.tensor.from_device(block.ptr + 4, silt.float32, silt.shape(*host.shape), keepalive=block)
        launch(hip, g, entry, _abi.Domain(H, W, 0, H, 0, H), scale, product_param(op), keep)
        flat = to_np(block)
        assert flat[0] == guard and flat[-1] == guard, "the floats around the plane"
        check(g, inp, col, want, before, (0, H), keep, colour, "%s off its 16 bytes, %s" % (which, pname))


# ---------------------------------------------------------------- the A/B variants are the same function

@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("H,W", [(256, 256), (252, 260)])
def test_every_launch_variant_is_the_same_function(hip, oracle, monkeypatch, H, W, variant, keep):
    """SOIL_CELLS_VARIANT is read on every call.  On (256, 256) 1 is the 512-thread kernel, 3 the 128-thread one, 4
    DIRECT; on (252, 260) 1 and 3 fall through to the 256-thread kernels; 2 switches the XCD remap off; 5 is the
    split (84-byte kernel and zeroing pass); 6 names no variant: the one re-zeroing kernel under remap.  With
    SOIL_CELLS_KEEP_FLUX every variant is the 84-byte kernel."""
    monkeypatch.setenv("SOIL_CELLS_VARIANT", str(variant))
    for pname in ("script", "random0"):
        run_case(hip, oracle, H, W, pname, "ex", keep, what="variant %d" % variant)
    if not keep:
        run_case(hip, oracle, H, W, "default", "plain", False, what="variant %d" % variant)
        run_case(hip, oracle, H, W, "script", "ex", False, rows=(1, H - 1), what="variant %d" % variant)


def child_main():
    """The child of test_knobs_read_once_per_process: the hostile case at three shapes against the oracle, under the
    environment it was started with; the exit status says whether every bit matched."""
    sys.path.insert(0, ROOT)
    from oracle import pyoracle
    from soillib_amd import _abi
    hip = _abi.lib()
    assert hip.soil_device_count() > 0
    for H, W in ((256, 256), (252, 260), (247, 260)):
        for pname in ("script", "random1"):
            run_case(hip, pyoracle, H, W, pname, "plain", False, what="child")
            run_case(hip, pyoracle, H, W, pname, "ex", True, what="child")
            run_case(hip, pyoracle, H, W, pname, "ex", False, rows=(1, H - 1), what="child")
    print("child ok")


@pytest.mark.parametrize("knobs", [{"SOIL_CELLS_SPLIT": "0"}, {"SOIL_CELLS_SPLIT": "0", "SOIL_CELLS_NT": "1"}],
                         ids=["one_kernel", "one_kernel_nontemporal"])
def test_knobs_read_once_per_process(hip, knobs):
    """SOIL_CELLS_SPLIT=0: the one 112-byte kernel that re-zeroes the flux planes itself, with and without the XCD
    remap.  SOIL_CELLS_NT=1 selects that kernel's non-temporal instantiations — only that kernel's: under the default
    split the 84-byte kernel runs and the knob selects nothing, so the child sets both.  One fresh child each."""
    env = dict(os.environ)
    env.update(knobs)
    env.pop("SOIL_CELLS_VARIANT", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0 and "child ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    child_main()
