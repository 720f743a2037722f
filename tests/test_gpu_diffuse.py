"""Hillslope diffusion on the device (include/soil_hip.h: soil_diffuse, soil_diffuse_batch; soillib_amd.soil.diffuse /
diffuse_batch, ErosionBatch.diffuse / evolve), bit for bit against solve_sweeps of tests/diffuse_ref.py: every
comparison with it is of float32 and float64 bit patterns, the NaN words included; there is no tolerance in them.

  shapes      (1, 1), (1, 7), (7, 1), (2, 2), (13, 21); (63, 65), (64, 64), (65, 63): either side of the wave and of two
              32-wide transpose tiles; (1, 129), (129, 1): one line, five tiles long; (130, 257): several work-groups
              and tiles both ways, more rows than two blocks of the prefetch and a tail
  arguments   both first axes, both borders, kappa with w in {0, 1e-3, 0.3, 7, 1e4, 1e9}, diffusivity planes with zeros,
              with one negative and one NaN entry, uplift, anisotropic scales, each output alone and both
  masks       isolated fixed cells, a fixed row, fixed cells at both ends of lines; void cells isolated, at line ends, a
              row, a column, a closed ring, the whole plane
  heights     +-0, +-inf, float32 denormals, +-3e38
  plumbing    planes 4 bytes off their alignment, a second stream, shapes in turn so that the scratch is reused and
              regrown, chunks and 64-bit offsets in child processes, the launch count (five with first_axis = 0, four
              with first_axis = 1, whatever B is)
  batches     B in {1, 3, 8} with one scale pair and B pairs, every slice against its single call, a hostile model
              between two benign ones
  batch class ErosionBatch.diffuse and ErosionBatch.evolve against the module functions
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import diffuse_ref as dref
from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (13, 21), (63, 65), (64, 64), (65, 63), (1, 129), (129, 1), (130, 257)]
SUBSET = [(13, 21), (65, 63), (130, 257)]
SCALE = (0.3, 0.7)
WS = [0.0, 1e-3, 0.3, 7.0, 1e4, 1e9]

_same_words = dref.same_words


def _dt(w):
    """dt that makes kappa dt / sx^2 == w (to rounding) with kappa = 1 and SCALE."""
    return w * float(np.float32(SCALE[0])) ** 2


def _info():
    from soillib_amd import soil
    return soil.diffuse_info()


def _ptr(t):
    return None if t is None else t.c_ptr


def _run(height, scale, dt, kappa=None, diffusivity=None, uplift=None, fixed=None, border=1, first_axis=0,
         outs=(True, True)):
    """One call of the C ABI on numpy planes, (H, W) or (B, H, W) by the height's rank: (out, out64) as numpy, None for
    an output not asked for.  `scale`: one pair, or for a batch one pair or B pairs."""
    from soillib_amd import _abi, silt
    lib = _abi.lib()
    height = np.asarray(height)
    shape = height.shape
    dev = lambda p: None if p is None else to_gpu(np.ascontiguousarray(p))
    planes = [dev(height), dev(diffusivity), dev(uplift), dev(fixed)]
    o32 = silt.tensor(silt.float32, silt.shape(*shape), silt.gpu) if outs[0] else None
    o64 = silt.tensor(silt.float64, silt.shape(*shape), silt.gpu) if outs[1] else None
    pairs = np.asarray(scale, np.float32).reshape(-1)
    sc = (C.c_float * len(pairs))(*pairs.tolist())
    tail = (sc,) if len(shape) == 2 else (sc, len(pairs) // 2)
    fn = lib.soil_diffuse if len(shape) == 2 else lib.soil_diffuse_batch
    _abi.check(fn(_ptr(o32), _ptr(o64), *[_ptr(p) for p in planes], *shape, *tail, 0.0 if kappa is None else float(kappa),
                  float(dt), int(border), int(first_axis), _abi.stream()))
    return (None if o32 is None else to_np(o32), None if o64 is None else to_np(o64))


# ------------------------------------------------------------------ inputs, made once and left as they are

@functools.lru_cache(maxsize=None)
def _planes(H, W, seed=0):
    """heights of standard deviation 100, the same with void cells, a diffusivity plane, uplift and a fixed mask."""
    r = np.random.default_rng([seed, H, W])
    h = (r.standard_normal((H, W)) * 100.0).astype(np.float32)
    hv = h.copy()
    hv[r.random((H, W)) < 0.08] = np.nan
    k = r.uniform(0.1, 2.0, (H, W)).astype(np.float32)
    u = r.uniform(0.0, 0.5, (H, W)).astype(np.float32)
    fixed = (r.random((H, W)) < 0.08).astype(np.int32)
    out = dict(h=h, hv=hv, k=k, u=u, fixed=fixed)
    for p in out.values():
        p.setflags(write=False)
    return out


def _check(what, height, scale, dt, **kw):
    """The device against the restatement on one case; returns the restatement's planes."""
    want = dref.solve_sweeps(height, scale, dt, **kw)
    _same_words(_run(height, scale, dt, **kw), want, what)
    return want


# ------------------------------------------------------------------ against the restatement

@pytest.mark.parametrize("H,W", SHAPES)
def test_every_shape_against_the_restatement(hip, H, W):
    """Both first axes and both borders: kappa alone on plain heights, and every plane at once — a diffusivity plane,
    uplift, a fixed mask, void cells — each output alone and both together."""
    p = _planes(H, W)
    k = 0
    for axis in (0, 1):
        for border in (0, 1):
            what = "%dx%d axis %d border %d" % (H, W, axis, border)
            _check(what + ", kappa", p["h"], SCALE, _dt(7.0), kappa=1.0, border=border, first_axis=axis)
            kw = dict(diffusivity=p["k"], uplift=p["u"], fixed=p["fixed"], border=border, first_axis=axis)
            want = dref.solve_sweeps(p["hv"], SCALE, _dt(7.0), **kw)
            assert (np.isnan(want[1]) == np.isnan(p["hv"])).all()
            for outs in ((True, True), ((True, False), (False, True))[k % 2]):
                got = _run(p["hv"], SCALE, _dt(7.0), outs=outs, **kw)
                assert [g is not None for g in got] == list(outs)
                _same_words(got, want, what + ", every plane, outputs %r" % (outs,))
            k += 1
    assert _info()["launches"] == 4 and _info()["chunks"] == 1 and _info()["idx64_chunks"] == 0    # (first_axis = 1)
    assert _info()["scratch_bytes"] >= 40 * H * W


@pytest.mark.parametrize("H,W", SUBSET)
@pytest.mark.parametrize("w", WS)
def test_scalar_kappa_from_nothing_to_stiff(hip, H, W, w):
    p = _planes(H, W, 1)
    for axis, border in ((0, 1), (1, 0)):
        want = _check("%dx%d w %g axis %d border %d" % (H, W, w, axis, border), p["h"], SCALE, _dt(w), kappa=1.0,
                      border=border, first_axis=axis)
        if w == 0.0:
            _same_words(want, (p["h"], p["h"].astype(np.float64)), "w = 0 returns the heights")
        want = _check("%dx%d w %g with voids and a mask" % (H, W, w), p["hv"], SCALE, _dt(w), kappa=1.0, fixed=p["fixed"],
                      border=border, first_axis=axis)
        assert (np.isnan(want[0]) == np.isnan(p["hv"])).all()
    if w == 0.0:                                                     # kappa = 0 with a dt: the same
        _check("kappa = 0", p["h"], SCALE, 5.0, kappa=0.0, border=0)


@pytest.mark.parametrize("H,W", SUBSET)
def test_diffusivity_planes(hip, H, W):
    p = _planes(H, W, 2)
    zeros = p["k"].copy()
    zeros[np.random.default_rng(H).random((H, W)) < 0.3] = 0.0       # faces of weight zero, and halves of them
    zeros[H // 2, :] = 0.0
    want = _check("zero entries", p["h"], SCALE, _dt(7.0), diffusivity=zeros, border=0)
    assert np.isfinite(want[1]).all()
    _check("all zero", p["h"], SCALE, _dt(7.0), diffusivity=np.zeros((H, W), np.float32), border=0)
    bad = p["k"].copy()
    bad[H // 3, W // 3] = -0.75                                      # used as it is
    bad[(2 * H) // 3, (2 * W) // 3] = np.nan
    for axis in (0, 1):
        want = _check("one negative and one NaN entry, axis %d" % axis, p["h"], SCALE, _dt(0.3), diffusivity=bad, border=0,
                      first_axis=axis)
        assert np.isnan(want[1]).any(), "the NaN weight is used as it is"
        _check("the same under a mask and voids", p["hv"], SCALE, _dt(0.3), diffusivity=bad, fixed=p["fixed"], border=1,
               first_axis=axis)


@pytest.mark.parametrize("H,W", SUBSET)
def test_uplift_and_anisotropic_scales(hip, H, W):
    p = _planes(H, W, 3)
    for scale in ((1.0, 1.0), (0.25, 3.0), (1e-3, 1e3), (40.0, 0.02)):
        for axis in (0, 1):
            what = "%dx%d scale %r axis %d" % (H, W, scale, axis)
            _check(what + ", uplift", p["h"], scale, 2.5, kappa=0.5, uplift=p["u"], border=1, first_axis=axis)
            _check(what + ", uplift under a mask", p["hv"], scale, 2.5, diffusivity=p["k"], uplift=p["u"], fixed=p["fixed"],
                   border=0, first_axis=axis)
    lifted = _check("uplift alone", p["h"], SCALE, 4.0, kappa=0.0, uplift=p["u"], border=1)
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    want = np.where(inner, p["h"].astype(np.float64) + 4.0 * p["u"].astype(np.float64), p["h"].astype(np.float64))
    assert (lifted[1] == want).all(), "dt u on the free cells, nothing on the border"


def _masks(H, W):
    """name -> fixed mask."""
    r = np.random.default_rng([9, H, W])
    iso = (r.random((H, W)) < 0.05).astype(np.int32)
    row = np.zeros((H, W), np.int32)
    row[H // 2, :] = 7                                               # any non-zero word
    ends = np.zeros((H, W), np.int32)
    ends[0, :] = ends[-1, :] = 1
    ends[:, 0] = ends[:, -1] = -1
    ends[0, W // 2] = ends[H // 2, 0] = 0
    first_only = np.zeros((H, W), np.int32)
    first_only[0, ::2] = first_only[::3, 0] = 1
    last_only = np.zeros((H, W), np.int32)
    last_only[-1, 1::2] = last_only[1::3, -1] = 1
    return dict(isolated=iso, row=row, ends=ends, first_only=first_only, last_only=last_only,
                all=np.ones((H, W), np.int32))


def _voids(H, W, h):
    """name -> heights with void cells."""
    r = np.random.default_rng([10, H, W])
    out = {name: h.copy() for name in ("isolated", "line_ends", "row", "column", "ring")}
    out["isolated"][r.random((H, W)) < 0.05] = np.nan
    v = out["line_ends"]
    v[0, ::2] = v[-1, 1::2] = np.nan
    v[::2, 0] = v[1::2, -1] = np.nan
    out["row"][H // 2, :] = np.nan
    out["column"][:, W // 2] = np.nan
    v = out["ring"]
    x0, x1, y0, y1 = H // 4, (3 * H) // 4, W // 4, (3 * W) // 4
    v[x0, y0:y1 + 1] = v[x1, y0:y1 + 1] = np.nan
    v[x0:x1 + 1, y0] = v[x0:x1 + 1, y1] = np.nan
    out["all"] = np.full((H, W), np.nan, np.float32)
    out["all_but_one"] = np.full((H, W), np.nan, np.float32)
    out["all_but_one"][H // 2, W // 2] = 5.0
    return out


@pytest.mark.parametrize("H,W", SUBSET)
def test_fixed_masks(hip, H, W):
    p = _planes(H, W, 4)
    for name, mask in _masks(H, W).items():
        for axis, border in ((0, 0), (1, 0), (0, 1)):
            want = _check("%dx%d mask %s axis %d border %d" % (H, W, name, axis, border), p["h"], SCALE, _dt(7.0), kappa=1.0,
                          fixed=mask, border=border, first_axis=axis)
            held = mask != 0
            assert (dref.words(want[0][held]) == dref.words(p["h"][held])).all(), "a fixed cell keeps its bits"
        _check("%dx%d mask %s, every plane" % (H, W, name), p["hv"], SCALE, _dt(1e4), diffusivity=p["k"], uplift=p["u"],
               fixed=mask, border=0)


@pytest.mark.parametrize("H,W", SUBSET)
def test_void_cells(hip, H, W):
    p = _planes(H, W, 5)
    for name, hv in _voids(H, W, p["h"]).items():
        for axis, border in ((0, 0), (1, 0), (1, 1)):
            want = _check("%dx%d voids %s axis %d border %d" % (H, W, name, axis, border), hv, SCALE, _dt(7.0), kappa=1.0,
                          border=border, first_axis=axis)
            assert (np.isnan(want[1]) == np.isnan(hv)).all(), "NaN where the height is, nowhere else"
        _check("%dx%d voids %s, every plane" % (H, W, name), hv, SCALE, _dt(1e4), diffusivity=p["k"], uplift=p["u"],
               fixed=p["fixed"], border=0)
    ring = _voids(H, W, p["h"])["ring"]                             # what is inside a closed ring sees nothing outside
    other = ring.copy()
    x0, x1, y0, y1 = H // 4, (3 * H) // 4, W // 4, (3 * W) // 4
    outside = np.ones((H, W), bool)
    outside[x0:x1 + 1, y0:y1 + 1] = False
    other[outside] = other[outside] * 2.0 + 1.0
    a, b = _run(ring, SCALE, _dt(1e4), kappa=1.0, border=0), _run(other, SCALE, _dt(1e4), kappa=1.0, border=0)
    inside = np.zeros((H, W), bool)
    inside[x0 + 1:x1, y0 + 1:y1] = True
    assert inside.any() and (dref.words(a[1][inside]) == dref.words(b[1][inside])).all()


@pytest.mark.parametrize("H,W", [(13, 21), (65, 63)])
def test_hostile_heights(hip, H, W):
    """+-0, float32 denormals and +-3e38 keep every result a number (3e38 averages stay below the float32 range with
    border = 0 only in fp64: the float may overflow to inf, as the restatement's does); +-inf make NaN along their
    lines (inf - inf), as the arithmetic does."""
    p = _planes(H, W, 6)
    N = H * W
    at = lambda k: divmod((k * 7919 + 13) % N, W)
    h = p["h"].copy()
    for i, v in enumerate([0.0, -0.0, 1e-44, -1e-40, 1.4e-45, 3e38, -3e38, 3e38]):
        h[at(i)] = v
    h[0, 0], h[-1, -1] = -0.0, 1e-45
    for axis in (0, 1):
        for border in (0, 1):
            for kw in (dict(kappa=1.0), dict(diffusivity=p["k"], uplift=p["u"], fixed=p["fixed"])):
                want = _check("finite, axis %d border %d %s" % (axis, border, sorted(kw)), h, SCALE, _dt(0.3), border=border,
                              first_axis=axis, **kw)
                assert not np.isnan(want[1]).any()
    zeros = np.zeros((H, W), np.float32)
    zeros[::2, 1::2] = -0.0
    _check("a plane of +-0", zeros, SCALE, _dt(7.0), kappa=1.0, border=0)
    tiny = np.full((H, W), 1e-45, np.float32)
    tiny[::3, ::2] = -1.2e-38
    want = _check("a plane of denormals", tiny, SCALE, _dt(7.0), kappa=1.0, border=0)
    assert (np.abs(want[0][want[0] != 0]) < 2.0 ** -126).any(), "float32 denormals among the results"
    for k, v in ((20, np.inf), (21, -np.inf)):
        h[at(k)] = v
    for axis in (0, 1):
        want = _check("with +-inf, axis %d" % axis, h, SCALE, _dt(0.3), kappa=1.0, border=0, first_axis=axis)
        assert np.isnan(want[1]).any()
        _check("with +-inf under a mask, axis %d" % axis, h, SCALE, _dt(0.3), diffusivity=p["k"], fixed=p["fixed"], border=1,
               first_axis=axis)


@pytest.mark.parametrize("H,W", SHAPES)
def test_the_transpose_identity_across_the_two_kernels(hip, H, W):
    """diffuse(h.T, (sy, sx), first_axis=1).T has the bits of diffuse(h, (sx, sy), first_axis=0): the column kernel and
    the tile kernel give each other's bits, on the device alone."""
    p = _planes(H, W, 7)
    t = lambda q: np.ascontiguousarray(q.T)
    for border in (0, 1):
        for axis in (0, 1):
            a = _run(p["hv"], SCALE, _dt(7.0), diffusivity=p["k"], uplift=p["u"], fixed=p["fixed"], border=border, first_axis=axis)
            b = _run(t(p["hv"]), SCALE[::-1], _dt(7.0), diffusivity=t(p["k"]), uplift=t(p["u"]), fixed=t(p["fixed"]),
                     border=border, first_axis=1 - axis)
            _same_words([t(q) for q in b], a, "%dx%d border %d axis %d" % (H, W, border, axis))


# ------------------------------------------------------------------ plumbing

def test_planes_off_their_alignment(hip):
    """Each plane in turn 4 bytes past a 16-byte boundary (out64: 8 bytes), and all of them at once."""
    from soillib_amd import _abi, silt
    B, H, W = 3, 65, 63
    hs = [_planes(H, W, 20 + b) for b in range(B)]
    host = dict(height=np.stack([q["hv"] for q in hs]), diffusivity=np.stack([q["k"] for q in hs]),
                uplift=np.stack([q["u"] for q in hs]), fixed=np.stack([q["fixed"] for q in hs]))
    scales = [(0.3, 0.7), (1.0, 2.0), (0.5, 0.25)]
    want = dref.solve_batch(dref.solve_sweeps, host["height"], scales, _dt(7.0), None, host["diffusivity"], host["uplift"],
                            host["fixed"], 0, 1)

    def placed(arr, dtype, off):
        buf = silt.tensor(dtype, silt.shape(B * H * W + 4), silt.gpu)
        assert buf.ptr % 16 == 0
        view = silt.tensor.from_device(buf.ptr + off, dtype, silt.shape(B, H, W), keepalive=buf)
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            _abi.check(hip.soil_memcpy_h2d(view.c_ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, _abi.stream()))
            _abi.check(hip.soil_stream_synchronize(_abi.stream()))
        return view

    pairs = (C.c_float * (2 * B))(*[v for s in scales for v in s])
    names = ("height", "diffusivity", "uplift", "fixed")
    for off_name in names + ("out", "out64", "all", None):
        off = lambda k: 4 if off_name in (k, "all") else 0
        d = {k: placed(host[k], silt.int32 if k == "fixed" else silt.float32, off(k)) for k in names}
        o32, o64 = placed(None, silt.float32, off("out")), placed(None, silt.float64, 2 * off("out64"))
        _abi.check(hip.soil_diffuse_batch(o32.c_ptr, o64.c_ptr, *[d[k].c_ptr for k in names], B, H, W, pairs, B, 0.0, _dt(7.0),
                                          0, 1, _abi.stream()))
        _same_words((to_np(o32), to_np(o64)), want, "%s off its alignment" % off_name)


def test_on_another_stream_and_with_other_sizes_in_between(hip):
    """A second stream; small, large, small, large: the cached scratch is reused, regrown and reused."""
    import torch
    from soillib_amd import _abi
    cases = []
    for (H, W), seed in (((13, 21), 30), ((130, 257), 31), ((7, 1), 32), ((65, 63), 33)):
        p = _planes(H, W, seed)
        kw = dict(diffusivity=p["k"], uplift=p["u"], fixed=p["fixed"], border=0, first_axis=seed % 2)
        cases.append((p["hv"], kw, dref.solve_sweeps(p["hv"], SCALE, _dt(7.0), **kw)))
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        sizes = []
        for i in (0, 1, 0, 0, 2, 3, 1):
            h, kw, want = cases[i]
            _same_words(_run(h, SCALE, _dt(7.0), **kw), want, "case %d on a second stream" % i)
            sizes.append(_info()["scratch_bytes"])
        assert sizes[0] < sizes[1] and sizes[2] == sizes[0], "the record is the call's own request, not the cached block's size"
    finally:
        _abi.set_stream(0)
    h, kw, want = cases[1]
    _same_words(_run(h, SCALE, _dt(7.0), **kw), want, "back on the default stream")


def test_the_launch_count_does_not_depend_on_b(hip):
    counts = {}
    for B in (1, 8, 64):
        hs = np.stack([_planes(64, 64, 40 + (b % 3))["h"] for b in range(B)])
        got = _run(hs, SCALE, _dt(7.0), kappa=1.0)
        counts[B] = _info()
        want = [dref.solve_sweeps(_planes(64, 64, 40 + m)["h"], SCALE, _dt(7.0), kappa=1.0) for m in range(3)]
        for b in (0, B // 2, B - 1):
            _same_words([g[b] for g in got], want[b % 3], "B %d model %d" % (B, b))
    assert counts[1]["launches"] == counts[8]["launches"] == counts[64]["launches"] == 5         # (first_axis = 0)
    assert all(c["chunks"] == 1 and c["idx64_chunks"] == 0 for c in counts.values())
    assert counts[64]["scratch_bytes"] >= 64 * 40 * 64 * 64


# ------------------------------------------------------------------ batches

BATCH_SHAPES = [(13, 21), (65, 63)]


@functools.lru_cache(maxsize=None)
def _stack(H, W, B):
    """The planes of B different models, their B scale pairs, and the restatement with B pairs and with one."""
    ps = [_planes(H, W, 50 + b) for b in range(B)]
    planes = dict(height=np.stack([q["hv"] for q in ps]), diffusivity=np.stack([q["k"] for q in ps]),
                  uplift=np.stack([q["u"] for q in ps]), fixed=np.stack([q["fixed"] for q in ps]))
    scales = tuple((0.3 + 0.1 * b, 0.7 / (1 + b)) for b in range(B))
    own = dref.solve_batch(dref.solve_sweeps, planes["height"], scales, _dt(7.0), None, planes["diffusivity"],
                           planes["uplift"], planes["fixed"], 0, 1)
    one = dref.solve_batch(dref.solve_sweeps, planes["height"], SCALE, _dt(7.0), 1.0, None, None, planes["fixed"], 1, 0)
    for q in list(planes.values()) + list(own) + list(one):
        q.setflags(write=False)
    return planes, scales, own, one


@pytest.mark.parametrize("H,W", BATCH_SHAPES)
@pytest.mark.parametrize("B", [1, 3, 8])
def test_batches_against_the_restatement_and_the_single_call(hip, H, W, B):
    planes, scales, own, one = _stack(H, W, B)
    got = _run(planes["height"], scales, _dt(7.0), diffusivity=planes["diffusivity"], uplift=planes["uplift"],
               fixed=planes["fixed"], border=0, first_axis=1)
    _same_words(got, own, "%dx%d x %d, own scales" % (H, W, B))
    got_one = _run(planes["height"], SCALE, _dt(7.0), kappa=1.0, fixed=planes["fixed"], border=1, first_axis=0)
    _same_words(got_one, one, "%dx%d x %d, one pair" % (H, W, B))
    for b in range(B):                                               # every slice is its single call
        single = _run(planes["height"][b], scales[b], _dt(7.0), diffusivity=planes["diffusivity"][b], uplift=planes["uplift"][b],
                      fixed=planes["fixed"][b], border=0, first_axis=1)
        _same_words([g[b] for g in got], single, "model %d against its single call" % b)
        single = _run(planes["height"][b], SCALE, _dt(7.0), kappa=1.0, fixed=planes["fixed"][b], border=1, first_axis=0)
        _same_words([g[b] for g in got_one], single, "model %d against its single call, one pair" % b)


def test_a_hostile_model_between_two_benign_ones(hip):
    H, W = 65, 63
    benign = [_planes(H, W, 60), _planes(H, W, 61)]
    r = np.random.default_rng(62)
    bad_h = np.where(r.random((H, W)) < 0.5, np.nan, np.where(r.random((H, W)) < 0.5, np.inf, -np.inf)).astype(np.float32)
    bad_k = np.where(r.random((H, W)) < 0.5, np.nan, -3e38).astype(np.float32)
    h = np.stack([benign[0]["h"], bad_h, benign[1]["h"]])
    k = np.stack([benign[0]["k"], bad_k, benign[1]["k"]])
    for axis in (0, 1):
        got = _run(h, SCALE, _dt(7.0), diffusivity=k, border=0, first_axis=axis)
        _same_words(got, dref.solve_batch(dref.solve_sweeps, h, SCALE, _dt(7.0), None, k, None, None, 0, axis), "axis %d" % axis)
        for m in (0, 2):
            assert np.isfinite(got[1][m]).all(), "model %d took something from its neighbour" % m
            _same_words([g[m] for g in got], _run(h[m], SCALE, _dt(7.0), diffusivity=k[m], border=0, first_axis=axis),
                        "model %d alone" % m)


def _child_main(path):
    """The child of test_chunks: B = 5 as chunks of 2 + 2 + 1 models and as five chunks of one."""
    out = {}
    for H, W in BATCH_SHAPES:
        planes, scales, _, _ = _stack(H, W, 5)
        for models in (2, 1):
            os.environ["SOIL_FLOW_BATCH_CELLS"] = str(models * H * W + (H * W // 2 if models == 2 else 0))
            key = "%dx%d_m%d" % (H, W, models)
            out[key + "_out"], out[key + "_out64"] = _run(planes["height"], scales, _dt(7.0), diffusivity=planes["diffusivity"],
                                                          uplift=planes["uplift"], fixed=planes["fixed"], border=0, first_axis=1)
            i = _info()
            out[key + "_info"] = np.array([i["launches"], i["chunks"], i["idx64_chunks"], i["scratch_bytes"]])
    np.savez(path, **out)


@pytest.mark.parametrize("knob", [None, "idx64"])
def test_chunks(hip, tmp_path, knob):
    """Chunks of 2 + 2 + 1 models and of one model (SOIL_FLOW_BATCH_CELLS) in a child process, on 32-bit offsets and
    ("idx64") under SOIL_PATHS_IDX64 = 1 on the 64-bit offsets of a very large model.  The restatement's bits whatever
    the chunking; the child reports what each call did (soil_diffuse_info)."""
    path = str(tmp_path / "chunks.npz")
    env = dict(os.environ)
    for name in ("SOIL_FLOW_BATCH_CELLS", "SOIL_PATHS_IDX64"):
        env.pop(name, None)
    if knob == "idx64":
        env["SOIL_PATHS_IDX64"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    for H, W in BATCH_SHAPES:
        want = _stack(H, W, 5)[2]
        for models in (2, 1):
            key = "%dx%d_m%d" % (H, W, models)
            _same_words((got[key + "_out"], got[key + "_out64"]), want, "%s, knob %s" % (key, knob))
            chunks = 3 if models == 2 else 5
            info = got[key + "_info"].tolist()
            assert info[:3] == [4 * chunks, chunks, chunks if knob == "idx64" else 0], (key, info)
            assert 40 * models * H * W <= info[3] < 40 * (models + 1) * H * W, "a chunk's scratch planes, and five scale records"


# ------------------------------------------------------------------ the Python surfaces

def test_the_module_functions(hip):
    from soillib_amd import soil
    H, W = 65, 63
    p = _planes(H, W, 70)
    hv, k, u, fixed = (to_gpu(p[n]) for n in ("hv", "k", "u", "fixed"))
    want = dref.solve_sweeps(p["hv"], SCALE, 2.0, diffusivity=p["k"], uplift=p["u"], fixed=p["fixed"], border=0, first_axis=1)
    _same_words((to_np(soil.diffuse(hv, SCALE, 2.0, diffusivity=k, uplift=u, fixed=fixed, border="free", first_axis=1)), None),
                want, "soil.diffuse")
    _same_words((None, to_np(soil.diffuse(hv, SCALE, 2.0, diffusivity=k, uplift=u, fixed=fixed, border="free", first_axis=1,
                                          double=True))), want, "soil.diffuse, double")
    want = dref.solve_sweeps(p["hv"], SCALE, 2.0, kappa=0.25)
    _same_words((to_np(soil.diffuse(hv, SCALE, 2.0, kappa=0.25)), None), want, "soil.diffuse, the defaults")
    planes, scales, own, _ = _stack(13, 21, 3)
    got = soil.diffuse_batch(to_gpu(planes["height"]), [list(s) for s in scales], _dt(7.0), diffusivity=to_gpu(planes["diffusivity"]),
                             uplift=to_gpu(planes["uplift"]), fixed=to_gpu(planes["fixed"]), border="free", first_axis=1)
    _same_words((to_np(got), None), own, "soil.diffuse_batch")
    assert soil.diffuse_info() == dict(launches=4, chunks=1, idx64_chunks=0, scratch_bytes=soil.diffuse_info()["scratch_bytes"])


def test_the_batch_methods(hip, oracle):
    """ErosionBatch.diffuse is diffuse_batch of its height; ErosionBatch.evolve is stream_power and then diffuse_batch,
    bit for bit; the batch's planes stay as they are.  With one scale and with a scale per model."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    B, H, W = 3, 64, 64
    prm = product_param(script_param(oracle.default_param()))
    prm.maxage = 32
    scales = [(20.0 / H * (1 + b), 20.0 / W, 4.0) for b in range(B)]
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    uplift = to_gpu((np.random.default_rng(2).random((B, H, W)) * 1e-3).astype(np.float32))
    kplane = to_gpu(np.random.default_rng(3).uniform(0.01, 0.1, (B, H, W)).astype(np.float32))
    for scale in ((20.0 / H, 20.0 / W, 4.0), scales):
        bt = ErosionBatch(B, H, W, scale, prm, 256, [11 + 7 * b for b in range(B)])
        bt.set_layers(to_gpu(layers))
        silt.set(bt.rainfall, 1.0)
        bt.step()
        before = {n: to_np(getattr(bt, n)).copy() for n in ("height", "layers", "rainfall")}
        pairs = [list(s[:2]) for s in scales] if scale is scales else list(scale[:2])
        got = to_np(bt.diffuse(25.0, kappa=0.02))
        assert (dref.words(got) == dref.words(to_np(soil.diffuse_batch(bt.height, pairs, 25.0, kappa=0.02)))).all()
        _same_words((got, None), dref.solve_batch(dref.solve_sweeps, before["height"], pairs, 25.0, 0.02), "against the restatement")
        got = to_np(bt.diffuse(25.0, diffusivity=kplane, uplift=uplift, border="free", first_axis=1, double=True))
        want = to_np(soil.diffuse_batch(bt.height, pairs, 25.0, diffusivity=kplane, uplift=uplift, border="free", first_axis=1, double=True))
        assert got.dtype == np.float64 and (dref.words(got) == dref.words(want)).all()
        for kw in (dict(), dict(uplift=uplift, m=0.4, edge=soil.d4, first_axis=1)):
            got = to_np(bt.evolve(25.0, 1e-3, kappa=0.02, **kw))
            sp = {k: v for k, v in kw.items() if k != "first_axis"}
            carved = bt.stream_power(25.0, 1e-3, **sp)
            want = to_np(soil.diffuse_batch(carved, pairs, 25.0, kappa=0.02, border="fixed", first_axis=kw.get("first_axis", 0)))
            assert (dref.words(got) == dref.words(want)).all(), "evolve(%r)" % sorted(kw)
            assert np.isfinite(got).all() and (got != to_np(carved)).any()
            _same_words((got, None), dref.solve_batch(dref.solve_sweeps, to_np(carved), pairs, 25.0, 0.02, None, None, None, 1,
                                                      kw.get("first_axis", 0)), "evolve against the restatement")
        for n, v in before.items():
            assert (dref.words(to_np(getattr(bt, n))) == dref.words(v)).all(), "the batch's %s is not touched" % n


def test_refusals_leave_the_outputs_untouched(hip):
    from soillib_amd import _abi
    B, H, W = 2, 5, 8
    mark = np.float32(-7.5)
    o32 = to_gpu(np.full((B, H, W), mark, np.float32))
    o64 = to_gpu(np.full((B, H, W), np.float64(mark), np.float64))
    f = [to_gpu(np.ones((B, H, W), np.float32)) for _ in range(3)]
    fx = to_gpu(np.zeros((B, H, W), np.int32))
    sc = (C.c_float * (2 * B))(1, 1, 1, 1)
    st = _abi.stream()

    def call(name, out=o32, out64=o64, height=f[0], k=f[1], Bn=B, h=H, w=W, s=sc, n=B, kappa=1.0, dt=1.0, border=1, axis=0):
        fn = getattr(hip, "soil_" + name)
        dims = (h, w, s) if name == "diffuse" else (Bn, h, w, s, n)
        return fn(_ptr(out), _ptr(out64), _ptr(height), _ptr(k), f[2].c_ptr, fx.c_ptr, *dims, kappa, dt, border, axis, st)

    for name in ("diffuse", "diffuse_batch"):
        for kw in (dict(height=None), dict(out=None, out64=None), dict(out=f[1]), dict(out64=fx), dict(s=None), dict(h=0),
                   dict(w=-1), dict(h=1 << 16, w=1 << 16), dict(dt=-1.0), dict(dt=float("nan")), dict(k=None, kappa=-1.0),
                   dict(k=None, kappa=float("inf")), dict(border=2), dict(axis=-1)) + \
                ((dict(Bn=0), dict(n=0), dict(n=3), dict(s=(C.c_float * 4)(1, 1, 0, 1))) if name == "diffuse_batch" else ()):
            assert call(name, **kw) == _abi.SOIL_ERR_INVALID_ARGUMENT, (name, kw)
            assert _abi.last_error().startswith(name + ": "), (name, kw, _abi.last_error())
    _abi.check(hip.soil_stream_synchronize(st))
    assert (to_np(o32) == mark).all() and (to_np(o64) == mark).all()


if __name__ == "__main__":
    _child_main(sys.argv[1])
