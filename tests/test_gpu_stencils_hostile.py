"""The stencil kernels (csrc/stencil.hip: soil_gradient, soil_negslope, soil_laplacian, soil_normal,
soil_gaussian_blur) against the CPU oracle where the rules that pick between a kernel's fast and its written-out form
decide: bit for bit (util.assert_bit_equal: two NaNs are equal whatever their sign), no tolerance anywhere.

  scales off the plain range   every scale of SCALES_OFF_PLAIN on x, on y and on both: the written-out builds
                               k_gradient4<false>, k_negslope4<false> and k_normal4 with fast = false
  scales at the ends           2^-40 and 2^40 in all four combinations: the fast form on values either side of
                               2^-54 | 2^48 (win_row_plain) and quotients either side of 2^-60 | 2^90 (QuotWatch)
  normal                       flat patches (a -0 numerator under a negative z scale), lengths either side of 2^40,
                               NaN and inf cells where lerp5 falls back; the host twin on the same inputs
  laplacian                    non-finite cells, a different plane per channel, clamp-to-self on the small shapes
  blur                         every sigma (denormal and zero outer taps, negative, infinite, 0 and NaN), grids inside
                               the 16-cell apron, a narrow tail after a wide segment, planes off their 16 bytes
  every window walk            SOIL_WIN_SHAPE 0 .. 8, a child process each, on the cases at the ends
  the band builds              SOIL_NORMAL_BAND / SOIL_LAP2_BAND (4, 4), (16, 8), (32, 32), a child process each

The planes, the cases and the informative-output cap that selects them are tests/stencils_ref.py; that they reach
what they were built for is asserted without a GPU by tests/test_stencils_hostile.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import stencils_ref as R
from util import assert_bit_equal, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIS = os.path.join(ROOT, "tests", "test_gpu_stencils_hostile.py")


class _Device:
    """The front-end of stencils_ref.run on the device: numpy in, numpy out."""

    @staticmethod
    def gradient(h, sc):
        from soillib_amd import soil
        return to_np(soil.gradient(to_gpu(h), sc))

    @staticmethod
    def negslope(h, sc):
        from soillib_amd import soil
        return to_np(soil.negslope(to_gpu(h), sc))

    @staticmethod
    def normal(h, sc):
        from soillib_amd import soil
        return to_np(soil.normal(to_gpu(h), sc))

    @staticmethod
    def laplacian(t, sc):
        from soillib_amd import soil
        return to_np(soil.laplacian(to_gpu(t), sc))

    @staticmethod
    def gaussian_blur(t, sigma):
        from soillib_amd import soil
        gt = to_gpu(t)
        ret = soil.gaussian_blur(gt, sigma)
        assert ret is gt                                    # in place: returns its input handle, filter.cu:90
        return to_np(gt)


def _compare(oracle, cases):
    kept, _ = R.select(oracle, cases)
    assert kept
    for name, op, plane, args, want in kept:
        assert_bit_equal(R.run(_Device, op, plane, args), want, name)
    return len(kept)


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_scales_off_the_plain_range(hip, oracle, H, W):
    """The first launch of the written-out window builds (any scale outside [2^-40, 2^40], a denormal, negative, zero,
    infinite or NaN one), and the scalar kernels under the same scales."""
    _compare(oracle, R.off_plain_cases(H, W))


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_scales_at_the_ends(hip, oracle, H, W):
    """2^-40 and 2^40 are inside the plain range: the fast form, with loaded values and quotients on either side of
    every threshold, in exponent planes and in single cells where one value decides for a whole wave."""
    _compare(oracle, R.ends_cases(H, W))


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_normal_under_every_z_scale(hip, oracle, H, W):
    from soillib_amd import silt, soil
    kept, _ = R.select(oracle, R.normal_cases(H, W))
    assert kept
    for name, op, plane, args, want in kept:
        got = R.run(_Device, op, plane, args)
        assert_bit_equal(got, want, name)
        host = soil.normal(silt.tensor.from_numpy(np.ascontiguousarray(plane)), args).numpy()   # soil_normal_host: normal_cell
        assert_bit_equal(host, want, name + ": the host twin against the oracle")
        assert_bit_equal(host, got, name + ": the host twin against the device")


@pytest.mark.parametrize("H,W", R.SHAPES)
@pytest.mark.parametrize("D", [1, 2])
def test_laplacian_on_non_finite_cells(hip, oracle, D, H, W):
    _compare(oracle, R.laplacian_cases(H, W, D))


@pytest.mark.parametrize("H,W", R.BLUR_SHAPES)
def test_blur_under_every_sigma(hip, oracle, H, W):
    for Cn in (1, 2):
        _compare(oracle, R.blur_cases(H, W, Cn))


def test_blur_with_planes_off_their_16_bytes(hip, oracle):
    """The launcher takes the 16-byte form of the axis-1 pass only when the tensor and the scratch plane are both
    aligned: each in turn 4 bytes off, at a width whose rows would otherwise be taken 16 bytes at a time."""
    from soillib_amd import _abi, silt
    H, W = 33, 1028
    t = R.blur_planes(H, W, 1)["normal"]

    def plane(arr, off):
        buf = silt.tensor(silt.float32, silt.shape(H * W + 4), silt.gpu)
        assert buf.ptr % 16 == 0
        view = silt.tensor.from_device(buf.ptr + off, silt.float32, silt.shape(H, W, 1), keepalive=buf)
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            _abi.check(hip.soil_memcpy_h2d(view.c_ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, _abi.stream()))
            _abi.check(hip.soil_stream_synchronize(_abi.stream()))
        return view

    for sigma in (2.5, 0.3):
        want = oracle.gaussian_blur(t, sigma)
        for off_t, off_s in ((0, 0), (4, 0), (0, 4), (4, 4)):
            gt, gs = plane(t, off_t), plane(None, off_s)
            _abi.check(hip.soil_gaussian_blur(gt.c_ptr, gs.c_ptr, H, W, 1, C.c_float(sigma), _abi.stream()))
            assert_bit_equal(to_np(gt), want, "blur, tensor %d and scratch %d bytes off" % (off_t, off_s))


def test_blur_twice_on_a_second_stream(hip, oracle):
    import torch
    from soillib_amd import _abi
    cases = [(name, plane, args) for H, W, Cn in ((33, 1030, 1), (40, 515, 2), (17, 15, 2))
             for name, op, plane, args in R.blur_cases(H, W, Cn) if args in (2.5, 0.05)]
    first = [_Device.gaussian_blur(plane, args) for name, plane, args in cases]
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        for _ in range(2):
            for (name, plane, args), want in zip(cases, first):
                got = _Device.gaussian_blur(plane, args)
                assert_bit_equal(got, want, name + ": a second stream against the default stream")
    finally:
        _abi.set_stream(0)
    for (name, plane, args), got in zip(cases, first):
        assert_bit_equal(got, oracle.gaussian_blur(plane, args), name)


def _child(env, ids, limit):
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + ids,
                       env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0, "%r:\n%s\n%s" % (env, r.stdout[-3000:], r.stderr[-1000:])
    assert "%d passed" % len(ids) in r.stdout and "failed" not in r.stdout, r.stdout[-1000:]


@pytest.mark.parametrize("shape", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_the_ends_under_every_window_walk(hip, shape):
    """SOIL_WIN_SHAPE is read once per process: each walk (four implementations of plain(), a has_up / has_dn rule
    each) meets the threshold cells in a process of its own."""
    _child({"SOIL_WIN_SHAPE": str(shape)}, ["%s::test_scales_at_the_ends[%d-%d]" % (THIS, H, W) for H, W in R.CHILD_SHAPES], 120)


@pytest.mark.parametrize("normal_band,lap2_band", [(4, 4), (16, 8), (32, 32)])
def test_the_band_builds(hip, normal_band, lap2_band):
    """k_normal4<BAND> and k_laplacian4x2<BAND> other than the defaults 8 and 16 (both knobs are read once per process)."""
    ids = ["%s::test_normal_under_every_z_scale[%d-%d]" % (THIS, H, W) for H, W in R.CHILD_SHAPES]
    ids += ["%s::test_laplacian_on_non_finite_cells[2-%d-%d]" % (THIS, H, W) for H, W in R.CHILD_SHAPES]
    ids += ["%s::test_scales_off_the_plain_range[%d-%d]" % (THIS, H, W) for H, W in R.CHILD_SHAPES[:1]]
    _child({"SOIL_NORMAL_BAND": str(normal_band), "SOIL_LAP2_BAND": str(lap2_band)}, ids, 120)
