"""Two independent numpy restatements of the hillslope-diffusion step of include/soil_hip.h ("hillslope diffusion":
soil_diffuse, soil_diffuse_batch).  Not a test module.

(i)  solve_sweeps: the two sweeps as the header writes them — float64, every operation rounded once in the header's
     order, vectorised across the lines of a sweep and serial along them, the selects by predicate.  The device must
     give these BITS.
(ii) solve_dense: per line, the tridiagonal matrix assembled in full and solved with numpy.linalg.solve (LU with
     pivoting).  Another algorithm: it agrees with (i) to rounding, not to the bit.

Both return (out, out64): float32 and float64 planes, NaN words canonical.  Planes are (H, W); `scale` = (sx, sy);
`border`: 1 the outermost rows and columns are fixed, 0 they are not."""
import numpy as np

NAN32 = np.uint32(0x7fc00000)
NAN64 = np.uint64(0x7ff8000000000000)


def words(p):
    """The bit patterns of a float32 or float64 array."""
    p = np.ascontiguousarray(p)
    return p.view(np.uint32 if p.dtype == np.float32 else np.uint64)


def same_words(got, want, what):
    """(out, out64) of the device against the restatement's; None: not asked for."""
    for g, w, name in zip(got, want, ("out", "out64")):
        if g is None:
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = words(g) != words(w)
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            raise AssertionError("%s: %s differs in %d of %d cells, first at %s: %r (0x%x) against %r (0x%x)" % (
                what, name, bad.sum(), bad.size, at, g[at], words(g)[at], w[at], words(w)[at]))


def ulps32(x, y):
    """The distance of two float32 arrays in units in the last place (equal words: 0; NaN against a number: huge)."""
    def key(v):
        w = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(w < 0, -(w & 0x7fffffff), w)
    return np.abs(key(x) - key(y))


def kinds(height, fixed, border):
    """(void, free) planes of a (H, W) grid."""
    h = np.asarray(height, np.float32)
    H, W = h.shape
    void = np.isnan(h)
    fx = np.zeros((H, W), bool) if fixed is None else np.asarray(fixed) != 0
    if border:
        fx = fx.copy()
        fx[0, :] = fx[-1, :] = True
        fx[:, 0] = fx[:, -1] = True
    return void, ~void & ~fx


def _finish(x):
    with np.errstate(over="ignore", invalid="ignore"):
        out = x.astype(np.float32)
    bad = np.isnan(x)
    w32 = np.where(bad, NAN32, out.view(np.uint32)).astype(np.uint32)
    w64 = np.where(bad, NAN64, np.ascontiguousarray(x).view(np.uint64)).astype(np.uint64)
    return w32.view(np.float32), w64.view(np.float64)


def _face_weights(k, kappa, dt, ss, shape):
    """w of the face between cells i and i + 1 of every line (lines along axis 1 of `shape`): (L, n - 1)."""
    L, n = shape
    if k is None:
        return np.full((L, max(n - 1, 0)), (np.float64(kappa) * dt) / ss)
    kf = 0.5 * (k[:, :-1] + k[:, 1:])
    return (kf * dt) / ss


def _sweep(d, void, free, k, kappa, dt, ss):
    """One sweep along axis 1 of (L, n) planes (float64 d, bool void and free, float64 k or None), the header's
    operations in the header's order."""
    L, n = d.shape
    dt, ss = np.float64(dt), np.float64(ss)
    with np.errstate(all="ignore"):
        w = _face_weights(k, kappa, dt, ss, (L, n))
        linked = ~void[:, :-1] & ~void[:, 1:]                       # cells i and i + 1
        zero = np.zeros(L, np.float64)
        e, g = np.empty((L, n), np.float64), np.empty((L, n), np.float64)
        for i in range(n):
            lp = free[:, i] & linked[:, i - 1] if i > 0 else np.zeros(L, bool)
            ln = free[:, i] & linked[:, i] if i < n - 1 else np.zeros(L, bool)
            p = np.where(lp, w[:, i - 1], zero) if i > 0 else zero
            q = np.where(ln, w[:, i], zero) if i < n - 1 else zero
            b = (1.0 + p) + q
            if i > 0:
                den = np.where(lp, b - p * g[:, i - 1], b)
                num = np.where(lp, d[:, i] + p * e[:, i - 1], d[:, i])
            else:
                den, num = b, d[:, i]
            e[:, i] = num / den
            g[:, i] = q / den
        x = np.empty((L, n), np.float64)
        for i in range(n - 1, -1, -1):
            if i < n - 1:
                ln = free[:, i] & linked[:, i]
                x[:, i] = np.where(ln, e[:, i] + g[:, i] * x[:, i + 1], e[:, i])
            else:
                x[:, i] = e[:, i]
    return x


def _dense_sweep(d, void, free, k, kappa, dt, ss):
    """The same sweep, line by line: the matrix in full, numpy.linalg.solve.  Void cells are taken out of the system
    (their rows would hold NaN) and come back as NaN."""
    L, n = d.shape
    dt, ss = np.float64(dt), np.float64(ss)
    x = np.full((L, n), np.nan, np.float64)
    with np.errstate(all="ignore"):
        w = _face_weights(k, kappa, dt, ss, (L, n))
        for l in range(L):
            A = np.eye(n, dtype=np.float64)
            for i in range(n):
                if not free[l, i]:
                    continue
                if i > 0 and not void[l, i - 1]:
                    A[i, i - 1] = -w[l, i - 1]
                    A[i, i] += w[l, i - 1]
                if i < n - 1 and not void[l, i + 1]:
                    A[i, i + 1] = -w[l, i]
                    A[i, i] += w[l, i]
            keep = np.flatnonzero(~void[l])
            if keep.size:
                x[l, keep] = np.linalg.solve(A[np.ix_(keep, keep)], d[l, keep])
    return x


def _solve(sweep, height, scale, dt, kappa, diffusivity, uplift, fixed, border, first_axis):
    h32 = np.asarray(height, np.float32)
    assert h32.ndim == 2 and first_axis in (0, 1) and border in (0, 1)
    assert (kappa is None) != (diffusivity is None)
    void, free = kinds(h32, fixed, border)
    h = h32.astype(np.float64)
    k = None if diffusivity is None else np.asarray(diffusivity, np.float32).astype(np.float64)
    sx, sy = np.float64(np.float32(scale[0])), np.float64(np.float32(scale[1]))
    ss = (sx * sx, sy * sy)
    dt = np.float64(dt)
    with np.errstate(all="ignore"):
        d = h
        if uplift is not None:
            d = np.where(free, h + dt * np.asarray(uplift, np.float32).astype(np.float64), h)
    for axis in (first_axis, 1 - first_axis):
        if axis == 1:
            d = sweep(d, void, free, k, kappa, dt, ss[1])
        else:
            d = sweep(np.ascontiguousarray(d.T), void.T, free.T, None if k is None else np.ascontiguousarray(k.T), kappa, dt, ss[0]).T
    return _finish(np.ascontiguousarray(d))


def solve_sweeps(height, scale, dt, kappa=None, diffusivity=None, uplift=None, fixed=None, border=1, first_axis=0):
    """(i): the definition.  The device must give these bits."""
    return _solve(_sweep, height, scale, dt, kappa, diffusivity, uplift, fixed, border, first_axis)


def solve_dense(height, scale, dt, kappa=None, diffusivity=None, uplift=None, fixed=None, border=1, first_axis=0):
    """(ii): dense matrices and numpy.linalg.solve, line by line."""
    return _solve(_dense_sweep, height, scale, dt, kappa, diffusivity, uplift, fixed, border, first_axis)


def solve_batch(solve, height, scale, dt, kappa=None, diffusivity=None, uplift=None, fixed=None, border=1, first_axis=0):
    """`solve` model by model on (B, H, W) planes; `scale`: one pair or B pairs."""
    height = np.asarray(height)
    pairs = np.asarray(scale, np.float32).reshape(-1, 2)
    at = lambda p, i: None if p is None else np.asarray(p)[i]
    outs = [solve(height[i], pairs[i % len(pairs)], dt, kappa, at(diffusivity, i), at(uplift, i), at(fixed, i), border, first_axis)
            for i in range(height.shape[0])]
    return tuple(np.stack([o[k] for o in outs]) for k in range(2))
