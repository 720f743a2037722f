"""Two numpy restatements of the stream-power step with a slope exponent above 1 of include/soil_hip.h ("flow graphs:
slope exponents above 1": soil_stream_power_n), on top of tests/downstream_ref.py and tests/deposit_ref.py.  Not a test
module.

(i)  solve_iterated: the header's operations in numpy float64 in its order — the start is solve_doubling's stream-power
     solve, every Newton step solve_doubling's rounds over the linearised coefficients.  `pow` is the power the
     coefficients take: np.power by default, the device's own function (soil_selftest_math64 op 0) for the comparison
     with the kernels, which must then give these BITS for out, out64 and residual; None: no power at all, P = S, which
     is what n == 2 means.  `from_old`: the iteration started from the old heights instead, a flag of the reference
     only — it is what the library does NOT do, and the tests show why.
(ii) solve_exact: the nonlinear implicit equation itself, cell by cell from the terminals upward: s + C s^n = R by
     bisection to the last bit.  No iteration, no linearisation: it agrees with (i) once (i) has converged.

solve_iterated returns a dict: out (float32), out64 (float64), residual (float64 scalar), final (the plane of resolved
cells), `residuals`, the residual of every iteration, and with `every` also `steps`: what a call with iters = 1, 2, ...
returns."""
import numpy as np

import deposit_ref as dep
import downstream_ref as dref
from flow_paths_ref import D4, D8  # noqa: F401


def planes(graph, edge, height, erosivity, scale, dt, uplift=None, stop=None):
    """is_edge (not stopped), the receiver (clipped), L, h, kd and the lifted height b, each as the header makes it."""
    graph = np.asarray(graph)
    N = graph.size
    is_edge, rc, dx, dy = dep._edges(graph, edge)
    if stop is not None:
        is_edge = is_edge & (np.asarray(stop).reshape(-1) == 0)
    sx, sy, dd = dref.path_scale(scale)
    L = np.where(dy == 0, sx, np.where(dx == 0, sy, dd))
    dt = np.float64(dt)
    with np.errstate(all="ignore"):
        h = dep._f64(height, N)
        kd = dep._f64(erosivity, N) * dt
        b = h if uplift is None else h + dt * dep._f64(uplift, N)
    return is_edge, rc, L, h, kd, b


def coefficients(x, rc, L, kd, b, n, pow=np.power):
    """A and B of the linearisation about the iterate x: the header's operations in its order."""
    n = np.float64(n)
    n1 = n - np.float64(1.0)
    with np.errstate(all="ignore"):
        d = x - x[rc]
        S = np.where(d <= 0, 0.0, d / L)                          # (a NaN d is not <= 0: d / L keeps it)
        if n == 2.0 or pow is None:
            assert n == 2.0, "without a power the exponent is 2"
            P = S
        else:
            P = np.asarray(pow(S, np.full_like(S, n1)), np.float64)
        F = ((n * kd) / L) * P
        c = (kd * n1) * (P * S)
        D = 1.0 + F
        return (b + c) / D, F / D


def solve_iterated(graph, edge, height, erosivity, scale, dt, n, uplift=None, stop=None, iters=8, pow=np.power,
                   every=False, from_old=False):
    graph = np.ascontiguousarray(graph, np.int32)
    H, W = graph.shape
    is_edge, rc, L, h, kd, b = planes(graph, edge, height, erosivity, scale, dt, uplift, stop)
    out, out64, final = dref.solve_doubling(graph, edge, scale=scale, stop=stop, power=(height, erosivity, uplift, dt))
    if np.float64(n) == 1.0:
        return dict(out=out, out64=out64, residual=np.float64(0.0), residuals=[], final=final, steps=[])
    x = h.copy() if from_old else out64.reshape(-1).copy()
    residuals, steps = [], []
    for _ in range(iters):
        A, B = coefficients(x, rc, L, kd, b, n, pow)
        out, out64, final = dep._doubling(graph, is_edge, A, B, h)
        before, x = x, out64.reshape(-1).copy()
        residuals.append(dep._residual(x, before))
        if every:
            steps.append(dict(out=out, out64=out64, residual=residuals[-1], final=final))
    return dict(out=out, out64=out64, residual=residuals[-1], residuals=residuals, final=final, steps=steps)


def order_upward(graph, is_edge):
    """The resolved cells in an order from the terminals upward (a cell on a cycle, or draining into one, is not in
    it), and the donors of every cell."""
    r = np.asarray(graph).reshape(-1)
    N = r.size
    donors = [[] for _ in range(N)]
    for i in np.flatnonzero(is_edge).tolist():
        donors[int(r[i])].append(i)
    order = np.flatnonzero(~is_edge).tolist()
    k = 0
    while k < len(order):
        order.extend(donors[order[k]])
        k += 1
    return order, donors


def solve_exact(graph, edge, height, erosivity, scale, dt, n, uplift=None, stop=None):
    """x[i] = b - kd S^n with S = max(x[i] - x[r], 0) / L, cell by cell: with s = S, s + (kd / L) s^n = (b - x[r]) / L,
    whose left side rises with s — bisection on [0, R] until the two ends are neighbouring doubles.  Returns the fp64
    plane (NaN where the cell is not resolved) and the number of edges of the longest way down."""
    graph = np.asarray(graph)
    H, W = graph.shape
    is_edge, rc, L, h, kd, b = planes(graph, edge, height, erosivity, scale, dt, uplift, stop)
    order, _ = order_upward(graph, is_edge)
    x = np.full(H * W, np.nan)
    depth = np.zeros(H * W, np.int64)
    n = float(n)
    for i in order:
        if not is_edge[i]:
            x[i] = h[i]
            continue
        r = int(rc[i])
        depth[i] = depth[r] + 1
        Li, C, R = float(L[i]), float(kd[i]) / float(L[i]), (float(b[i]) - float(x[r])) / float(L[i])
        if not R > 0:                                             # the receiver is not below: no erosion (or a NaN)
            x[i] = b[i] if R == R else np.nan
            continue
        lo, hi = 0.0, R
        while True:
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if mid + C * mid ** n > R:
                hi = mid
            else:
                lo = mid
        x[i] = float(x[r]) + lo * Li
    return x.reshape(H, W), int(depth.max())


def defect(x, graph, edge, height, erosivity, scale, dt, n, uplift=None, stop=None):
    """|x[i] - b[i] + kd S^n| of every cell with an edge, S from x itself; the largest term of the equation the solver
    solves for the cell, (1 + F) x = b + c + F x[r] with F = n kd S^(n-1) / L: the largest of |x|, |b|, kd S^n, F |x| and
    F |x[r]|; and F.  Zeros on the terminals."""
    graph = np.asarray(graph)
    is_edge, rc, L, h, kd, b = planes(graph, edge, height, erosivity, scale, dt, uplift, stop)
    x = np.asarray(x, np.float64).reshape(-1)
    n = np.float64(n)
    with np.errstate(all="ignore"):
        d = x - x[rc]
        S = np.where(d <= 0, 0.0, d / L)
        term = kd * np.power(S, n)
        F = ((n * kd) / L) * np.power(S, n - 1.0)
        miss = np.where(is_edge, np.abs((x - b) + term), 0.0)
        largest = np.maximum.reduce([np.abs(x), np.abs(b), term, F * np.abs(x), F * np.abs(x[rc])])
    shape = graph.shape
    return miss.reshape(shape), np.where(is_edge, largest, 0.0).reshape(shape), np.where(is_edge, F, 0.0).reshape(shape)


def solve_batch(graph, edge, height, erosivity, scale, dt, n, uplift=None, stop=None, iters=8, pow=np.power):
    """solve_iterated model by model on (B, H, W) planes; `scale`: one pair or B pairs."""
    graph = np.asarray(graph)
    pairs = np.asarray(scale, np.float32).reshape(-1, 2)
    at = lambda p, i: None if p is None else np.asarray(p)[i]
    outs = [solve_iterated(graph[i], edge, height[i], erosivity[i], pairs[i % len(pairs)], dt, n, at(uplift, i),
                           at(stop, i), iters, pow) for i in range(graph.shape[0])]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in ("out", "out64", "residual", "final")}


def same_words(got, want, what):
    """out, out64 and residual of the device (a dict; None or missing: not asked for) against a restatement's."""
    for name in ("out", "out64", "residual"):
        g = got.get(name)
        if g is None:
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(want[name])
        if name == "residual":
            g, w = g.reshape(-1), w.reshape(-1)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = dref.words(g) != dref.words(w)
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            raise AssertionError("%s: %s differs in %d of %d cells, first at %s: %r (0x%x) against %r (0x%x)" % (
                what, name, bad.sum(), bad.size, at, g[at], dref.words(g)[at], w[at], dref.words(w)[at]))
