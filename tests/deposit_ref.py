"""Two numpy restatements of the erosion-deposition step of include/soil_hip.h ("flow graphs: erosion-deposition":
soil_stream_power_deposit), on top of tests/downstream_ref.py and the oracle's accumulate.  Not a test module.

(i)  solve_iterated: the header's operations in numpy float64 in its order, oracle.accumulate for Qs (the bits
     soil_accumulate gives), solve_doubling's rounds for the solve.  The device must give these BITS for out, out64,
     flux and residual.
(ii) solve_serial: the same iteration with a cell-by-cell walker for the solve and a plain Python upstream sum in
     fp64: another order of association, and no float32 rounding of Qs.  It agrees with (i) to rounding.

Both return a dict: out (float32), out64 (float64), flux (float32), residual (float64 scalar), final (the plane of
resolved cells), and `residuals`, the residual of every iteration."""
import numpy as np

import downstream_ref as dref
from flow_paths_ref import D4, D8, edge_of  # noqa: F401


def _edges(graph, edge):
    """is_edge, receiver (clipped) and the edge's L selector planes of solve_doubling, for a (H, W) graph."""
    graph = np.asarray(graph)
    H, W = graph.shape
    N = H * W
    n = np.arange(N, dtype=np.int64)
    x, y = n // W, n % W
    r = graph.reshape(-1).astype(np.int64)
    inside = (r >= 0) & (r < N)
    rc = np.where(inside, r, 0)
    dx, dy = rc // W - x, rc % W - y
    is_edge = inside & (np.abs(dx) <= 1) & (np.abs(dy) <= 1) & ((dx != 0) | (dy != 0))
    if edge == D4:
        is_edge &= (dx == 0) | (dy == 0)
    return is_edge, rc, dx, dy


def _f64(p, N):
    return np.asarray(p, np.float32).reshape(-1).astype(np.float64)


def coefficients(graph, edge, height, erosivity, deposition, uplift, scale, dt):
    """is_edge, b, g, d, B0 and the terminals' heights, each operation as the header orders it."""
    graph = np.asarray(graph)
    N = graph.size
    is_edge, rc, dx, dy = _edges(graph, edge)
    sx, sy, dd = dref.path_scale(scale)
    L = np.where(dy == 0, sx, np.where(dx == 0, sy, dd))
    dt = np.float64(dt)
    with np.errstate(all="ignore"):
        h = _f64(height, N)
        F = (_f64(erosivity, N) * dt) / L
        g = _f64(deposition, N)
        d = (1.0 + F) + g
        b = h if uplift is None else h + dt * _f64(uplift, N)
        B0 = F / d
    return is_edge, h, b, g, d, B0


def make_q(is_edge, b, x):
    """q of an iterate: (float)(b - x), +0 on terminals and wherever that float is not finite."""
    with np.errstate(all="ignore"):
        q = (b - x).astype(np.float32)
    return np.where(is_edge & np.isfinite(q), q, np.float32(0.0)).astype(np.float32)


def _residual(x, before):
    with np.errstate(all="ignore"):
        diff = np.abs(x - before)
    diff = diff[~np.isnan(diff)]
    return np.float64(diff.max()) if diff.size else np.float64(0.0)


def solve_iterated(oracle, graph, edge, height, erosivity, deposition, scale, dt, uplift=None, iters=8, every=False):
    """`every`: also `steps`, what a call with iters = 1, 2, ... returns (out, out64, flux, residual, final), from this
    one run of the iteration."""
    graph = np.ascontiguousarray(graph, np.int32)
    H, W = graph.shape
    is_edge, h, b, g, d, B0 = coefficients(graph, edge, height, erosivity, deposition, uplift, scale, dt)
    x = np.where(is_edge, b, h)
    residuals, steps = [], []
    for k in range(1, iters + 1):
        q = make_q(is_edge, b, x)
        Qs = oracle.accumulate(graph, q.reshape(H, W), edge).reshape(-1) if k > 1 else np.zeros(H * W, np.float32)
        with np.errstate(all="ignore"):
            Qup = Qs.astype(np.float64) - q.astype(np.float64)
            A0 = (((1.0 + g) * b) + (g * Qup)) / d
        # the solve with these coefficients: a = A0 (L == 1 without a scale), b = B0 — but they are fp64, so the
        # rounds are restated here as solve_doubling writes them
        out, out64, final = _doubling(graph, is_edge, A0, B0, h)
        before, x = x, out64.reshape(-1).copy()
        residuals.append(_residual(x, before))
        if every and k < iters:
            steps.append(dict(out=out, out64=out64, flux=oracle.accumulate(graph, make_q(is_edge, b, x).reshape(H, W), edge),
                              residual=residuals[-1], final=final))
    flux = oracle.accumulate(graph, make_q(is_edge, b, x).reshape(H, W), edge)
    result = dict(out=out, out64=out64, flux=flux, residual=residuals[-1], residuals=residuals, final=final)
    if every:
        result["steps"] = steps + [dict(out=out, out64=out64, flux=flux, residual=residuals[-1], final=final)]
    return result


def _doubling(graph, is_edge, A0, B0, h):
    """solve_doubling's rounds (tests/downstream_ref.py) over fp64 coefficients: terminals hold h and B = 0."""
    H, W = graph.shape
    N = H * W
    n = np.arange(N, dtype=np.int64)
    rc = np.where(is_edge, graph.reshape(-1).astype(np.int64), n)
    with np.errstate(all="ignore"):
        A = np.where(is_edge, A0, h)
        B = np.where(is_edge, B0, 0.0)
        ptr = rc
        final = ~is_edge
        rounds = 0
        while (1 << rounds) < N:
            rounds += 1
        for _ in range(rounds):
            move = ~final
            A = np.where(move, A + (B * A[ptr]), A)
            B = np.where(move, B * B[ptr], B)
            final = final | final[ptr]
            ptr = np.where(move, ptr[ptr], ptr)
    return dref._finish(A, final, (H, W))


def solve_serial(graph, edge, height, erosivity, deposition, scale, dt, uplift=None, iters=8):
    """Cell by cell: the solve from the terminals upward, x[n] = A0 + B0 x[r] once per cell; the upstream sum from the
    heads downward in fp64 Python floats."""
    graph = np.asarray(graph)
    H, W = graph.shape
    N = H * W
    is_edge, h, b, g, d, B0 = coefficients(graph, edge, height, erosivity, deposition, uplift, scale, dt)
    r = graph.reshape(-1)
    donors = [[] for _ in range(N)]
    for i in range(N):
        if is_edge[i]:
            donors[int(r[i])].append(i)
    # cells in an order from the terminals upward (cells on a cycle or draining into one never enter it)
    order = [i for i in range(N) if not is_edge[i]]
    k = 0
    while k < len(order):
        order.extend(donors[order[k]])
        k += 1
    reached = np.zeros(N, bool)
    reached[order] = True

    def upstream(q):
        total = [float(v) for v in q]
        for i in reversed(order):
            if is_edge[i]:
                total[int(r[i])] += total[i]
        return np.array(total, np.float64)

    x = np.where(is_edge, b, h)
    residuals = []
    with np.errstate(all="ignore"):
        for _ in range(iters):
            diff = b - x
            q = np.where(is_edge & reached & np.isfinite(diff.astype(np.float32)), diff, 0.0)
            Qup = upstream(q) - q
            A0 = (((1.0 + g) * b) + (g * Qup)) / d
            new = np.full(N, np.nan)
            for i in order:
                new[i] = A0[i] + B0[i] * new[int(r[i])] if is_edge[i] else h[i]
            before, x = x, new
            residuals.append(_residual(x, before))
        diff = b - x
        q = np.where(is_edge & reached & np.isfinite(diff.astype(np.float32)), diff, 0.0)
        flux = upstream(q)
    out, out64, final = dref._finish(x, reached, (H, W))
    return dict(out=out, out64=out64, flux=flux.astype(np.float32).reshape(H, W), residual=residuals[-1],
                residuals=residuals, final=final)


def solve_batch(solve, graph, edge, height, erosivity, deposition, scale, dt, uplift=None, iters=8):
    """`solve` (a callable of the planes of one model) model by model on (B, H, W) planes; `scale`: one pair or B."""
    graph = np.asarray(graph)
    pairs = np.asarray(scale, np.float32).reshape(-1, 2)
    outs = [solve(graph[i], edge, height[i], erosivity[i], deposition[i], pairs[i % len(pairs)], dt,
                  None if uplift is None else uplift[i], iters) for i in range(graph.shape[0])]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in ("out", "out64", "flux", "residual", "final")}


def same_words(got, want, what):
    """out, out64, flux and residual of the device (a dict; None or missing: not asked for) against a restatement's."""
    for name in ("out", "out64", "flux", "residual"):
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
