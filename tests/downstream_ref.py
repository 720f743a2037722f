"""Two independent numpy restatements of the downstream sums of include/soil_hip.h ("flow graphs: downstream sums":
soil_downstream, soil_stream_power).  Not a test module.  The edge rule and the graphs are tests/flow_paths_ref.py's.

(i)  solve_doubling: the rounds as the header writes them — vectorised float64, the product rounded, then the sum,
     final cells frozen.  The device must give these BITS.
(ii) solve_serial: a walker from the terminals upward, cell by cell in Python floats, x[n] = a L + b x[r] evaluated
     once per cell (for the stream-power step: the implicit formula itself); cells it never reaches are on a cycle or
     drain into one.  Another order of association: it agrees with (i) to rounding, not to the bit.

Both return (out, out64, final): float32 and float64 planes, NaN words canonical, and the plane of resolved cells.
`power`: None for soil_downstream, else (height, erosivity, uplift or None, dt) for soil_stream_power."""
import numpy as np

from flow_paths_ref import D4, D8, DIAG, ROW, edge_of  # noqa: F401

NAN32 = np.uint32(0x7fc00000)
NAN64 = np.uint64(0x7ff8000000000000)


def path_scale(scale):
    """(sx, sy, dd) as the library makes them, or three ones without a scale."""
    if scale is None:
        return np.float64(1.0), np.float64(1.0), np.float64(1.0)
    sx, sy = np.float64(np.float32(scale[0])), np.float64(np.float32(scale[1]))
    return sx, sy, np.sqrt(sx * sx + sy * sy)


def _finish(A, final, shape):
    with np.errstate(over="ignore", invalid="ignore"):
        out = A.astype(np.float32)
    bad = ~final | np.isnan(A)
    w32 = np.where(bad, NAN32, out.view(np.uint32)).astype(np.uint32)
    w64 = np.where(bad, NAN64, A.view(np.uint64)).astype(np.uint64)
    return w32.view(np.float32).reshape(shape), w64.view(np.float64).reshape(shape), final.reshape(shape).copy()


def _plane(p, N, default):
    return np.full(N, default, np.float64) if p is None else np.asarray(p, np.float32).reshape(-1).astype(np.float64)


def solve_doubling(graph, edge, a=None, b=None, t=None, scale=None, stop=None, power=None):
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
    if stop is not None:
        is_edge &= np.asarray(stop).reshape(-1) == 0
    sx, sy, dd = path_scale(scale)
    L = np.where(dy == 0, sx, np.where(dx == 0, sy, dd))       # a row step: only the row changed
    with np.errstate(all="ignore"):
        if power is None:
            A = np.where(is_edge, _plane(a, N, 1.0) * L, _plane(t, N, 0.0))
            B = np.where(is_edge, _plane(b, N, 1.0), 0.0)
        else:
            height, erosivity, uplift, dt = power
            h, dt = _plane(height, N, 0.0), np.float64(dt)
            F = (_plane(erosivity, N, 0.0) * dt) / L
            d = 1.0 + F
            lifted = h if uplift is None else h + dt * _plane(uplift, N, 0.0)
            A = np.where(is_edge, lifted / d, h)
            B = np.where(is_edge, F / d, 0.0)
        ptr = np.where(is_edge, rc, n)
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
    return _finish(A, final, (H, W))


def solve_serial(graph, edge, a=None, b=None, t=None, scale=None, stop=None, power=None):
    graph = np.asarray(graph)
    H, W = graph.shape
    N = H * W
    g = graph.reshape(-1)
    s = np.zeros(N, np.int32) if stop is None else np.asarray(stop).reshape(-1)
    scales = [float(v) for v in path_scale(scale)]
    f = lambda p, i, default: default if p is None else float(np.asarray(p, np.float32).reshape(-1)[i])
    receiver, kind, donors, todo = [-1] * N, [0] * N, [[] for _ in range(N)], []
    for i in range(N):
        e = None if s[i] != 0 else edge_of(g[i], i // W, i % W, H, W, edge)
        if e is None:
            todo.append(i)
        else:
            receiver[i], kind[i] = e
            donors[e[0]].append(i)
    xs = np.zeros(N, np.float64)
    final = np.zeros(N, bool)
    with np.errstate(all="ignore"):
        for i in todo:
            xs[i] = f(t, i, 0.0) if power is None else f(power[0], i, 0.0)
            final[i] = True
        while todo:                                            # every cell is appended at most once: a tree per terminal
            at = todo.pop()
            for i in donors[at]:
                Li = np.float64(scales[kind[i]])
                below = np.float64(xs[at])
                if power is None:
                    xs[i] = np.float64(f(a, i, 1.0)) * Li + np.float64(f(b, i, 1.0)) * below
                else:
                    height, erosivity, uplift, dt = power
                    F = np.float64(f(erosivity, i, 0.0)) * np.float64(dt) / Li
                    xs[i] = (np.float64(f(height, i, 0.0)) + np.float64(dt) * np.float64(f(uplift, i, 0.0)) + F * below) / (1.0 + F)
                final[i] = True
                todo.append(i)
    return _finish(xs, final, (H, W))


def solve_batch(solve, graph, edge, a=None, b=None, t=None, scale=None, stop=None, power=None):
    """`solve` model by model on (B, H, W) planes; `scale`: None, one pair or B pairs."""
    graph = np.asarray(graph)
    B = graph.shape[0]
    pairs = None if scale is None else np.asarray(scale, np.float32).reshape(-1, 2)
    at = lambda p, i: None if p is None else np.asarray(p)[i]
    outs = []
    for i in range(B):
        pw = None if power is None else (power[0][i], power[1][i], at(power[2], i), power[3])
        outs.append(solve(graph[i], edge, at(a, i), at(b, i), at(t, i), None if pairs is None else pairs[i % len(pairs)],
                          at(stop, i), pw))
    return tuple(np.stack([o[k] for o in outs]) for k in range(3))


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
    """The distance of two float32 arrays in units in the last place, cell by cell (equal words: 0; NaN against a
    number, or two different NaN words: a huge count)."""
    def key(v):
        w = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(w < 0, -(w & 0x7fffffff), w)
    return np.abs(key(x) - key(y))
