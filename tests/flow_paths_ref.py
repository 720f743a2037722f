"""Two independent numpy restatements of the downstream walk of include/soil_hip.h ("flow graphs: downstream"), and
the graphs the flow-path tests run on.  Not a test module.

(i)  walk_serial: a plain walker, cell by cell, with a visited set for cycles.
(ii) walk_doubling: vectorised int64 pointer doubling, for the larger shapes.

Both return (terminal, steps, length): int32, int32 and float32 planes; `length` is None without a scale."""
import numpy as np

D4, D8 = 0, 1
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
NAN_WORD = 0x7fc00000
ROW, COL, DIAG = 0, 1, 2


def edge_of(g, x, y, H, W, edge):
    """The edge rule: (receiver, kind) of cell (x, y) with graph entry g, or None for no edge."""
    r = int(g)
    if not 0 <= r < H * W:
        return None
    qx, qy = r // W, r % W
    dx, dy = qx - x, qy - y
    if abs(dx) > 1 or abs(dy) > 1 or (dx == 0 and dy == 0):
        return None
    if edge == D4 and dx != 0 and dy != 0:
        return None
    return r, (DIAG if dx != 0 and dy != 0 else (ROW if dx != 0 else COL))


def lengths(n_row, n_col, n_diag, scale):
    """(float)(((double)n_row * sx + (double)n_col * sy) + (double)n_diag * dd), one rounding per operation."""
    sx, sy = np.float64(np.float32(scale[0])), np.float64(np.float32(scale[1]))
    dd = np.sqrt(sx * sx + sy * sy)
    rows = np.asarray(n_row, np.float64) * sx
    cols = np.asarray(n_col, np.float64) * sy
    diag = np.asarray(n_diag, np.float64) * dd
    with np.errstate(over="ignore"):
        return ((rows + cols) + diag).astype(np.float32)


def _finish(terminal, counts, resolved, shape, scale):
    terminal = np.where(resolved, terminal, -1).astype(np.int32).reshape(shape)
    steps = np.where(resolved, counts.sum(axis=0), -1).astype(np.int32).reshape(shape)
    length = None
    if scale is not None:
        length = lengths(counts[ROW], counts[COL], counts[DIAG], scale)
        length = np.where(resolved, length.view(np.uint32), np.uint32(NAN_WORD)).astype(np.uint32).view(np.float32)
        length = length.reshape(shape)
    return terminal, steps, length


def walk_serial(graph, edge, scale=None, stop=None):
    graph = np.asarray(graph)
    H, W = graph.shape
    g = graph.reshape(-1)
    s = np.zeros(H * W, np.int32) if stop is None else np.asarray(stop).reshape(-1)
    terminal = np.zeros(H * W, np.int64)
    counts = np.zeros((3, H * W), np.int64)
    resolved = np.zeros(H * W, bool)
    for n in range(H * W):
        at, seen, c = n, set(), [0, 0, 0]
        while True:
            if at in seen:
                break                                  # a cycle: the walk never ends
            seen.add(at)
            e = None if s[at] != 0 else edge_of(g[at], at // W, at % W, H, W, edge)
            if e is None:
                resolved[n] = True
                break
            at = e[0]
            c[e[1]] += 1
        terminal[n] = at
        counts[:, n] = c
    return _finish(terminal, counts, resolved, (H, W), scale)


def walk_doubling(graph, edge, scale=None, stop=None):
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
    ptr = np.where(is_edge, rc, n)
    counts = np.zeros((3, N), np.int64)
    counts[ROW] = is_edge & (dx != 0) & (dy == 0)
    counts[COL] = is_edge & (dx == 0)
    counts[DIAG] = is_edge & (dx != 0) & (dy != 0)
    rounds = 0
    while (1 << rounds) < N:
        rounds += 1
    for _ in range(rounds):
        counts = counts + counts[:, ptr]
        ptr = ptr[ptr]
    return _finish(ptr, counts, ~is_edge[ptr], (H, W), scale)


def walk_batch(walk, graph, edge, scale=None, stop=None):
    """`walk` model by model on (B, H, W) planes; `scale`: one pair or B pairs."""
    graph = np.asarray(graph)
    B = graph.shape[0]
    pairs = None if scale is None else np.asarray(scale, np.float32).reshape(-1, 2)
    outs = [walk(graph[b], edge, None if pairs is None else pairs[b % len(pairs)],
                 None if stop is None else np.asarray(stop)[b]) for b in range(B)]
    return tuple(None if outs[0][i] is None else np.stack([o[i] for o in outs]) for i in range(3))


# ---- graphs ----------------------------------------------------------------------------------------------------

def serpentine(H, W):
    """A chain through every cell, H W - 1 edges long, straight steps only: row 0 left to right, row 1 back, ..."""
    g = np.full((H, W), -1, np.int64)
    for x in range(H):
        cols = range(W) if x % 2 == 0 else range(W - 1, -1, -1)
        cols = list(cols)
        for i, y in enumerate(cols):
            if i + 1 < W:
                g[x, y] = x * W + cols[i + 1]
            elif x + 1 < H:
                g[x, y] = (x + 1) * W + y
    return g.astype(np.int32)


def all_donors(H, W, edge):
    """Centres on a lattice of pitch three, every neighbour (K of them inside the grid) draining into its centre."""
    g = np.full((H, W), -1, np.int64)
    for x in range(H):
        for y in range(W):
            cx, cy = x - x % 3 + 1, y - y % 3 + 1
            if cx >= H or cy >= W or (cx, cy) == (x, y):
                continue
            if edge == D4 and cx != x and cy != y:
                continue
            g[x, y] = cx * W + cy
    return g.astype(np.int32)


def all_minus_one(H, W):
    return np.full((H, W), -1, np.int32)


def hostile(H, W, seed, model=0):
    """Every kind of entry that is no edge next to the ones that are: the cell itself, non-neighbours, diagonals
    (no edges under D4), INT32_MIN / INT32_MAX, negative numbers, entries in the neighbouring models' numbering
    (H W and above, and the same below zero), and random neighbours, off the grid's edge included."""
    rng = np.random.default_rng([seed, H, W, model])
    N = H * W
    n = np.arange(N, dtype=np.int64)
    x, y = n // W, n % W
    kind = rng.integers(0, 10, N)
    dx, dy = rng.integers(-1, 2, N), rng.integers(-1, 2, N)
    g = (x + dx) * W + (y + dy)                        # a neighbour, perhaps off the edge or wrapped into the next row
    g = np.where(kind == 0, n, g)
    g = np.where(kind == 1, rng.integers(0, N, N), g)  # anywhere in the model
    g = np.where(kind == 2, INT32_MIN, g)
    g = np.where(kind == 3, INT32_MAX, g)
    g = np.where(kind == 4, n + N + rng.integers(-1, 2, N) * W, g)   # the next model's numbering
    g = np.where(kind == 5, n - N + rng.integers(-1, 2, N), g)       # the model before
    g = np.where(kind == 6, -1, g)
    return np.clip(g, INT32_MIN, INT32_MAX).astype(np.int32).reshape(H, W)


def cycles(H, W):
    """Rows 0 and 1 drain into a ring of four cells, the last row into a two-cell cycle, every other row to its
    cell in column 1, a terminal.  H >= 4, W >= 3."""
    assert H >= 4 and W >= 3
    g = np.full((H, W), -1, np.int64)
    for x in range(H):
        for y in range(2, W):
            g[x, y] = x * W + y - 1
        g[x, 0] = x * W + 1
    g[0, 0], g[0, 1], g[1, 1], g[1, 0] = 1, W + 1, W, 0               # the ring
    g[H - 1, 0], g[H - 1, 1] = (H - 1) * W + 1, (H - 1) * W           # the pair
    return g.astype(np.int32)


def terrain(H, W, seed, plateaus=False):
    rng = np.random.default_rng([seed, H, W])
    xx, yy = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    h = (np.sin(xx * 0.37 + seed) * np.cos(yy * 0.23) * 3.0 + 0.02 * xx + rng.random((H, W))).astype(np.float32)
    if plateaus:
        h = np.round(h * 2.0) / 2.0
    return h.astype(np.float32)


_SHIFT = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))


def descent(height, edge, seed=None):
    """A downhill receiver per cell, in numpy: the steepest one (seed None), or a random one of the lower
    neighbours — stand-ins, on the CPU, for the graphs the library's `steepest` and `random_weighted` make."""
    H, W = height.shape
    rng = None if seed is None else np.random.default_rng(seed)
    g = np.full((H, W), -1, np.int64)
    for x in range(H):
        for y in range(W):
            best, smax, lower = -1, 0.0, []
            for k, (dx, dy) in enumerate(_SHIFT[:4 if edge == D4 else 8]):
                qx, qy = x + dx, y + dy
                if not (0 <= qx < H and 0 <= qy < W):
                    continue
                s = float(height[x, y] - height[qx, qy]) / (1.0 if k < 4 else 2.0 ** 0.5)
                if s > 0:
                    lower.append(qx * W + qy)
                if s > smax:
                    best, smax = qx * W + qy, s
            g[x, y] = best if rng is None or not lower else lower[rng.integers(len(lower))]
    return g.astype(np.int32)


def built_graphs(H, W, edge, seed=1):
    """(name, graph) of every constructed graph a (H, W) grid takes."""
    out = [("serpentine", serpentine(H, W)), ("all_donors", all_donors(H, W, edge)),
           ("minus_one", all_minus_one(H, W)), ("hostile", hostile(H, W, seed)),
           ("hostile2", hostile(H, W, seed + 1))]
    if H >= 4 and W >= 3:
        out.append(("cycles", cycles(H, W)))
    return out


def stop_planes(H, W, graph=None):
    """(name, plane or None): none, one pour point in mid-grid, every cell, and a cell of the ring of `cycles`."""
    mid = np.zeros((H, W), np.int32)
    mid[H // 2, W // 2] = 1
    out = [("none", None), ("mid", mid), ("all", np.ones((H, W), np.int32))]
    if H >= 4 and W >= 3:
        ring = np.zeros((H, W), np.int32)
        ring[1, 1] = 7                                 # any non-zero value stops
        out.append(("ring", ring))
    return out


def words(a):
    """The bit patterns of an int32 or float32 array."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.int32).view(np.uint32)


NAMES = ("terminal", "steps", "length")


def same_words(got, want, what):
    """(terminal, steps, length) of the device against a restatement's, word for word; None: not asked for."""
    for g, w, name in zip(got, want, NAMES):
        assert (g is None) == (w is None), (what, name)
        if g is None:
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = words(g) != words(w)
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            raise AssertionError("%s: %s differs in %d of %d cells, first at %s: %r (0x%08x) against %r (0x%08x)" % (
                what, name, bad.sum(), bad.size, at, g[at], words(g)[at], w[at], words(w)[at]))
