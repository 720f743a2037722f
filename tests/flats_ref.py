"""Numpy restatements of include/soil_hip.h, "flow graphs: conditioning" (not a test module): the flat distance twice —
(i) a breadth-first search with a queue, (ii) a vectorised relaxation over shifted planes run to a fixed point — and
the receiver rule as a loop over cells; and the constructions the tests of both kinds share.  Heights are compared
as float32: -0 == +0, inf == inf, NaN equals nothing."""
import collections

import numpy as np

D4, D8 = 0, 1
DX = (-1, 0, 0, 1, -1, -1, 1, 1)          # the order of the graph calls' tables; the first four for D4
DY = (0, -1, 1, 0, -1, 1, -1, 1)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _k(edge):
    return 4 if edge == D4 else 8


def seeds(h, edge):
    """The cells that can drain: non-NaN, with a neighbour position off the grid, a NaN neighbour or a lower one."""
    h = np.asarray(h, np.float32)
    H, W = h.shape
    pad = np.full((H + 2, W + 2), np.nan, np.float32)           # off the grid reads as NaN: both are outlets
    pad[1:-1, 1:-1] = h
    out = np.zeros((H, W), bool)
    with np.errstate(invalid="ignore"):
        for k in range(_k(edge)):
            nb = pad[1 + DX[k]:1 + DX[k] + H, 1 + DY[k]:1 + DY[k] + W]
            out |= np.isnan(nb) | (nb < h)
    return out & ~np.isnan(h)


def distance_bfs(h, edge):
    """(i) breadth-first from all seeds at once, a cell at a time (on Python lists: float32 values widen exactly)."""
    h = np.asarray(h, np.float32)
    H, W = h.shape
    hl = h.tolist()
    dist = [[-1] * W for _ in range(H)]
    queue = collections.deque()
    for x, y in np.argwhere(seeds(h, edge)).tolist():
        dist[x][y] = 0
        queue.append((x, y))
    steps = list(zip(DX, DY))[:_k(edge)]
    while queue:
        x, y = queue.popleft()
        for dx, dy in steps:
            nx, ny = x + dx, y + dy
            if 0 <= nx < H and 0 <= ny < W and dist[nx][ny] < 0 and hl[nx][ny] == hl[x][y]:
                dist[nx][ny] = dist[x][y] + 1
                queue.append((nx, ny))
    return np.array(dist, np.int32).reshape(H, W)


def distance_relax(h, edge):
    """(ii) d <- min(d, 1 + d of every equal neighbour) on whole planes until nothing moves."""
    h = np.asarray(h, np.float32)
    H, W = h.shape
    big = np.int64(1) << 40
    d = np.where(seeds(h, edge), np.int64(0), big)
    hp = np.full((H + 2, W + 2), np.nan, np.float32)
    hp[1:-1, 1:-1] = h
    equal = [hp[1 + DX[k]:1 + DX[k] + H, 1 + DY[k]:1 + DY[k] + W] == h for k in range(_k(edge))]
    while True:
        dp = np.full((H + 2, W + 2), big, np.int64)
        dp[1:-1, 1:-1] = d
        new = d
        for k, eq in enumerate(equal):
            new = np.minimum(new, np.where(eq, dp[1 + DX[k]:1 + DX[k] + H, 1 + DY[k]:1 + DY[k] + W] + 1, big))
        if (new == d).all():
            break
        d = new
    return np.where(d >= big, -1, d).astype(np.int32)


def receivers(graph, h, dist, edge):
    """The receiver rule, cell by cell."""
    graph, dist, h = np.asarray(graph, np.int32), np.asarray(dist, np.int32), np.asarray(h, np.float32)
    H, W = h.shape
    out = graph.copy()
    hl, dl = h.tolist(), dist.tolist()
    steps = list(zip(DX, DY))[:_k(edge)]
    for x, y in np.argwhere((graph < 0) & (dist > 0)).tolist():
        for dx, dy in steps:
            nx, ny = x + dx, y + dy
            if 0 <= nx < H and 0 <= ny < W and hl[nx][ny] == hl[x][y] and dl[nx][ny] == dl[x][y] - 1:
                out[x, y] = nx * W + ny
                break
    return out


def same(got, want, what):
    """Two int32 planes, cell for cell."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = got != want
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d cells differ, first at %s: %d against %d" % (
            what, bad.sum(), bad.size, at, got[at], want[at]))


def interior_terminals(graph):
    """Cells without a receiver that are not on the grid's border."""
    t = np.asarray(graph) < 0
    t[0, :] = t[-1, :] = False
    t[:, 0] = t[:, -1] = False
    return t


# ---- constructions ---------------------------------------------------------------------------------------------

def level(H, W, v=5.0):
    return np.full((H, W), v, np.float32)


def corridor(L):
    """A corridor one cell wide and L long inside higher walls, open at its left end only: (3, L + 1)."""
    h = np.full((3, L + 1), 9.0, np.float32)
    h[1, :L] = 2.0
    return h


def nan_blocks(H, W):
    """A level plane with a NaN block over the corner of the first tile and NaN cells on the seams."""
    h = level(H, W)
    for x in range(60, 68):
        for y in range(60, 68):
            if x < H and y < W:
                h[x, y] = np.nan
    for x, y in ((63, 10), (64, 11), (20, 63), (21, 64), (127, 127), (128, 128), (64, 64)):
        if x < H and y < W:
            h[x, y] = np.nan
    if H > 2 and W > 2:
        h[H // 2, W // 2] = np.nan
    return h


def closed(H, W):
    """A closed level depression inside higher ground (no way out: all -1), and single pits (-1 each) in the ground
    below it; the ground itself is a flat that drains over the border and into the depression and the pits."""
    h = level(H, W, 9.0)
    if H >= 8 and W >= 5:
        h[2:H // 2, 2:W - 2] = 3.0
        for y in range(2, W - 2, 9):
            h[H - 3, y] = 1.0
    return h


def terraces(H, W):
    """Two level terraces that touch along a ragged line, the lower one left."""
    h = level(H, W, 7.0)
    for x in range(H):
        h[x, :max(0, W // 2 + (x % 5) - 2)] = 4.0
    return h


def diagonal_flats(H, W):
    """Equal-height flats that touch only diagonally (a chequerboard of 3 x 3 blocks on higher ground); the blocks of
    the border ring drain, the inner ones only through their corners — under D8."""
    h = level(H, W, 9.0)
    for x in range(H):
        for y in range(W):
            if ((x // 3) + (y // 3)) % 2 == 0:
                h[x, y] = 2.0
    return h


def signed_zeros(H, W):
    r = np.random.default_rng(5)
    return np.where(r.random((H, W)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)


def infinities(H, W):
    """A flat at +inf beside a flat at -inf, and a finite strip between them in the middle rows."""
    h = np.full((H, W), np.inf, np.float32)
    h[:, W // 2:] = -np.inf
    if H > 4:
        h[H // 3:H // 2, max(0, W // 2 - 1):W // 2 + 1] = 0.0
    return h


def denormals(H, W):
    """Heights that differ in the last bits of denormal numbers: plateaus of 1e-45 steps."""
    r = np.random.default_rng(7)
    words = (r.integers(0, 3, (H, W)) + (np.arange(W)[None, :] // 7)).astype(np.uint32)
    return words.view(np.float32)


def quantised(oracle, H, W):
    """floor(noise * 20): many natural flats of every shape."""
    return np.floor(oracle.noise(H, W, seed=3.0, ext=(float(H), float(W))) * np.float32(20.0)).astype(np.float32)


def serpentine(H, W):
    """A level corridor of pitch 2 through higher ground with one outlet, the border cell (1, 0): rows 1, 3, 5, ... are
    corridor, joined alternately at the right and the left end."""
    h = level(H, W, 9.0)
    rows = list(range(1, H - 1, 2)) if W >= 3 else []
    for i, x in enumerate(rows):
        h[x, 1:W - 1] = 1.0
        if i + 1 < len(rows):
            h[x + 1, W - 2 if i % 2 == 0 else 1] = 1.0
    if rows:
        h[1, 0] = 1.0
    return h


def constructions(H, W):
    """(name, height) of the plain constructions at one shape."""
    return [("level", level(H, W)), ("nan blocks", nan_blocks(H, W)), ("closed", closed(H, W)),
            ("terraces", terraces(H, W)), ("diagonal flats", diagonal_flats(H, W)),
            ("signed zeros", signed_zeros(H, W)), ("infinities", infinities(H, W)), ("denormals", denormals(H, W))]


def hostile_graph(H, W, seed=3):
    """A graph plane of entries no graph call makes: -1, -7, INT32_MIN, the cell itself, INT32_MAX, a far cell."""
    r = np.random.default_rng(seed)
    n = np.arange(H * W, dtype=np.int64).reshape(H, W)
    pick = r.integers(0, 6, (H, W))
    g = np.choose(pick, [np.full((H, W), -1), np.full((H, W), -7), np.full((H, W), INT32_MIN), n,
                         np.full((H, W), INT32_MAX), (n * 7 + 3) % (H * W)])
    return g.astype(np.int32)
