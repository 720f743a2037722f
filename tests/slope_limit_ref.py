"""Two CPU restatements of soil_slope_limit (include/soil_hip.h: "Threshold hillslopes"), and the inputs that
tests/test_slope_limit_abi.py and tests/test_gpu_slope_limit.py share.

    jacobi(h, scale, slope, edge)     numpy, float32 throughout: every cell takes the candidates of its neighbours'
                                      values of the sweep before, sweeps until nothing moves.  Vectorised: the
                                      reference at GPU sizes.
    dijkstra(h, scale, slope, edge)   a heap: cells settle in the order of their final values.  Valid because
                                      w (+) c >= w for c >= 0; independent of any sweep order.  For small grids.

Both apply nothing but the one rounded update  w[n] <- cand if cand < w[n], cand = w[k] (+) c_k[n]  with
c_k[n] = (float)((double)slope[n] * L_k), c never -0, +inf where the slope entry is not >= 0."""
import functools
import heapq

import numpy as np

D4, D8 = 0, 1
DX = (-1, 0, 0, 1, -1, -1, 1, 1)           # the graph calls' neighbour table
DY = (0, -1, 1, 0, -1, 1, -1, 1)


def edge_count(edge):
    return 4 if edge == D4 else 8


def steps(slope, scale, shape):
    """(cx, cy, cd): the float32 planes of the step toward a row, a column and a diagonal neighbour."""
    sx, sy = np.float64(np.float32(scale[0])), np.float64(np.float32(scale[1]))
    lens = (sx, sy, np.sqrt(sx * sx + sy * sy))
    s = np.broadcast_to(np.asarray(slope, np.float32), shape).astype(np.float64)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        ok = s >= 0
        for L in lens:
            c = np.where(ok, s * L, np.inf).astype(np.float32)
            out.append(np.where(c == 0, np.float32(0), c).astype(np.float32))      # never -0
    return out


def _step_of(k, c3):
    return c3[2] if k >= 4 else (c3[0] if DX[k] != 0 else c3[1])


def _shifted(w, k):
    """w[x + dx, y + dy] for every cell, NaN where that lies off the grid."""
    H, W = w.shape
    v = np.full((H, W), np.nan, np.float32)
    dx, dy = DX[k], DY[k]
    xs = slice(max(0, -dx), H - max(0, dx))
    ys = slice(max(0, -dy), W - max(0, dy))
    xn = slice(max(0, dx), H - max(0, -dx))
    yn = slice(max(0, dy), W - max(0, -dy))
    v[xs, ys] = w[xn, yn]
    return v


def jacobi(h, scale, slope, edge, sweeps=None):
    """The slope-limited surface; `sweeps`: a list that receives the number of sweeps."""
    h = np.asarray(h, np.float32)
    c3 = steps(slope, scale, h.shape)
    w = h.copy()
    n = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            new = w.copy()
            for k in range(edge_count(edge)):
                cand = (_shifted(w, k) + _step_of(k, c3)).astype(np.float32)
                new = np.where(cand < new, cand, new)
            n += 1
            if new.view(np.uint32).tobytes() == w.view(np.uint32).tobytes():
                break
            w = new
    if sweeps is not None:
        sweeps.append(n)
    return w


def dijkstra(h, scale, slope, edge):
    h = np.asarray(h, np.float32)
    H, W = h.shape
    c3 = steps(slope, scale, h.shape)
    w = h.copy()
    heap = [(float(w[x, y]), x, y) for x in range(H) for y in range(W) if w[x, y] == w[x, y]]
    heapq.heapify(heap)
    K = edge_count(edge)
    with np.errstate(invalid="ignore", over="ignore"):
        while heap:
            v, x, y = heapq.heappop(heap)
            if v > w[x, y]:
                continue                                                      # a stale entry
            for k in range(K):
                mx, my = x - DX[k], y - DY[k]                                 # the cell whose neighbour k is (x, y)
                if mx < 0 or my < 0 or mx >= H or my >= W:
                    continue
                cand = np.float32(w[x, y] + _step_of(k, c3)[mx, my])
                if cand < w[mx, my]:
                    w[mx, my] = cand
                    heapq.heappush(heap, (float(cand), mx, my))
    return w


def excess(h, w):
    """h (-) w: +0 where the cell was not lowered, the height's NaN on voids."""
    h = np.asarray(h, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(w < h, (h - w).astype(np.float32), np.where(np.isnan(h), h, np.float32(0))).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def lowered_share(h, w):
    with np.errstate(invalid="ignore"):
        return float((w < h).mean())


# ---- the shared inputs: name -> (h, scale, slope, edge), made once and read-only -------------------------------------

SCALES = (0.3, 0.7)


def smooth(H, W, seed):
    """A smooth terrain: three long waves and a little noise, heights of a few tens."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = 12.0 * np.sin(x / 9.0 + rng.uniform(0, 6)) * np.cos(y / 13.0 + rng.uniform(0, 6))
    z += 6.0 * np.sin((x + 2 * y) / 17.0 + rng.uniform(0, 6)) + 0.3 * x / max(H, 1)
    z += 0.02 * rng.standard_normal((H, W))
    return z.astype(np.float32)


def lithology(H, W, seed, base):
    """A per-cell slope plane: two rock types in bands, all entries > 0."""
    rng = np.random.default_rng(seed + 100)
    s = np.where((np.arange(W)[None, :] // 11 + np.arange(H)[:, None] // 23) % 2 == 0, base, 1.7 * base)
    return (s * (1.0 + 0.1 * rng.random((H, W)))).astype(np.float32)


TERRAIN_SHAPES = ((63, 65), (64, 64), (65, 129), (130, 67))
TERRAIN_SLOPE = 2.0


@functools.lru_cache(maxsize=None)
def terrain_case(shape, edge, plane):
    H, W = shape
    h = smooth(H, W, H * 1000 + W)
    slope = lithology(H, W, H + W, 0.75 * TERRAIN_SLOPE) if plane else TERRAIN_SLOPE
    for a in (h, slope):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return h, SCALES, slope, edge


TINY_SHAPES = ((1, 1), (1, 7), (5, 1))


@functools.lru_cache(maxsize=None)
def tiny_case(shape, edge):
    H, W = shape
    h = (np.random.default_rng(H * 10 + W).random((H, W)) * 10).astype(np.float32)
    h.setflags(write=False)
    return h, SCALES, 0.5, edge


def plateau_pit(H, W, at, depth=100.0):
    h = np.full((H, W), 50.0, np.float32)
    h[at] = np.float32(50.0 - depth)
    return h


@functools.lru_cache(maxsize=None)
def reach_case(corner):
    """A single pit in a 200 x 200 plateau: its cone (depth 100 over steps of 0.15 .. 0.38) crosses three tiles each
    way.  `corner`: the pit in a tile corner instead of the middle."""
    h = plateau_pit(200, 200, (64, 64) if corner else (100, 100))
    h.setflags(write=False)
    return h, SCALES, 0.5, D8


@functools.lru_cache(maxsize=None)
def pit_batch():
    """(heights, a scale pair per model, slope planes) of B = 3 of 65 x 129: the plateau pit beside two smooth models."""
    H, W = 65, 129
    hs = np.stack([smooth(H, W, 1), plateau_pit(H, W, (32, 64)), smooth(H, W, 2)])
    scales = [[0.3, 0.7], [0.25, 0.5], [0.6, 0.4]]
    slope = np.stack([lithology(H, W, 9, 1.5), np.full((H, W), 0.5, np.float32), lithology(H, W, 10, 1.5)])
    for a in (hs, slope):
        a.setflags(write=False)
    return hs, scales, slope


@functools.lru_cache(maxsize=None)
def serpentine_case():
    """A corridor one cell wide that winds between NaN walls over 130 x 130, a low cell at one end: every cell of it
    is lowered from the cell before, a way of more than 8000 cells."""
    H = W = 130
    h = np.full((H, W), np.nan, np.float32)
    for x in range(0, H, 2):
        h[x, :] = 1000.0
        if x + 1 < H:
            h[x + 1, W - 1 if (x // 2) % 2 == 0 else 0] = 1000.0
    h[0, 0] = 0.0
    h.setflags(write=False)
    return h, (1.0, 1.0), 0.01, D4


@functools.lru_cache(maxsize=None)
def banded_case():
    """The same corridor wound inside bands 64 columns wide: down the first band row by row, up the second, down the
    sliver that is left.  Inside one tile the way is some 2000 cells long, many times the kernel's inner cap, while
    nothing moves in the tiles around it: a tile that stops at the cap has only its own dirty mark to come back by."""
    H = W = 130
    h = np.full((H, W), np.nan, np.float32)
    for band, (y0, y1) in enumerate(((0, 62), (64, 126), (128, 129))):
        rows = range(0, H, 2) if band % 2 == 0 else range(H - 2, -1, -2)
        for i, x in enumerate(rows):
            h[x, y0:y1 + 1] = 1000.0
            step = 1 if band % 2 == 0 else -1
            if 0 <= x + step < H and 0 <= x + 2 * step < H:
                h[x + step, y1 if i % 2 == 0 else y0] = 1000.0
    h[128, 63], h[0, 127] = 1000.0, 1000.0                                    # from band to band
    h[0, 0] = 0.0
    h.setflags(write=False)
    return h, (1.0, 1.0), 0.01, D4


# the cells the hostile constructions put their values on: tile corners, tile edges, the apron of a neighbouring tile
SPOTS = ((63, 63), (63, 64), (64, 63), (64, 64), (64, 30), (30, 63), (65, 100), (100, 64), (127, 128), (128, 65), (0, 64),
         (129, 129))


def _walled(h, box):
    """NaN walls around the box (x0, x1, y0, y1), so that what happens inside stays inside."""
    x0, x1, y0, y1 = box
    h[x0:x1 + 1, [y0, y1]] = np.nan
    h[[x0, x1], y0:y1 + 1] = np.nan


@functools.lru_cache(maxsize=None)
def hostile_cases():
    H = W = 130
    base = smooth(H, W, 77)
    out = {}
    # NaN voids on the spots and a wall across two seams
    h = base.copy()
    for s in SPOTS:
        h[s] = np.nan
    h[20:110, 64] = np.nan
    h[63, 5:60] = np.nan
    out["nan"] = (h, SCALES, TERRAIN_SLOPE, D8)
    # +-0: a level floor of +0 with -0 on the spots, in a terrain that is partly below it
    h = np.where(base > 0, np.float32(0), base).astype(np.float32)
    for s in SPOTS:
        h[s] = np.float32(-0.0)
    out["zeros"] = (h, SCALES, TERRAIN_SLOPE, D8)
    out["zeros d4 slope 0"] = (h, SCALES, 0.0, D4)
    # a floor of +0 and -0 under hills, slope 0: the hills come down to +0, every zero keeps its sign
    h = np.where(base > 0, base, np.float32(0)).astype(np.float32)
    h[((np.arange(H)[:, None] + np.arange(W)[None, :]) % 3 == 0) & (h == 0)] = np.float32(-0.0)
    for s in SPOTS:
        h[s] = np.float32(-0.0)
    out["zero floor slope 0"] = (h, SCALES, 0.0, D8)
    # denormal heights and denormal steps
    h = (base.astype(np.float64) * 1e-42).astype(np.float32)
    out["denormal"] = (h, (1e-20, 2e-20), 6e-23, D8)
    # +-inf and +-3e38 on the spots; the low ones walled in, or they take the whole grid
    h = base.copy()
    _walled(h, (56, 72, 56, 72))
    h[64, 64] = -np.inf
    _walled(h, (120, 129, 120, 129))
    h[127, 128] = np.float32(-3e38)
    for s in ((63, 30), (30, 64), (0, 64), (100, 63)):
        h[s] = np.inf
    for s in ((64, 100), (65, 10), (128, 65)):
        h[s] = np.float32(3e38)
    out["inf"] = (h, SCALES, TERRAIN_SLOPE, D8)
    out["inf d4"] = (h, SCALES, TERRAIN_SLOPE, D4)
    # slope entries NaN, negative, +inf and 0 on the spots
    s = lithology(H, W, 5, 0.75 * TERRAIN_SLOPE)
    vals = (np.nan, -1.0, np.inf, 0.0, -0.0, -np.inf)
    for i, at in enumerate(SPOTS):
        s[at] = vals[i % len(vals)]
    s[90:110, 60:70] = np.nan                                  # a block without a limit across a seam
    s[10:20, 60:70] = 0.0                                      # and a level one
    out["slope entries"] = (base, SCALES, s, D8)
    out["slope entries d4"] = (base, SCALES, s, D4)
    # a tile of voids and a tile without a limit (the kernel marks both inert), and -inf over a third of another
    h = base.copy()
    h[64:128, 64:128] = np.nan
    s = lithology(H, W, 6, 0.75 * TERRAIN_SLOPE)
    s[0:64, 64:128] = np.nan
    _walled(h, (70, 100, 10, 40))
    h[71:100, 11:20] = -np.inf
    out["inert tiles"] = (h, SCALES, s, D8)
    # a scalar slope of 0 levels every component: two components behind a wall
    h = base.copy()
    h[:, 64] = np.nan
    h[64, 70:] = np.nan
    out["slope 0"] = (h, SCALES, 0.0, D8)
    for name, (h, sc, sl, e) in out.items():
        for a in (h, sl):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(key):
    """The Jacobi surface of a case, made once: key = ("terrain", shape, edge, plane) | ("tiny", shape, edge) |
    ("reach", corner) | ("serpentine",) | ("banded",) | ("hostile", name)."""
    w = jacobi(*case(key))
    w.setflags(write=False)
    return w


def case(key):
    kind = key[0]
    if kind == "terrain":
        return terrain_case(*key[1:])
    if kind == "tiny":
        return tiny_case(*key[1:])
    if kind == "reach":
        return reach_case(key[1])
    if kind == "serpentine":
        return serpentine_case()
    if kind == "banded":
        return banded_case()
    return hostile_cases()[key[1]]


def all_keys():
    keys = [("terrain", s, e, p) for s in TERRAIN_SHAPES for e in (D4, D8) for p in (False, True)]
    keys += [("tiny", s, e) for s in TINY_SHAPES for e in (D4, D8)]
    keys += [("reach", False), ("reach", True), ("serpentine",), ("banded",)]
    keys += [("hostile", n) for n in hostile_cases()]
    return keys
