"""Exact multiple-flow accumulation (include/soil_hip.h: soil_mfd_weights, soil_mfd_accumulate) restated in numpy, step
for step as the header states it, plus the inputs that tests/test_mfd_abi.py and tests/test_gpu_mfd.py share.

  weights()           the K outgoing shares of every cell.  The two primitives are arguments: `exp2(a, b)` — rw_exp2, on the
                      device soil_selftest_math op 12 — and `pow_(S, e)` — sp_pow, soil_selftest_math64 op 0.  The
                      defaults are numpy's, good for everything but a bit-for-bit comparison with the device.
  accumulate()        whole-grid Jacobi in fp64 until no bit changes
  accumulate_tiled()  the same cells' expression under the kernel's schedule: 64 x 64 tiles, at most 256 sweeps a tile
                      and launch, a tile runs if it or one of its eight neighbours moved in the launch before
  dense()             (I - W^T) as a dense fp64 matrix, for np.linalg.solve
"""
import numpy as np

D4, D8 = 0, 1
SHIFT = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))    # the neighbour table
OPP = (3, 2, 1, 0, 7, 6, 5, 4)                                                    # the neighbour's direction back
SQRT2 = np.float32(1.41421354)                                                    # soil_math.hpp: kSqrt2
LOG2E = 1.4426950408889634
QNAN64 = np.uint64(0x7FF8000000000000)
TILE, INNER = 64, 256


def k_of(edge):
    return 4 if edge == D4 else 8


def host_exp2(a, b):
    with np.errstate(all="ignore"):
        return np.exp2((np.asarray(a, np.float32) * np.asarray(b, np.float32)).astype(np.float32)).astype(np.float32)


def host_pow(S, e):
    with np.errstate(all="ignore"):
        return np.power(np.asarray(S, np.float64), np.asarray(e, np.float64))


def rw_const(T):
    """rw_const: a double quotient, then a float, for the straight and the diagonal neighbours."""
    T = np.float64(np.float32(T))
    with np.errstate(all="ignore"):
        return np.float32(np.float64(LOG2E) / T), np.float32(np.float64(LOG2E) / (np.float64(SQRT2) * T))


def lengths(scale):
    sx, sy = np.float64(np.float32(scale[0])), np.float64(np.float32(scale[1]))
    return sx, sy, np.sqrt(sx * sx + sy * sy)


def shifted(a, k, fill):
    """Plane of neighbour k's entries of `a`, `fill` off the grid."""
    H, W = a.shape
    pad = np.full((H + 2, W + 2), fill, a.dtype)
    pad[1:-1, 1:-1] = a
    dx, dy = SHIFT[k]
    return pad[1 + dx:1 + dx + H, 1 + dy:1 + dy + W]


def weights(h, edge, T=None, p=None, scale=None, dist=None, exp2=host_exp2, pow_=host_pow):
    """(K, H, W) float32: the outgoing shares."""
    assert (T is None) != (p is None)
    K = k_of(edge)
    h = np.ascontiguousarray(h, np.float32)
    ok = np.stack([shifted(np.ones(h.shape, bool), k, False) for k in range(K)])
    hn = np.stack([shifted(h, k, np.float32(0)) for k in range(K)])
    with np.errstate(all="ignore"):
        diff = (h[None] - hn).astype(np.float32)                      # one fp32 subtraction
        if T is not None:
            c = np.empty_like(diff)
            c[:4], c[4:] = rw_const(T)
            raw = np.asarray(exp2(diff, c), np.float32).reshape(diff.shape)
        else:
            lx, ly, ld = lengths(scale)
            L = np.array([lx if SHIFT[k][0] != 0 and SHIFT[k][1] == 0 else ly if SHIFT[k][0] == 0 else ld
                          for k in range(K)], np.float64)[:, None, None]
            S = diff.astype(np.float64) / L                           # one fp64 division
            raw = np.asarray(pow_(S, np.full(S.shape, np.float64(p))), np.float64).reshape(S.shape).astype(np.float32)
            raw = np.where(np.isnan(diff), np.float32(np.nan), raw)   # the NaN diff is tested for itself
        P = np.where(diff <= 0, np.float32(0), raw)                   # (NaN <= 0 is false: the weight is NaN)
        P = np.where(ok, P, np.float32(0)).astype(np.float32)
        Z = np.zeros(h.shape, np.float32)
        for k in range(K):                                            # ((P_0 + P_1) + ...) in fp32
            Z = (Z + P[k]).astype(np.float32)
        sends = np.isfinite(Z) & (Z > 0)
        w = np.where(sends[None], (P / np.where(sends, Z, np.float32(1))[None]).astype(np.float32), np.float32(0))
    w = w.astype(np.float32)
    if dist is not None:
        dist = np.ascontiguousarray(dist, np.int32)
        flat = ~sends & (Z == 0) & (dist > 0)
        found = np.zeros(h.shape, bool)
        for k in range(K):
            dn = shifted(dist, k, np.int32(-(2 ** 31)))
            take = flat & ~found & ok[k] & (hn[k] == h) & (dn.astype(np.int64) == dist.astype(np.int64) - 1)
            w[k][take] = 1.0
            found |= take
    return w


def incoming(w):
    """(K, H, W): share k of a cell is neighbour k's outgoing share towards it (0 off the grid)."""
    return np.stack([shifted(w[OPP[k]], k, np.float32(0)) for k in range(w.shape[0])])


def _source(w, source):
    return (np.ones(w.shape[1:], np.float64) if source is None
            else np.ascontiguousarray(source, np.float32).astype(np.float64))


def _sweep(a, src, win):
    """One Jacobi sweep: the header's accumulation on every cell of `a` (any window of the grid with its apron cut
    by the caller).  `a` carries a one-cell apron; src and win[k] are the inner cells'."""
    H, W = src.shape
    s = src.copy()
    with np.errstate(all="ignore"):
        for k in range(win.shape[0]):
            dx, dy = SHIFT[k]
            an = a[1 + dx:1 + dx + H, 1 + dy:1 + dy + W]
            wk = win[k].astype(np.float64)
            nz = win[k] != 0
            s = np.where(nz, s + an * np.where(nz, wk, 0.0), s)       # a zero share is skipped
    s.view(np.uint64)[np.isnan(s)] = QNAN64
    return s


def _start(src):
    """a = source on a one-cell apron of zeros (never read: nothing off the grid has a share), NaN canonical."""
    H, W = src.shape
    inner = src.copy()
    inner.view(np.uint64)[np.isnan(inner)] = QNAN64
    a = np.zeros((H + 2, W + 2), np.float64)
    a[1:-1, 1:-1] = inner
    return a


def accumulate(w, source=None, max_sweeps=None):
    """Whole-grid Jacobi from a = source until no bit changes: (a, sweeps)."""
    src = _source(w, source)
    win = incoming(w)
    H, W = src.shape
    a = _start(src)
    for sweep in range(1, (max_sweeps or H * W + 2) + 1):
        new = _sweep(a, src, win)
        if (new.view(np.uint64) == np.ascontiguousarray(a[1:-1, 1:-1]).view(np.uint64)).all():
            return new, sweep
        a[1:-1, 1:-1] = new
    raise AssertionError("the restatement did not settle: the shares are no DAG")


def accumulate_tiled(w, source=None, tile=TILE, inner=INNER, wake=8):
    """The kernel's schedule: (a, launches, tile runs).  `wake`: 8 or 4 neighbours wake a tile (4 is the seeded slip)."""
    src = _source(w, source)
    win = incoming(w)
    H, W = src.shape
    th, tw = -(-H // tile), -(-W // tile)
    a = _start(src)
    dirty = np.ones((th, tw), bool)
    launches = runs = 0
    first = True
    while dirty.any():
        launches += 1
        assert launches <= th * tw * (4 * tile + tile * tile // inner) + 2, "the launch bound"
        prev, old = dirty, a.copy()                                   # Jacobi across tiles: aprons from the launch before
        dirty = np.zeros_like(prev)
        for i in range(th):
            for j in range(tw):
                near = prev[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2]
                if wake == 4:
                    near = np.array([prev[x, y] for x, y in ((i, j), (i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1))
                                     if 0 <= x < th and 0 <= y < tw])
                if not (first or near.any()):
                    continue
                runs += 1
                r0, r1, c0, c1 = i * tile, min((i + 1) * tile, H), j * tile, min((j + 1) * tile, W)
                loc = old[r0:r1 + 2, c0:c1 + 2].copy()
                loc[1:-1, 1:-1] = a[r0 + 1:r1 + 1, c0 + 1:c1 + 1]
                s_loc, w_loc = src[r0:r1, c0:c1], win[:, r0:r1, c0:c1]
                moved = False
                for _ in range(inner):
                    new = _sweep(loc, s_loc, w_loc)
                    if (new.view(np.uint64) == np.ascontiguousarray(loc[1:-1, 1:-1]).view(np.uint64)).all():
                        break
                    loc[1:-1, 1:-1] = new
                    moved = True
                a[r0 + 1:r1 + 1, c0 + 1:c1 + 1] = loc[1:-1, 1:-1]
                dirty[i, j] = moved
        first = False
    return a[1:-1, 1:-1].copy(), launches, runs


def dense(w):
    """M = I - W^T as a dense fp64 matrix: M a = source."""
    K, H, W = w.shape
    n = H * W
    M = np.eye(n)
    idx = np.arange(n).reshape(H, W)
    for k in range(K):
        to = shifted(idx, k, -1)
        sel = (to >= 0) & (w[k] != 0)
        M[to[sel], idx[sel]] -= w[k][sel].astype(np.float64)
    return M


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what):
    """Every word equal (float32 or float64 by `want`)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = bits64 if want.dtype == np.float64 else bits32
    bad = view(got) != view(want)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d words differ, first at %s: %r vs %r" % (what, bad.sum(), bad.size, at,
                                                                                  got[at], want[at]))


# ---- inputs ------------------------------------------------------------------------------------------------------

def fractal(H, W, seed=7, amplitude=40.0):
    """A rough terrain without the oracle: octaves of smoothed noise on a tilt."""
    r = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    h = 0.15 * x + 0.1 * y
    for o in range(1, 6):
        n = 2 ** o + 1
        coarse = r.standard_normal((n, n))
        gx, gy = np.linspace(0, n - 1, H), np.linspace(0, n - 1, W)
        x0, y0 = np.minimum(gx.astype(int), n - 2), np.minimum(gy.astype(int), n - 2)
        fx, fy = (gx - x0)[:, None], (gy - y0)[None, :]
        c = (coarse[x0][:, y0] * (1 - fx) * (1 - fy) + coarse[x0 + 1][:, y0] * fx * (1 - fy) +
             coarse[x0][:, y0 + 1] * (1 - fx) * fy + coarse[x0 + 1][:, y0 + 1] * fx * fy)
        h = h + amplitude * 0.5 ** o * c
    return np.ascontiguousarray(h, np.float32)


def ramp(H, W):
    """h = -x: on D4 every cell has one lower neighbour, the row below."""
    return np.ascontiguousarray(np.repeat(-np.arange(H, dtype=np.float32)[:, None], W, axis=1))


def snake(H, W):
    """A D4 serpentine through every cell of a level (H, W) grid, routed by `dist` alone (the flats rule takes the one
    neighbour whose dist is one less): (h, dist, position), position the 1-based place along the way, which is the
    accumulation of a unit source there.  The last cell has dist 0 and is the terminal."""
    pos = np.empty((H, W), np.int64)
    for i in range(H):
        cols = np.arange(W) if i % 2 == 0 else np.arange(W - 1, -1, -1)
        pos[i, cols] = i * W + np.arange(W) + 1
    return np.zeros((H, W), np.float32), (H * W - pos).astype(np.int32), pos


def staircase(n, H=None, W=None):
    """A D8 diagonal staircase on a level grid, routed by `dist`: cell (t, t) has dist n - t, every other cell 0 (a
    terminal).  (h, dist): a[t, t] = t + 1 with a unit source; the last step, dist 1, hands its n to the first table
    neighbour with dist 0, the cell above it."""
    H, W = H or n, W or n
    dist = np.zeros((H, W), np.int32)
    dist[np.arange(n), np.arange(n)] = n - np.arange(n)
    return np.zeros((H, W), np.float32), dist


def corner_chain():
    """A way on a level 129 x 129 grid, routed by `dist`: a serpentine through every cell of the first tile that ends in
    its corner (63, 63), then down the diagonal through (64, 64) to (128, 128).  The source is 1 on the way's first cell
    and 0 elsewhere: a pulse that needs sixteen launches to cross the first tile.  Nothing else moves meanwhile, so the
    diagonal tile is quiet when the pulse arrives, and only the mark of its diagonal neighbour wakes it.
    (h, dist, source, want): want is 1 on the way and on the cell above its last one (the first table neighbour with
    dist 0), 0 elsewhere."""
    n = 129
    pos = np.zeros((n, n), np.int64)
    for i in range(64):
        cols = np.arange(63, -1, -1) if i % 2 == 0 else np.arange(64)
        pos[i, cols] = i * 64 + np.arange(64) + 1
    pos[np.arange(64, n), np.arange(64, n)] = 4096 + 1 + np.arange(n - 64)
    length = 4096 + n - 64
    dist = np.where(pos > 0, length + 1 - pos, 0).astype(np.int32)
    want = (pos > 0).astype(np.float64)
    want[n - 2, n - 1] = 1.0
    return np.zeros((n, n), np.float32), dist, (pos == 1).astype(np.float32), want


def hostile(H, W, seed=5):
    """A fractal with NaN cells, +-0 plateaus, +-inf and huge heights on tile seams and corners."""
    h = fractal(H, W, seed)
    r = np.random.default_rng(seed)
    spots = [(0, 0), (H - 1, W - 1), (min(63, H - 1), min(63, W - 1)), (min(64, H - 1), min(64, W - 1)),
             (min(63, H - 1), min(64, W - 1)), (H // 2, W // 2), (H // 3, min(65, W - 1))]
    vals = [np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0]
    for (x, y), v in zip(spots, vals):
        h[x, y] = v
    for _ in range(max(3, H * W // 200)):
        x, y = r.integers(H), r.integers(W)
        h[x, y] = vals[r.integers(len(vals))]
    if H > 8 and W > 8:
        h[H // 4:H // 4 + 3, W // 4:W // 4 + 3] = 0.0
        h[H // 4 + 1, W // 4 + 1] = -0.0
    return h


def hostile_source(H, W, seed=6):
    s = np.random.default_rng(seed).random((H, W)).astype(np.float32)
    for (x, y), v in zip([(0, 0), (H // 2, W // 3), (H - 1, 0), (H // 3, W // 2), (H // 5, W // 5)],
                         [np.nan, np.inf, -np.inf, -0.0, 0.0]):
        s[x, y] = v
    return s
