"""Upstream extrema along a receiver graph (include/soil_hip.h: "flow graphs: upstream extrema"; soil_upstream_extreme,
soil_upstream_extreme_batch), restated in numpy and plain Python from the DEFINITION — who reaches whom, the integer
key order, the smallest index among equals — not from the rounds of csrc/upstream.hip.  Not a test module.

  extreme        a sweep in Kahn order (a cell is done when all its donors are) over the cells off cycles, then, for
                 the cells that are left — they lie on cycles, each with one receiver and one donor among them — the
                 least word round the cycle, given to every cell of it
  brute          reachability itself: every cell's walk, cell by cell, for small grids
  chain_extreme  the closed form on paths_cap_ref's serpentine: a running minimum along the chain, no loop over cells

A cell's word is (key << 32) | index; every comparison is of such words, as unsigned integers."""
import numpy as np

import flow_paths_ref as ref
import paths_cap_ref as cap
from flow_paths_ref import D4, D8  # noqa: F401

MIN, MAX = 0, 1
NAN_WORD = np.uint32(0x7FC00000)
NAN_KEY = np.uint32(0xFFC00000)
SIGN = np.uint32(0x80000000)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def key_of(u):
    """csrc/erosion_quantiles.hip key_of on bit patterns: -inf < .. < -0 < +0 < .. < +inf < NaN, every NaN one key."""
    u = np.asarray(u, np.uint32).copy()
    u[(u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = NAN_WORD
    return np.where(u >> np.uint32(31) != 0, ~u, u | SIGN).astype(np.uint32)


def bits_of(key):
    key = np.asarray(key, np.uint32)
    return np.where(key >> np.uint32(31) != 0, key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)


def words(value, op):
    """The packed word of every cell of a (H, W) plane, flat uint64: the key of the value (negated for max) above the
    cell's index."""
    u = bits(value).reshape(-1)
    if op == MAX:
        u = u ^ SIGN
    return (key_of(u).astype(np.uint64) << np.uint64(32)) | np.arange(u.size, dtype=np.uint64)


def unpack(m, op, shape):
    """(out, arg) from the least word of every cell."""
    key = (m >> np.uint64(32)).astype(np.uint32)
    nan = key == NAN_KEY
    out = bits_of(key)
    if op == MAX:
        out = out ^ SIGN
    out = np.where(nan, NAN_WORD, out).astype(np.uint32).view(np.float32)
    arg = np.where(nan, -1, (m & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    return out.reshape(shape), arg.reshape(shape)


def receivers(graph, edge, stop=None):
    """The receiver of every cell under soil_flow_paths' edge rule, flat int64, -1 for a cell without an edge."""
    graph = np.asarray(graph)
    H, W = graph.shape
    N = H * W
    g = graph.reshape(-1).astype(np.int64)
    n = np.arange(N, dtype=np.int64)
    inside = (g >= 0) & (g < N)
    r = np.where(inside, g, 0)
    dx, dy = r // W - n // W, r % W - n % W
    ok = inside & (np.abs(dx) <= 1) & (np.abs(dy) <= 1) & ((dx != 0) | (dy != 0))
    if edge == D4:
        ok &= (dx == 0) | (dy == 0)
    if stop is not None:
        ok &= np.asarray(stop).reshape(-1) == 0
    return np.where(ok, g, -1)


def extreme(graph, value, edge, op=MIN, stop=None):
    """(out, arg) of soil_upstream_extreme."""
    shape = np.asarray(graph).shape
    r = receivers(graph, edge, stop).tolist()
    N = len(r)
    m = words(value, op).tolist()
    waiting = [0] * N
    for q in r:
        if q >= 0:
            waiting[q] += 1
    ready = [n for n in range(N) if waiting[n] == 0]
    done = 0
    while ready:
        n = ready.pop()
        done += 1
        q = r[n]
        if q >= 0:
            if m[n] < m[q]:
                m[q] = m[n]
            waiting[q] -= 1
            if waiting[q] == 0:
                ready.append(q)
    if done < N:                                                  # what is left lies on cycles
        seen = [False] * N
        for n in range(N):
            if waiting[n] > 0 and not seen[n]:
                ring, q = [], n
                while not seen[q]:
                    seen[q] = True
                    ring.append(q)
                    q = r[q]
                assert q == n and all(waiting[c] == 1 for c in ring)
                least = min(m[c] for c in ring)
                for c in ring:
                    m[c] = least
    return unpack(np.array(m, np.uint64), op, shape)


def brute(graph, value, edge, op=MIN, stop=None):
    """The definition as it stands: out[n] = the least word of all u whose walk passes n.  Small grids only."""
    shape = np.asarray(graph).shape
    r = receivers(graph, edge, stop).tolist()
    N = len(r)
    w = words(value, op).tolist()
    m = list(w)
    for u in range(N):
        seen, q = set(), u
        while q >= 0 and q not in seen:
            seen.add(q)
            if w[u] < m[q]:
                m[q] = w[u]
            q = r[q]
    return unpack(np.array(m, np.uint64), op, shape)


def extreme_batch(graph, value, edge, op=MIN, stop=None):
    outs = [extreme(graph[b], value[b], edge, op, None if stop is None else stop[b]) for b in range(len(graph))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def chain_extreme(H, W, value, op=MIN):
    """(graph, out, arg) on the serpentine of paths_cap_ref: the cells in chain order, a running minimum of the words."""
    c = cap.Chains("serpentine", H, W, D8)
    m = np.empty(H * W, np.uint64)
    m[c.order] = np.minimum.accumulate(words(value, op)[c.order])
    return (c.graph,) + unpack(m, op, (H, W))


# ---- graphs ----------------------------------------------------------------------------------------------------

def funnel(H, W):
    """Every row drains to column 0 and column 0 up to cell 0: no way is longer than H + W - 2 edges, so in the late
    rounds of a pointer-doubling scheme every cell points straight at cell 0."""
    n = np.arange(H * W, dtype=np.int64).reshape(H, W)
    g = n - 1
    g[:, 0] = n[:, 0] - W
    g[0, 0] = -1
    return g.astype(np.int32)


def ring(H, W):
    """A cycle round the border, 2 (H + W) - 4 cells long, with every inner row draining into it as tributaries."""
    assert H >= 3 and W >= 3
    n = np.arange(H * W, dtype=np.int64).reshape(H, W)
    g = n - 1                                                     # inner cells: to the left, onto column 0
    g[0, :] = n[0, :] + 1                                         # top row to the right
    g[:, W - 1] = n[:, W - 1] + W                                 # right column down
    g[H - 1, :] = n[H - 1, :] - 1                                 # bottom row to the left
    g[:, 0] = n[:, 0] - W                                         # left column up
    g[0, 0], g[0, W - 1], g[H - 1, W - 1], g[H - 1, 0] = 1, 2 * W - 1, H * W - 2, (H - 2) * W
    return g.astype(np.int32)


def graphs(H, W, edge):
    """name -> graph of every kind a (H, W) grid takes."""
    out = dict(serpentine=ref.serpentine(H, W), all_donors=ref.all_donors(H, W, edge), hostile=ref.hostile(H, W, 3),
               comb=cap.graph_of("comb", H, W)[0], funnel=funnel(H, W))
    if H >= 4 and W >= 3:
        out["cycles"] = ref.cycles(H, W)
    if H >= 3 and W >= 3:
        out["ring"] = ring(H, W)
    if H * W > 1:
        out["descent"] = ref.descent(ref.terrain(H, W, 2, True), edge)
    return {k: np.ascontiguousarray(v, np.int32) for k, v in out.items()}


# ---- values ----------------------------------------------------------------------------------------------------

VALUES = ("random", "plateau", "zeros", "denormal", "inf", "nan_third", "all_nan")


def values(H, W, kind, seed=0):
    """A float32 plane of the given kind; the bit patterns are what counts."""
    r = np.random.default_rng([seed, H, W, VALUES.index(kind)])
    N = H * W
    if kind == "random":
        v = ((r.random(N) - 0.5) * 200.0).astype(np.float32)
    elif kind == "plateau":                                       # equal values everywhere but a few lower spots
        v = np.full(N, 2.5, np.float32)
        v[r.integers(0, N, max(1, N // 97))] = -1.0
    elif kind == "zeros":                                         # +0 and -0 side by side, a few numbers around them
        u = np.where(r.random(N) < 0.5, SIGN, np.uint32(0))
        v = u.astype(np.uint32).view(np.float32).copy()
        at = r.integers(0, N, N // 9)
        v[at] = r.choice(np.array([1.0, -1.0], np.float32), at.size)
    elif kind == "denormal":
        u = r.integers(1, 1 << 23, N).astype(np.uint32) | np.where(r.random(N) < 0.5, SIGN, np.uint32(0))
        v = u.astype(np.uint32).view(np.float32).copy()
        v[r.integers(0, N, N // 5)] = 0.0
    elif kind == "inf":
        v = r.choice(np.array([np.inf, -np.inf, 0.0, 3.0, -3.0, 3.4e38, -3.4e38], np.float32), N, p=[.3, .1, .1, .2, .1, .1, .1])
    elif kind == "nan_third":                                     # NaNs of either sign with payloads, quiet and signalling
        v = ((r.random(N) - 0.5) * 8.0).astype(np.float32)
        u = v.view(np.uint32).copy()
        at = r.random(N) < 1.0 / 3.0
        nan = np.uint32(0x7F800000) | r.integers(1, 1 << 23, N).astype(np.uint32) | np.where(r.random(N) < 0.5, SIGN, np.uint32(0))
        u[at] = nan.astype(np.uint32)[at]
        v = u.view(np.float32)
    elif kind == "all_nan":
        u = np.uint32(0x7F800000) | r.integers(1, 1 << 23, N).astype(np.uint32) | np.where(r.random(N) < 0.5, SIGN, np.uint32(0))
        v = u.astype(np.uint32).view(np.float32)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(v, np.float32).reshape(H, W).copy()


def stop_plane(H, W, seed=0):
    r = np.random.default_rng([seed, H, W, 99])
    return ((r.random((H, W)) < 0.08) * r.integers(1, 9, (H, W))).astype(np.int32)


def same(got, want, what):
    """(out, arg) of the device against the reference's, word for word; None: not asked for."""
    for g, w, name in zip(got, want, ("out", "arg")):
        if g is None:
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.flatnonzero(g.view(np.uint32).reshape(-1) != w.view(np.uint32).reshape(-1))
        assert bad.size == 0, "%s: %s differs in %d cells, first %d: %#x, want %#x" % (
            what, name, bad.size, bad[0], g.view(np.uint32).reshape(-1)[bad[0]], w.view(np.uint32).reshape(-1)[bad[0]])


# ---- the four properties of a breached surface -----------------------------------------------------------------

def key_plane(a):
    return key_of(bits(a)).reshape(np.asarray(a).shape)


def check_breached(height, breached, graph, edge):
    """breached <= height in key order, and breached[r(n)] <= breached[n] along every edge."""
    kb, kh = key_plane(breached).reshape(-1), key_plane(height).reshape(-1)
    assert (kb <= kh).all(), "the breached surface stands above the DEM somewhere"
    r = receivers(graph, edge)
    has = r >= 0
    assert (kb[r[has]] <= kb[has]).all(), "the breached surface rises along an edge"
