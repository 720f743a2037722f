"""Stream order and channel segments on a receiver graph (include/soil_hip.h: "flow graphs: stream order";
soil_stream_order, soil_stream_order_batch), restated in numpy and plain Python from the DEFINITION — channel cells, the
channel graph, the level sets M_k — not from the passes of csrc/stream_order.hip.  Not a test module.

  by_levels   the definition as it stands: M_1 the channel cells, J_k the cells with two donors in M_k, M_{k+1} by
              repeated receiver steps from J_k; cycles allowed
  by_walk     the forest rule in Kahn order: a head 1, else the greatest order among the donors, plus one where two or
              more share it; acyclic channel graphs only (it asserts that)
  segments    flow_paths_ref's serial walk down channel_graph with a foot plane as `stop`
  magnitude   the heads summed down channel_graph in Kahn order (float32, exact: small integers)
  dyadic      a binary tree of order m + 1 on (m + 1) x 2^m with its closed form, no loop over cells

and the built cases of tests/test_stream_order_abi.py and tests/test_gpu_stream_order.py."""
import numpy as np

import flow_paths_ref as fref
from flow_paths_ref import D4, D8  # noqa: F401
from upstream_ref import receivers

OUTPUTS = ("order", "donors", "link_foot", "order_foot", "channel_graph")


# ---- the definition --------------------------------------------------------------------------------------------

def channel_cells(shape, channel=None, area=None, threshold=None):
    """Which cells are channel cells, flat bool."""
    ok = np.ones(int(np.prod(shape)), bool)
    if channel is not None:
        ok &= np.asarray(channel).reshape(-1) != 0
    if area is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(area, np.float32).reshape(-1) >= np.float32(threshold)   # a NaN area fails
    return ok


def channel_receivers(graph, edge, channel=None, area=None, threshold=None, stop=None):
    """(r, chan): the receiver of every cell along the CHANNEL graph, flat int64, -1 without an edge."""
    chan = channel_cells(np.asarray(graph).shape, channel, area, threshold)
    r = receivers(graph, edge, stop)
    has = r >= 0
    ok = has & chan & chan[np.where(has, r, 0)]
    return np.where(ok, r, -1), chan


def _planes(r, chan, order, shape):
    """Every output plane from the channel graph and the order."""
    N = r.size
    has = r >= 0
    donors = np.bincount(r[has], minlength=N)
    rr = np.where(has, r, 0)
    link_foot = chan & (~has | (donors[rr] >= 2))
    order_foot = chan & (~has | (order[rr] > order))
    out = dict(order=order, donors=donors, link_foot=link_foot, order_foot=order_foot, channel_graph=r)
    out = {k: np.ascontiguousarray(v.astype(np.int32).reshape(shape)) for k, v in out.items()}
    out["levels"] = max(1, int(order.max()))
    return out


def by_levels(graph, edge, channel=None, area=None, threshold=None, stop=None):
    """dict of the five planes and `levels`, by the level sets."""
    shape = np.asarray(graph).shape
    r, chan = channel_receivers(graph, edge, channel, area, threshold, stop)
    N = r.size
    has = r >= 0
    src, dst = np.flatnonzero(has), r[has]
    order = chan.astype(np.int64)
    M = chan.copy()                                                # M_k
    k = 1
    while True:
        J = chan & (np.bincount(dst[M[src]], minlength=N) >= 2)      # two donors in M_k
        if not J.any():
            break
        nxt = np.zeros(N, bool)                                    # M_{k+1}: what J reaches, by receiver steps
        cur = np.flatnonzero(J)
        nxt[cur] = True
        while cur.size:
            q = r[cur]
            q = q[q >= 0]
            q = np.unique(q[~nxt[q]])
            nxt[q] = True
            cur = q
        k += 1
        order[nxt] = k
        M = nxt
        assert k <= N.bit_length() + 1
    return _planes(r, chan, order, shape)


def by_walk(graph, edge, channel=None, area=None, threshold=None, stop=None):
    """The same dict by the forest rule; the channel graph must be acyclic."""
    shape = np.asarray(graph).shape
    r_np, chan = channel_receivers(graph, edge, channel, area, threshold, stop)
    r = r_np.tolist()
    N = len(r)
    waiting = [0] * N
    for q in r:
        if q >= 0:
            waiting[q] += 1
    top, shared = [0] * N, [0] * N                                 # the greatest donor order, and how many hold it
    order = [0] * N
    ready = [n for n in range(N) if waiting[n] == 0]
    done = 0
    while ready:
        n = ready.pop()
        done += 1
        if chan[n]:
            order[n] = 1 if top[n] == 0 else top[n] + (1 if shared[n] >= 2 else 0)
        q = r[n]
        if q >= 0:
            if order[n] > top[q]:
                top[q], shared[q] = order[n], 1
            elif order[n] == top[q]:
                shared[q] += 1
            waiting[q] -= 1
            if waiting[q] == 0:
                ready.append(q)
    assert done == N, "by_walk: the channel graph has a cycle"
    return _planes(r_np, chan, np.array(order, np.int64), shape)


def is_acyclic(graph, edge, channel=None, area=None, threshold=None, stop=None):
    r, _ = channel_receivers(graph, edge, channel, area, threshold, stop)
    N = r.size
    waiting = np.bincount(r[r >= 0], minlength=N)
    ready = np.flatnonzero(waiting == 0)
    done = 0
    while ready.size:
        done += ready.size
        q = r[ready]
        q = q[q >= 0]
        np.subtract.at(waiting, q, 1)
        q = np.unique(q)
        ready = q[waiting[q] == 0]
    return done == N


def batch(fn, graph, edge, channel=None, area=None, threshold=None, stop=None):
    """`fn` model by model, stacked; `levels` is the most over the models."""
    pick = lambda a, b: None if a is None else a[b]                 # noqa: E731
    outs = [fn(graph[b], edge, pick(channel, b), pick(area, b), threshold, pick(stop, b)) for b in range(len(graph))]
    out = {k: np.stack([o[k] for o in outs]) for k in OUTPUTS}
    out["levels"] = max(o["levels"] for o in outs)
    return out


def segments(planes, edge, scale=None, by="link"):
    """(order, segment, steps, length) of soil.stream_segments from the planes of by_levels."""
    seg, steps, length = fref.walk_serial(planes["channel_graph"], edge, scale, planes[by + "_foot"])
    return planes["order"], seg, steps, length


def magnitude(planes):
    """The Shreve magnitude: heads summed down channel_graph (acyclic), float32."""
    shape = planes["order"].shape
    r = planes["channel_graph"].reshape(-1).astype(np.int64).tolist()
    N = len(r)
    m = ((planes["order"].reshape(-1) > 0) & (planes["donors"].reshape(-1) == 0)).astype(np.int64).tolist()
    waiting = planes["donors"].reshape(-1).tolist()
    ready = [n for n in range(N) if waiting[n] == 0]
    done = 0
    while ready:
        n = ready.pop()
        done += 1
        q = r[n]
        if q >= 0:
            m[q] += m[n]
            waiting[q] -= 1
            if waiting[q] == 0:
                ready.append(q)
    assert done == N
    return np.array(m, np.float32).reshape(shape)


# ---- built graphs ----------------------------------------------------------------------------------------------

def dyadic(m):
    """(graph, order, donors) of the binary tree on (m + 1) x 2^m: row 0 all heads flowing down; in row j >= 1 the
    survivors are the columns that are multiples of 2^(j-1), the odd one runs left along the row to the even one, which
    flows down; the other cells have no edge.  order and donors are the closed form: row 0 has order 1, an odd
    survivor and its path cells in row j have j, an even survivor j + 1, an off-tree cell 1 with no donor."""
    H, W = m + 1, 1 << m
    x, c = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    n = x * W + c
    full, half = np.int64(1) << x, np.int64(1) << np.maximum(x - 1, 0)
    mod = c % full
    head = x == 0
    even = ~head & (mod == 0)
    path = ~head & (mod > 0) & (mod <= half)                       # the odd survivor (mod == half) and the way left
    g = np.where(head | even, n + W, np.where(path, n - 1, -1))
    g[H - 1, 0] = -1                                               # the outlet
    order = np.where(head, 1, np.where(even, x + 1, np.where(path, x, 1)))
    donors = np.where(head, 0, np.where(even, 2, np.where(path, 1, 0)))
    return g.astype(np.int32), order.astype(np.int32), donors.astype(np.int32)


def comb(H, W):
    """Every row drains left into column 0, column 0 down to the last row: order 2 along the spine from row 1 on
    (H, W >= 2)."""
    n = np.arange(H * W, dtype=np.int64).reshape(H, W)
    g = n - 1
    g[:, 0] = n[:, 0] + W
    g[H - 1, 0] = -1
    return g.astype(np.int32)


_ARROWS = {">": (0, 1), "<": (0, -1), "v": (1, 0), "^": (-1, 0)}


def drawn(rows, H=None, W=None):
    """A graph from a drawing: > < v ^ an edge to that neighbour, anything else none; padded with no-edge cells to
    (H, W)."""
    h, w = len(rows), max(len(r) for r in rows)
    H, W = H or h, W or w
    assert H >= h and W >= w
    g = np.full((H, W), -1, np.int64)
    for x, row in enumerate(rows):
        for y, ch in enumerate(row):
            if ch in _ARROWS:
                dx, dy = _ARROWS[ch]
                g[x, y] = (x + dx) * W + (y + dy)
    return g.astype(np.int32)


# Junctions with donors of mixed orders, straight edges only (the same graph under D4 and D8).  (row, column): order
#   (2, 3): donors W 2, E 2, N 1      -> 3          (4, 3): donors N 3, W 2, E 2 -> 3
#   (2, 10): donors W 2, N 1, E 1     -> 2          (3, 3), (5, 3), (6, 3): a single donor of order 3 -> 3
MIXED = [".............",
         "..vvv....vv..",
         ".>>v<<..>>v<.",
         "...v......o..",
         ".>>v<<.......",
         "..^v^........",
         "...o........."]
MIXED_ORDERS = {(2, 2): 2, (2, 4): 2, (1, 3): 1, (2, 3): 3, (3, 3): 3, (4, 2): 2, (4, 4): 2, (4, 3): 3, (5, 3): 3,
                (6, 3): 3, (2, 9): 2, (1, 10): 1, (2, 11): 1, (2, 10): 2, (3, 10): 2, (0, 0): 1}
MIXED_DONORS = {(2, 3): 3, (4, 3): 3, (2, 10): 3, (3, 3): 1, (6, 3): 1, (2, 2): 2, (1, 3): 0, (0, 0): 0}


def mixed(H=7, W=13):
    return drawn(MIXED, H, W)


def area_plane(H, W, seed=0):
    """A float32 "area": numbers around the threshold 4.0 with NaN (both signs, payloads), +inf and -inf among them."""
    r = np.random.default_rng([seed, H, W, 41])
    a = (r.random(H * W) * 8.0).astype(np.float32)
    u = a.view(np.uint32).copy()
    kind = r.integers(0, 12, H * W)
    u[kind == 0] = (np.uint32(0x7F800000) | r.integers(1, 1 << 23, H * W).astype(np.uint32))[kind == 0]
    u[kind == 1] = 0xFFC00001
    u[kind == 2] = 0x7F800000
    u[kind == 3] = 0xFF800000
    u[kind == 4] = np.float32(4.0).view(np.uint32)                 # the threshold itself: a channel cell
    return u.view(np.float32).reshape(H, W).copy()


def holes(H, W):
    """A channel mask with a column of holes (and any non-zero value a mark): a stream that runs along a row leaves
    the channels and re-enters them."""
    m = np.arange(1, H * W + 1, dtype=np.int64).reshape(H, W) % 7 + 1
    m[:, W // 2] = 0
    m[H // 2, :: 3] = 0
    m[:, 0] = -5
    return m.astype(np.int32)


def junction_stop(graph, edge):
    """A stop plane with a mark on one donor of every second junction of the plain graph."""
    r = receivers(graph, edge)
    N = r.size
    donors = np.bincount(r[r >= 0], minlength=N)
    s = np.zeros(N, np.int32)
    first = {}
    for n in np.flatnonzero(r >= 0).tolist():
        first.setdefault(int(r[n]), n)
    for i, j in enumerate(np.flatnonzero(donors >= 2).tolist()):
        if i % 2 == 0:
            s[first[j]] = 3
    return s.reshape(np.asarray(graph).shape)


def noise_height(oracle, H, W):
    return np.ascontiguousarray(oracle.noise(H, W, seed=3.0, ext=(float(H), float(W))) * np.float32(100.0), np.float32)


def upstream_count(graph, edge):
    """The number of cells that drain through each cell, itself included (acyclic graphs), float32."""
    r = receivers(graph, edge)
    N = r.size
    a = np.ones(N, np.int64)
    waiting = np.bincount(r[r >= 0], minlength=N)
    ready = np.flatnonzero(waiting == 0)
    while ready.size:
        q = r[ready]
        ok = q >= 0
        np.add.at(a, q[ok], a[ready[ok]])
        np.subtract.at(waiting, q[ok], 1)
        u = np.unique(q[ok])
        ready = u[waiting[u] == 0]
    return a.astype(np.float32).reshape(np.asarray(graph).shape)


def cases(H, W, edge):
    """name -> dict(graph=, channel=, area=, threshold=, stop=) of every built case a (H, W) grid takes."""
    def case(graph, channel=None, area=None, threshold=None, stop=None):
        return dict(graph=np.ascontiguousarray(graph, np.int32), channel=channel, area=area, threshold=threshold,
                    stop=stop)
    out = dict(chain=case(fref.serpentine(H, W)), hostile=case(fref.hostile(H, W, 3)),
               all_donors=case(fref.all_donors(H, W, edge)), all_donors_d8=case(fref.all_donors(H, W, D8)))
    if H >= 2 and W >= 2:
        out["comb"] = case(comb(H, W))
        out["comb_holes"] = case(comb(H, W), channel=holes(H, W))
        out["comb_stop"] = case(comb(H, W), stop=junction_stop(comb(H, W), edge))
        # the chain with its head turned down into (1, 0), which the chain reaches after two rows: order 2 from there
        # to the foot, H W - 2 W edges on — at (12, 20), (67, 131) and (1027, 2051) more than half the cells, so only
        # the last of the ceil(log2(H W)) rounds of the closure brings the 2 to the foot
        g = fref.serpentine(H, W)
        g[0, 0] = W
        out["chain_join"] = case(g)
    if H >= 4 and W >= 3:
        out["cycles"] = case(fref.cycles(H, W))
        out["cycles_area"] = case(fref.cycles(H, W), area=area_plane(H, W, 1), threshold=4.0)
    if H >= 7 and W >= 13:
        g = mixed(H, W)
        out["mixed"] = case(g)
        s = np.zeros((H, W), np.int32)
        s[2, 2] = 1                                                # a donor of the junction (2, 3)
        out["mixed_stop"] = case(g, stop=s)
    if H * W > 1:
        g = fref.descent(fref.terrain(H, W, 2, True), edge)
        out["descent"] = case(g)
        out["descent_area"] = case(g, area=upstream_count(g, edge), threshold=3.0)
        out["descent_all"] = case(g, channel=holes(H, W), area=area_plane(H, W, 2), threshold=4.0,
                                  stop=junction_stop(g, edge))
        out["hostile_all"] = case(fref.hostile(H, W, 4), channel=holes(H, W), area=area_plane(H, W, 3), threshold=4.0,
                                  stop=fref.stop_planes(H, W)[1][1])
    return out


def same(got, want, what, levels=None):
    """The planes of the device (a dict; a missing or None plane: not asked for) against the reference's, word for
    word, and the level count."""
    for name in OUTPUTS:
        g = got.get(name)
        if g is None:
            continue
        g, w = np.ascontiguousarray(g), want[name]
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, "%s: %s differs in %d cells, first %d: %d, want %d" % (
            what, name, bad.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])
    if levels is not None:
        assert levels == want["levels"], "%s: %d levels run, want %d" % (what, levels, want["levels"])
