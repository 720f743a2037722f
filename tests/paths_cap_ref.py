"""Closed-form references for the pointer-doubling engine (csrc/flow_paths.hpp) at sizes the numpy restatements of
tests/flow_paths_ref.py and tests/downstream_ref.py cannot afford, and a restatement of the engine's scratch layout.
Not a test module.  tests/test_paths_above_cap.py holds every answer here to the restatement it replaces.

Three graphs whose cells lie on chains, a cell's place on its chain known in closed form; no Python loop over cells:

  serpentine  ref.serpentine's chain through every cell: position p = x W + (y on an even row, W - 1 - y on an odd one)
  comb        every cell drains to its left neighbour, column 0 is terminal: a chain per row, position W - 1 - y
  staircase   (x, y) -> (x + 1, y + 1) while inside the grid: a chain per diagonal, position min(x, y); diagonal
              steps are edges under D8 alone, so under D4 every cell is its own terminal

A walk ends on the next end along its chain — a cell without an edge, or one with stop != 0 — found by `searchsorted`
on the sorted ends; the steps of each kind are differences of running counts along the chain.  Without a stop plane
that is steps = H W - 1 - p, n_row = H - 1 - x on the serpentine, steps = y, terminal = x W on the comb and
steps = min(H - 1 - x, W - 1 - y) on the staircase (test_paths_above_cap.py asserts these too).

The downstream sums x[n] = a L + b x[r(n)] on these graphs with a in {0, 1, 2, 3}, small integer terminals, b absent
or in {0, 1} and a scale whose three lengths are multiples of one unit: every partial sum, in any order of
association, is a multiple of that unit far below 2^53 units, so exact in fp64, and the result is a suffix sum along
the chain, cut where b == 0: np.cumsum in float64.  `exact` is the condition itself."""
import numpy as np

import downstream_ref as dref
import flow_paths_ref as ref
from flow_paths_ref import COL, D4, D8, DIAG, ROW  # noqa: F401

NAMES = ("serpentine", "comb", "staircase")


def graph_of(name, H, W):
    """(graph, chain, position, kind of the cell's step) of a built graph, flat int64 / int8 planes but the graph."""
    N = H * W
    n = np.arange(N, dtype=np.int64)
    x, y = n // W, n % W
    if name == "serpentine":
        even = x % 2 == 0
        turn = np.where(even, y == W - 1, y == 0)                 # the row's last cell: a row step, or the chain's end
        g = np.where(turn, np.where(x < H - 1, n + W, -1), np.where(even, n + 1, n - 1))
        chain, pos = np.zeros(N, np.int64), x * W + np.where(even, y, W - 1 - y)
        kind = np.where(turn, ROW, COL)
    elif name == "comb":
        g = np.where(y > 0, n - 1, -1)
        chain, pos, kind = x, W - 1 - y, np.full(N, COL)
    elif name == "staircase":
        g = np.where((x < H - 1) & (y < W - 1), n + W + 1, -1)
        chain, pos, kind = y - x + (H - 1), np.minimum(x, y), np.full(N, DIAG)
    else:
        raise KeyError(name)
    return g.astype(np.int32).reshape(H, W), chain, pos, kind.astype(np.int8)


class Chains:
    """A built graph with its cells in the order of their walks: chain by chain, downstream."""

    def __init__(self, name, H, W, edge):
        self.name, self.H, self.W, self.edge = name, H, W, edge
        self.graph, chain, pos, self.kind = graph_of(name, H, W)
        self.graph.setflags(write=False)
        self.has_edge = (self.graph.reshape(-1) >= 0) & ((edge == D8) | (self.kind != DIAG))
        if name == "serpentine":                                  # one chain: the order is the inverse of `pos`
            self.order = np.empty(H * W, np.int64)
            self.order[pos] = np.arange(H * W, dtype=np.int64)
        else:
            self.order = np.argsort(chain * np.int64(H * W) + pos, kind="stable")

    def _next(self, is_break):
        """For every cell in chain order, the index (in that order) of the first break at or after it.  The last cell
        of a chain is a break: the search never leaves the chain."""
        at = np.flatnonzero(is_break[self.order])
        return at[np.searchsorted(at, np.arange(self.order.size, dtype=np.int64), side="left")]

    def _ends(self, stop):
        is_end = ~self.has_edge
        if stop is not None:
            is_end = is_end | (np.asarray(stop).reshape(-1) != 0)
        return is_end

    def walk(self, scale=None, stop=None):
        """(terminal, steps, length) as ref.walk_doubling returns them."""
        N, order = self.order.size, self.order
        i = np.arange(N, dtype=np.int64)
        m = self._next(self._ends(stop))
        shape = (self.H, self.W)

        def back(sorted_plane, dtype):
            out = np.empty(N, dtype)
            out[order] = sorted_plane
            return out.reshape(shape)

        terminal, steps = back(order[m], np.int32), back(m - i, np.int32)
        if scale is None:
            return terminal, steps, None
        counts = []
        for k in (ROW, COL, DIAG):                                # the cells i .. m - 1 of a walk all step
            run = np.concatenate(([0], np.cumsum(self.kind[order] == k, dtype=np.int64)))
            counts.append(back(run[m] - run[i], np.int64))
        return terminal, steps, ref.lengths(*counts, scale).reshape(shape)

    def weights(self, a, t, scale, stop=None):
        """What a cell adds to the sums that pass it, fp64: a L on a cell that steps, t on an end (None: 1, 0)."""
        N = self.order.size
        sx, sy, dd = dref.path_scale(scale)
        L = np.where(self.kind == ROW, sx, np.where(self.kind == COL, sy, dd))
        a64 = np.ones(N) if a is None else np.asarray(a, np.float32).reshape(-1).astype(np.float64)
        t64 = np.zeros(N) if t is None else np.asarray(t, np.float32).reshape(-1).astype(np.float64)
        return np.where(self._ends(stop), t64, a64 * L)

    def sums(self, a=None, b=None, t=None, scale=None, stop=None):
        """(out, out64) of soil_downstream where `exact` holds: the sum of the weights from the cell to the first
        cell with b == 0 (it adds its a L and nothing of what lies below) or to the end, both included."""
        order = self.order
        w = self.weights(a, t, scale, stop)[order]
        is_break = self._ends(stop)
        if b is not None:
            is_break = is_break | (np.asarray(b).reshape(-1) == 0)
        m = self._next(is_break)
        run = np.cumsum(w)
        out64 = np.empty(order.size, np.float64)
        out64[order] = run[m] - (run - w)
        out64 = out64.reshape(self.H, self.W)
        return out64.astype(np.float32), out64


def exact(weights, unit):
    """The exactness condition of `sums`: every weight a multiple of `unit`, and the sum of their magnitudes — a bound
    on every partial sum in any order of association — below 2^53 units."""
    q = np.asarray(weights, np.float64) / unit
    return bool((q == np.rint(q)).all() and np.abs(q).sum() < 2.0 ** 53)


def exact_planes(H, W, seed, cut=0.02):
    """a in {0, 1, 2, 3}, b in {0, 1} (a share `cut` of zeros) and t in {0 .. 7}, float32 planes."""
    r = np.random.default_rng([seed, H, W])
    a = r.integers(0, 4, (H, W)).astype(np.float32)
    b = (r.random((H, W)) >= cut).astype(np.float32)
    t = r.integers(0, 8, (H, W)).astype(np.float32)
    return a, b, t


def stop_plane(H, W, seed, share):
    """A share `share` of pour points, with values other than 1 among them."""
    r = np.random.default_rng([seed, H, W, 77])
    return ((r.random((H, W)) < share) * r.integers(1, 9, (H, W))).astype(np.int32)


# ---- the engine's scratch, restated (csrc/flow_paths.hpp ptr_layout; csrc/downstream.hip deposit_run) ------------

CAP = 8192                                                        # work-groups of a round, unless SOIL_PATHS_GROUPS


def _align256(b):
    return (b + 255) // 256 * 256


def layout(elem, extra, cap=CAP):
    """groups, seg (entries of a work-group's list segment) and the bytes of a chunk of `elem` cells with `extra`
    bytes a cell of coefficient planes."""
    groups = min((elem + 255) // 256, cap)
    seg = ((elem + groups - 1) // groups + 255) // 256 * 256
    b_rec, b_extra = _align256(16 * elem), _align256(extra * elem)
    b_list, b_fill = _align256(4 * seg * groups), _align256(4 * groups)
    return dict(groups=groups, seg=seg, bytes=2 * b_rec + 2 * b_extra + 2 * b_list + 2 * b_fill + 256)


def deposit_bytes(cells, B, per_model_scales, cap=CAP):
    """`scratch_bytes` of a soil_stream_power_deposit call of one chunk of `cells` cells that accumulates nothing
    (iters == 1, no flux): the iterate, q and Qs, the scale records of B models, the engine's chunk with its B planes."""
    b_scales = _align256(24 * B) if per_model_scales else 0
    return _align256(8 * cells) + 2 * _align256(4 * cells) + b_scales + layout(cells, 8, cap)["bytes"]


def above(elem, cap=CAP):
    """Whether a round of a chunk of `elem` cells strides: more blocks of 256 cells than work-groups."""
    return (elem + 255) // 256 > cap


def ceil_log2(v):
    return len(bin(v - 1)) - 2 if v > 1 else 0
