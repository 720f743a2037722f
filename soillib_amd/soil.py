"""Host-side mirror of the reference's `soillib` Python module for the erosion path.

Same names, argument order and meaning as the nanobind module
(python/source/model.cpp:23-60 param_t, :148-151 edge, :157-203 graph/stencil
ops returning new tensors, :209-227 solve_uniform, :237-407 in-place erosion /
albedo ops returning None, :413-421 noise_t / noise; python/source/util.cpp:47-73
timer).  Every op forwards to the C ABI (include/soil_hip.h); tensors are
`silt` tensors (soillib_amd.silt).  GPU ops given a CPU tensor raise, like
silt::error::mismatch_host in the reference (graph.cu:75-76).
"""
import contextlib
import ctypes as C
import math
import time

import numpy as np

from . import _abi, _check, silt
from ._check import valid_temperature  # noqa: F401 (soil.valid_temperature)

# ---------------------------------------------------------------- edge enum


class edge:
    """soil::edge_t, graph.hpp:11-14 / model.cpp:148-151."""
    d4 = _abi.D4
    d8 = _abi.D8


d4, d8 = edge.d4, edge.d8  # export_values()


# ------------------------------------------------------------------ param_t

class param_t:
    """soil::param_t (erosion.hpp:17-58), bound field by field at model.cpp:23-60."""

    _FIELDS = ("maxage",) + _abi._PARAM_FLOATS

    def __init__(self):
        object.__setattr__(self, "_c", _abi.Param())
        _abi.lib().soil_param_default(C.byref(self._c))

    def __getattr__(self, name):
        if name == "force":
            return [self._c.force[0], self._c.force[1]]
        if name in param_t._FIELDS:
            return getattr(self._c, name)
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name == "force":
            self._c.force[0], self._c.force[1] = float(value[0]), float(value[1])
        elif name == "maxage":
            self._c.maxage = int(value)
        elif name in param_t._FIELDS:
            setattr(self._c, name, float(value))
        else:
            raise AttributeError("param_t has no field %r" % name)

    def _ref(self):
        return C.byref(self._c)


# ------------------------------------------------------------------ helpers

def _gpu(t, dtype, what):
    if not isinstance(t, silt.tensor):
        raise TypeError("%s: expected a silt.tensor" % what)
    if t.host is not silt.gpu:
        raise _abi.SoilError("mismatch_host: %s must be a silt.gpu tensor" % what)
    if t.type is not dtype:
        raise TypeError("%s: expected %s, got %s" % (what, dtype.name, t.type.name))
    return t.c_ptr


def _f(t, what):
    return _gpu(t, silt.float32, what)


def _opt_f(t, what):
    return None if t is None else _gpu(t, silt.float32, what)


def _hw(t):
    s = t.shape
    return s[0], s[1]


def _call(name, *args):
    _abi.check(getattr(_abi.lib(), name)(*args))


# --------------------------------------------------------- graph / stencils

def direction(height, edge_):
    """model.cpp:157-159 -> soil::direction (graph.cu:246-264)."""
    H, W = _hw(height)
    out = silt.tensor(silt.int32, silt.shape(H, W), silt.gpu)
    _call("soil_direction", out.c_ptr, _f(height, "height"), H, W, edge_, _abi.stream())
    return out


def steepest(height, edge_):
    """model.cpp:169-171 -> soil::steepest (graph.cu:73-91)."""
    H, W = _hw(height)
    out = silt.tensor(silt.int32, silt.shape(H, W), silt.gpu)
    _call("soil_steepest", out.c_ptr, _f(height, "height"), H, W, edge_, _abi.stream())
    return out


def random_weighted(height, edge_, seed, offset, T):
    """model.cpp:173-175 -> soil::random_weighted (graph.cu:175-195).  T: see valid_temperature."""
    H, W = _hw(height)
    out = silt.tensor(silt.int32, silt.shape(H, W), silt.gpu)
    _call("soil_random_weighted", out.c_ptr, _f(height, "height"), H, W, edge_, int(seed),
          int(offset), float(T), _abi.stream())
    return out


def slope(tensor, flow, scale):
    """model.cpp:161-163 -> soil::slope (graph.cu:297-311)."""
    H, W = _hw(tensor)
    out = silt.tensor(silt.float32, silt.shape(H, W), silt.gpu)
    _call("soil_slope", out.c_ptr, _f(tensor, "tensor"), _gpu(flow, silt.int32, "flow"), H, W,
          _abi.vec(scale, 2), _abi.stream())
    return out


def accumulate(graph, field, edge_):
    """model.cpp:181-183 -> soil::accumulate (graph.cu:578-584)."""
    H, W = _hw(graph)
    out = silt.tensor(silt.float32, silt.shape(H, W), silt.gpu)
    _call("soil_accumulate", out.c_ptr, _gpu(graph, silt.int32, "graph"), _f(field, "field"), None,
          H, W, edge_, _abi.stream())
    return out


def accumulate_decay(graph, field, decay, edge_):
    """model.cpp:185-187 -> soil::accumulate_decay (graph.cu:586-593)."""
    H, W = _hw(graph)
    out = silt.tensor(silt.float32, silt.shape(H, W), silt.gpu)
    _call("soil_accumulate", out.c_ptr, _gpu(graph, silt.int32, "graph"), _f(field, "field"),
          _f(decay, "decay"), H, W, edge_, _abi.stream())
    return out


# ---- the same for B models of one (H, W) in one call (soil_hip.h: "flow graphs: batches of models"; not in the
# reference): (B, H, W) tensors, model b's slice bit for bit what the single-grid function gives for it alone; a
# graph entry is an index within its model.  Stream-ordered, nothing synchronises.

def _bhw(t, what):
    s = tuple(t.shape) if isinstance(t, silt.tensor) else ()
    if len(s) != 3:
        raise ValueError("%s: expected a (B, H, W) tensor, got shape %r" % (what, s))
    return s


def _same(t, shape, what):
    if not isinstance(t, silt.tensor) or tuple(t.shape) != tuple(shape):
        raise ValueError("%s: expected a tensor of shape %r, got %r" % (
            what, tuple(shape), tuple(t.shape) if isinstance(t, silt.tensor) else type(t).__name__))


def direction_batch(height, edge_):
    """soil_direction_batch: `direction` of each of the B models of a (B, H, W) height tensor."""
    B, H, W = _bhw(height, "direction_batch: height")
    ptr = _f(height, "height")
    out = silt.tensor(silt.int32, silt.shape(B, H, W), silt.gpu)
    _call("soil_direction_batch", out.c_ptr, ptr, B, H, W, edge_, _abi.stream())
    return out


def steepest_batch(height, edge_):
    """soil_steepest_batch: `steepest` of each of the B models of a (B, H, W) height tensor."""
    B, H, W = _bhw(height, "steepest_batch: height")
    ptr = _f(height, "height")
    out = silt.tensor(silt.int32, silt.shape(B, H, W), silt.gpu)
    _call("soil_steepest_batch", out.c_ptr, ptr, B, H, W, edge_, _abi.stream())
    return out


def random_weighted_batch(height, edge_, seeds, offset, T):
    """soil_random_weighted_batch: model b as `random_weighted(height[b], edge, seeds[b], offset, T)`."""
    B, H, W = _bhw(height, "random_weighted_batch: height")
    seeds = [int(v) for v in seeds]
    if len(seeds) != B:
        raise ValueError("random_weighted_batch: %d seeds for %d models" % (len(seeds), B))
    ptr = _f(height, "height")
    out = silt.tensor(silt.int32, silt.shape(B, H, W), silt.gpu)
    _call("soil_random_weighted_batch", out.c_ptr, ptr, B, H, W, edge_, (C.c_uint64 * B)(*seeds), int(offset),
          float(T), _abi.stream())
    return out


def _scale_pairs(scale, B, what):
    """`scale` — one (sx, sy) pair or B pairs — as (C array of floats, number of pairs)."""
    try:
        items = list(scale)
        pairs = [items] if len(items) == 2 and not hasattr(items[0], "__len__") else [list(p) for p in items]
        flat = [float(v) for p in pairs for v in p]
    except (TypeError, ValueError):
        raise ValueError("%s: scale must be one (sx, sy) pair or %d pairs" % (what, B))
    if any(len(p) != 2 for p in pairs) or len(pairs) not in (1, B):
        raise ValueError("%s: scale must be one (sx, sy) pair or %d pairs, got %r" % (what, B, scale))
    return (C.c_float * len(flat))(*flat), len(pairs)


def slope_batch(tensor, flow, scale):
    """soil_slope_batch: model b as `slope(tensor[b], flow[b], scale)`; `scale` is one pair or B pairs."""
    B, H, W = _bhw(tensor, "slope_batch: tensor")
    _same(flow, (B, H, W), "slope_batch: flow")
    pairs, n = _scale_pairs(scale, B, "slope_batch")
    t_ptr, f_ptr = _f(tensor, "tensor"), _gpu(flow, silt.int32, "flow")
    out = silt.tensor(silt.float32, silt.shape(B, H, W), silt.gpu)
    _call("soil_slope_batch", out.c_ptr, t_ptr, f_ptr, B, H, W, pairs, n, _abi.stream())
    return out


def accumulate_batch(graph, field, edge_, decay=None):
    """soil_accumulate_batch: model b as `accumulate(graph[b], field[b], edge)`, with `decay` as
    `accumulate_decay`.  Unlike those it does not synchronise."""
    B, H, W = _bhw(graph, "accumulate_batch: graph")
    _same(field, (B, H, W), "accumulate_batch: field")
    if decay is not None:
        _same(decay, (B, H, W), "accumulate_batch: decay")
    g_ptr, f_ptr, d_ptr = _gpu(graph, silt.int32, "graph"), _f(field, "field"), _opt_f(decay, "decay")
    out = silt.tensor(silt.float32, silt.shape(B, H, W), silt.gpu)
    _call("soil_accumulate_batch", out.c_ptr, g_ptr, f_ptr, d_ptr, B, H, W, edge_, _abi.stream())
    return out


# ---- downstream walks (soil_hip.h: "flow graphs: downstream"; the reference's commented-out `upstream` and
# `distance`, model.cpp): where a cell drains to, how many edges away, how long the way.  Stream-ordered.

def _hw2(t, what):
    s = tuple(t.shape) if isinstance(t, silt.tensor) else ()
    if len(s) != 2:
        raise ValueError("%s: expected a (H, W) tensor, got shape %r" % (what, s))
    return s


def _int_plane(t, shape, what):
    """`t` must be an int32 tensor of `shape`, or ValueError."""
    _same(t, shape, what)
    if t.type is not silt.int32:
        raise ValueError("%s: expected an int32 tensor, got %s" % (what, t.type.name))


def _one_pair(scale, what):
    try:
        pair = [float(v) for v in scale]
    except (TypeError, ValueError):
        raise ValueError("%s: scale must be one (sx, sy) pair, got %r" % (what, scale))
    if len(pair) != 2:
        raise ValueError("%s: scale must be one (sx, sy) pair, got %r" % (what, scale))
    return (C.c_float * 2)(*pair)


def _float_plane(t, shape, what):
    _same(t, shape, what)
    if t.type is not silt.float32:
        raise ValueError("%s: expected a float32 tensor, got %s" % (what, t.type.name))


def _opt_i(t, what):
    return None if t is None else _gpu(t, silt.int32, what)


def _shape(dims, t, what):
    """The (H, W) of a grid (dims 2) or the (B, H, W) of a batch (dims 3)."""
    return (_hw2 if dims == 2 else _bhw)(t, what)


def _float_planes(who, shape, planes):
    """`planes`, a list of (name, tensor or None, required), are float32 planes of `shape`."""
    for name, t, required in planes:
        if t is None and required:
            raise ValueError("%s: %s is required" % (who, name))
        if t is not None:
            _float_plane(t, shape, "%s: %s" % (who, name))


def _scales(who, dims, scale, B, none_ok=False):
    """`scale` — one pair for a grid, one pair or B pairs for a batch — as (C array of floats, what the C call takes
    for it: the array, and for a batch the number of pairs)."""
    if scale is None and not none_ok:
        raise ValueError("%s: scale must be one (sx, sy) pair%s" % (who, "" if dims == 2 else " or B pairs"))
    pairs, n = (None, 1) if scale is None else (_one_pair(scale, who), 1) if dims == 2 else _scale_pairs(scale, B, who)
    return pairs, (pairs,) if dims == 2 else (pairs, n)


def _positive(who, pairs, scale):
    if any(not (v > 0 and math.isfinite(v)) for v in pairs):
        raise ValueError("%s: scale entries must be positive finite floats, got %r" % (who, scale))


def _out_pair(shape, double):
    """The result tensor, float64 with `double`, and the C call's (out, out64)."""
    out = silt.tensor(silt.float64 if double else silt.float32, silt.shape(*shape), silt.gpu)
    return out, (None, out.c_ptr) if double else (out.c_ptr, None)


def _on_stream():
    """torch's current stream set to the one the library's calls go to."""
    import torch
    return torch.cuda.stream(torch.cuda.ExternalStream(_abi._stream)) if _abi._stream else contextlib.nullcontext()


def _call_info(entry, names=("chunks", "vec_chunks", "idx64_chunks", "rounds")):
    """The four-word info record of `entry` as a dict; the default names are those of a pointer-doubling entry
    (csrc/flow_paths.hpp PtrInfo)."""
    info = (C.c_int64 * 4)()
    _call(entry, info)
    return dict(zip(names, (int(v) for v in info)))


def _flow_paths(who, dims, graph, edge_, scale, stop, want):
    """soil_flow_paths on a (H, W) graph, soil_flow_paths_batch on (B, H, W); `want`: which of (terminal, steps,
    length) to make."""
    shape = _shape(dims, graph, "%s: graph" % who)
    e = _check.edge(who, edge_)
    _int_plane(graph, shape, "%s: graph" % who)
    if stop is not None:
        _int_plane(stop, shape, "%s: stop" % who)
    if not want[2]:
        tail = (None,) if dims == 2 else (None, 1)
    else:
        tail = (_one_pair(scale, who),) if dims == 2 else _scale_pairs(scale, shape[0], who)
    g_ptr, s_ptr = _gpu(graph, silt.int32, "graph"), _opt_i(stop, "stop")
    outs = [silt.tensor(dt, silt.shape(*shape), silt.gpu) if w else None
            for w, dt in zip(want, (silt.int32, silt.int32, silt.float32))]
    _call("soil_flow_paths" + ("" if dims == 2 else "_batch"), *[o.c_ptr if o is not None else None for o in outs],
          g_ptr, s_ptr, *shape, e, *tail, _abi.stream())
    return tuple(outs)

def flow_paths(graph, edge_, scale=None, stop=None):
    """soil_flow_paths: (terminal, steps, length) of every cell's walk down `graph` — the cell it ends on, the
    number of edges, and the way's length with the (sx, sy) of `scale` (None: no length, the third item is None).
    `stop`: an optional int32 plane of pour points (non-zero: the walk ends here).  Cells on a cycle, or draining into
    one, get -1 / -1 / NaN."""
    return _flow_paths("flow_paths", 2, graph, edge_, scale, stop, (True, True, scale is not None))


def basins(graph, edge_, stop=None):
    """The terminal of every cell's walk (flow_paths): cells with the same value form a basin."""
    return _flow_paths("basins", 2, graph, edge_, None, stop, (True, False, False))[0]


def flow_length(graph, edge_, scale, stop=None):
    """The length of every cell's way to its terminal (flow_paths)."""
    return _flow_paths("flow_length", 2, graph, edge_, scale, stop, (False, False, True))[2]


def watershed(graph, edge_, cells):
    """The catchment of the pour points `cells`, a list of (x, y): an int32 (H, W) mask, 1 where the cell's walk —
    stopped at the pour points — ends on one of them, the points themselves included (the reference's commented-out
    `upstream`)."""
    H, W = _hw2(graph, "watershed: graph")
    try:
        points = [(int(x), int(y)) for x, y in cells]
    except (TypeError, ValueError):
        raise ValueError("watershed: cells must be a list of (x, y) pairs, got %r" % (cells,))
    if not points or any(not (0 <= x < H and 0 <= y < W) for x, y in points):
        raise ValueError("watershed: cells must be one or more (x, y) inside the (%d, %d) grid, got %r" % (H, W, cells))
    _int_plane(graph, (H, W), "watershed: graph")
    _check.edge("watershed", edge_)
    import torch
    plane = np.zeros((H, W), np.int32)
    for x, y in points:
        plane[x, y] = 1
    stop = silt.tensor.from_numpy(plane).gpu()
    terminal = basins(graph, edge_, stop)
    # a walk that ends on a pour point: its terminal carries the stop mark (unresolved cells: -1, no mark) — a gather
    # in torch, on the stream the library's calls go to
    with _on_stream():
        t, marks = terminal.view_torch().view(-1), stop.view_torch().view(-1)
        mask = torch.where(t >= 0, marks[t.clamp(min=0).long()], torch.zeros_like(t))
    return silt.tensor.from_torch(mask.view(H, W).contiguous())


def flow_paths_batch(graph, edge_, scale=None, stop=None):
    """soil_flow_paths_batch: model b as `flow_paths(graph[b], edge, scale, stop[b])`; `scale` is one pair or B
    pairs (None: no length); entries of `graph`, `stop` and the terminals are indices within their model."""
    return _flow_paths("flow_paths_batch", 3, graph, edge_, scale, stop, (True, True, scale is not None))


def basins_batch(graph, edge_, stop=None):
    """`basins` of each of the B models."""
    return _flow_paths("basins_batch", 3, graph, edge_, None, stop, (True, False, False))[0]


def flow_length_batch(graph, edge_, scale, stop=None):
    """`flow_length` of each of the B models; `scale` is one pair or B pairs."""
    return _flow_paths("flow_length_batch", 3, graph, edge_, scale, stop, (False, False, True))[2]


def flow_paths_info():
    """What this thread's last flow_paths / flow_paths_batch call did (soil_flow_paths_info): a dict with the number of
    `chunks`, of chunks whose init pass took the 16-byte form (`vec_chunks`), of chunks on 64-bit offsets
    (`idx64_chunks`) and the `rounds` per chunk."""
    return _call_info("soil_flow_paths_info")


# ---- downstream sums (soil_hip.h: "flow graphs: downstream sums"): x[n] = a[n] L(n) + b[n] x[r(n)] down a receiver
# graph, x = t on the terminals, and the implicit stream-power step, the same recurrence.  Stream-ordered.

def _downstream(who, dims, graph, edge_, planes, scale, stop, double, dt=None):
    """soil_downstream / soil_stream_power and their _batch forms: `planes` is a list of (name, tensor or None,
    required) in the order of the C call's float planes; `dt` None: the sum, else the stream-power step.  Every check
    comes before any device work."""
    shape = _shape(dims, graph, "%s: graph" % who)
    e = _check.edge(who, edge_)
    _int_plane(graph, shape, "%s: graph" % who)
    _float_planes(who, shape, planes)
    if stop is not None:
        _int_plane(stop, shape, "%s: stop" % who)
    pairs, tail = _scales(who, dims, scale, shape[0], none_ok=dt is None)
    if dt is not None:
        dt = _check.number(who, "dt", dt)
        _positive(who, pairs, scale)
    g_ptr = _gpu(graph, silt.int32, "graph")
    f_ptrs = [_opt_f(t, name) for name, t, _ in planes]
    s_ptr = _opt_i(stop, "stop")
    out, outs = _out_pair(shape, double)
    batch = "" if dims == 2 else "_batch"
    if dt is None:
        _call("soil_downstream" + batch, *outs, g_ptr, *f_ptrs, s_ptr, *shape, e, *tail, _abi.stream())
    else:
        _call("soil_stream_power" + batch, *outs, f_ptrs[0], g_ptr, *f_ptrs[1:], s_ptr, *shape, e, *tail, dt,
              _abi.stream())
    return out


def downstream(graph, edge_, a=None, b=None, terminal=None, scale=None, stop=None, double=False):
    """soil_downstream: x[n] = a[n] L(n) + b[n] x[r(n)] for a cell with an edge to r(n) = graph[n], x[n] = terminal[n]
    on a cell without one (or with stop[n] != 0).  `a`, `b`, `terminal`: float32 planes or None (1, 1, 0); L: the
    edge's length under the (sx, sy) of `scale` (None: 1).  Returns a float32 GPU tensor, float64 with `double`; NaN
    for a cell on a cycle or draining into one.  Examples: a=None — the number of edges to the outlet, or with a
    scale the flow length; terminal=height, a=zeros — the height of each cell's outlet; b=decay — what survives."""
    return _downstream("downstream", 2, graph, edge_, [("a", a, False), ("b", b, False), ("terminal", terminal, False)],
                       scale, stop, double)


def downstream_batch(graph, edge_, a=None, b=None, terminal=None, scale=None, stop=None, double=False):
    """`downstream` of each of the B models of (B, H, W) planes (soil_downstream_batch); `scale` is one pair or B
    pairs; graph entries are indices within their model."""
    return _downstream("downstream_batch", 3, graph, edge_,
                       [("a", a, False), ("b", b, False), ("terminal", terminal, False)], scale, stop, double)


def stream_power(height, graph, erosivity, edge_, scale, dt, uplift=None, stop=None, double=False):
    """soil_stream_power: one implicit step of stream-power incision with slope exponent n = 1 along `graph` (any other
    exponent in 1 .. 16: stream_power_n),
    h'[n] = (h[n] + dt u[n] + F h'[r]) / (1 + F) with F = erosivity[n] dt / L(n); a terminal keeps its height.
    `erosivity` is K A^m (soil.erosivity), `uplift` a float32 plane or None.  Returns the new heights, float32 (float64
    with `double`); `height` is left as it is.  The graph should be acyclic and reach an outlet from every cell
    (soil.condition); after a step, float32 ties can appear along edges that went strictly downhill, so the next step
    starts again from condition()."""
    return _downstream("stream_power", 2, graph, edge_,
                       [("height", height, True), ("erosivity", erosivity, True), ("uplift", uplift, False)], scale, stop,
                       double, dt)


def stream_power_batch(height, graph, erosivity, edge_, scale, dt, uplift=None, stop=None, double=False):
    """`stream_power` of each of the B models of (B, H, W) planes (soil_stream_power_batch); `scale` is one pair or B
    pairs."""
    return _downstream("stream_power_batch", 3, graph, edge_,
                       [("height", height, True), ("erosivity", erosivity, True), ("uplift", uplift, False)], scale, stop,
                       double, dt)


def erosivity(area, K, m):
    """K * area ** m of a float32 drainage-area tensor of any shape, on the device through torch, float32: the
    `erosivity` of stream_power.  torch's pow is not correctly rounded, so this plane is not bit-pinned; what
    stream_power makes of a given plane is."""
    if not isinstance(area, silt.tensor) or area.type is not silt.float32:
        raise ValueError("erosivity: area must be a float32 silt tensor")
    if area.host is not silt.gpu:
        raise _abi.SoilError("mismatch_host: area must be a silt.gpu tensor")
    with _on_stream():
        out = area.view_torch().pow(float(m)).mul_(float(K))
    return silt.tensor.from_torch(out.contiguous())


def chi(graph, area, edge_, scale, theta=0.45, A0=1.0, stop=None):
    """The chi coordinate of every cell of a (H, W) graph: the sum of (A0 / area) ** theta * L along the way to the
    terminal, downstream(a=(A0 / area) ** theta, scale=scale).  The weights are made through torch in float32 (not
    bit-pinned); the sum is soil_downstream's."""
    shape = _hw2(graph, "chi: graph")
    _float_plane(area, shape, "chi: area")
    if area.host is not silt.gpu:
        raise _abi.SoilError("mismatch_host: area must be a silt.gpu tensor")
    _check.edge("chi", edge_)
    _one_pair(scale, "chi")
    with _on_stream():
        w = (float(A0) / area.view_torch()).pow_(float(theta))
    return _downstream("chi", 2, graph, edge_, [("a", silt.tensor.from_torch(w.contiguous()), False), ("b", None, False),
                                                ("terminal", None, False)], scale, stop, False)


# ---- erosion-deposition (soil_hip.h: "flow graphs: erosion-deposition"): the stream-power step with a deposition
# term fed by the upstream sum of what the step removes, a fixed number of iterations.  Stream-ordered.

# The default `iters` of stream_power_deposit_n: the count at which n <= 2 with G <= 1 has converged on the bench
# terrains at every size (the table of "Erosion-deposition at slope exponents above 1")
DEPOSIT_N_ITERS = 28


def _stream_power_deposit(who, dims, height, graph, erosivity, deposition, edge_, scale, dt, uplift, iters, double,
                          flux, residual, n=None):
    """soil_stream_power_deposit and its _batch form; with `n` soil_stream_power_deposit_n and its _batch form.  Every
    check comes before any device work."""
    shape = _shape(dims, graph, "%s: graph" % who)
    e = _check.edge(who, edge_)
    _int_plane(graph, shape, "%s: graph" % who)
    planes = [("height", height, True), ("erosivity", erosivity, True), ("deposition", deposition, True),
              ("uplift", uplift, False)]
    _float_planes(who, shape, planes)
    pairs, tail = _scales(who, dims, scale, shape[0])
    _positive(who, pairs, scale)
    dt = _check.number(who, "dt", dt)
    exponent = () if n is None else (_check.exponent(who, n),)
    iters = _check.count(who, "iters", iters)
    g_ptr = _gpu(graph, silt.int32, "graph")
    h_ptr, k_ptr, d_ptr, u_ptr = (_opt_f(t, name) for name, t, _ in planes)
    out, outs = _out_pair(shape, double)
    f = silt.tensor(silt.float32, silt.shape(*shape), silt.gpu) if flux else None
    r = silt.tensor(silt.float64, silt.shape(1 if dims == 2 else shape[0]), silt.gpu) if residual else None
    _call("soil_stream_power_deposit" + ("" if n is None else "_n") + ("" if dims == 2 else "_batch"), *outs,
          None if f is None else f.c_ptr, None if r is None else r.c_ptr, h_ptr, g_ptr, k_ptr, d_ptr, u_ptr, *shape, e,
          *tail, dt, *exponent, iters, _abi.stream())
    extras = tuple(t for t in (f, r) if t is not None)
    return (out,) + extras if extras else out


def stream_power_deposit(height, graph, erosivity, deposition, edge_, scale, dt, uplift=None, iters=8, double=False,
                         flux=False, residual=False):
    """soil_stream_power_deposit: one implicit step of stream-power incision with sediment deposition (the
    erosion-deposition model; slope exponent 1 — any other exponent in 1 .. 16: stream_power_deposit_n) along
    `graph`: stream_power's step plus (G / A) Qs, Qs the net material
    removed upstream, by `iters` fixed-point iterations of an upstream sum and a downstream solve.  `erosivity` is
    K A^m (soil.erosivity), `deposition` G cell / A (soil.deposition), `uplift` a float32 plane or None.  Returns the
    new heights, float32 (float64 with `double`); with `flux` and / or `residual` a tuple (heights, flux, residual) of
    those asked for: the float32 sediment flux through every cell (at a terminal: what reached that base level) and a
    one-element float64 tensor, the largest change of the last iteration.  `height` is left as it is.  A zero
    deposition plane gives stream_power's bits."""
    return _stream_power_deposit("stream_power_deposit", 2, height, graph, erosivity, deposition, edge_, scale, dt,
                                 uplift, iters, double, flux, residual)


def stream_power_deposit_batch(height, graph, erosivity, deposition, edge_, scale, dt, uplift=None, iters=8,
                               double=False, flux=False, residual=False):
    """`stream_power_deposit` of each of the B models of (B, H, W) planes (soil_stream_power_deposit_batch); `scale`
    is one pair or B pairs; the residual tensor has B entries."""
    return _stream_power_deposit("stream_power_deposit_batch", 3, height, graph, erosivity, deposition, edge_, scale,
                                 dt, uplift, iters, double, flux, residual)


def deposition(area, G, cell=1.0):
    """G * cell / area of a float32 drainage-area tensor, on the device through torch, float32: the `deposition` of
    stream_power_deposit.  `cell`: the area of a cell, a number, or a tensor that broadcasts against `area` (one value
    per model: shape (B, 1, 1)).  Not bit-pinned, as soil.erosivity is not; what stream_power_deposit makes of a
    given plane is."""
    if not isinstance(area, silt.tensor) or area.type is not silt.float32:
        raise ValueError("deposition: area must be a float32 silt tensor")
    G = _check.number("deposition", "G", G)
    if area.host is not silt.gpu:
        raise _abi.SoilError("mismatch_host: area must be a silt.gpu tensor")
    with _on_stream():
        c = cell.view_torch() if isinstance(cell, silt.tensor) else float(cell)
        out = (G * c / area.view_torch()).float()
    return silt.tensor.from_torch(out.contiguous())


def stream_power_deposit_info():
    """What this thread's last stream_power_deposit / _batch call did (soil_stream_power_deposit_info): a dict with the
    number of kernel `launches`, of `chunks`, the `iters` run and the `scratch_bytes` it asked for."""
    return _call_info("soil_stream_power_deposit_info", ("launches", "chunks", "iters", "scratch_bytes"))


# The deposit step at a slope exponent above 1 (soil_hip.h: "flow graphs: erosion-deposition at slope exponents above
# 1"): each iteration renews the Newton tangent of stream_power_n and the upstream sum of the deposit step together.

def stream_power_deposit_n(height, graph, erosivity, deposition, edge_, scale, dt, n, uplift=None,
                           iters=DEPOSIT_N_ITERS, double=False, flux=False, residual=False):
    """soil_stream_power_deposit_n: one implicit step of dh/dt = u - K A^m S^n + (G / A) Qs along `graph` with a slope
    exponent `n` in 1 .. 16: `iters` iterations, each the deposit step's upstream sum of what the iterate before
    removed and one solve of stream_power's rounds with the coefficients of stream_power_n's linearisation about that
    iterate, started from stream_power's own result.  The planes and the returned values are stream_power_deposit's:
    the heights, or with `flux` and / or `residual` a tuple (heights, flux, residual) of those asked for.  The
    iteration has a domain: for K dt / L up to order 1 and G <= 1 it contracts for n up to 3, with
    G = 2 it can diverge for n >= 2; under a K dt / L of order 100 it stalls across lakes for n >= 2 and diverges for
    G = 2, while every value stays finite — so read the residual.  The default of `iters` is the count at which
    n <= 2 with G <= 1 has reached the float32 floor of the upstream sum on the bench terrains at every size.  A zero
    deposition plane gives stream_power_n's bits, n == 1 stream_power_deposit's; n < 1 is refused.  `height` is left
    as it is."""
    return _stream_power_deposit("stream_power_deposit_n", 2, height, graph, erosivity, deposition, edge_, scale, dt,
                                 uplift, iters, double, flux, residual, n)


def stream_power_deposit_n_batch(height, graph, erosivity, deposition, edge_, scale, dt, n, uplift=None,
                                 iters=DEPOSIT_N_ITERS, double=False, flux=False, residual=False):
    """`stream_power_deposit_n` of each of the B models of (B, H, W) planes (soil_stream_power_deposit_n_batch);
    `scale` is one pair or B pairs; the residual tensor has B entries."""
    return _stream_power_deposit("stream_power_deposit_n_batch", 3, height, graph, erosivity, deposition, edge_, scale,
                                 dt, uplift, iters, double, flux, residual, n)


def stream_power_deposit_n_info():
    """What this thread's last stream_power_deposit_n / _batch call did (soil_stream_power_deposit_n_info): a dict
    with the number of kernel `launches`, of `chunks`, the `iters` run and the `scratch_bytes` it asked for."""
    return _call_info("soil_stream_power_deposit_n_info", ("launches", "chunks", "iters", "scratch_bytes"))


# ---- slope exponents above 1 (soil_hip.h: "flow graphs: slope exponents above 1"): the stream-power step as Newton
# steps on the whole triangular system, each one solve of stream_power's rounds, from stream_power's own result.

def _stream_power_n(who, dims, height, graph, erosivity, edge_, scale, dt, n, uplift, stop, iters, double, residual):
    """soil_stream_power_n and its _batch form.  Every check comes before any device work."""
    shape = _shape(dims, graph, "%s: graph" % who)
    e = _check.edge(who, edge_)
    _int_plane(graph, shape, "%s: graph" % who)
    planes = [("height", height, True), ("erosivity", erosivity, True), ("uplift", uplift, False)]
    _float_planes(who, shape, planes)
    if stop is not None:
        _int_plane(stop, shape, "%s: stop" % who)
    pairs, tail = _scales(who, dims, scale, shape[0])
    _positive(who, pairs, scale)
    dt = _check.number(who, "dt", dt)
    n = _check.exponent(who, n)
    iters = _check.count(who, "iters", iters)
    g_ptr = _gpu(graph, silt.int32, "graph")
    h_ptr, k_ptr, u_ptr = (_opt_f(t, name) for name, t, _ in planes)
    s_ptr = _opt_i(stop, "stop")
    out, outs = _out_pair(shape, double)
    r = silt.tensor(silt.float64, silt.shape(1 if dims == 2 else shape[0]), silt.gpu) if residual else None
    _call("soil_stream_power_n" + ("" if dims == 2 else "_batch"), *outs, None if r is None else r.c_ptr, h_ptr, g_ptr,
          k_ptr, u_ptr, s_ptr, *shape, e, *tail, dt, n, iters, _abi.stream())
    return out if r is None else (out, r)


def stream_power_n(height, graph, erosivity, edge_, scale, dt, n, uplift=None, stop=None, iters=12, double=False,
                   residual=False):
    """soil_stream_power_n: one implicit step of stream-power incision dh/dt = u - K A^m S^n along `graph` with a slope
    exponent `n` in 1 .. 16: `iters` Newton steps on the whole system, each one solve of stream_power's rounds with the
    coefficients of the linearisation about the iterate before, started from stream_power's own result (from the old
    heights the iteration stalls across flats and filled lakes).  `erosivity` is K A^m (soil.erosivity), `uplift` and
    `stop` as in stream_power.  Returns the new heights, float32 (float64 with `double`), or with `residual` the tuple
    (heights, residual): a one-element float64 tensor, the largest change of the last iteration — judge convergence by
    it; under a very large K dt the iteration crosses a flat one cell per step.  n == 1 is stream_power, bit for bit;
    n < 1 is refused.  `height` is left as it is."""
    return _stream_power_n("stream_power_n", 2, height, graph, erosivity, edge_, scale, dt, n, uplift, stop, iters,
                           double, residual)


def stream_power_n_batch(height, graph, erosivity, edge_, scale, dt, n, uplift=None, stop=None, iters=12, double=False,
                         residual=False):
    """`stream_power_n` of each of the B models of (B, H, W) planes (soil_stream_power_n_batch); `scale` is one pair or
    B pairs; the residual tensor has B entries."""
    return _stream_power_n("stream_power_n_batch", 3, height, graph, erosivity, edge_, scale, dt, n, uplift, stop, iters,
                           double, residual)


def stream_power_n_info():
    """What this thread's last stream_power_n / _batch call did (soil_stream_power_n_info): a dict with the number of
    kernel `launches`, of `chunks`, the `iters` run (0 for n == 1) and the `scratch_bytes` it asked for."""
    return _call_info("soil_stream_power_n_info", ("launches", "chunks", "iters", "scratch_bytes"))


def downstream_info():
    """What this thread's last downstream / stream_power call (or _batch form) did (soil_downstream_info): a dict with
    the number of `chunks`, of chunks whose init pass took the 16-byte form (`vec_chunks`), of chunks on 64-bit
    offsets (`idx64_chunks`) and the `rounds` per chunk."""
    return _call_info("soil_downstream_info")


# ---- upstream extrema (soil_hip.h: "flow graphs: upstream extrema"): the least or the greatest of a plane over
# everything that drains through a cell, in the integer key order of the floats; breaching is the minimum of the
# heights.  Stream-ordered.

def _upstream(who, dims, graph, value, edge_, stop, arg, op, name="value"):
    """soil_upstream_extreme on (H, W) planes, soil_upstream_extreme_batch on (B, H, W); `name`: what the caller calls
    the value plane, for the messages.  Every check comes before any device work."""
    shape = _shape(dims, graph, "%s: graph" % who)
    e = _check.edge(who, edge_)
    _int_plane(graph, shape, "%s: graph" % who)
    _float_plane(value, shape, "%s: %s" % (who, name))
    if stop is not None:
        _int_plane(stop, shape, "%s: stop" % who)
    g_ptr, v_ptr, s_ptr = _gpu(graph, silt.int32, "graph"), _f(value, name), _opt_i(stop, "stop")
    out = silt.tensor(silt.float32, silt.shape(*shape), silt.gpu)
    where = silt.tensor(silt.int32, silt.shape(*shape), silt.gpu) if arg else None
    _call("soil_upstream_extreme" + ("" if dims == 2 else "_batch"), out.c_ptr, None if where is None else where.c_ptr,
          g_ptr, v_ptr, s_ptr, *shape, e, op, _abi.stream())
    return (out, where) if arg else out


def upstream_min(graph, value, edge_, stop=None, arg=False):
    """soil_upstream_extreme, op min: for every cell of a (H, W) receiver graph the least `value` (a float32 plane) over
    all the cells that reach it — the cell itself and everything whose walk along the edges passes through it; cycles
    are allowed.  The order is the integer key order -inf < .. < -0 < +0 < .. < +inf < NaN: a NaN is ignored wherever a
    number reaches the cell, and the result is NaN (0x7fc00000) only where nothing else does.  `stop`: an optional
    int32 plane; a non-zero cell collects its catchment and passes nothing on.  With `arg` returns (out, arg), arg the
    int32 index of the cell that attains the value, the smallest among equals, -1 where out is NaN.  One definite bit
    pattern."""
    return _upstream("upstream_min", 2, graph, value, edge_, stop, arg, 0)


def upstream_max(graph, value, edge_, stop=None, arg=False):
    """soil_upstream_extreme, op max: -upstream_min(-value), the negations exact.  NaN is ignored as there, +0 wins
    over -0, and `arg` is again the smallest index among equals."""
    return _upstream("upstream_max", 2, graph, value, edge_, stop, arg, 1)


def upstream_min_batch(graph, value, edge_, stop=None, arg=False):
    """`upstream_min` of each of the B models of (B, H, W) planes (soil_upstream_extreme_batch); entries of `graph`
    and of arg are indices within their model."""
    return _upstream("upstream_min_batch", 3, graph, value, edge_, stop, arg, 0)


def upstream_max_batch(graph, value, edge_, stop=None, arg=False):
    """`upstream_max` of each of the B models of (B, H, W) planes."""
    return _upstream("upstream_max_batch", 3, graph, value, edge_, stop, arg, 1)


def upstream_info():
    """What this thread's last upstream_min / upstream_max call (or _batch form) did (soil_upstream_extreme_info): a
    dict with the number of `chunks`, of chunks whose init pass took the 16-byte form (`vec_chunks`), of chunks on
    64-bit offsets (`idx64_chunks`) and the `rounds` per chunk."""
    return _call_info("soil_upstream_extreme_info")


def _minus(a, b):
    """a - b of two float32 GPU tensors as a new tensor: an exact negation and one fp32 addition (silt.multiply,
    silt.add)."""
    out = silt.clone(b)
    silt.multiply(out, -1.0)
    silt.add(out, a)
    return out


def _breach(who, dims, height, graph, edge_, cut):
    breached = _upstream(who, dims, graph, height, edge_, None, False, 0, name="height")
    return (breached, _minus(height, breached)) if cut else breached


def breach(height, graph, edge_, cut=False):
    """The DEM `height` carved along `graph`: upstream_min(graph, height, edge_), every cell lowered to the lowest
    height of anything that drains through it.  The surface never stands above `height` and never rises along an edge
    of `graph`.  With `cut` returns (breached, height - breached), the depth carved: one fp32 subtraction, NaN where
    the height is NaN."""
    return _breach("breach", 2, height, graph, edge_, cut)


def breach_batch(height, graph, edge_, cut=False):
    """`breach` of each of the B models of (B, H, W) planes."""
    return _breach("breach_batch", 3, height, graph, edge_, cut)


def _upstream_length(who, dims, graph, edge_, scale, stop):
    length = _flow_paths(who, dims, graph, edge_, scale, stop, (False, False, True))[2]
    out = _upstream(who, dims, graph, length, edge_, stop, False, 1)
    silt.multiply(length, -1.0)
    silt.add(out, length)
    return out


def upstream_length(graph, edge_, scale, stop=None):
    """The length of the longest way down to every cell: upstream_max(graph, L) + (-1 * L) with L = flow_length(graph,
    edge_, scale, stop) — the greatest distance to the outlet in the cell's catchment less the cell's own, an exact
    negation and one fp32 addition.  0 on a cell nothing drains into; NaN where L is NaN (a cell on a cycle or
    draining into one)."""
    return _upstream_length("upstream_length", 2, graph, edge_, scale, stop)


def upstream_length_batch(graph, edge_, scale, stop=None):
    """`upstream_length` of each of the B models; `scale` is one pair or B pairs."""
    return _upstream_length("upstream_length_batch", 3, graph, edge_, scale, stop)


# ---- stream order and channel segments (soil_hip.h: "flow graphs: stream order"): the channel network of a receiver
# graph — which cells are channels, their Strahler order, their donors, where links and Strahler streams end, and the
# graph restricted to the channels.  One host look per level: the calls synchronise the stream.

_SO_OUTPUTS = ("order", "donors", "link_foot", "order_foot", "channel_graph")


def _stream_order(who, dims, graph, edge_, channel, area, threshold, stop, want):
    """soil_stream_order on (H, W) planes, soil_stream_order_batch on (B, H, W); `want`: the names of the outputs to
    make, returned as a dict.  Every check comes before any device work."""
    shape = _shape(dims, graph, "%s: graph" % who)
    e = _check.edge(who, edge_)
    _int_plane(graph, shape, "%s: graph" % who)
    if channel is not None:
        _int_plane(channel, shape, "%s: channel" % who)
    if area is not None:
        _float_plane(area, shape, "%s: area" % who)
        if threshold is None:
            raise ValueError("%s: area needs a threshold" % who)
    elif threshold is not None:
        raise ValueError("%s: threshold needs an area" % who)
    if stop is not None:
        _int_plane(stop, shape, "%s: stop" % who)
    th = 0.0 if threshold is None else float(threshold)
    if th != th:
        raise ValueError("%s: threshold is NaN" % who)
    g_ptr, c_ptr, a_ptr, s_ptr = (_gpu(graph, silt.int32, "graph"), _opt_i(channel, "channel"), _opt_f(area, "area"),
                                  _opt_i(stop, "stop"))
    outs = {k: silt.tensor(silt.int32, silt.shape(*shape), silt.gpu) for k in _SO_OUTPUTS if k in want}
    _call("soil_stream_order" + ("" if dims == 2 else "_batch"),
          *[outs[k].c_ptr if k in outs else None for k in _SO_OUTPUTS], g_ptr, c_ptr, a_ptr, th, s_ptr, *shape, e,
          _abi.stream())
    return outs


def _order(who, dims, graph, edge_, channel, area, threshold, stop, donors):
    o = _stream_order(who, dims, graph, edge_, channel, area, threshold, stop, ("order", "donors") if donors else ("order",))
    return (o["order"], o["donors"]) if donors else o["order"]


def stream_order(graph, edge_, channel=None, area=None, threshold=None, stop=None, donors=False):
    """soil_stream_order: the Strahler order of every cell of a (H, W) receiver graph, int32, 0 off the channels.  A
    cell is a channel cell iff `channel` (an optional int32 mask) is non-zero there and `area` (an optional float32
    plane, with `threshold`) is >= threshold — a float comparison, a NaN area fails; with neither, every cell is one.
    The channel graph keeps the edges of `graph` (the edge rule and `stop` of flow_paths) between channel cells.  A
    head has order 1; a cell has the greatest order among its donors, plus one where two or more share it.  Cycles
    are allowed: the order is defined by levels (soil_hip.h) and nothing is special-cased.  With `donors` returns
    (order, donors), the number of channel-graph edges into each cell.  Synchronises the stream once per level."""
    return _order("stream_order", 2, graph, edge_, channel, area, threshold, stop, donors)


def stream_order_batch(graph, edge_, channel=None, area=None, threshold=None, stop=None, donors=False):
    """`stream_order` of each of the B models of (B, H, W) planes (soil_stream_order_batch); entries of `graph` are
    indices within their model, `threshold` is one number for all models."""
    return _order("stream_order_batch", 3, graph, edge_, channel, area, threshold, stop, donors)


def stream_order_info():
    """What this thread's last stream_order / stream_segments / stream_magnitude call (or _batch form) did
    (soil_stream_order_info): `chunks`, `vec_chunks`, `idx64_chunks` and `rounds` as upstream_info(), and `levels`,
    the seed passes run: the greatest order found (1 where there is no channel), the most over a batch's models."""
    info = (C.c_int64 * 5)()
    _call("soil_stream_order_info", info)
    return dict(zip(("chunks", "vec_chunks", "idx64_chunks", "rounds", "levels"), (int(v) for v in info)))


def _stream_segments(who, dims, graph, edge_, channel, area, threshold, stop, scale, by):
    if by not in ("link", "order"):
        raise ValueError("%s: by must be 'link' or 'order', got %r" % (who, by))
    foot = by + "_foot"
    o = _stream_order(who, dims, graph, edge_, channel, area, threshold, stop, ("order", foot, "channel_graph"))
    segment, steps, length = _flow_paths(who, dims, o["channel_graph"], edge_, scale, o[foot],
                                         (True, True, scale is not None))
    return o["order"], segment, steps, length


def stream_segments(graph, edge_, channel=None, area=None, threshold=None, stop=None, scale=None, by="link"):
    """(order, segment, steps, length) of the channel network of `graph` (inputs as stream_order): segment[n] is the
    index of the foot cell of n's link (`by="link"`: a link ends just above a junction — a cell with two or more
    donors — or at an outlet of the channel graph) or of n's Strahler stream (`by="order"`: it ends where the order
    rises or at an outlet); steps and length are the way to that foot along the channels, length with the (sx, sy) of
    `scale` (None: no length, the last item is None).  One soil_stream_order call for the restricted graph and the
    foot plane, then flow_paths(channel_graph, edge_, scale, stop=foot).  A non-channel cell is its own foot at
    distance 0: segment[n] == n, steps 0, length 0 — its order == 0 tells it apart.  Cells on a cycle of the channel
    graph, or draining into one, get -1 / -1 / NaN as in flow_paths."""
    return _stream_segments("stream_segments", 2, graph, edge_, channel, area, threshold, stop, scale, by)


def stream_segments_batch(graph, edge_, channel=None, area=None, threshold=None, stop=None, scale=None, by="link"):
    """`stream_segments` of each of the B models of (B, H, W) planes; `scale` is one pair or B pairs; segment entries
    are indices within their model."""
    return _stream_segments("stream_segments_batch", 3, graph, edge_, channel, area, threshold, stop, scale, by)


def _stream_magnitude(who, dims, graph, edge_, channel, area, threshold, stop):
    o = _stream_order(who, dims, graph, edge_, channel, area, threshold, stop, ("order", "donors", "channel_graph"))
    with _on_stream():
        heads = ((o["donors"].view_torch() == 0) & (o["order"].view_torch() > 0)).float()
    heads = silt.tensor.from_torch(heads.contiguous())
    return (accumulate if dims == 2 else accumulate_batch)(o["channel_graph"], heads, edge_)


def stream_magnitude(graph, edge_, channel=None, area=None, threshold=None, stop=None):
    """The Shreve magnitude of every cell (inputs as stream_order): the number of channel heads — channel cells with
    no donor — that drain through it along the channel graph, float32: accumulate(channel_graph, heads).  0 off the
    channels; on and below a cycle it is whatever accumulate gives there."""
    return _stream_magnitude("stream_magnitude", 2, graph, edge_, channel, area, threshold, stop)


def stream_magnitude_batch(graph, edge_, channel=None, area=None, threshold=None, stop=None):
    """`stream_magnitude` of each of the B models of (B, H, W) planes."""
    return _stream_magnitude("stream_magnitude_batch", 3, graph, edge_, channel, area, threshold, stop)


# ---- hillslope diffusion (soil_hip.h: "hillslope diffusion"): one implicit step of dh/dt = div(kappa grad h) + u, a
# tridiagonal solve per grid line along one axis, then along the other.  Stream-ordered.

def _diffuse(who, dims, height, scale, dt, kappa, diffusivity, uplift, fixed, border, first_axis, double):
    """soil_diffuse and soil_diffuse_batch.  Every check comes before any device work."""
    shape = _shape(dims, height, "%s: height" % who)
    _float_plane(height, shape, "%s: height" % who)
    _check.kappa_or_diffusivity(who, kappa, diffusivity)
    _float_planes(who, shape, [("diffusivity", diffusivity, False), ("uplift", uplift, False)])
    if fixed is not None:
        _int_plane(fixed, shape, "%s: fixed" % who)
    pairs, tail = _scales(who, dims, scale, shape[0])
    _positive(who, pairs, scale)
    dt = _check.number(who, "dt", dt)
    border = _check.border(who, border)
    first_axis = _check.first_axis(who, first_axis)
    h_ptr = _f(height, "height")
    k_ptr, u_ptr = _opt_f(diffusivity, "diffusivity"), _opt_f(uplift, "uplift")
    f_ptr = _opt_i(fixed, "fixed")
    out, outs = _out_pair(shape, double)
    _call("soil_diffuse" + ("" if dims == 2 else "_batch"), *outs, h_ptr, k_ptr, u_ptr, f_ptr, *shape, *tail,
          0.0 if kappa is None else float(kappa), dt, border, first_axis, _abi.stream())
    return out


def diffuse(height, scale, dt, kappa=None, diffusivity=None, uplift=None, fixed=None, border="fixed", first_axis=0,
            double=False):
    """soil_diffuse: one implicit (backward Euler, one sweep per axis) step of hillslope diffusion
    dh/dt = div(kappa grad h) + uplift over `dt` on a (H, W) float32 height plane with the spacings (sx, sy) of
    `scale`; stable for any dt.  Exactly one of `kappa` (a number) and `diffusivity` (a float32 plane) is given.
    `fixed`: an int32 plane, non-zero cells keep their height; border="fixed" keeps the outermost rows and columns
    too, "free" closes the edges (no flux: the sum is conserved).  NaN cells are voids: walls without flux, NaN in the
    result.  `first_axis`: the axis of the first sweep.  Returns the new heights, float32 (float64 with `double`);
    `height` is left as it is."""
    return _diffuse("diffuse", 2, height, scale, dt, kappa, diffusivity, uplift, fixed, border, first_axis, double)


def diffuse_batch(height, scale, dt, kappa=None, diffusivity=None, uplift=None, fixed=None, border="fixed",
                  first_axis=0, double=False):
    """`diffuse` of each of the B models of (B, H, W) planes (soil_diffuse_batch); `scale` is one pair or B pairs."""
    return _diffuse("diffuse_batch", 3, height, scale, dt, kappa, diffusivity, uplift, fixed, border, first_axis,
                    double)


def diffuse_info():
    """What this thread's last diffuse / diffuse_batch call did (soil_diffuse_info): a dict with the number of kernel
    `launches`, of `chunks`, of chunks on 64-bit offsets (`idx64_chunks`) and the `scratch_bytes` it asked for."""
    return _call_info("soil_diffuse_info", ("launches", "chunks", "idx64_chunks", "scratch_bytes"))


def fill_depressions(height, edge_=None):
    """Priority-flood surface of a DEM (soil_hip.h: soil_fill_depressions) — the
    conditioning step the reference leaves to pysheds (example/dem_condition.py:35-41)."""
    H, W = _hw(height)
    out = silt.tensor(silt.float32, silt.shape(H, W), silt.gpu)
    _call("soil_fill_depressions", out.c_ptr, _f(height, "height"), H, W,
          int(d8 if edge_ is None else edge_), _abi.stream())
    return out


# ---- flats and filled lakes (soil_hip.h: "flow graphs: conditioning"): on the surface fill_depressions returns every
# lake cell is a terminal of steepest / random_weighted; these give them receivers, as indices.

def _flat_distance(who, height, edge_, dims):
    shape = (_hw2 if dims == 2 else _bhw)(height, "%s: height" % who)
    e = _check.edge(who, edge_)
    _float_plane(height, shape, "%s: height" % who)
    ptr = _f(height, "height")
    out = silt.tensor(silt.int32, silt.shape(*shape), silt.gpu)
    _call("soil_flat_distance" + ("" if dims == 2 else "_batch"), out.c_ptr, ptr, *shape, e, _abi.stream())
    return out


def _flat_receivers(who, graph, height, dist, edge_, dims):
    shape = (_hw2 if dims == 2 else _bhw)(graph, "%s: graph" % who)
    e = _check.edge(who, edge_)
    _int_plane(graph, shape, "%s: graph" % who)
    _float_plane(height, shape, "%s: height" % who)
    _int_plane(dist, shape, "%s: dist" % who)
    g, h, d = _gpu(graph, silt.int32, "graph"), _f(height, "height"), _gpu(dist, silt.int32, "dist")
    out = silt.tensor(silt.int32, silt.shape(*shape), silt.gpu)
    _call("soil_flat_receivers" + ("" if dims == 2 else "_batch"), out.c_ptr, g, h, d, *shape, e, _abi.stream())
    return out


def flat_distance(height, edge_):
    """soil_flat_distance: for every cell of a (H, W) DEM the shortest way, over cells of equal height, to a cell that
    can drain (a neighbour off the grid, NaN or strictly lower): 0 there, -1 where no such way exists and on NaN
    cells.  int32; synchronises the stream."""
    return _flat_distance("flat_distance", height, edge_, 2)


def flat_receivers(graph, height, dist, edge_):
    """soil_flat_receivers: a copy of `graph` in which every cell without a receiver (an entry < 0) and with
    dist > 0 takes the first neighbour, in table order, of equal height and dist one less.  A strictly downhill
    `graph` (steepest, random_weighted) stays acyclic."""
    return _flat_receivers("flat_receivers", graph, height, dist, edge_, 2)


def resolve_flats(height, edge_, graph=None):
    """The receiver graph of `height` with its flats routed: flat_receivers of `graph` (None: steepest(height, edge))
    along flat_distance(height, edge).  On a surface fill_depressions made, the only terminals left are cells on the
    border or beside NaN cells."""
    e = _check.edge("resolve_flats", edge_)
    dist = _flat_distance("resolve_flats", height, e, 2)
    return _flat_receivers("resolve_flats", steepest(height, e) if graph is None else graph, height, dist, e, 2)


def flat_distance_batch(height, edge_):
    """flat_distance of each of the B models of a (B, H, W) tensor, side by side (soil_flat_distance_batch)."""
    return _flat_distance("flat_distance_batch", height, edge_, 3)


def flat_receivers_batch(graph, height, dist, edge_):
    """flat_receivers of each of the B models; entries are indices within their model."""
    return _flat_receivers("flat_receivers_batch", graph, height, dist, edge_, 3)


def resolve_flats_batch(height, edge_, graph=None):
    """resolve_flats of each of the B models of a (B, H, W) tensor."""
    e = _check.edge("resolve_flats_batch", edge_)
    dist = _flat_distance("resolve_flats_batch", height, e, 3)
    return _flat_receivers("resolve_flats_batch", steepest_batch(height, e) if graph is None else graph, height, dist,
                           e, 3)


def flat_distance_info():
    """What this thread's last flat_distance / flat_distance_batch call did (soil_flat_distance_info): a dict with the
    relaxation `launches`, the `tiles` of a model, the `models` and the `looks` at the "changed" word."""
    return _call_info("soil_flat_distance_info", ("launches", "tiles", "models", "looks"))


# ---- threshold hillslopes (soil_hip.h: soil_slope_limit): the greatest surface below a DEM on which no cell stands
# higher above a neighbour than a critical slope times the distance allows.  Synchronises the stream.

def _slope_limit(who, dims, height, scale, slope, edge_, excess):
    """soil_slope_limit and soil_slope_limit_batch.  Every check comes before any device work."""
    shape = _shape(dims, height, "%s: height" % who)
    _float_plane(height, shape, "%s: height" % who)
    e = _check.edge(who, d8 if edge_ is None else edge_)
    pairs, tail = _scales(who, dims, scale, shape[0])
    _positive(who, pairs, scale)
    if isinstance(slope, silt.tensor):
        _float_plane(slope, shape, "%s: slope" % who)
        s_ptr, s = _f(slope, "slope"), 0.0
    else:
        s_ptr, s = None, _check.number(who, "slope", slope)
    h_ptr = _f(height, "height")
    out = silt.tensor(silt.float32, silt.shape(*shape), silt.gpu)
    ex = silt.tensor(silt.float32, silt.shape(*shape), silt.gpu) if excess else None
    _call("soil_slope_limit" + ("" if dims == 2 else "_batch"), out.c_ptr, None if ex is None else ex.c_ptr, h_ptr,
          s_ptr, s, *shape, *tail, e, _abi.stream())
    return (out, ex) if excess else out


def slope_limit(height, scale, slope, edge_=None, excess=False):
    """soil_slope_limit: the slope-limited surface of a (H, W) float32 DEM with the spacings (sx, sy) of `scale` — the
    greatest surface w <= height with w[n] <= w[k] + slope[n] * L_k for every neighbour k (`edge_`, d8 by default),
    L_k the length of the step.  `slope`: a finite number >= 0, or a float32 plane of the height's shape (an entry that
    is NaN or negative: no limit at that cell).  NaN heights are voids.  One definite bit pattern (soil_hip.h states
    the arithmetic).  Returns the new heights, or with `excess` the tuple (heights, excess), excess = height - heights:
    what stands above the threshold.  `height` is left as it is; synchronises the stream."""
    return _slope_limit("slope_limit", 2, height, scale, slope, edge_, excess)


def slope_limit_batch(height, scale, slope, edge_=None, excess=False):
    """`slope_limit` of each of the B models of a (B, H, W) tensor, side by side (soil_slope_limit_batch): launches
    that do not grow with B.  `scale` is one pair or B pairs; `slope` a number or a (B, H, W) float32 plane."""
    return _slope_limit("slope_limit_batch", 3, height, scale, slope, edge_, excess)


def slope_limit_info():
    """What this thread's last slope_limit / slope_limit_batch call did (soil_slope_limit_info): a dict with the
    relaxation `launches`, the `tiles` of a model, the `models` and the `looks` at the "changed" word."""
    return _call_info("soil_slope_limit_info", ("launches", "tiles", "models", "looks"))


# ---- exact multiple-flow accumulation (soil_hip.h: soil_mfd_weights, soil_mfd_accumulate): what the mean of
# multiflow's K random_weighted accumulations tends to, in one call; with `p` the MFD of Freeman, Quinn and Holmgren.

def _mfd_args(who, dims, height, edge_, T, p, scale, dist):
    """What both mfd calls check, before any device work: (shape, edge, kind, param, C scale arguments)."""
    shape = _shape(dims, height, "%s: height" % who)
    _float_plane(height, shape, "%s: height" % who)
    e = _check.edge(who, edge_)
    if (T is None) == (p is None):
        raise ValueError("%s: exactly one of T and p must be given" % who)
    if dist is not None:
        _int_plane(dist, shape, "%s: dist" % who)
    if T is not None:
        _check.number(who, "T", T, lo=None)
        if not valid_temperature(T):
            raise ValueError("%s: T must be 0 or a normal positive float32, got %r" % (who, T))
        pairs, tail = _scales(who, dims, scale, shape[0], none_ok=True)
        return shape, e, _abi.MFD_GIBBS, float(T), tail
    param = _check.number(who, "p", p)
    if param > 16:
        raise ValueError("%s: p must be a finite number in 0 .. 16, got %r" % (who, p))
    pairs, tail = _scales(who, dims, scale, shape[0])
    _positive(who, pairs, scale)
    return shape, e, _abi.MFD_POWER, param, tail


def _mfd_weights(who, dims, height, edge_, T, p, scale, dist):
    shape, e, kind, param, tail = _mfd_args(who, dims, height, edge_, T, p, scale, dist)
    h_ptr, d_ptr = _f(height, "height"), _opt_i(dist, "dist")
    K = 8 if e == d8 else 4
    out = silt.tensor(silt.float32, silt.shape(*(shape[:-2] + (K,) + shape[-2:])), silt.gpu)
    _call("soil_mfd_weights" + ("" if dims == 2 else "_batch"), out.c_ptr, h_ptr, d_ptr, kind, param, *shape, *tail, e,
          _abi.stream())
    return out


def _mfd_accumulate(who, dims, height, source, edge_, T, p, scale, dist, double):
    shape, e, kind, param, tail = _mfd_args(who, dims, height, edge_, T, p, scale, dist)
    if source is not None:
        _float_plane(source, shape, "%s: source" % who)
    h_ptr, s_ptr, d_ptr = _f(height, "height"), _opt_f(source, "source"), _opt_i(dist, "dist")
    out, ptrs = _out_pair(shape, double)
    _call("soil_mfd_accumulate" + ("" if dims == 2 else "_batch"), *ptrs, h_ptr, s_ptr, d_ptr, kind, param, *shape,
          *tail, e, _abi.stream())
    return out


def mfd_weights(height, edge_, T=None, p=None, scale=None, dist=None):
    """soil_mfd_weights: the K (4 or 8) outgoing multiple-flow shares of every cell of a (H, W) float32 DEM, a
    (K, H, W) float32 tensor in the neighbour table's order.  Exactly one of `T` and `p` is given.  `T`: the Gibbs
    shares random_weighted draws by at that temperature (soil.valid_temperature).  `p`: shares proportional to
    (drop / length) ** p, 0 <= p <= 16, with the spacings (sx, sy) of `scale`.  A cell whose partition sum is not
    finite and positive is a terminal: all shares 0.  `dist` (int32, soil.flat_distance): a flat cell with dist > 0
    sends share 1 to the neighbour flat_receivers picks.  Nothing synchronises."""
    return _mfd_weights("mfd_weights", 2, height, edge_, T, p, scale, dist)


def mfd_weights_batch(height, edge_, T=None, p=None, scale=None, dist=None):
    """`mfd_weights` of each of the B models of a (B, H, W) tensor (soil_mfd_weights_batch): (B, K, H, W); `scale` is
    one pair or B pairs."""
    return _mfd_weights("mfd_weights_batch", 3, height, edge_, T, p, scale, dist)


def mfd_accumulate(height, source, edge_, T=None, p=None, scale=None, dist=None, double=False):
    """soil_mfd_accumulate: the exact multiple-flow accumulation of `source` (a float32 plane, or None for ones) over a
    (H, W) float32 DEM: a[n] = source[n] + the sum over the donors d of share(d -> n) * a[d], the shares those of
    mfd_weights, the sums in fp64 in the neighbour table's order.  With `T` it is what the mean of multiflow's
    random_weighted accumulations tends to; with `p` the multiple-flow accumulation of Freeman, Quinn and Holmgren.  One
    definite bit pattern (soil_hip.h states the arithmetic).  Returns float32 (float64 with `double`); synchronises the
    stream."""
    return _mfd_accumulate("mfd_accumulate", 2, height, source, edge_, T, p, scale, dist, double)


def mfd_accumulate_batch(height, source, edge_, T=None, p=None, scale=None, dist=None, double=False):
    """`mfd_accumulate` of each of the B models of (B, H, W) planes, side by side (soil_mfd_accumulate_batch): launches
    that do not grow with B.  `scale` is one pair or B pairs."""
    return _mfd_accumulate("mfd_accumulate_batch", 3, height, source, edge_, T, p, scale, dist, double)


def mfd_info():
    """What this thread's last mfd_accumulate / mfd_accumulate_batch call did (soil_mfd_info): a dict with the
    relaxation `launches`, the `tiles` of a model, the `models` and the `looks` at the "changed" word."""
    return _call_info("soil_mfd_info", ("launches", "tiles", "models", "looks"))


# ---- the fill of a batch, and the conditioned drainage graph: fill -> steepest / random_weighted -> resolve_flats

def fill_depressions_batch(height, edge_=None):
    """fill_depressions of each of the B models of a (B, H, W) float32 tensor in one call
    (soil_fill_depressions_batch): all models on the same pyramid level at the same time, a launch grid of tiles x
    models, relaxation passes that do not grow with B.  Returns a new (B, H, W) tensor; synchronises the stream."""
    shape = _bhw(height, "fill_depressions_batch: height")
    e = _check.edge("fill_depressions_batch", d8 if edge_ is None else edge_)
    _float_plane(height, shape, "fill_depressions_batch: height")
    ptr = _f(height, "height")
    out = silt.tensor(silt.float32, silt.shape(*shape), silt.gpu)
    _call("soil_fill_depressions_batch", out.c_ptr, ptr, *shape, e, _abi.stream())
    return out


def fill_info():
    """What this thread's last fill_depressions / fill_depressions_batch call did (soil_fill_depressions_info): a dict
    with the relaxation `launches` (passes over the batch), the pyramid's `levels`, the `models`, the `looks` at the
    "changed" word and `per_level`, the launches of each level (0: the DEM itself)."""
    info = (C.c_int64 * 16)()
    _call("soil_fill_depressions_info", info)
    v = [int(x) for x in info]
    return {"launches": v[0], "levels": v[1], "models": v[2], "looks": v[3], "per_level": v[4:4 + min(v[1], 12)]}


def condition(height, edge_=None):
    """A (H, W) DEM made ready for routing: (filled, graph) with filled = fill_depressions(height, edge) and graph =
    resolve_flats(filled, edge), the steepest graph of the filled surface with its flats and lakes routed."""
    shape = _hw2(height, "condition: height")
    e = _check.edge("condition", d8 if edge_ is None else edge_)
    _float_plane(height, shape, "condition: height")
    filled = fill_depressions(height, e)
    return filled, resolve_flats(filled, e)


def condition_batch(height, edge_=None, graph=None):
    """`condition` of each of the B models of a (B, H, W) tensor.  `graph`: the receivers to complete instead of
    steepest_batch's — a caller who wants a random_weighted graph routed across the lakes makes it on the filled
    surface (fill_depressions_batch) and passes it here."""
    shape = _bhw(height, "condition_batch: height")
    e = _check.edge("condition_batch", d8 if edge_ is None else edge_)
    _float_plane(height, shape, "condition_batch: height")
    if graph is not None:
        _int_plane(graph, shape, "condition_batch: graph")
    filled = fill_depressions_batch(height, e)
    return filled, resolve_flats_batch(filled, e, graph)


def condition_breached(height, edge_=None):
    """A (H, W) DEM made ready for routing by carving instead of filling: (breached, graph) with graph that of
    condition(height, edge) and breached = breach(height, graph, edge), the ORIGINAL heights lowered along it.  No cell
    is raised: a lake drains through a cut in its rim, not over a surface that was added."""
    e = _check.edge("condition_breached", d8 if edge_ is None else edge_)
    _float_plane(height, _hw2(height, "condition_breached: height"), "condition_breached: height")
    _, graph = condition(height, e)
    return _breach("condition_breached", 2, height, graph, e, False), graph


def condition_breached_batch(height, edge_=None, graph=None):
    """`condition_breached` of each of the B models of a (B, H, W) tensor; `graph` as in condition_batch."""
    e = _check.edge("condition_breached_batch", d8 if edge_ is None else edge_)
    shape = _bhw(height, "condition_breached_batch: height")
    _float_plane(height, shape, "condition_breached_batch: height")
    if graph is not None:
        _int_plane(graph, shape, "condition_breached_batch: graph")
    _, routed = condition_batch(height, e, graph)
    return _breach("condition_breached_batch", 3, height, routed, e, False), routed


def multiflow(height, source, K, T, edge_=None, seed=0, first=0, stride=1, out=None):
    """Mean of `accumulate(random_weighted(height, edge, seed, k, T), source)` over the
    realisations k = first, first+stride, ... < K, each term divided by K in float32 and
    summed in float64 — the loop of example/dem_multiflow.py:43-49 kept on the GPU
    (soil_hip.h: soil_multiflow).  Returns (or adds into `out`) a float64 GPU tensor."""
    H, W = _hw(height)
    if out is None:
        out = silt.tensor(silt.float64, silt.shape(H, W), silt.gpu)
        _call("soil_set_f32", out.c_ptr, 0.0, 2 * H * W, _abi.stream())   # all-zero bits = 0.0
    e = d8 if edge_ is None else edge_
    _call("soil_multiflow", out.c_ptr, _f(height, "height"), _f(source, "source"), H, W, int(e),
          int(seed), int(first), int(stride), int(K), int(K), float(T), _abi.stream())
    return out


def gaussian_blur(tensor, sigma):
    """model.cpp:189-191 -> soil::gaussian_blur (filter.cu:72-91): blurs IN PLACE
    and returns its input handle (filter.cu:90)."""
    H, W = _hw(tensor)
    Cn = tensor.shape[2]
    scratch = silt.tensor(silt.float32, tensor.shape, silt.gpu)
    _call("soil_gaussian_blur", _f(tensor, "tensor"), scratch.c_ptr, H, W, Cn, float(sigma),
          _abi.stream())
    return tensor


def gradient(tensor, scale):
    """model.cpp:193-195 -> soil::gradient (grad.cu:89-97); returns (H, W, 2)."""
    H, W = _hw(tensor)
    out = silt.tensor(silt.float32, silt.shape(H, W, 2), silt.gpu)
    _call("soil_gradient", out.c_ptr, _f(tensor, "tensor"), H, W, _abi.vec(scale, 2),
          _abi.stream())
    return out


def laplacian(tensor, scale):
    """model.cpp:197-199 -> soil::laplacian (grad.cu:186-206); same shape as the input."""
    H, W = _hw(tensor)
    D = tensor.shape[2]
    out = silt.tensor(silt.float32, tensor.shape, silt.gpu)
    _call("soil_laplacian", out.c_ptr, _f(tensor, "tensor"), H, W, D, _abi.vec(scale, 2),
          _abi.stream())
    return out


def negslope(tensor, scale):
    """model.cpp:201-203 -> soil::negslope (grad.cu:133-141)."""
    H, W = _hw(tensor)
    out = silt.tensor(silt.float32, silt.shape(H, W), silt.gpu)
    _call("soil_negslope", out.c_ptr, _f(tensor, "tensor"), H, W, _abi.vec(scale, 2),
          _abi.stream())
    return out


def normal(tensor, scale=(1.0, 1.0, 1.0)):
    """soil::op::normal (op/normal.hpp:19-39; example/tiff_normal.py:14).  CPU
    tensors are processed on the host like in the reference, GPU tensors in HBM."""
    s = tensor.shape
    if s.dim() != 2:
        raise ValueError("normal map can not be computed for non 2D-indexed buffers")  # :22-23
    H, W = s[0], s[1]
    if tensor.host is silt.gpu:
        out = silt.tensor(silt.float32, silt.shape(H, W, 3), silt.gpu)
        _call("soil_normal", out.c_ptr, _f(tensor, "tensor"), H, W, _abi.vec(scale, 3),
              _abi.stream())
        return out
    src = np.ascontiguousarray(tensor.numpy(), dtype=np.float32)
    dst = np.empty((H, W, 3), np.float32)
    _call("soil_normal_host", dst.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p), H,
          W, _abi.vec(scale, 3))
    return silt.tensor._wrap_numpy(dst)


# ----------------------------------------------------------- solve_uniform

def solve_uniform(flow, source, decay, rng, scale, count):
    """model.cpp:209-227 -> soil::solve_uniform (path.cu:180-219)."""
    s = source.shape
    H, W, K = s[0], s[1], s[2]
    flux = silt.tensor(silt.float32, silt.shape(H, W, K), silt.gpu)
    _call("soil_solve_uniform", flux.c_ptr, _f(flow, "flow"), _f(source, "source"),
          _f(decay, "decay"), _gpu(rng, silt.rng, "rng"), rng.elem(), H, W, K, _abi.vec(scale, 2),
          int(count), _abi.stream())
    return flux


# ------------------------------------------------------------- erosion ops

def transport_fluvial(layers, rainfall, discharge, discharge_track, mass, mass_track, momentum,
                      momentum_track, albedo_bedrock, albedo_transport, albedo_surface, rng, scale,
                      param):
    """model.cpp:237-268 -> soil::transport_fluvial (erosion.cu:189-239)."""
    H, W = _hw(layers)
    _call("soil_transport_fluvial", _f(layers, "layers"), _f(rainfall, "rainfall"),
          _f(discharge, "discharge"), _f(discharge_track, "discharge_track"), _f(mass, "mass"),
          _f(mass_track, "mass_track"), _f(momentum, "momentum"),
          _f(momentum_track, "momentum_track"), _opt_f(albedo_bedrock, "albedo_bedrock"),
          _opt_f(albedo_transport, "albedo_transport"), _opt_f(albedo_surface, "albedo_surface"),
          _gpu(rng, silt.rng, "rng"), rng.elem(), H, W, _abi.vec(scale, 3), param._ref(),
          _abi.stream())


def transport_debris(layers, velocity, velocity_track, mass, mass_track, albedo_bedrock,
                     albedo_transport, albedo_surface, rng, scale, param):
    """model.cpp:270-295 -> soil::transport_debris (erosion.cu:395-436)."""
    H, W = _hw(layers)
    _call("soil_transport_debris", _f(layers, "layers"), _f(velocity, "velocity"),
          _f(velocity_track, "velocity_track"), _f(mass, "mass"), _f(mass_track, "mass_track"),
          _opt_f(albedo_bedrock, "albedo_bedrock"), _opt_f(albedo_transport, "albedo_transport"),
          _opt_f(albedo_surface, "albedo_surface"), _gpu(rng, silt.rng, "rng"), rng.elem(), H, W,
          _abi.vec(scale, 3), param._ref(), _abi.stream())


def mass_transfer(deltas, layers, uplift, discharge, mass, momentumFluvial, debris, momentumDebris,
                  albedo_bedrock, albedo_transport_fluvial, albedo_transport_debris,
                  albedo_surface, scale, param):
    """model.cpp:297-328 -> soil::mass_transfer (erosion.cu:576-611)."""
    H, W = _hw(uplift)
    _call("soil_mass_transfer", _f(deltas, "deltas"), _f(layers, "layers"), _f(uplift, "uplift"),
          _f(discharge, "discharge"), _f(mass, "mass"), _f(momentumFluvial, "momentumFluvial"),
          _f(debris, "debris"), _f(momentumDebris, "momentumDebris"),
          _opt_f(albedo_bedrock, "albedo_bedrock"),
          _opt_f(albedo_transport_fluvial, "albedo_transport_fluvial"),
          _opt_f(albedo_transport_debris, "albedo_transport_debris"),
          _opt_f(albedo_surface, "albedo_surface"), H, W, _abi.vec(scale, 3), param._ref(),
          _abi.stream())


def mass_creep(delta, layers, scale, param):
    """model.cpp:330-341 -> soil::mass_creep (erosion.cu:712-727)."""
    H, W = _hw(layers)
    _call("soil_mass_creep", _f(delta, "delta"), _f(layers, "layers"), H, W, _abi.vec(scale, 3),
          param._ref(), _abi.stream())


def particle_steps(reset=True):
    """Particle steps executed on the current GPU since the last reset (soil_hip.h:
    soil_particle_steps) — not in the reference; the numerator of Mparticle-steps/s."""
    n = C.c_uint64(0)
    _call("soil_particle_steps", C.byref(n), 1 if reset else 0, _abi.stream())
    return n.value


def particle_arith(mode=None):
    """Arithmetic of the particle step in the tiled launch shape (soil_hip.h: soil_set_particle_arith;
    not in the reference): "exact" — IEEE quotients, the oracle's walks step for step (default) — or
    "fast" — v_rcp_f32 quotients, statistical parity (tests/test_fast_particles.py).  Returns the mode
    in force; with an argument, sets it first."""
    names = {"exact": 0, "ieee": 0, 0: 0, "fast": 1, 1: 1}
    if mode is not None:
        if mode not in names:
            raise ValueError("particle_arith: 'exact' or 'fast'")
        _call("soil_set_particle_arith", names[mode])
    return "fast" if _abi.lib().soil_get_particle_arith() == 1 else "exact"


def debris_retire(mode=None):
    """What becomes of spent debris walkers in the tiled launch shape (soil_hip.h: soil_set_debris_retire; not
    in the reference): 1 / "on" (default) — a walker whose every further deposit is certain to be an exact
    zero ends its walk; 0 / "off" — every walker is walked to the end as the reference does (same flux planes);
    2 / "watch" — marked and walked on, deposits counted (debris_retire_violations).  Returns the mode in
    force (0, 1, 2); with an argument, sets it first."""
    names = {"off": 0, 0: 0, "on": 1, 1: 1, "watch": 2, 2: 2}
    if mode is not None:
        if mode not in names:
            raise ValueError("debris_retire: 'off', 'on' or 'watch'")
        _call("soil_set_debris_retire", names[mode])
    return _abi.lib().soil_get_debris_retire()


def debris_retire_violations(reset=True):
    """Deposits other than exact zeros made by walkers the watched mode had marked as spent (must be 0)."""
    n = C.c_uint64(0)
    _call("soil_debris_retire_violations", C.byref(n), 1 if reset else 0, _abi.stream())
    return n.value


def layer_merge(height, layers):
    """model.cpp:343-351 -> soil::layer_merge (erosion.cu:747-757)."""
    _call("soil_layer_merge", _f(height, "height"), _f(layers, "layers"), height.elem(),
          _abi.stream())


def albedo_layer(albedo, albedoBedrock, albedoSediment, layers, scaleSediment, shiftSediment):
    """model.cpp:353-369 -> soil::albedo_layer (erosion.cu:877-898)."""
    H, W = _hw(albedo)
    _call("soil_albedo_layer", _f(albedo, "albedo"), _f(albedoBedrock, "albedoBedrock"),
          _f(albedoSediment, "albedoSediment"), _f(layers, "layers"), H * W, float(scaleSediment),
          _abi.vec(shiftSediment, 3), _abi.stream())


def albedo_stratum(albedoBedrock, uplift, layers, scale, param, colorA, colorB, age, freq):
    """model.cpp:371-390 -> soil::albedo_stratum (erosion.cu:828-854)."""
    _call("soil_albedo_stratum", _f(albedoBedrock, "albedoBedrock"), _f(uplift, "uplift"),
          _f(layers, "layers"), uplift.elem(), _abi.vec(scale, 3), param._ref(),
          _abi.vec(colorA, 3), _abi.vec(colorB, 3), float(age), float(freq), _abi.stream())


def albedo_discharge(albedo, discharge, colorDischarge, extinction, scale):
    """model.cpp:393-407 -> soil::albedo_discharge (erosion.cu:900-919)."""
    H, W = _hw(albedo)
    _call("soil_albedo_discharge", _f(albedo, "albedo"), _f(discharge, "discharge"), H * W,
          _abi.vec(colorDischarge, 3), float(extinction), float(scale), _abi.stream())


# -------------------------------------------------------------------- noise

class noise_t:
    """soil::noise_param_t (noise.hpp:14-40), fields bound at model.cpp:413-420."""

    def __init__(self):
        self._c = _abi.NoiseParam()
        _abi.lib().soil_noise_param_default(C.byref(self._c))

    seed = property(lambda s: s._c.seed, lambda s, v: setattr(s._c, "seed", float(v)))
    gain = property(lambda s: s._c.gain, lambda s, v: setattr(s._c, "gain", float(v)))
    lacunarity = property(lambda s: s._c.lacunarity,
                          lambda s, v: setattr(s._c, "lacunarity", float(v)))
    octaves = property(lambda s: s._c.octaves, lambda s, v: setattr(s._c, "octaves", int(v)))
    frequency = property(lambda s: s._c.frequency,
                         lambda s, v: setattr(s._c, "frequency", float(v)))

    @property
    def ext(self):
        return [self._c.ext[0], self._c.ext[1]]

    @ext.setter
    def ext(self, v):
        self._c.ext[0], self._c.ext[1] = float(v[0]), float(v[1])


def noise(shape, param, host=silt.cpu):
    """model.cpp:421 -> soil::noise (noise.hpp:42-56): (H, W) float32 heightmap.
    The reference fills a CPU tensor; `host=silt.gpu` generates straight into HBM
    with the same bits."""
    if not isinstance(shape, silt.shape):
        shape = silt.shape(*shape)
    if shape.dim() != 2:
        raise ValueError("can't extract a full noise buffer from a non-2D index")  # noise.hpp:44-45
    H, W = shape[0], shape[1]
    if host is silt.gpu:
        out = silt.tensor(silt.float32, shape, silt.gpu)
        _call("soil_noise", out.c_ptr, H, W, C.byref(param._c), _abi.stream())
        return out
    dst = np.empty((H, W), np.float32)
    _call("soil_noise_host", dst.ctypes.data_as(C.c_void_p), H, W, C.byref(param._c))
    return silt.tensor._wrap_numpy(dst)


# -------------------------------------------------------------------- timer

s, ms, us, ns = "s", "ms", "us", "ns"  # soil::timer::duration, util.cpp:47-52
_UNIT = {"s": 1.0, "ms": 1e3, "us": 1e6, "ns": 1e9}


class timer:
    """soil::timer (util/timer.hpp:15-69; util.cpp:54-73): wall-clock context
    manager.  Like the reference it does NOT synchronise the device."""

    def __init__(self, duration=ms):
        self._unit = duration
        self._t0 = 0.0
        self.count = 0

    def __enter__(self):
        self._t0 = time.perf_counter()

    def __exit__(self, *exc):
        self.count = int((time.perf_counter() - self._t0) * _UNIT[self._unit])
        return False
