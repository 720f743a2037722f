"""A numpy restatement of the erosion-deposition step at a slope exponent above 1 of include/soil_hip.h ("flow graphs:
erosion-deposition at slope exponents above 1": soil_stream_power_deposit_n), on top of tests/downstream_ref.py,
tests/deposit_ref.py (the q pass, the accumulation through the oracle, the rounds) and tests/power_n_ref.py (the planes,
the slope and the power).  Not a test module.

solve_iterated: the header's operations in numpy float64 in its order.  `pow` as in power_n_ref.solve_iterated: np.power
by default, the device's own function (soil_selftest_math64 op 0) for the comparison with the kernels, which must then
give these BITS for out, out64, flux and residual; None: no power at all, which is what n == 2 means.  n == 1 is
deposit_ref.solve_iterated and nothing else.

Returns a dict: out (float32), out64 (float64), flux (float32), residual (float64 scalar), final, `residuals`, and with
`every` also `steps`, what a call with iters = 1, 2, ... returns.

defect: the residual of the nonlinear equation itself at a surface, Qs summed in fp64."""
import numpy as np

import deposit_ref as dep
import downstream_ref as dref
import power_n_ref as pn
from flow_paths_ref import D4, D8  # noqa: F401


def coefficients(x, Qup, rc, L, kd, b, g, n, pow=np.power):
    """A and B of one iteration about the iterate x with the upstream sum Qup: the header's operations in its order."""
    n = np.float64(n)
    n1 = n - np.float64(1.0)
    with np.errstate(all="ignore"):
        d = x - x[rc]
        S = np.where(d <= 0, 0.0, d / L)                          # (a NaN d is not <= 0: d / L keeps it)
        if n == 2.0 or pow is None:
            assert n == 2.0, "without a power the exponent is 2"
            P = S
        else:
            P = np.asarray(pow(S, np.full_like(S, n1)), np.float64)
        F = ((n * kd) / L) * P
        c = (kd * n1) * (P * S)
        D = (1.0 + F) + g
        return ((((1.0 + g) * b) + (g * Qup)) + c) / D, F / D


def solve_iterated(oracle, graph, edge, height, erosivity, deposition, scale, dt, n, uplift=None, iters=8, pow=np.power,
                   every=False):
    if np.float64(n) == 1.0:
        return dep.solve_iterated(oracle, graph, edge, height, erosivity, deposition, scale, dt, uplift, iters, every)
    graph = np.ascontiguousarray(graph, np.int32)
    H, W = graph.shape
    is_edge, rc, L, h, kd, b = pn.planes(graph, edge, height, erosivity, scale, dt, uplift)
    g = dep._f64(deposition, H * W)
    _, out64, _ = dref.solve_doubling(graph, edge, scale=scale, power=(height, erosivity, uplift, dt))
    x = out64.reshape(-1).copy()
    flux_of = lambda x: oracle.accumulate(graph, dep.make_q(is_edge, b, x).reshape(H, W), edge)
    residuals, steps = [], []
    for j in range(1, iters + 1):
        q = dep.make_q(is_edge, b, x)
        Qs = oracle.accumulate(graph, q.reshape(H, W), edge).reshape(-1)
        with np.errstate(all="ignore"):
            Qup = Qs.astype(np.float64) - q.astype(np.float64)
        A, B = coefficients(x, Qup, rc, L, kd, b, g, n, pow)
        out, out64, final = dep._doubling(graph, is_edge, A, B, h)
        before, x = x, out64.reshape(-1).copy()
        residuals.append(dep._residual(x, before))
        if every and j < iters:
            steps.append(dict(out=out, out64=out64, flux=flux_of(x), residual=residuals[-1], final=final))
    flux = flux_of(x)
    result = dict(out=out, out64=out64, flux=flux, residual=residuals[-1], residuals=residuals, final=final)
    if every:
        result["steps"] = steps + [dict(out=out, out64=out64, flux=flux, residual=residuals[-1], final=final)]
    return result


def defect(x, graph, edge, height, erosivity, deposition, scale, dt, n, uplift=None):
    """|(x - b) + kd S^n - g (Qup + (b - x))| of every cell with an edge: the equation the iteration solves, S from x
    itself and Qup the upstream sum of b - x over the cells that drain into the cell, the cell left out, in fp64 (no
    float32 rounding of q or Qs).  Zeros on the terminals.  Returns the plane and the height range max(x) - min(x)."""
    graph = np.asarray(graph)
    H, W = graph.shape
    is_edge, rc, L, h, kd, b = pn.planes(graph, edge, height, erosivity, scale, dt, uplift)
    g = dep._f64(deposition, H * W)
    x = np.asarray(x, np.float64).reshape(-1)
    order, _ = pn.order_upward(graph, is_edge)
    q = np.where(is_edge, b - x, 0.0)
    total = q.copy()
    for i in reversed(order):
        if is_edge[i]:
            total[int(rc[i])] += total[i]
    with np.errstate(all="ignore"):
        d = x - x[rc]
        S = np.where(d <= 0, 0.0, d / L)
        miss = (x - b) + kd * np.power(S, np.float64(n)) - g * ((total - q) + (b - x))
    return np.where(is_edge, np.abs(miss), 0.0).reshape(H, W), np.nanmax(x) - np.nanmin(x)


def solve_batch(oracle, graph, edge, height, erosivity, deposition, scale, dt, n, uplift=None, iters=8, pow=np.power):
    """solve_iterated model by model on (B, H, W) planes; `scale`: one pair or B pairs."""
    graph = np.asarray(graph)
    pairs = np.asarray(scale, np.float32).reshape(-1, 2)
    outs = [solve_iterated(oracle, graph[i], edge, height[i], erosivity[i], deposition[i], pairs[i % len(pairs)], dt, n,
                           None if uplift is None else uplift[i], iters, pow) for i in range(graph.shape[0])]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in ("out", "out64", "flux", "residual", "final")}


same_words = dep.same_words
