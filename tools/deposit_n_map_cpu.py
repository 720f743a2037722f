#!/usr/bin/env python
"""Where the iteration of soil_stream_power_deposit_n converges, on the CPU: the numpy restatement of
tests/deposit_n_ref.py (no GPU) on an H x H noise terrain x 100 with a basin pressed into it, conditioned for D8 by the
oracle — m = 0.5, dt = 50, uplift 0.01, scale (1, 1), deposition G / A — for K = 2e-3 and 0.2, n = 1, 1.5, 2, 3 and
G = 0.5, 1, 2, 4.  One line per case: the residual of every iteration up to --steps, and the defect of the nonlinear
equation at the last iterate with Qs re-summed in fp64.  DESIGN.md 3.5 "Erosion-deposition at slope exponents above 1"
quotes profiles/stream_power_deposit_n/map_cpu_48.txt, this script's output at its defaults.

    python tools/deposit_n_map_cpu.py [--size 48] [--steps 28]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import deposit_n_ref as dn  # noqa: E402
import flats_ref  # noqa: E402
from flow_paths_ref import D8  # noqa: E402
from oracle import pyoracle as o  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--steps", type=int, default=28)
    args = ap.parse_args()
    o.lib()
    H = W = args.size
    dem = (o.noise(H, W, seed=5.0, ext=(float(H), float(W))) * 100).astype(np.float32)
    dem[H // 3:2 * H // 3, W * 10 // 36:W * 24 // 36] -= np.float32(40.0)
    filled = o.fill_depressions(dem, D8)
    g = o.steepest(filled, D8)
    g = flats_ref.receivers(g, filled, flats_ref.distance_bfs(filled, D8), D8)
    area = o.accumulate(g, np.ones((H, W), np.float32), D8)
    u = np.full((H, W), 0.01, np.float32)
    span = float(filled.max() - filled.min())
    print("%d x %d, D8, heights spanning %g, %d terminals, 1e-9 of the range %.3g" % (H, W, span, (g < 0).sum(), 1e-9 * span))
    for K in (2e-3, 0.2):
        k = (K * area.astype(np.float64) ** 0.5).astype(np.float32)
        print("K = %g: K A^m dt / L %.3g in the median, %.3g at the most" % (K, np.median(k) * 50.0, k.max() * 50.0))
        for n in (1.0, 1.5, 2.0, 3.0):
            for G in (0.5, 1.0, 2.0, 4.0):
                d = (G / area.astype(np.float64)).astype(np.float32)
                r = dn.solve_iterated(o, g, D8, filled, k, d, (1.0, 1.0), 50.0, n, u, args.steps)
                miss, _ = dn.defect(r["out64"], g, D8, filled, k, d, (1.0, 1.0), 50.0, n, u)
                print("  n %g G %g: residuals %s | defect %.3g" % (n, G, " ".join("%.1e" % v for v in r["residuals"]), miss.max()))


if __name__ == "__main__":
    main()
