"""Worker of tests/test_gpu_slab_colour.py::test_two_processes_share_one_gpu_over_gloo_with_colour: one rank
of a coloured SlabRunner world whose ranks are separate processes on the SAME GPU, talking through
torch.distributed's gloo backend (SOIL_DEVICE=0, SOIL_DIST_BACKEND=gloo)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def param(p, maxage):
    """The example's parameters with landslides on the noise terrain (debris colour flux that is not all zeros)."""
    from util import script_param
    script_param(p)
    p.maxage = maxage
    p.critSlopeBedrock = 0.05
    p.yieldStress = 0.001
    return p


def inputs(H, W, seed=5):
    """Noise bedrock (NaN walkers live on it), random per-cell colours: the global grid's, on every rank."""
    from soillib_amd import silt, soil
    from util import to_np
    npar = soil.noise_t()
    npar.seed = 3.0
    npar.ext = [H, W]
    layers = np.zeros((H, W, 2), np.float32)
    layers[..., 0] = to_np(soil.noise(silt.shape(H, W), npar, host=silt.gpu))
    r = np.random.default_rng(seed)
    return {"layers": layers,
            "albedo_bedrock": (r.random((H, W, 3)) * 1.3).astype(np.float32),
            "albedo_surface": (r.random((H, W, 3)) * 1.3).astype(np.float32)}


def main():
    out_dir, S, W, maxage, steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    from soillib_amd import parallel, soil
    r = parallel.SlabRunner(rows_per_rank=S, W=W, param=param(soil.param_t(), maxage), particles_div=8, seed=0,
                            init=False, colour=True)
    inp = inputs(r.H, W)
    rows = slice(r.x0, r.x0 + r.rows)
    r.set_plane("layers", inp["layers"][rows])
    r.set_plane("rainfall", np.ones((r.rows, W), np.float32))
    for name in ("albedo_bedrock", "albedo_surface"):
        r.set_plane(name, inp[name][rows])
    for _ in range(steps):
        r.step()
    r.sync()
    planes = {k: r.plane(k, owned=True) for k in ("layers", "waterHeight", "velocity", "debris", "albedo_surface",
                                                  "albedo_fluvial", "albedo_debris")}
    np.savez(os.path.join(out_dir, "rank%d.npz" % r.rank), **planes)
    assert r.max_over_ranks(float(r.rank)) == r.world - 1
    r.shutdown()


if __name__ == "__main__":
    main()
