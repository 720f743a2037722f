"""The default debris mode — spent walkers end their walks (soil_set_debris_retire(1); csrc/
erosion_particles_tiled.hip: debris_spent, the spawn's own first step, the early exits of the round and tail
kernels) — against the oracle's restatement of the rule (oracle/soil_oracle.c: orc_debris_spent,
pyoracle.particles_debris_retire): in every launch shape the step count is the oracle's count under the rule (up to
the walkers whose attenuation underflows at the edge of the fp32 range: util.retired_steps_close), and the planes
are those of the oracle's full walk.  The session's mode (watched, tests/conftest.py) is set back
after every test; its violation count checks nothing in this mode — the equalities below do."""
import ctypes as C

import numpy as np
import pytest

from test_debris_retire import _same_planes, retire  # noqa: F401  (the fixture: the mode for one test)
from test_gpu_parity import particle_mode  # noqa: F401  (the fixture: every launch shape)
from util import product_param, retired_steps_close, rng_to_gpu, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu


def _oracle(oracle, layers, vel, N, scale, op, seed=(6, 0), dom=None, remote0=None):
    H, W = layers.shape[:2]
    mf, vf = np.zeros((H, W), np.float32), np.zeros((H, W, 2), np.float32)
    r = oracle.particles_debris_retire(mf, vf, None, oracle.rng_seed(N, *seed), layers, vel, None, scale,
                                       op, dom=dom, remote0=remote0)
    assert r["violations"] == 0 and r["lapses"] == 0, r
    r["mf"], r["vf"] = mf, vf
    return r


def _launch(hip, layers, vel, N, scale, pp, seed=(6, 0), dom=None, remote0=None):
    """soil_particles_debris_slab alone, through the C ABI (no colour planes: they switch the retirement off)."""
    from oracle import pyoracle
    from soillib_amd import _abi, soil
    H, W = layers.shape[:2]
    g = dict(mf=to_gpu(np.zeros((H, W), np.float32)), vf=to_gpu(np.zeros((H, W, 2), np.float32)))
    grng = rng_to_gpu(pyoracle.rng_seed(N, *seed)) if N else None
    lay, gv = to_gpu(layers), to_gpu(vel)
    grem = None if remote0 is None else to_gpu(remote0)
    dom = dom or _abi.Domain(H, W, 0, H, 0, H)
    soil.particle_steps(reset=True)
    _abi.check(hip.soil_particles_debris_slab(
        g["mf"].c_ptr, g["vf"].c_ptr, None, grng.c_ptr if grng is not None else None, N, lay.c_ptr, gv.c_ptr, None,
        grem.c_ptr if grem is not None else None, C.byref(dom), _abi.vec(scale, 3), pp._ref(), None))
    out = dict(steps=soil.particle_steps(reset=True), mf=to_np(g["mf"]), vf=to_np(g["vf"]))
    if grem is not None:
        out["rem"] = to_np(grem)
    return out


def _planes(got, want, what, rtol=2e-5):
    _same_planes(got["mf"], want["mf"], what + ": debris mass flux", rtol)
    _same_planes(got["vf"], want["vf"], what + ": debris velocity flux", rtol)


# ---- every launch shape ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,N", [(64, 64, 4096), (40, 96, 3000), (50, 33, 700), (136, 200, 20000)])
def test_every_launch_shape(hip, oracle, retire, particle_mode, H, W, N):  # noqa: F811
    """The grids and parameters of tests/test_gpu_parity.py::test_transport_debris_parity without the colour
    planes.  Tiled shapes: the oracle's steps under the rule, exactly; direct and staged do not retire: the full
    walk, exactly."""
    op = script_param(oracle.default_param())
    op.maxage = 128
    op.critSlopeBedrock = 0.05
    op.yieldStress = 0.001
    scale = (20.0 / H, 20.0 / W, 4.0)
    layers = terrain(oracle, H, W, sediment=0.01)
    vel = (np.random.default_rng(22).standard_normal((H, W, 2)) * 0.5).astype(np.float32)
    want = _oracle(oracle, layers, vel, N, scale, op)
    assert want["gate"] and want["rule_steps"] < want["steps"]
    retire("on")
    got = _launch(hip, layers, vel, N, scale, product_param(op))
    tiled = particle_mode.startswith("tiled")
    if tiled:
        assert retired_steps_close(got["steps"], want, N), (particle_mode, got["steps"], want)
    else:
        assert got["steps"] == want["steps"], (particle_mode, got["steps"], want)
    _planes(got, want, particle_mode)


# ---- the spawn's own first step -------------------------------------------------------------------------------

def _head_param(oracle, kind, maxage):
    op = script_param(oracle.default_param())
    op.maxage = maxage
    if kind == "spent late":
        # att_v = exp(-dL * tau / eps), dL * tau / eps < 60 per step: not zero after the first step, later
        op.bedShearDebris = 0.8e-10
        op.viscosityDebris = 0.0
    return op


@pytest.mark.parametrize("kind", ["spent at once", "spent late"])
@pytest.mark.parametrize("maxage", [0, 1, 2, 3, 33])
@pytest.mark.parametrize("N", [0, 1, 63, 5000])
def test_head_step(hip, oracle, retire, kind, maxage, N):
    """maxage 2: the spawn's step is the walker's only one (:306), round 0 takes none — the counts are equal;
    maxage 0 and 1: none at all.
    "spent at once": the example's parameters, the first step spends nearly everyone; "spent late": nobody is
    spent by it, the rounds retire them."""
    H, W = 64, 48
    scale = (20.0 / H, 20.0 / W, 4.0)
    layers = terrain(oracle, H, W, sediment=0.01)
    vel = (np.random.default_rng(7).standard_normal((H, W, 2)) * 0.5).astype(np.float32)
    op = _head_param(oracle, kind, maxage)
    want = _oracle(oracle, layers, vel, N, scale, op)
    assert want["gate"]
    if N and maxage >= 3:
        # the walkers left after the first step under the rule: fewer than half of them, or all of them
        one = _oracle(oracle, layers, vel, N, scale, _head_param(oracle, kind, 2))
        two = _oracle(oracle, layers, vel, N, scale, _head_param(oracle, kind, 3))
        on, full = two["rule_steps"] - one["rule_steps"], two["steps"] - one["steps"]
        assert full > 0 and (on * 2 < full if kind == "spent at once" else on == full), (kind, on, full)
        assert want["rule_steps"] < want["steps"] or (kind == "spent late" and maxage == 3)
    assert hip.soil_set_particle_mode(3) == 0
    try:
        retire("on")
        got = _launch(hip, layers, vel, N, scale, product_param(op))
    finally:
        hip.soil_set_particle_mode(0)
    if maxage <= 1 or N == 0:
        assert want["steps"] == 0
    if maxage == 2:
        assert want["rule_steps"] == want["steps"]
    assert retired_steps_close(got["steps"], want, N), (got["steps"], want)
    if maxage <= 2:
        assert got["steps"] == want["rule_steps"]             # the spawn's step alone: no attenuation has decayed yet
    _planes(got, want, "%s, maxage %d, N %d" % (kind, maxage, N))


def test_head_steps_on_row_slabs(hip, oracle, retire, particle_mode):  # noqa: F811
    """Three row slabs (ghost depth from soil_ghost_rows, remote0 for the NaN walkers) in the default mode: first
    steps that leave the slab's rows or the grid.  Each slab walks the oracle's steps under the rule on that slab;
    the slabs' planes add up to the whole grid's full walk."""
    from soillib_amd import _abi
    H, W, N = 96, 48, 6000
    op = script_param(oracle.default_param())
    op.maxage = 8
    op.critSlopeBedrock = 0.05
    pp = product_param(op)
    G = int(hip.soil_ghost_rows(pp._ref()))
    scale = (20.0 / H, 20.0 / W, 4.0)
    layers = terrain(oracle, H, W, sediment=0.01)
    vel = np.zeros((H, W, 2), np.float32)
    whole = _oracle(oracle, layers, vel, N, scale, op, seed=(2, 0))
    assert np.isnan(whole["mf"][0, 0])            # NaN walkers: the pits of the terrain
    retire("on")
    tiled = particle_mode.startswith("tiled")
    acc = dict(mf=np.zeros((H, W)), vf=np.zeros((H, W, 2)), rem=np.zeros(8))
    for o0, o1 in [(0, 32), (32, 64), (64, 96)]:
        x0, x1 = max(0, o0 - G), min(H, o1 + G)
        lay, v = np.ascontiguousarray(layers[x0:x1]), np.ascontiguousarray(vel[x0:x1])
        odom = oracle.domain(H, W, x0, x1 - x0, o0 - x0, o1 - x0)
        want = _oracle(oracle, lay, v, N, scale, op, seed=(2, 0), dom=odom, remote0=np.zeros(8, np.float32))
        assert want["gate"] and want["rule_steps"] < want["steps"]
        got = _launch(hip, lay, v, N, scale, pp, seed=(2, 0), dom=_abi.Domain(H, W, x0, x1 - x0, o0 - x0, o1 - x0),
                      remote0=np.zeros(8, np.float32))
        if tiled:
            assert retired_steps_close(got["steps"], want, N), (particle_mode, o0, got["steps"], want)
        else:
            assert got["steps"] == want["steps"], (particle_mode, o0, got["steps"], want)
        acc["mf"][x0:x1] += got["mf"]
        acc["vf"][x0:x1] += got["vf"]
        acc["rem"] += got["rem"]
    acc["mf"][0, 0] += acc["rem"][4]              # the owner of row 0 takes the parked NaN-walker deposits
    acc["vf"][0, 0] += acc["rem"][5:7]
    for k in ("mf", "vf"):
        np.testing.assert_allclose(acc[k], whole[k], rtol=2e-5, atol=2e-6 * (np.nanmax(np.abs(whole[k])) + 1e-30),
                                   err_msg=k)


# ---- fast arithmetic ------------------------------------------------------------------------------------------

def test_fast_arithmetic(hip, oracle, retire):
    """The FAST instances (advance<DEBRIS, true> in the spawn, step_apply_fast in the rounds) in the default mode:
    against the oracle statistically (the fast walk is chaotic in the last bit), never more steps than the full
    walk; against the fast mode's own full walk on the device, the same planes."""
    from test_fast_particles import TOL, _statistics
    H, W = 200, 168
    scale = (20.0 / H, 20.0 / W, 4.0)
    layers = terrain(oracle, H, W, sediment=0.01)
    op = script_param(oracle.default_param())
    op.maxage = 128
    op.critSlopeBedrock = 0.05
    op.yieldStress = 0.001
    N = H * W // 8
    vel = (np.random.default_rng(22).standard_normal((H, W, 2)) * 0.5).astype(np.float32)
    want = _oracle(oracle, layers, vel, N, scale, op)
    assert want["gate"] and want["rule_steps"] < want["steps"]
    pp = product_param(op)
    assert hip.soil_get_particle_arith() == 0
    assert hip.soil_set_particle_arith(1) == 0 and hip.soil_set_particle_mode(3) == 0
    try:
        out = {}
        for mode in ("off", "on"):
            retire(mode)
            out[mode] = _launch(hip, layers, vel, N, scale, pp)
    finally:
        hip.soil_set_particle_mode(0)
        assert hip.soil_set_particle_arith(0) == 0
    assert abs(out["off"]["steps"] - want["steps"]) <= TOL["steps_rel"] * want["steps"]
    assert out["on"]["steps"] < out["off"]["steps"]
    assert abs(out["on"]["steps"] - want["rule_steps"]) <= TOL["steps_rel"] * want["rule_steps"], (out["on"]["steps"], want)
    _statistics({"mf": out["on"]["mf"], "vf": out["on"]["vf"]}, want, ("mf",), "debris launch, fast, retired")
    _planes(out["on"], out["off"], "fast: retired against walked to the end")


# ---- whole steps ----------------------------------------------------------------------------------------------

def test_three_steps_at_1024(hip, oracle, retire):
    """tests/test_gpu_oracle_fullsize.py's three consecutive 1024^2 steps in the default mode: its step-count check
    then wants the oracle's count under the rule (util.debris_steps_agree)."""
    from test_gpu_oracle_fullsize import _run
    retire("on")
    _run(hip, oracle, 1024, 1024, steps=3)


# ---- the corners of the argument ------------------------------------------------------------------------------

# From tests/test_oracle_retire.py's sweep (32^2, 512 walkers, maxage 64): launches whose gate is open and where
# walkers are retired — cells of 1 to 1e10, z scales of 1e-30 to 1e19 (infinite deposits among them), a gravity of
# 1e18, nu and tau at the top of their range.  (nu, tau, cell, z scale, gravity, yieldStress)
CORNERS = [
    (0.004, 0.024, 1.0, 1.0, 1e18, 1e8),
    (0.004, 0.024, 1e10, 1e19, 9.81, 2e6),
    (0.004, 0.024, 1e10, 1e19, 1e18, 1e8),
    (1e30, 1e25, 1e-10, 1.0, 9.81, 2e6),
    (1e30, 1e25, 1e-10, 1e-30, 1e18, 2e6),
]
# ... and tests/test_oracle_retire.py's cliffs (gravity, nu, tau): the round-6 advice's hole — nu + tau / eps = 1e-9
# against g grad = 1e30 at the edge, which took spent walkers to an infinite speed and on as NaN walkers; the
# speed bound (debris_cell_bad) shuts its gate — and one whose gate stays open.
CLIFFS = [(1e12, 1e-9, 0.0), (1e8, 1e-9, 0.024)]


def _corner(oracle, corner):
    H = W = 32
    if corner[0] == "cliff":
        from test_oracle_retire import _cliff
        g, nu, tau = corner[1:]
        layers, vel, scale = _cliff(g, nu, tau)
        op = script_param(oracle.default_param())
        op.viscosityDebris, op.bedShearDebris, op.gravity, op.yieldStress = nu, tau, g, 1e7
        return layers, vel, scale, op
    nu, tau, L, zs, g, ty = corner
    layers = terrain(oracle, H, W, sediment=0.01)
    layers[..., 0] *= 8.0
    vel = (np.random.default_rng(1).standard_normal((H, W, 2)) * 0.5).astype(np.float32)
    op = script_param(oracle.default_param())
    op.viscosityDebris, op.bedShearDebris, op.gravity, op.yieldStress = nu, tau, g, ty
    return layers, vel, (L, L, zs), op


@pytest.mark.parametrize("corner", CORNERS + [("cliff",) + c for c in CLIFFS],
                         ids=[str(i) for i in range(len(CORNERS))] + ["cliff%d" % i for i in range(len(CLIFFS))])
def test_corners(hip, oracle, retire, corner):
    """Retired, watched and walked to the end on the device against the oracle: the steps, the planes (NaN cells
    included), and nothing counted in the watched mode."""
    from soillib_amd import soil
    N = 512
    layers, vel, scale, op = _corner(oracle, corner)
    op.maxage = 64
    want = _oracle(oracle, layers, vel, N, scale, op)
    if corner[:2] == ("cliff", 1e12):
        assert not want["gate"] and want["steps"] > 10 * N     # the speed bound shuts it; long NaN walks
    else:
        assert want["gate"] and want["rule_steps"] < want["steps"], want
    pp = product_param(op)
    assert hip.soil_set_particle_mode(3) == 0
    try:
        out = {}
        soil.debris_retire_violations(reset=True)
        for mode in ("off", "watch", "on"):
            retire(mode)
            out[mode] = _launch(hip, layers, vel, N, scale, pp)
        assert soil.debris_retire_violations(reset=True) == 0
    finally:
        hip.soil_set_particle_mode(0)
    assert out["off"]["steps"] == want["steps"] and out["watch"]["steps"] == want["steps"], (out["off"]["steps"], want)
    assert retired_steps_close(out["on"]["steps"], want, N), (out["on"]["steps"], want)
    for mode in ("off", "watch", "on"):
        _planes(out[mode], want, mode + " against the oracle", rtol=1e-4)
    _planes(out["on"], out["off"], "retired against walked to the end", rtol=1e-4)
