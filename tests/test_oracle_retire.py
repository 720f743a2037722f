"""The argument behind the retirement of spent debris walkers (csrc/erosion_particles_tiled.hip, "spent debris
walkers"; include/soil_hip.h: soil_set_debris_retire), checked on the CPU oracle alone.  The oracle walks every
walker to the end as the reference does (erosion.cu:306-347) and, where its own gate says the launch allows it
(oracle/soil_oracle.c: orc_debris_retire_gate), counts the deposits that a walker makes after it first meets the
rule (orc_debris_spent) and that are not exact zeros.  The argument says there are none.  Here: the reference's
example parameters, seeded random parameter sets, and a sweep of the corners where the argument's finiteness
reasoning is thinnest."""
import itertools

import numpy as np
import pytest

from util import script_param, terrain


def _walk(oracle, layers, vel, N, scale, op, dom=None, remote0=None, seed=(6, 0)):
    """The rule-aware walk, and the plain entry point on the same inputs: the planes and the full count must be
    the same bit for bit (the rule only watches)."""
    H, W = layers.shape[:2]
    mf, vf = np.zeros((H, W), np.float32), np.zeros((H, W, 2), np.float32)
    r = oracle.particles_debris_retire(mf, vf, None, oracle.rng_seed(N, *seed), layers, vel, None, scale, op,
                                       dom=dom, remote0=remote0)
    mf0, vf0 = np.zeros((H, W), np.float32), np.zeros((H, W, 2), np.float32)
    rem0 = None if remote0 is None else np.zeros_like(remote0)
    steps = oracle.particles_debris(mf0, vf0, None, oracle.rng_seed(N, *seed), layers, vel, None, scale, op,
                                    dom=dom, remote0=rem0)
    assert r["steps"] == steps
    assert (mf.view(np.uint32) == mf0.view(np.uint32)).all() and (vf.view(np.uint32) == vf0.view(np.uint32)).all()
    assert r["gate"] == oracle.debris_retire_gate(layers, vel, scale, op, dom=dom)
    r["mf"], r["vf"] = mf, vf
    return r


def _check(r, what):
    assert 0 <= r["rule_steps"] <= r["steps"], what
    if r["gate"]:
        assert r["violations"] == 0, "%s: a spent walker added something: %s" % (what, r)
        assert r["lapses"] == 0, "%s: a spent walker stopped meeting the rule: %s" % (what, r)
    else:
        assert r["rule_steps"] == r["steps"] and r["violations"] == 0 and r["lapses"] == 0, what


@pytest.mark.parametrize("H,W", [(128, 128), (96, 160)])
def test_example_parameters(oracle, H, W):
    """example/erosion_gpu.py's parameters: the gate is open, walkers are spent within a few steps, and none of
    them adds anything afterwards."""
    op = script_param(oracle.default_param())
    op.maxage = 128
    scale = (20.0 / H, 20.0 / W, 4.0)
    layers = terrain(oracle, H, W, sediment=0.01)
    vel = (np.random.default_rng(5).standard_normal((H, W, 2)) * 0.5).astype(np.float32)
    r = _walk(oracle, layers, vel, H * W // 8, scale, op)
    assert r["gate"]
    _check(r, "example parameters")
    assert r["rule_steps"] < r["steps"] // 3


@pytest.mark.parametrize("seed", range(12))
def test_random_parameter_sets(oracle, seed):
    """The draws of tests/test_debris_retire.py::test_random_parameter_sets_watched, and more of them."""
    r = np.random.default_rng(100 + seed)
    op = script_param(oracle.default_param())
    op.maxage = int(r.integers(40, 200))
    op.critSlopeBedrock = float(r.choice([0.01, 0.2, 0.57, 2.0]))
    op.yieldStress = float(r.choice([0.0, 1e-6, 1e-3, 1.0, 2e6]))
    op.landslideRateDebris = float(r.choice([0.0, 0.0025, 0.5]))
    op.depositionRateDebris = float(r.choice([0.0, 1e-4, 0.1]))
    op.suspensionRateDebris = float(r.choice([0.0, 2.5e-4, 0.1]))
    op.viscosityDebris = float(r.choice([0.0, 0.004, 1.0]))
    op.bedShearDebris = float(r.choice([0.0, 0.024, 0.99]))
    H, W = int(r.integers(64, 200)), int(r.integers(64, 200))
    N = H * W // int(r.choice([2, 8]))
    zs = float(r.choice([0.5, 4.0, 40.0]))
    layers = terrain(oracle, H, W, sediment=float(r.choice([0.0, 0.01])), rng_seed=seed)
    vel = (r.standard_normal((H, W, 2)) * float(r.choice([0.0, 0.5, 5.0]))).astype(np.float32)
    _check(_walk(oracle, layers, vel, N, (20.0 / H, 20.0 / W, zs), op), "seed %d" % seed)


# The corners of the argument: a small decay nu + tau / eps (a spent walker's speed barely
# damped), cells from 1e-30 to 1e30 (lengths whose squares under- or overflow), z scales and a gravity that put
# g * grad near 1e19 and beyond, yield stresses that put tau_y / eps near FLT_MAX, and long walks.
CORNER_NU_TAU = [(0.0, 0.0), (0.0, 1e-30), (1e-30, 0.0), (0.0, 1e-24), (1e-30, 1e-24), (0.004, 0.024), (1e30, 1e25)]
CORNER_CELL = [1e-30, 1e-10, 1.0, 1e10, 1e18, 1e19, 1e30]
CORNER_Z = [1e-30, 1.0, 1e19, 1e30]
CORNER_G = [9.81, 1e18, 1e30]
CORNER_YIELD = [2e6, 1e8, 3e26]
CORNER_MAXAGE = [64, 4096]


@pytest.mark.parametrize("nu,tau", CORNER_NU_TAU)
def test_corner_sweep(oracle, nu, tau):
    H = W = 16
    layers = terrain(oracle, H, W, sediment=0.01)
    layers[..., 0] *= 8.0      # relief: grad = dh * z / cell
    vel = (np.random.default_rng(1).standard_normal((H, W, 2)) * 0.5).astype(np.float32)
    opened = retired = 0
    for L, zs, g, ty, maxage in itertools.product(CORNER_CELL, CORNER_Z, CORNER_G, CORNER_YIELD, CORNER_MAXAGE):
        op = script_param(oracle.default_param())
        op.viscosityDebris, op.bedShearDebris = nu, tau
        op.gravity, op.yieldStress, op.maxage = g, ty, maxage
        r = _walk(oracle, layers, vel, 64, (L, L, zs), op)
        _check(r, "nu %g tau %g cell %g z %g g %g tau_y %g maxage %d" % (nu, tau, L, zs, g, ty, maxage))
        opened += r["gate"]
        retired += r["rule_steps"] < r["steps"]
    if nu + tau / 1e-12 >= 1e-12:    # (below, the speed bound |record| <= 1e17 (nu + tau / eps) shuts every gate)
        assert opened > 0 and retired > 0    # the sweep does reach launches the product retires in


def _cliff(g, nu, tau):
    """A plateau of 1e14-sized cells, flat but for the velocity (nu vel = 1 along x), above a cliff of 1e22 (z scale
    1e10): a walker is spent by its first step on the plateau and carried to the edge, where the record is
    -(g grad) = g * 1e18."""
    H = W = 32
    layers = np.zeros((H, W, 2), np.float32)
    layers[:16, :, 0] = 1e22
    vel = np.zeros((H, W, 2), np.float32)
    vel[..., 0] = 1.0 / nu
    return layers, vel, (1e14, 1e14, 1e10)


# (gravity, nu, tau): the first is the round-6 advice's hole — nu + tau / eps = 1e-9 against g grad = 1e30 takes the
# speed of a spent walker to infinity (v_norm = inf / inf: a NaN walker) — the rest around it
CLIFFS = [(1e12, 1e-9, 0.0), (1e12, 1e-9, 1e-12), (1e8, 1e-9, 0.024), (1e12, 0.004, 0.024), (1e3, 1e-9, 0.0),
          (1e6, 1e-9, 1e-21), (1e10, 1.0, 0.0), (1e8, 0.004, 0.024), (1e2, 1e-9, 1e-3)]


@pytest.mark.parametrize("g,nu,tau", CLIFFS)
def test_cliff(oracle, g, nu, tau):
    """Spent walkers carried onto a steep edge: where the gate is open no spent walker ever stops meeting the rule
    (its speed stays under the bound the gate and the rule put on it); the advice's own case shuts the gate."""
    layers, vel, scale = _cliff(g, nu, tau)
    op = script_param(oracle.default_param())
    op.viscosityDebris, op.bedShearDebris, op.gravity, op.yieldStress, op.maxage = nu, tau, g, 1e7, 64
    r = _walk(oracle, layers, vel, 512, scale, op)
    _check(r, "cliff g %g nu %g tau %g" % (g, nu, tau))
    D = nu + tau / 1e-12
    A = g * 1e22 * 1e10 / 1e14          # the edge's record
    assert r["gate"] == (A <= 1e17 * D), r
    if (g, nu, tau) == CLIFFS[0]:
        assert not r["gate"] and r["rule_steps"] == r["steps"]
    if r["gate"]:
        assert r["rule_steps"] < r["steps"]


@pytest.mark.parametrize("case", ["nan cell", "inf cell", "negative viscosity", "huge bed shear",
                                  "no yield stress on a cliff", "infinite gravity"])
def test_gate(oracle, case):
    """The gate shuts where the argument does not hold (tests/test_debris_retire.py::
    test_guards_switch_the_retirement_off: the product walks every walker there); a NaN height is the reference's
    'outside the grid' and leaves every record finite: open."""
    H = W = 64
    op = script_param(oracle.default_param())
    op.maxage = 64
    layers = terrain(oracle, H, W, sediment=0.0)
    scale = (20.0 / H, 20.0 / W, 4.0)
    if case == "nan cell":
        layers[40, 31, 0] = np.nan
    elif case == "inf cell":
        layers[20, 50, 0] = np.inf
    elif case == "negative viscosity":
        op.viscosityDebris = -0.004
    elif case == "huge bed shear":
        op.bedShearDebris = 1e30
    elif case == "infinite gravity":
        op.gravity = np.inf
    else:
        op.yieldStress = 0.0
        layers[32:, :, 0] += 50.0
    vel = np.zeros((H, W, 2), np.float32)
    r = _walk(oracle, layers, vel, H * W // 4, scale, op)
    assert r["gate"] == (case == "nan cell"), case
    _check(r, case)
    if case == "nan cell":
        assert r["rule_steps"] < r["steps"]


@pytest.mark.parametrize("maxage", [0, 1, 2, 3, 33])
def test_head_step_edges(oracle, maxage):
    """maxage 0 and 1: nobody steps; 2: every walker's only step is its first, so the rule takes none away."""
    H, W = 48, 40
    op = script_param(oracle.default_param())
    op.maxage = maxage
    layers = terrain(oracle, H, W, sediment=0.01)
    vel = np.zeros((H, W, 2), np.float32)
    r = _walk(oracle, layers, vel, 2000, (20.0 / H, 20.0 / W, 4.0), op)
    assert r["gate"]
    _check(r, "maxage %d" % maxage)
    if maxage <= 1:
        assert r["steps"] == 0
    if maxage == 2:
        assert r["rule_steps"] == r["steps"] > 0
    if maxage >= 3:
        assert r["rule_steps"] < r["steps"]


def test_row_slabs(oracle):
    """Three row slabs, remote0 taking the NaN walkers' deposits: the gate is open on each slab and the
    rule takes away from each slab's walks the steps it takes away on the whole grid."""
    H, W, N = 96, 48, 6000
    op = script_param(oracle.default_param())
    op.maxage = 12
    op.critSlopeBedrock = 0.05
    scale = (20.0 / H, 20.0 / W, 4.0)
    layers = terrain(oracle, H, W, sediment=0.01)
    vel = np.zeros((H, W, 2), np.float32)
    whole = _walk(oracle, layers, vel, N, scale, op, seed=(2, 0))
    _check(whole, "whole grid")
    G = int(np.ceil(np.sqrt(2.0) * op.maxage)) + 2    # soil_ghost_rows: no walk leaves its slab's rows
    rule = steps = 0
    for o0, o1 in [(0, 32), (32, 64), (64, 96)]:
        x0, x1 = max(0, o0 - G), min(H, o1 + G)
        dom = oracle.domain(H, W, x0, x1 - x0, o0 - x0, o1 - x0)
        part = _walk(oracle, np.ascontiguousarray(layers[x0:x1]), np.ascontiguousarray(vel[x0:x1]), N, scale, op,
                     dom=dom, remote0=np.zeros(8, np.float32), seed=(2, 0))
        assert part["gate"]
        _check(part, "slab %d" % o0)
        rule += part["rule_steps"]
        steps += part["steps"]
    # a finite walker walks on its own slab exactly as on the whole grid; a NaN walker (never spent) parks its
    # deposit in remote0 on a slab that does not hold row 0 and walks on at cell (0, 0) on the whole grid:
    # the two counts differ by the same number of steps
    assert rule < steps
    assert whole["steps"] - steps == whole["rule_steps"] - rule
