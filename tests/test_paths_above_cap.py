"""The closed-form references of tests/paths_cap_ref.py, which the GPU tests above the engine's work-group cap
(tests/test_gpu_paths_above_cap.py) use at 4096^2, held to the restatements they replace: ref.walk_doubling and
ref.walk_serial for the walks, dref.solve_doubling for the sums, word for word.  Without a GPU.

  shapes   those of test_flow_paths_abi.py and (33, 260); D4 and D8
  graphs   serpentine (against ref.serpentine, entry by entry), comb, staircase
  walks    with and without a stop plane, with and without a scale; the formulas of the issue without a stop plane
  sums     with and without b, with and without a stop plane, a / t absent; the exactness condition itself
  layout   the restated ptr_layout: a segment holds a work-group's share of the cells, whatever the cap"""
import numpy as np
import pytest

import downstream_ref as dref
import flow_paths_ref as ref
import paths_cap_ref as cap
from flow_paths_ref import D4, D8

SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 4), (4, 3), (7, 9), (37, 53), (33, 260)]
SCALES = {"serpentine": (0.25, 2.0), "comb": (0.25, 2.0), "staircase": (3.0, 4.0)}   # sqrt(9 + 16) = 5: dd is exact
UNITS = {"serpentine": 0.25, "comb": 0.25, "staircase": 1.0}


def _stops(H, W):
    return [("none", None)] + ref.stop_planes(H, W)[1:] + [("drawn", cap.stop_plane(H, W, 3, 0.05))]


def test_the_serpentine_is_the_restatement_s():
    for H, W in SHAPES + [(6, 1), (1, 2), (2, 7)]:
        assert (cap.graph_of("serpentine", H, W)[0] == ref.serpentine(H, W)).all(), (H, W)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("name", cap.NAMES)
def test_the_closed_form_walks(name, H, W, edge):
    c = cap.Chains(name, H, W, edge)
    for sname, stop in _stops(H, W):
        for scale in (None, (0.25, 3.0), SCALES[name]):
            got = c.walk(scale, stop)
            ref.same_words(got, ref.walk_doubling(c.graph, edge, scale, stop), "%s %dx%d edge %d stop %s" % (name, H, W, edge, sname))
            if H * W <= 63:
                ref.same_words(got, ref.walk_serial(c.graph, edge, scale, stop), "%s %dx%d edge %d stop %s, serial" % (name, H, W, edge, sname))


@pytest.mark.parametrize("H,W", SHAPES)
def test_the_formulas_without_a_stop_plane(H, W):
    n = np.arange(H * W, dtype=np.int64).reshape(H, W)
    x, y = n // W, n % W
    t, s, l = cap.Chains("serpentine", H, W, D4).walk((0.25, 3.0))
    p = x * W + np.where(x % 2 == 0, y, W - 1 - y)
    steps = H * W - 1 - p
    assert (s == steps).all() and (t == n.reshape(-1)[np.argmax(p)]).all()
    assert (ref.words(l) == ref.words(ref.lengths(H - 1 - x, steps - (H - 1 - x), 0, (0.25, 3.0)))).all()
    t, s, l = cap.Chains("comb", H, W, D4).walk((0.25, 3.0))
    assert (s == y).all() and (t == x * W).all() and (ref.words(l) == ref.words(ref.lengths(0, y, 0, (0.25, 3.0)))).all()
    t, s, l = cap.Chains("staircase", H, W, D8).walk((0.25, 3.0))
    steps = np.minimum(H - 1 - x, W - 1 - y)
    assert (s == steps).all() and (t == n + steps * (W + 1)).all()
    assert (ref.words(l) == ref.words(ref.lengths(0, 0, steps, (0.25, 3.0)))).all()
    t, s, _ = cap.Chains("staircase", H, W, D4).walk()
    assert (s == 0).all() and (t == n).all(), "a diagonal is no edge under D4"


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("name", cap.NAMES)
def test_the_closed_form_sums(name, H, W, edge):
    c = cap.Chains(name, H, W, edge)
    a, b, t = cap.exact_planes(H, W, 5, cut=0.1)
    scale, unit = SCALES[name], UNITS[name]
    for sname, stop in _stops(H, W):
        for aa, bb, tt, sc in ((a, b, t, scale), (a, None, t, scale), (None, None, None, None), (None, b, t, None), (a, b, None, scale)):
            assert cap.exact(c.weights(aa, tt, sc, stop), unit if sc is not None else 1.0)
            want = dref.solve_doubling(c.graph, edge, aa, bb, tt, sc, stop)
            assert want[2].all() and not np.isnan(want[1]).any()
            dref.same_words(c.sums(aa, bb, tt, sc, stop), want, "%s %dx%d edge %d stop %s" % (name, H, W, edge, sname))
    if H * W >= 63 and (name != "staircase" or edge == D8):
        assert ((b.reshape(-1) == 0) & c.has_edge).any(), "no cell cuts its chain"


def test_the_exactness_condition_has_teeth():
    assert cap.exact([0.25, 2.0, 6.0, 0.0], 0.25) and not cap.exact([0.25, 0.3], 0.25)
    assert not cap.exact([2.0 ** 52, 2.0 ** 52], 1.0) and cap.exact([2.0 ** 52, 2.0 ** 51], 1.0)
    # the largest case of the GPU file: 4096^2 weights of at most 3 * 2.0, in units of 0.25
    assert 4096 * 4096 * 8 * 4 < 2 ** 53
    # a scale whose diagonal is not a multiple of the unit is refused
    c = cap.Chains("staircase", 4, 5, D8)
    assert not cap.exact(c.weights(None, None, (0.25, 2.0)), 0.25)


def test_every_iteration_of_one_run_is_the_run_of_that_many(oracle):
    """dep.solve_iterated(every=True), which the GPU file takes its iters = 1, 2, 3 references from in one run."""
    import deposit_ref as dep
    H, W = 13, 21
    r = np.random.default_rng(3)
    height = (ref.terrain(H, W, 2) * 10).astype(np.float32)
    planes = [height, r.uniform(1e-3, 10.0, (H, W)).astype(np.float32), r.uniform(0.0, 2.0, (H, W)).astype(np.float32)]
    uplift = (r.random((H, W)) * 0.01).astype(np.float32)
    for edge, graph in ((D8, ref.descent(height, D8)), (D4, ref.cycles(H, W))):
        steps = dep.solve_iterated(oracle, graph, edge, *planes, (0.3, 0.7), 10.0, uplift, 3, every=True)["steps"]
        assert len(steps) == 3
        for k in (1, 2, 3):
            dep.same_words(steps[k - 1], dep.solve_iterated(oracle, graph, edge, *planes, (0.3, 0.7), 10.0, uplift, k), "iters %d" % k)


@pytest.mark.parametrize("capg", [1, 3, 7, 64, cap.CAP])
def test_a_segment_holds_a_work_group_s_share(capg):
    """The dense round in front of the lists: work-group g takes the blocks g, g + groups, ...; its segment must hold
    256 entries a trip."""
    for elem in (1, 255, 256, 257, 1961, 8580, 9252, 42900, 256 * capg, 256 * capg + 1, 2 * 256 * capg + 9, 2106377, 16777216):
        L = cap.layout(elem, 8, capg)
        blocks = (elem + 255) // 256
        assert L["groups"] == min(blocks, capg) and L["seg"] % 256 == 0
        trips = (blocks + L["groups"] - 1) // L["groups"]         # of work-group 0, the most any makes
        assert L["seg"] == 256 * trips
        assert cap.above(elem, capg) == (trips > 1)
    assert cap.layout(4096 * 4096, 0)["seg"] == 2048 and cap.layout(1027 * 2051, 0)["seg"] == 512
    assert [cap.ceil_log2(v) for v in (1, 2, 3, 4, 5, 1 << 20, (1 << 20) + 1)] == [0, 1, 2, 2, 3, 20, 21]
