"""The constructions of tests/stencils_ref.py and the oracle they are compared against, without a GPU.

tests/test_gpu_stencils_hostile.py compares the stencil kernels with the oracle bit for bit on these planes, under
scales off and at the ends of the plain range.  That comparison says something only while the planes put values,
quotients and normal lengths on BOTH sides of every threshold that picks between a kernel's fast and written-out
form, while lerp5 takes each of its branches, and while most of what comes out is a number.  All of that is asserted
here, from numpy and the oracle alone:

  * every threshold class is populated on both sides — loaded values against 2^-54 and 2^48 (window.hpp:
    win_row_plain), quotients against 2^-60 and 2^90 (soil_math.hpp: QuotWatch), the normal's length against 2^40
    (k_normal4): at least 16 of each on grids of 1000 cells and more, at least one on the small ones that can hold one;
  * a -0 numerator occurs in `normal_planes` under z = -3, in a group of four that is away from the grid's edge;
  * each of the four branches of lerp5 and its final 0.0 is taken, along both axes;
  * the informative-output cap: every case the GPU file compares (stencils_ref.select) has an oracle output that is
    at most half NaN and has at least 1000 distinct words (half as many as cells on grids under 2000 cells) — or is one
    of the degenerate cases whose whole output is written down here: sigma 0 or NaN (all NaN), sigma inf (all +0), a z
    scale of +-0 (zeros of the sign the statements give them, and 1), a laplacian whose 1 / s / s overflows.  What
    breaks the cap is left out of both files; how many cases that is, is pinned per shape.
"""
import numpy as np
import pytest

import stencils_ref as R
from util import assert_bit_equal, bits

f32 = np.float32
BIG = 1000                       # cells from which a class wants 16 members


def _need(H, W):
    return 16 if H * W >= BIG else 1


def _families(oracle, H, W):
    return {"off": R.select(oracle, R.off_plain_cases(H, W)), "ends": R.select(oracle, R.ends_cases(H, W)),
            "normal": R.select(oracle, R.normal_cases(H, W)), "lap1": R.select(oracle, R.laplacian_cases(H, W, 1)),
            "lap2": R.select(oracle, R.laplacian_cases(H, W, 2))}


# (kept, left out) of each family of cases per shape: what the GPU file compares, and what the cap took away
CASE_COUNTS = {
    (37, 260): {'off': (206, 58), 'ends': (147, 33), 'normal': (37, 17), 'lap1': (3, 0), 'lap2': (3, 0)},
    (9, 1028): {'off': (206, 58), 'ends': (147, 33), 'normal': (37, 17), 'lap1': (3, 0), 'lap2': (3, 0)},
    (70, 264): {'off': (206, 58), 'ends': (147, 33), 'normal': (37, 17), 'lap1': (3, 0), 'lap2': (3, 0)},
    (5, 8): {'off': (189, 75), 'ends': (138, 42), 'normal': (36, 18), 'lap1': (3, 0), 'lap2': (3, 0)},
    (4, 4): {'off': (187, 77), 'ends': (136, 44), 'normal': (36, 18), 'lap1': (3, 0), 'lap2': (3, 0)},
    (2, 8): {'off': (196, 68), 'ends': (139, 41), 'normal': (37, 17), 'lap1': (3, 0), 'lap2': (3, 0)},
    (1, 4): {'off': (220, 44), 'ends': (173, 7), 'normal': (42, 12), 'lap1': (3, 0), 'lap2': (3, 0)},
    (37, 53): {'off': (194, 70), 'ends': (139, 41), 'normal': (37, 17), 'lap1': (3, 0), 'lap2': (3, 0)},
    (3, 5): {'off': (192, 72), 'ends': (139, 41), 'normal': (37, 17), 'lap1': (3, 0), 'lap2': (3, 0)},
    (1, 1): {'off': (240, 24), 'ends': (180, 0), 'normal': (42, 12), 'lap1': (3, 0), 'lap2': (3, 0)},
}


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_every_compared_case_is_informative_or_has_a_closed_form(oracle, H, W):
    fam = _families(oracle, H, W)
    counts = {k: (len(v[0]), len(v[1])) for k, v in fam.items()}
    print("case counts", (H, W), counts)
    assert counts == CASE_COUNTS[(H, W)], counts
    for kept, _ in fam.values():
        for name, op, plane, args, want in kept:
            share, distinct, need = R.informative(want)
            form = R.closed_form(name, op, plane, args)
            if form is not None:
                assert_bit_equal(want, form, name + ": the closed form")
            else:
                assert share <= 0.5 and distinct >= need, (name, share, distinct, need)
    # the written-out builds, the band builds and the fast form are all still asked for: scales off the plain range on
    # every operator, both ends in all four combinations, both z signs
    names = [c[0] for kept, _ in fam.values() for c in kept]
    for op in R.OPS3 + ("laplacian D=1", "laplacian D=2"):
        for s in R.SCALES_OFF_PLAIN[:4]:
            for way in ("x", "y") + (("both",) if H * W > 1 else ()):
                assert any(n.startswith(op) and n.endswith("%s = %s" % (way, R.name_of(s))) for n in names), (op, way, s)
    lo, hi = (R.name_of(s) for s in R.SCALES_AT_ENDS)
    for op in R.OPS3:
        for a in (lo, hi):
            for b in (lo, hi):
                assert any(n.startswith(op) and n.endswith("(%s, %s)" % (a, b)) for n in names), (op, a, b)
    for z in R.Z_SCALES[:6]:
        assert any(n.startswith("normal, flats") and n.endswith(", %s)" % R.name_of(z)) for n in names), z


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_every_threshold_is_populated_on_both_sides(oracle, H, W):
    need = _need(H, W)
    planes = R.threshold_planes(H, W)
    # loaded values against win_row_plain's range
    below, inside, above = (sum(c) for c in zip(*[R.classes(p, R.p2(-54), R.p2(48)) for p in planes.values()]))
    assert min(below, inside, above) >= need, (below, inside, above)
    mags = R.threshold_cells()
    if len(R.sites(H, W)) >= 12:
        for m in mags:                                      # ... and in the mixed plane, each magnitude itself
            assert (np.abs(planes["mixed"]) == m).any(), float(m)
        assert R.classes(planes["mixed"], R.p2(-54), R.p2(48))[1] >= H * W - len(R.sites(H, W))
    assert mags[1] < mags[2] == R.p2(-54) and mags[3] == R.p2(48) < mags[4]
    if H * W < 8:
        return
    # quotients against QuotWatch's range: the gradients the oracle stores, over the cases at the ends
    kept, _ = R.select(oracle, R.ends_cases(H, W))
    q = [R.classes(want, R.p2(-60), R.p2(90)) for name, op, plane, args, want in kept if op == "gradient"]
    below, inside, above = (sum(c) for c in zip(*q))
    assert min(below, inside, above) >= need, (below, inside, above)
    if H >= 3 and W >= 3:                                   # ... and the watched ones themselves, inside the grid
        for sc in R.end_pairs():
            c = [R.classes(R.central_quotients(p, sc), R.p2(-60), R.p2(90)) for p in R.quotient_planes(H, W, sc).values()]
            below, inside, above = (sum(v) for v in zip(*c))
            assert below >= 1 and inside >= 1, (sc, below, inside, above)
            if max(sc) < 1e6:                               # (2^90 x 2^40 is no float)
                assert above >= 1, (sc, below, inside, above)
    # the normal's length against 2^40, under each of the two scales
    for sc in (R.PLAIN, R.SCALES_AT_ENDS):
        lens = []
        for name, op, plane, args, want in R.select(oracle, R.normal_cases(H, W))[0]:
            if tuple(args[:2]) == tuple(sc) and args[2] in (3.0, -3.0):
                lens.append(R.normal(plane, args)[2])
        _, short, long_ = (sum(v) for v in zip(*[R.classes(l, f32(1), R.p2(40)) for l in lens]))
        assert short >= need and long_ >= need, (sc, short, long_)


def _away_from_the_edge(H, W):
    """The cells of groups of four that k_normal4 does not redo for the grid's edge alone."""
    m = np.zeros((H, W), bool)
    for y0 in range(0, W - W % 4, 4):
        if y0 >= 2 and y0 + 5 < W:
            m[2:max(2, H - 2), y0:y0 + 4] = True
    return m


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_normal_planes_hold_what_they_were_built_for(oracle, H, W):
    planes = R.normal_planes(H, W)
    again = R.normal_planes(H, W)
    for k in planes:
        assert_bit_equal(planes[k], again[k], k + " is deterministic")
    need = _need(H, W)
    # the numpy restatement is the oracle's operator, bit for bit
    for name, op, plane, args, want in R.select(oracle, R.normal_cases(H, W))[0]:
        assert_bit_equal(R.normal(plane, args)[0], want, name + ": numpy against the oracle")
    # a -0 numerator under z = -3
    inner = _away_from_the_edge(H, W)
    for sc in (R.PLAIN, R.SCALES_AT_ENDS):
        ax, ay = R.normal(planes["flats"], tuple(sc) + (-3.0,))[1]
        neg0 = (bits(ax) == 0x80000000) | (bits(ay) == 0x80000000)
        if H * W >= 8:
            assert neg0.sum() >= need, neg0.sum()
        if H * W >= BIG:
            assert (neg0 & inner).sum() >= need, "no -0 numerator away from the grid's edge"
            ax3, ay3 = R.normal(planes["flats"], tuple(sc) + (3.0,))[1]        # (differences of equal values are +0,
            assert not ((bits(ax3) == 0x80000000) & inner).any()              # of -0 as well: only z's sign makes a -0)
    # the flat patches: 5 x 5 or more, across columns 255 | 256 and a band boundary where the grid reaches them
    patches = R.flat_patches(H, W)
    if H * W >= BIG and W % 4 == 0:
        assert len(patches) == 3
        for x0, x1, y0, y1, v in patches:
            assert x1 - x0 >= 5 and y1 - y0 >= 5 and any(y0 < b < y1 for b in (256, 512, 768))
            assert any(b % (8 if H >= 28 else 4) == 0 for b in range(x0 + 1, x1)), "no band boundary inside the patch"
            assert (bits(planes["flats"][x0:x1, y0:y1]) == bits(np.array([v], f32))[0]).all()
        assert any(y0 < 256 < y1 for _, _, y0, y1, _ in patches)
    # lerp5: every branch along both axes
    if H * W >= BIG:
        for axis in (0, 1):
            taken = np.bincount(R.lerp5(planes["nonfinite"], axis)[1].ravel(), minlength=5)
            assert (taken >= 1).all(), (axis, taken)
            assert taken[0] >= H * W // 2
        bad = R.nonfinite_sites(H, W)
        for test in (np.isnan, np.isposinf, np.isneginf):
            at = {(x, y) for x, y, v in bad if test(v)}
            assert {x for x, y in at} >= ({0, 1, H - 2, H - 1} | ({6, 7, 8, 9} if H > 12 else set())), test.__name__
            assert {y for x, y in at} >= {0, 1, W - 2, W - 1}, test.__name__
            if W > 258:
                assert {y for x, y in at} >= {254, 255, 256, 257}, test.__name__
            assert any((x + 1, y) in at for x, y in at) and any((x, y + 1) in at for x, y in at), test.__name__
            assert any((x + 2, y) in at for x, y in at) and any((x, y + 2) in at for x, y in at), test.__name__


def test_the_degenerate_cases_have_the_outputs_written_down_here(oracle):
    H, W = 17, 15
    t = R.blur_planes(H, W, 2)["normal"]
    for sigma in (0.0, float("nan")):
        assert np.isnan(oracle.gaussian_blur(t, sigma)).all()
    assert (bits(oracle.gaussian_blur(t, float("inf"))) == 0).all(), "sigma inf: all +0"
    # z = +-0: the components are zeros, of the sign (lerp5 x z) / s gives, negated; the third is 1 — on every plane
    for pname, plane in R.normal_planes(37, 260).items():
        for z in (0.0, -0.0):
            want = oracle.normal(plane, R.PLAIN + (z,))
            assert (want[..., :2] == 0).all() and (want[..., 2] == 1).all(), pname
            assert_bit_equal(want, R.closed_form("", "normal", plane, R.PLAIN + (z,)), pname)
            neg = bits(want[..., 0]) == 0x80000000
            assert neg.any() and (~neg).any(), "both zeros occur"
    # a laplacian whose 1 / s / s overflows: no finite output away from ... anywhere, and numpy's restatement agrees
    t = R.lap_planes(37, 260, 2)
    for s in (float(f32(1e-40)), 0.0, -0.0):
        assert R.lap_overflows((s, 1.7))
        for sc in R.three_ways(s):
            want = oracle.laplacian(t, sc[1])
            assert not np.isfinite(want).any(), sc
            assert_bit_equal(want, R.laplacian(t, sc[1]), "laplacian over %r" % (sc,))
    assert not R.lap_overflows((R.SCALES_OFF_PLAIN[1], 1.7)) and not R.lap_overflows(R.SCALES_AT_ENDS)


@pytest.mark.parametrize("H,W", R.BLUR_SHAPES)
def test_the_blur_cases_are_informative(oracle, H, W):
    for C in (1, 2):
        kept, left_out = R.select(oracle, R.blur_cases(H, W, C))
        assert not left_out, left_out
        assert len(kept) == (19 if W >= 500 else 11)
        for name, op, plane, args, want in kept:
            form = R.closed_form(name, op, plane, args)
            if form is not None:
                assert_bit_equal(want, form, name)
                continue
            share, distinct, need = R.informative(want)
            assert share <= 0.5 and distinct >= need, (name, share, distinct, need)
            if "nonfinite" not in name:
                assert share == 0, name                  # no sigma of SIGMAS makes a NaN of finite cells
    planes = R.blur_planes(H, W, 1)
    if "nonfinite" in planes:
        bad = planes["nonfinite"][..., 0]
        for test in (np.isnan, np.isposinf, np.isneginf):
            xs, ys = np.nonzero(test(bad))
            assert len(xs) == 5, test.__name__
            assert (0 in ys or W - 1 in ys) and W // 2 in ys or 0 in ys and W // 4 in ys, "corner, mid-edge, interior"
            assert any(1024 - 16 <= y < 1024 for y in ys) or W < 1024, "within 16 cells of a segment's end"


def test_the_laplacian_restatement_is_the_oracles(oracle):
    for H, W in R.SHAPES:
        for D in (1, 2):
            for name, op, plane, args in R.laplacian_cases(H, W, D):
                want = oracle.laplacian(plane, args)
                assert_bit_equal(R.laplacian(plane, args), want, name)
                if D == 2 and H * W >= BIG:            # the channels differ: a mix-up would show
                    both = np.isfinite(want).all(-1)
                    assert both.mean() > 0.5 and (bits(want[..., 0]) != bits(want[..., 1]))[both].mean() > 0.99
