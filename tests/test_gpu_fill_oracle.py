"""soil_fill_depressions (soillib_amd/csrc/conditioning.hip) against the priority-flood oracle, bit for bit, on the
inputs its pyramid and its tile relaxation find hard: several coarse levels on ragged grids, integer DEMs with wide
flats, NoData through the coarsening (blocks partly and wholly NaN), infinite heights, lakes over many tiles with the
spill point on the far side, nested lakes, and corridors that carry a level across thousands of tile seams in series.

The operator is min/max only, so the surface is exact in fp32 whatever the update order; -0.0 is kept out of the
inputs (min/max do not order the two zeros)."""
import numpy as np
import pytest

from util import assert_bit_equal, to_gpu, to_np

pytestmark = pytest.mark.gpu

D4, D8 = 0, 1
WALL = np.float32(100.0)


# ------------------------------------------------------------------------------------------------ DEMs

def crater_dem(noise, k=1):
    """Integer heights round(40 noise) with a ring wall of 100 (radius 150 k, 4 thick, off-centre) notched down to 7
    on its north side only, a pit of -50 (radius 40 k) inside, NoData that the 4x4 coarsening meets in every way, and
    one cell each of +inf and -inf.  Returns the DEM and the places the tests look at."""
    H, W = noise.shape
    dem = np.round(noise * np.float32(40.0)) + np.float32(0.0)        # (+ 0: no -0.0)
    cx, cy, R = H // 2 - 8 * k, W // 2 + 9 * k, 150 * k
    x, y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rad = np.hypot(x - cx, y - cy)
    ring = (rad >= R - 2) & (rad < R + 2)
    dem[ring] = WALL
    dem[ring & (x < cx) & (np.abs(y - cy) <= 1)] = 7.0                # the notch: 3 wide, through the whole wall
    dem[np.hypot(x - cx - 60 * k, y - cy + 50 * k) < 40 * k] = -50.0   # the pit, far from the notch
    dem[13:31, 37:62] = np.nan                                         # not aligned to 4: blocks partly NaN
    bx = (H - 60) // 16 * 16
    dem[bx:bx + 16, 32:48] = np.nan                                    # a whole 16 x 16 block: -inf on two coarse levels
    dem[H - 1, W // 3] = np.nan                                        # on the rim
    where = {"pinf": (H - 40, W - 50), "ninf": (H - 30, W // 2), "inside": rad < R - 2,
             "pit": (cx + 60 * k, cy - 50 * k), "ring": ring}
    dem[where["pinf"]] = np.inf
    dem[where["ninf"]] = -np.inf
    assert not (np.signbit(dem) & (dem == 0)).any()
    return dem.astype(np.float32), where


def nested_dem(noise):
    """330 x 300.  An outer lake (wall 40, spill 30 on the east) that holds a terrace (wall 45, spill 38 on the west)
    with a walled pit in it (wall 60, spill 50 on the north, floor -10), and beside it a basin that the outer lake
    drowns (wall 25, spill 22 on the south, floor 5, pit -20).  Every spill lies in another 64-tile than its pit."""
    dem = np.round(noise * np.float32(3.0)) + np.float32(10.0)

    def box(x0, x1, y0, y1, wall, floor):
        dem[x0:x1, y0:y1] = wall
        dem[x0 + 3:x1 - 3, y0 + 3:y1 - 3] = floor
    box(20, 310, 20, 280, 40, 20)
    dem[150:153, 277:280] = 30           # east
    box(40, 200, 40, 180, 45, 24)
    dem[60:63, 40:43] = 38               # west
    box(100, 180, 90, 160, 60, -10)
    dem[100:103, 150:153] = 50           # north
    box(220, 300, 60, 260, 25, 5)
    dem[297:300, 70:73] = 22             # south
    dem[240:250, 200:220] = -20
    return dem.astype(np.float32)


def serpentine_dem(H, W, slope=0):
    """Walls of 100, a corridor one cell wide on every other row, joined at alternate ends inside the rim columns,
    with one exit on the rim at (1, 0): a single path through all H/2 rows.  slope = +1: the floor rises by one per
    row going inwards (nothing to fill), -1: it falls (one long lake at the exit's level), 0: level."""
    dem = np.full((H, W), WALL, np.float32)
    rows = list(range(1, H - 1, 2))
    for i, r in enumerate(rows):
        dem[r, 1:W - 1] = slope * (i - len(rows)) if slope > 0 else slope * i
        if r + 2 < H - 1:
            dem[r + 1, W - 2 if i % 2 == 0 else 1] = dem[r, 1]
    dem[1, 0] = dem[1, 1]
    dem += np.float32(0.0)
    corridor = dem != WALL
    return dem, corridor


# --------------------------------------------------------------------------------------------- comparisons

_NOISE = {}


def _noise(oracle, H, W):
    if (H, W) not in _NOISE:
        _NOISE[H, W] = oracle.noise(H, W, seed=4.0, ext=(float(H), float(W)))
    return _NOISE[H, W]


def _equal_the_oracle(oracle, dem, edges=(D4, D8), what="fill"):
    from soillib_amd import soil
    d = to_gpu(dem)
    out = {}
    for edge in edges:
        want = oracle.fill_depressions(dem, edge)
        got = to_np(soil.fill_depressions(d, edge))
        assert_bit_equal(got, want, "%s, %s" % (what, "D8" if edge else "D4"))
        out[edge] = want
    return out


@pytest.mark.parametrize("H,W", [(517, 523), (700, 389)])
def test_two_coarse_levels_ragged(hip, oracle, H, W):
    """517 x 523 -> 130 x 131 (17030 cells, above the 16384 at which a level is added) -> 33 x 33."""
    assert -(-H // 4) * -(-W // 4) > 16384
    dem, at = crater_dem(_noise(oracle, H, W))
    want = _equal_the_oracle(oracle, dem)
    for edge in (D4, D8):
        w = want[edge]
        ok = np.isfinite(dem)
        raised = (w[ok] > dem[ok]).mean()
        assert 0.2 < raised < 0.5, raised                              # the crater and the flats' pits
        assert w[at["pit"]] == 7.0 and (w[at["inside"] & ok] >= 7.0).all()   # the lake stands at the notch
        assert ((w == 7.0) & at["inside"]).sum() > 12 * 64 * 64               # one level over more than 12 tiles' worth
        assert w[at["pinf"]] == np.inf and np.isnan(w[np.isnan(dem)]).all()
        x, y = at["ninf"]
        nb = [w[x - 1, y], w[x + 1, y], w[x, y - 1], w[x, y + 1]]
        if edge == D8:
            nb += [w[x - 1, y - 1], w[x - 1, y + 1], w[x + 1, y - 1], w[x + 1, y + 1]]
        assert w[x, y] == min(nb) and np.isfinite(w[x, y])             # -inf comes up to its lowest neighbour


def test_three_coarse_levels_d4(hip, oracle):
    """2049 x 2056 -> 513 x 514 -> 129 x 129 (16641 cells) -> 33 x 33.  D4 (D8 at 4096^2: tests/test_gpu_fullsize.py)."""
    from soillib_amd import silt, soil
    H, W = 2049, 2056
    p = soil.noise_t()
    p.seed = 4.0
    p.ext = [H, W]
    dem, at = crater_dem(to_np(soil.noise(silt.shape(H, W), p, host=silt.gpu)), k=4)
    want = _equal_the_oracle(oracle, dem, edges=(D4,))[D4]
    assert want[at["pit"]] == 7.0


def test_pyramid_against_flat(hip, oracle, monkeypatch):
    """SOIL_FILL_FLAT (read on every call) leaves the coarse levels out: the same surface."""
    from soillib_amd import soil
    dem, _ = crater_dem(_noise(oracle, 517, 523))
    d = to_gpu(dem)
    for edge in (D4, D8):
        want = oracle.fill_depressions(dem, edge)
        monkeypatch.delenv("SOIL_FILL_FLAT", raising=False)
        pyramid = to_np(soil.fill_depressions(d, edge))
        monkeypatch.setenv("SOIL_FILL_FLAT", "1")
        flat = to_np(soil.fill_depressions(d, edge))
        monkeypatch.delenv("SOIL_FILL_FLAT")
        assert_bit_equal(flat, want, "flat")
        assert_bit_equal(pyramid, flat, "pyramid against flat")


def test_nested_depressions(hip, oracle):
    dem = nested_dem(_noise(oracle, 330, 300))
    want = _equal_the_oracle(oracle, dem)
    for w in want.values():
        assert w[260, 100] == 30 and w[245, 210] == 30      # the drowned basin and its pit: the outer lake's level
        assert w[50, 200] == 30                              # the outer lake's own floor
        assert w[70, 100] == 38 and w[140, 120] == 50        # the terrace, and the pit on it


@pytest.mark.parametrize("slope", [0, 1, -1], ids=["level", "rising", "falling"])
def test_serpentine_corridor(hip, oracle, slope):
    H, W = 517, 523
    dem, corridor = serpentine_dem(H, W, slope)
    want = _equal_the_oracle(oracle, dem)
    for w in want.values():
        assert (w[~corridor] == WALL).all()
        if slope > 0:
            assert (w == dem).all()
        else:
            assert (w[corridor] == 0).all()


def test_serpentine_across_twelve_thousand_seams(hip, oracle):
    """1280 x 1280: 639 corridor rows of 20 tiles each, about 12 000 tile seams in series, and a launch carries a
    level across one seam (12 165 launches on the fine level, measured).  A cap of 4 (tiles_w + tiles_h) 64 + 16 =
    10 256 launches per level refused this legal DEM ("did not converge"); the cap now follows from the number of
    tiles and is a bound (conditioning.hip: fill_level)."""
    dem, corridor = serpentine_dem(1280, 1280)
    want = _equal_the_oracle(oracle, dem, edges=(D4,))[D4]
    assert (want[corridor] == 0).all() and (want[~corridor] == WALL).all()
