"""soil_fill_depressions_batch (soillib_amd/csrc/conditioning.hip) on the device: every slice of a batch against the
single call on that model and against the priority-flood oracle, under D4 and D8, without a tolerance (the rule of
tests/fill_ref.py: compare()); the launches per level against those of the single calls; what a batch can get wrong
and a single grid cannot — a model's apron, marks, changed word or coarse start taken from its neighbour in memory,
an offset in 32 bits, more models than a grid dimension holds; and the Python surface up to the conditioned drainage
of an ErosionBatch.

The launches are compared exactly.  That rests on this: on these DEMs the tile loop settles far below its cap of 256
inner iterations, so what a launch leaves in a tile is the tile's fixed point under its apron, whatever the order in
which the waves of the work-group ran, and a launch's result is one definite plane.  A model in a batch then moves
exactly as it moves alone, launch by launch."""
import numpy as np
import pytest

import fill_ref as ref
import flats_ref
from fill_ref import D4, D8
from util import assert_bit_equal, to_gpu, to_np

pytestmark = pytest.mark.gpu

EDGES = [D4, D8]
_SINGLE = {}


def _single(oracle, name, H, W, edge):
    """(the single call's surface, its launches per level) of model(name, H, W); checked against the oracle once."""
    from soillib_amd import soil
    key = (name, H, W, edge)
    if key not in _SINGLE:
        dem = ref.model(name, H, W)
        got = to_np(soil.fill_depressions(to_gpu(dem), edge))
        info = soil.fill_info()
        assert info["models"] == 1 and info["launches"] == sum(info["per_level"]) and len(info["per_level"]) == info["levels"]
        ref.compare(got, ref.want(oracle, name, H, W, edge), dem, "single call, %s" % name)
        got.setflags(write=False)
        _SINGLE[key] = (got, info["per_level"])
    return _SINGLE[key]


def _fill_batch(stack, edge):
    from soillib_amd import soil
    out = soil.fill_depressions_batch(to_gpu(np.ascontiguousarray(stack)), edge)
    assert tuple(out.shape) == stack.shape
    return to_np(out), soil.fill_info()


def _check_named_batch(oracle, names, H, W, edge):
    """The batch of the named models: every slice equals the single call and the oracle; launches as the singles'."""
    stack = np.stack([ref.model(n, H, W) for n in names])
    got, info = _fill_batch(stack, edge)
    singles = [_single(oracle, n, H, W, edge) for n in names]
    for b, n in enumerate(names):
        what = "model %d (%s) of %s at %dx%d edge %d" % (b, n, names, H, W, edge)
        ref.compare(got[b], singles[b][0], stack[b], what + " against the single call")
        ref.compare(got[b], ref.want(oracle, n, H, W, edge), stack[b], what + " against the oracle")
    per = [s[1] for s in singles]
    print("%s %dx%d edge %d: batch per level %s, singles %s" % (names, H, W, edge, info["per_level"], per))
    assert info["models"] == len(names) and info["levels"] == len(per[0])
    assert info["per_level"] == [max(p[l] for p in per) for l in range(info["levels"])]
    assert info["launches"] == sum(info["per_level"])
    if len(names) > 1:
        assert info["launches"] < sum(sum(p) for p in per)
    return got, info


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("H,W", [(65, 129), (130, 130)])
@pytest.mark.parametrize("B,where", [(1, "mid"), (3, "mid"), (3, "last"), (7, "mid"), (7, "last")])
def test_every_slice_equals_the_single_call_and_the_oracle(hip, oracle, B, where, H, W, edge):
    """Pitted models and constructions, an all-NaN and an all-+inf model among them, around the serpentine corridor
    (which needs some hundred launches where the others need three to nine).  65 x 129: one level, ragged tiles, an
    odd H W, so model 1 starts 4 bytes off every wider alignment; 130 x 130: two levels, 3 x 3 tiles, a 33 x 33 coarse
    plane."""
    names = ref.batch_names(B, B // 2 if where == "mid" else B - 1)
    assert names.count("serpentine") == 1 and (B < 3 or ("nan" in names and "inf" in names))
    _check_named_batch(oracle, names, H, W, edge)


@pytest.mark.parametrize("edge", EDGES)
def test_every_construction_in_one_batch(hip, oracle, edge):
    """63 x 65: all eight constructions side by side, the plane of zeros of both signs among them."""
    names = [n for n, _ in flats_ref.constructions(63, 65)]
    assert "signed zeros" in names
    _check_named_batch(oracle, names, 63, 65, edge)


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("H,W", [(1, 1), (1, 200), (3, 3)])
def test_degenerate_shapes(hip, oracle, H, W, edge):
    from soillib_amd import soil
    stack = np.stack([ref.small(H, W, s) for s in range(3)])
    if H == W == 3:
        stack[1] = np.float32([[7, 7, 7], [7, 1, 7], [7, 7, 7]])
    got, info = _fill_batch(stack, edge)
    assert info["models"] == 3 and info["levels"] == 1
    for b in range(3):
        assert_bit_equal(got[b], oracle.fill_depressions(stack[b], edge), "model %d against the oracle" % b)
        assert_bit_equal(got[b], to_np(soil.fill_depressions(to_gpu(stack[b]), edge)), "model %d against the single call" % b)
    if H == W == 3:
        assert got[1, 1, 1] == 7


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("H,W", [(65, 129), (130, 130)])
def test_nothing_crosses_a_model_boundary(hip, oracle, H, W, edge):
    """Model 1's bits stay when both its neighbours in memory are replaced by planes far below, far above, or NaN: an
    apron that reads past a model's last row, or marks or a start indexed without the model, would show."""
    mine = ref.model("pitted0", H, W)
    want, _ = _single(oracle, "pitted0", H, W, edge)
    for v in (-3e38, 3e38, np.nan):
        side = np.full((H, W), v, np.float32)
        got, info = _fill_batch(np.stack([side, mine, side]), edge)
        assert_bit_equal(got[1], want, "between planes of %r" % v)
        for b in (0, 2):
            assert_bit_equal(got[b], side, "a level plane is its own fill")
    # and between two other models that move
    got, _ = _fill_batch(np.stack([ref.model("pitted1", H, W), mine, ref.model("serpentine", H, W)]), edge)
    assert_bit_equal(got[1], want, "between pitted1 and the serpentine")


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("H,W,B", [(130, 130, 3), (516, 516, 2)])
def test_the_coarse_start_comes_from_the_own_model(hip, oracle, monkeypatch, H, W, B, edge):
    """Models 1000 b above one another, and 1000 b below: a start taken from a lower neighbour lies below the fixed
    point, which the iteration never repairs (a start from a higher one only costs launches) — hence both orders.
    516 x 516: three levels (129^2 > 16384).  And the batch without the coarse levels (SOIL_FILL_FLAT, read on every
    call) gives the same planes."""
    monkeypatch.delenv("SOIL_FILL_FLAT", raising=False)
    for sign in (1, -1):
        stack = np.stack([ref.used(H, W, b) + np.float32(sign * 1000.0 * b) for b in range(B)])
        got, info = _fill_batch(stack, edge)
        assert info["levels"] == (2 if H == 130 else 3) and info["models"] == B
        for b in range(B):
            assert_bit_equal(got[b], oracle.fill_depressions(stack[b], edge), "sign %d, model %d" % (sign, b))
        monkeypatch.setenv("SOIL_FILL_FLAT", "1")
        flat, flat_info = _fill_batch(stack, edge)
        monkeypatch.delenv("SOIL_FILL_FLAT")
        assert flat_info["levels"] == 1 and flat_info["per_level"] == [flat_info["launches"]]
        assert_bit_equal(got, flat, "the pyramid against the flat schedule, sign %d" % sign)


@pytest.mark.parametrize("edge", EDGES)
def test_only_the_last_model_still_moves(hip, oracle, edge):
    """Four level planes settle in the first look; the serpentine corridor behind them goes on alone, on its own marks,
    for exactly the launches it needs alone."""
    H, W = 65, 129
    stack = np.stack([flats_ref.level(H, W, float(v)) for v in (1, 2, 3, 4)] + [ref.model("serpentine", H, W)])
    got, info = _fill_batch(stack, edge)
    alone, per_level = _single(oracle, "serpentine", H, W, edge)
    assert_bit_equal(got[4], alone, "the serpentine")
    assert_bit_equal(got[:4], stack[:4], "the level planes")
    assert info["per_level"] == per_level and info["launches"] == sum(per_level) and info["launches"] > 30
    assert info["models"] == 5


@pytest.mark.parametrize("edge", EDGES)
def test_more_models_than_a_grid_dimension(hip, oracle, edge):
    """65537 models of 3 x 3 (every cell of a 2 x 3 model is on the border: nothing to fill), four patterns in turn,
    one of them a pit in the centre.  A grid's y extent ends at 65535."""
    from soillib_amd import soil
    B = 65537
    patterns = np.float32([[[7, 7, 7], [7, 1, 7], [7, 7, 7]],
                           [[5, 9, 5], [9, 2, 9], [4, 9, 5]],
                           [[1, 2, 3], [4, 5, 6], [7, 8, 9]],
                           [[3, 3, 3], [3, np.nan, 3], [3, 0, 3]]])
    single = [to_np(soil.fill_depressions(to_gpu(p), edge)) for p in patterns]
    for p, s in zip(patterns, single):
        assert_bit_equal(s, oracle.fill_depressions(p, edge), "a pattern alone")
    assert single[0][1, 1] == 7 and single[1][1, 1] == (9 if edge == D4 else 4)
    stack = patterns[np.arange(B) % 4]
    got, info = _fill_batch(stack, edge)
    assert info["models"] == B and info["levels"] == 1
    for k in range(4):
        mine = got[k::4]
        assert_bit_equal(mine, np.broadcast_to(single[k], mine.shape), "pattern %d" % k)


@pytest.mark.parametrize("edge", EDGES)
def test_model_offsets_beyond_two_to_the_31(hip, oracle, edge):
    """8067 models of 516 x 516 in one launch: the kernel's offsets of the last models pass element 2^31 of the DEM and
    of the surface (8.6 GB each), which 32 bits do not hold.  Level planes made on the device; a pitted model as the
    first, in the middle and as the last.  (With more models than a launch holds the host adds the chunk's offset, in
    int64 by its types, and the kernel's own part stays small: 127 074 models of 130 x 130 passed with kernel offsets
    cut to 31 bits, so this is the shape that bites.)"""
    import ctypes as C
    from soillib_amd import _abi, silt, soil
    H = W = 516
    B = 2 ** 31 // (H * W) + 2
    assert (B - 1) * H * W > 2 ** 31 and B <= 65535
    dem = np.ascontiguousarray(ref.model("pitted0", H, W))
    want, _ = _single(oracle, "pitted0", H, W, edge)
    hb = silt.tensor(silt.float32, silt.shape(B, H, W), silt.gpu)
    silt.set(hb, 5.0)
    per = H * W * 4
    at = (0, B // 2, B - 1)

    def view(t, b):
        return silt.tensor.from_device(t.ptr + b * per, silt.float32, silt.shape(H, W), keepalive=t)
    for b in at:
        _abi.check(hip.soil_memcpy_h2d(view(hb, b).c_ptr, dem.ctypes.data_as(C.c_void_p), dem.nbytes, _abi.stream()))
    _abi.check(hip.soil_stream_synchronize(_abi.stream()))
    out = soil.fill_depressions_batch(hb, edge)
    info = soil.fill_info()
    assert info["models"] == B and info["levels"] == 3
    for b in at:
        assert_bit_equal(to_np(view(out, b)), want, "model %d" % b)
    flat = out.view_torch().view(B, H * W)
    for lo, hi in ((1, B // 2), (B // 2 + 1, B - 1)):
        assert bool((flat[lo:hi] == 5.0).all()), "the level planes %d .. %d" % (lo, hi - 1)
    flat = out = hb = None
    silt.empty_cache()


# ---- the Python surface -----------------------------------------------------------------------------------------

def _batch_of(oracle, stack, seeds=None):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionBatch
    from util import product_param
    B, H, W = stack.shape
    bt = ErosionBatch(B, H, W, (20.0 / H, 20.0 / W, 4.0), product_param(oracle.default_param()), 64,
                      seeds or [11 + 7 * b for b in range(B)])
    silt.set(bt.height, to_gpu(stack))
    return bt


def test_the_python_surface(hip, oracle):
    from soillib_amd import silt, soil
    H, W = 65, 129
    stack = np.stack([ref.used(H, W, s) for s in (0, 1, 2)])
    d = to_gpu(stack)

    def is_plane(t, dtype, shape):
        return isinstance(t, silt.tensor) and t.type is dtype and tuple(t.shape) == shape and t.host is silt.gpu

    filled = soil.fill_depressions_batch(d)                                  # d8 by default
    assert is_plane(filled, silt.float32, (3, H, W)) and filled.ptr != d.ptr
    want = np.stack([oracle.fill_depressions(stack[b], D8) for b in range(3)])
    assert_bit_equal(to_np(filled), want, "fill_depressions_batch")
    assert_bit_equal(to_np(d), stack, "the input is left as it is")
    info = soil.fill_info()
    assert set(info) == {"launches", "levels", "models", "looks", "per_level"} and info["models"] == 3
    assert len(info["per_level"]) == info["levels"] == 1 and info["looks"] >= 1

    for edge in EDGES:
        f1, g1 = soil.condition(to_gpu(stack[0]), edge)
        assert is_plane(f1, silt.float32, (H, W)) and is_plane(g1, silt.int32, (H, W))
        fb, gb = soil.condition_batch(d, edge)
        assert is_plane(fb, silt.float32, (3, H, W)) and is_plane(gb, silt.int32, (3, H, W))
        assert_bit_equal(to_np(fb)[0], to_np(f1), "condition_batch against condition, the surface")
        assert_bit_equal(to_np(gb)[0], to_np(g1), "condition_batch against condition, the graph")
        assert_bit_equal(to_np(g1), to_np(soil.resolve_flats(f1, edge)), "condition's graph")
        assert not flats_ref.interior_terminals(to_np(g1)).any()
        rw = soil.random_weighted_batch(fb, edge, [5, 6, 7], 0, 0.5)
        _, gr = soil.condition_batch(d, edge, graph=rw)
        assert_bit_equal(to_np(gr), to_np(soil.resolve_flats_batch(fb, edge, rw)), "condition_batch with a graph")

    bt = _batch_of(oracle, stack)
    for edge in (None, soil.d4, soil.d8):
        e = D8 if edge is None else int(edge)
        f = bt.filled(edge)
        assert is_plane(f, silt.float32, (3, H, W))
        assert_bit_equal(to_np(f), to_np(soil.fill_depressions_batch(d, e)), "ErosionBatch.filled")
        f2, g = bt.conditioned(edge=edge)
        assert is_plane(f2, silt.float32, (3, H, W)) and is_plane(g, silt.int32, (3, H, W))
        assert_bit_equal(to_np(f2), to_np(f), "conditioned: the surface")
        assert_bit_equal(to_np(g), to_np(soil.resolve_flats_batch(f, e)), "conditioned: the steepest graph")
        f3, gr = bt.conditioned("random_weighted", edge=edge, T=0.25, offset=3)
        rw = soil.random_weighted_batch(f, e, bt.seeds, 3, 0.25)
        assert_bit_equal(to_np(gr), to_np(soil.resolve_flats_batch(f, e, rw)), "conditioned: random_weighted")
        assert (to_np(gr) != to_np(g)).any(), "the draw changes some receiver"
    with pytest.raises(ValueError, match="not indices"):
        bt.conditioned("direction")


def test_an_ensemble_drains_off_the_grid_once_conditioned(hip, oracle):
    """200 x 200, B = 3, pitted models as an ErosionBatch's heights: with the conditioned graph every cell drains to the
    border, where the unconditioned graph ends in interior pits."""
    from soillib_amd import soil
    B, H, W = 3, 200, 200
    stack = np.stack([ref.used(H, W, s) for s in range(B)])
    bt = _batch_of(oracle, stack)
    filled, g = bt.conditioned()
    basins, area = to_np(bt.basins(graph=g)), to_np(bt.drainage(graph=g))
    graph, filled_np = to_np(g), to_np(filled)
    assert (basins >= 0).all(), "no cell on a cycle"
    ones = to_gpu(np.ones((H, W), np.float32))
    for b in range(B):
        assert_bit_equal(filled_np[b], oracle.fill_depressions(stack[b], D8), "model %d: the surface" % b)
        terminal = graph[b] < 0
        assert terminal.any() and not flats_ref.interior_terminals(graph[b]).any(), "every terminal lies on the border"
        tx, ty = basins[b] // W, basins[b] % W
        assert ((tx == 0) | (tx == H - 1) | (ty == 0) | (ty == W - 1)).all()
        assert area[b][terminal].sum(dtype=np.float64) == H * W          # integers below 2^24: exact in float32
        one = soil.fill_depressions(to_gpu(stack[b]), soil.d8)
        g1 = soil.resolve_flats(one, soil.d8)
        assert_bit_equal(graph[b], to_np(g1), "model %d: the graph of the single-grid route" % b)
        assert_bit_equal(area[b], to_np(soil.accumulate(g1, ones, soil.d8)), "model %d: its accumulation" % b)
    raw = to_np(bt.flow())
    raw_basins = to_np(bt.basins())
    for b in range(B):
        pits = flats_ref.interior_terminals(raw[b])
        assert pits.sum() > 100, "the unconditioned models stop in interior pits"
        tx, ty = raw_basins[b] // W, raw_basins[b] % W
        assert not ((tx == 0) | (tx == H - 1) | (ty == 0) | (ty == W - 1)).all()
