"""Order statistics across the models of a batch (include/soil_hip.h, "erosion: summaries":
soil_erode_batch_quantiles, soil_erode_batch_exceedance; ErosionBatch.quantiles, order_statistics, median,
exceedance) against the contract restated in numpy here; the oracle has no such reductions.

  1. known answers by construction: every cell-channel holds a permutation of 0 .. B-1;
  2. hostile bits: random uint32 patterns as floats (NaN payloads of both signs, infinities, denormals, both zeros),
     every rank and fractional positions, on every path the B allows (SOIL_QUANTILE_PATH);
  3. invariance: the models permuted, or embedded off an aligned boundary in a larger allocation;
  4. other request shapes: nq = 1, 16, 17, duplicated and unsorted q, another stream, a poisoned cell;
  5. after real steps, against numpy over model_planes(b);
  6. the exceedance maps;
  7. refused arguments, a forced path at a B it cannot hold, a row slab.

Every comparison is of bit patterns (`view(uint32)`), none is a tolerance: the contract fixes the order (an integer
key), the two order statistics and three fp64 operations.  One exception, and it is not a tolerance either: where
the interpolation ITSELF yields NaN (-inf next to a finite value, a NaN model next to a finite one) the result must
be a NaN, but IEEE 754 leaves the sign and payload of a NaN an operation generates to the implementation (x86
generates the negative "indefinite" quiet NaN; another fp64 unit need not), so there the bits are not compared.  An order statistic that IS a NaN (frac == 0) is 0x7FC00000 on both sides and is compared.

The restatement was checked on the CPU: it agrees with np.sort on finite data, lies within one fp32 ulp of
np.quantile, and orders [-inf, -1e-45, -0, +0, 1e-45, inf, inf, nan, nan] as the header states
(test_the_restatement_itself)."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_erosion_batch import _batch, _inputs, _param
from test_gpu_erosion_stats import _filled
from util import to_np

pytestmark = pytest.mark.gpu

READ = ("layers", "waterHeight", "mass", "debris")
RAGGED = [(1, 1), (5, 1), (1, 8), (37, 53)]
# either side of every width of a network (4, 8, 16, 32, 64, 128, 256), which include the paths' largest B and
# that plus one (64 | 65, 256 | 257) and where the entry changes path unforced (16 | 17, 256 | 257)
B_LIST = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
CASES = [(size, B) for size in RAGGED for B in B_LIST] + [((1, 8), 4099)] + [((256, 256), B) for B in B_LIST if B <= 64]
PATH_MAX = {"reg": 64, "lds": 256, "bisect": None}


def _case_id(case):
    return "%dx%d-B%d" % (case[0] + (case[1],))


# ---------------------------------------------------------------- the contract in numpy

def _keys(x):
    u = np.ascontiguousarray(x).view(np.uint32).copy()
    u[(u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0x7FC00000)
    return np.where(u >> np.uint32(31) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unkey(k):
    return np.where(k >> np.uint32(31) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)


def _channels(host):
    """(B, H, W, 6) float32: the six channels of every model; height is the fp32 sum."""
    l = host["layers"]
    with np.errstate(invalid="ignore", over="ignore"):
        height = l[..., 0] + l[..., 1]
    return np.stack([l[..., 0], l[..., 1], height, host["waterHeight"], host["mass"], host["debris"]], axis=-1)


def _sorted_bits(vals):
    """(B, ...) uint32: per trailing index the B bit patterns in the order of the keys."""
    B = vals.shape[0]
    k = np.ascontiguousarray(_keys(vals).reshape(B, -1).T)
    k.sort(axis=1)
    return _unkey(np.ascontiguousarray(k.T)).reshape(vals.shape)


def _at(s, B, pos):
    """(bits, generated): the contract's value at fractional rank `pos` from the sorted bit patterns `s`, and where
    the interpolation itself yielded NaN."""
    lo = math.floor(pos)
    frac = pos - lo
    ua = s[lo]
    a, b = ua.view(np.float32), s[min(lo + 1, B - 1)].view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b.astype(np.float64) - a.astype(np.float64)
        p = np.float64(frac) * d
        r = (a.astype(np.float64) + p).astype(np.float32)
        keep = (a == b) | (frac == 0)
    return np.where(keep, ua, r.view(np.uint32)), ~keep & np.isnan(r)


def _expected(vals, pos):
    s = _sorted_bits(vals)
    got = [_at(s, vals.shape[0], p) for p in pos]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def _assert_bits(got, want, generated, what):
    got = np.ascontiguousarray(got).view(np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got != want) & ~generated
    assert not bad.any(), "%s: %d of %d differ, first at %s: %08x, expected %08x" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0].tolist(), got[tuple(np.argwhere(bad)[0])],
        want[tuple(np.argwhere(bad)[0])])
    assert np.isnan(got.view(np.float32)[generated]).all(), what + ": a NaN of the interpolation is not a NaN"


def _fractions(B):
    """Fractional positions across the range, the ends and the last interval among them."""
    top = float(B - 1)
    return sorted({0.0, top, top / 2, top / 3, top * 0.1, top * 0.9, max(top - 0.25, 0.0), min(0.5, top)})


def test_the_restatement_itself():
    r = np.random.default_rng(0)
    x = r.standard_normal((33, 50)).astype(np.float32)
    s = _sorted_bits(x)
    assert np.array_equal(s.view(np.float32), np.sort(x, axis=0))
    for q in (0.0, 0.1, 0.5, 0.77, 1.0):
        got = _at(s, 33, q * 32)[0].view(np.float32)
        want = np.quantile(x.astype(np.float64), q, axis=0)
        assert (np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    odd = np.array([np.nan, np.inf, 0.0, -1e-45, -np.inf, -0.0, 1e-45, np.inf, -np.nan], np.float32)
    want = np.array([-np.inf, -1e-45, -0.0, 0.0, 1e-45, np.inf, np.inf, np.nan, np.nan], np.float32)
    got = _sorted_bits(odd.reshape(9, 1)).reshape(9)
    assert np.array_equal(got[:7], want[:7].view(np.uint32)) and (got[7:] == 0x7FC00000).all()


# ---------------------------------------------------------------- data

def _permutations(B, H, W, seed):
    """Every cell of waterHeight, mass, debris, sediment and height holds a permutation of 0 .. B-1 of its own across
    the models; bedrock = height - sediment, integers of magnitude < B, so the fp32 sum is that integer exactly."""
    r = np.random.default_rng(seed)
    perm = np.argsort(r.random((H * W * 5, B), dtype=np.float32), axis=1).T.reshape(B, H, W, 5).astype(np.float32)
    layers = np.stack([perm[..., 4] - perm[..., 3], perm[..., 3]], axis=-1)
    return {"layers": np.ascontiguousarray(layers), "waterHeight": np.ascontiguousarray(perm[..., 0]),
            "mass": np.ascontiguousarray(perm[..., 1]), "debris": np.ascontiguousarray(perm[..., 2])}


def _hostile(B, H, W, seed):
    """Random bit patterns: one value in 256 has an all-ones exponent (NaNs with payloads), one in 256 a zero exponent
    (denormals); to make ties, infinities and zeros common, one value in eleven is planted from a short list."""
    r = np.random.default_rng(seed)
    host = {}
    for name in READ:
        shape = (B, H, W, 2) if name == "layers" else (B, H, W)
        u = r.integers(0, 1 << 32, size=shape, dtype=np.uint32)
        plant = r.integers(0, 96, size=shape)
        for k, pattern in enumerate((0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                                     0x7FC00001, 0xFFFFFFFF, 0x3F800000)):
            u[plant == k] = pattern
        host[name] = u.view(np.float32)
    return host


def _with_path(monkeypatch, path):
    if path is None:
        monkeypatch.delenv("SOIL_QUANTILE_PATH", raising=False)
    else:
        monkeypatch.setenv("SOIL_QUANTILE_PATH", path)   # read at every call


def _paths(B):
    return [None] + [p for p, top in PATH_MAX.items() if top is None or B <= top]


# ---------------------------------------------------------------- 1. known answers by construction

@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_known_answers(hip, case):
    (H, W), B = case
    host = _permutations(B, H, W, seed=B + 7 * H)
    bt = _filled(host, B, H, W)
    known = [1, 2, 3, 4, 5]   # every channel but bedrock holds a permutation
    ranks = list(range(B)) if B <= 33 else sorted({0, 1, B // 2 - 1, B // 2, B - 2, B - 1, 15, 16, 17, 31, 32, 33, 63})
    ranks = [k for k in ranks if 0 <= k < B]
    got = bt.order_statistics(ranks)
    assert tuple(got.shape) == (len(ranks), H, W, 6) and got.host.name == "gpu"
    got = to_np(got)
    for j, k in enumerate(ranks):
        assert (got[j][..., known] == np.float32(k)).all(), "rank %d" % k
    med = bt.median()
    assert tuple(med.shape) == (H, W, 6)
    assert (to_np(med)[..., known] == np.float32((B - 1) / 2)).all()
    q = [0.0, 0.1, 0.5, 0.9, 1.0, 1.0 / 3.0]
    got = to_np(bt.quantiles(q))
    for j, v in enumerate(q):
        pos = v * (B - 1)
        lo = math.floor(pos)
        frac = pos - lo
        want = np.float32(lo) if frac == 0 else np.float32(float(lo) + frac * (float(min(lo + 1, B - 1)) - float(lo)))
        assert (got[j][..., known] == want).all(), "q = %r" % v
    # bedrock, and everything once more, against the restatement
    vals = _channels(host)
    want, gen = _expected(vals, [v * (B - 1) for v in q])
    _assert_bits(got, want, gen, "quantiles")
    for name, a in host.items():
        assert np.array_equal(to_np(getattr(bt, name)).view(np.uint32), a.view(np.uint32)), "the source: " + name


# ---------------------------------------------------------------- 2. hostile bits, on every path

@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_hostile_bits_on_every_path(hip, monkeypatch, case):
    (H, W), B = case
    host = _hostile(B, H, W, seed=3 * B + H)
    vals = _channels(host)
    s = _sorted_bits(vals)
    if B <= 300:
        ranks = list(range(B))       # every rank, 16 to a call
    else:                            # B = 4099 takes the bisection, seconds per call: the ends, the middle and a stride
        ranks = sorted(set(range(8)) | set(range(B - 8, B)) | {B // 2 - 1, B // 2} | set(range(0, B, 293)))
    fractions = _fractions(B)
    bt = _filled(host, B, H, W)
    big = H * W > 4096
    first = None
    for path in _paths(B):
        if big and path == "bisect":
            continue                 # 32 walks per rank over 64 Ki cells: covered at the ragged sizes
        _with_path(monkeypatch, path)
        got_ranks = to_np(bt.order_statistics(ranks))
        got_frac = to_np(bt._at_positions(fractions))
        if first is None:
            for j, k in enumerate(ranks):
                _assert_bits(got_ranks[j], s[k], np.zeros(s[k].shape, bool), "rank %d" % k)
            want, gen = _expected(vals, fractions)
            _assert_bits(got_frac, want, gen, "fractional positions")
            first = (got_ranks, got_frac, gen)
        else:
            assert np.array_equal(got_ranks.view(np.uint32), first[0].view(np.uint32)), "path %s: ranks" % path
            same = (got_frac.view(np.uint32) == first[1].view(np.uint32)) | first[2]
            assert same.all(), "path %s: fractional positions" % path


def test_minus_infinity_next_to_a_finite_value(hip, monkeypatch):
    """The two cases the header derives from the arithmetic: -inf next to a finite value is NaN at a fractional
    position between them and -inf at the rank itself; a NaN model spoils only positions above the last finite
    rank of its own cell."""
    B, H, W = 5, 3, 7
    r = np.random.default_rng(11)
    host = {name: r.standard_normal((B, H, W, 2) if name == "layers" else (B, H, W)).astype(np.float32)
            for name in READ}
    host["mass"][2, 1, 3] = -np.inf
    host["debris"][4, 2, 6] = np.nan
    host["waterHeight"][0, 0, 0] = np.inf
    vals = _channels(host)
    pos = [0.0, 0.5, 1.0, 1.5, 3.0, 3.5, 4.0]
    want, gen = _expected(vals, pos)
    bt = _filled(host, B, H, W)
    for path in _paths(B):
        _with_path(monkeypatch, path)
        got = to_np(bt._at_positions(pos))
        _assert_bits(got, want, gen, "path %s" % path)
        assert got[0][1, 3, 4] == -np.inf and np.isnan(got[1][1, 3, 4]) and np.isfinite(got[2:, 1, 3, 4]).all()
        assert np.isfinite(got[:5, 2, 6, 5]).all() and np.isnan(got[5:, 2, 6, 5]).all()
        assert np.isfinite(got[:5, 0, 0, 3]).all() and (got[5:, 0, 0, 3] == np.inf).all()
        touched = np.zeros((H, W, 6), bool)
        touched[1, 3, 4] = touched[2, 6, 5] = touched[0, 0, 3] = True
        assert np.isfinite(got[:, ~touched]).all()


# ---------------------------------------------------------------- 3. invariance

@pytest.mark.parametrize("B", [7, 64, 65, 257])
def test_permuting_or_moving_the_models_changes_no_bit(hip, B):
    """37 x 53 has an odd cell count: models embedded one model into a larger allocation start off an 8-byte
    (layers) and off any wider boundary."""
    from soillib_amd import _abi, silt
    H, W = 37, 53
    host = _hostile(B, H, W, seed=B)
    pos = _fractions(B) + [float(k) for k in range(0, B, max(1, B // 6))]
    pos = pos[:16]
    bt = _filled(host, B, H, W)
    want = to_np(bt._at_positions(pos)).view(np.uint32)
    t = [0.0, 1.0, -1.0, 0.5, 1e-40, np.inf]
    want_x = to_np(bt.exceedance(t)).view(np.uint32)
    order = np.random.default_rng(B).permutation(B)
    other = _filled({name: np.ascontiguousarray(a[order]) for name, a in host.items()}, B, H, W)
    assert np.array_equal(to_np(other._at_positions(pos)).view(np.uint32), want), "permuted"
    assert np.array_equal(to_np(other.exceedance(t)).view(np.uint32), want_x), "permuted: exceedance"
    # models 1 .. B of a batch of B + 2, through the entry points themselves
    pad = {name: np.concatenate([a[-1:], a, a[:1]]) for name, a in host.items()}
    big = _filled(pad, B + 2, H, W)
    planes = _abi.ErosionPlanes()
    for name in READ:
        per = getattr(big, name).nbytes() // (B + 2)
        setattr(planes, name, getattr(big, name).ptr + per)
    out = silt.tensor(silt.float32, silt.shape(len(pos), H, W, 6), silt.gpu)
    _abi.check(_abi.lib().soil_erode_batch_quantiles(C.byref(planes), B, H, W, (C.c_double * len(pos))(*pos), len(pos),
                                                     out.c_ptr, None))
    assert np.array_equal(to_np(out).view(np.uint32), want), "embedded"
    out_x = silt.tensor(silt.float32, silt.shape(H, W, 6), silt.gpu)
    _abi.check(_abi.lib().soil_erode_batch_exceedance(C.byref(planes), B, H, W, (C.c_float * 6)(*t), out_x.c_ptr, None))
    assert np.array_equal(to_np(out_x).view(np.uint32), want_x), "embedded: exceedance"


# ---------------------------------------------------------------- 4. other request shapes

@pytest.mark.parametrize("B", [9, 100])
def test_request_shapes(hip, B):
    H, W = 37, 53
    host = _hostile(B, H, W, seed=40 + B)
    vals = _channels(host)
    bt = _filled(host, B, H, W)
    r = np.random.default_rng(B)
    for q in ([0.37], list(r.random(16)), list(r.random(17)), [0.9, 0.1, 0.5, 0.1, 0.1, 1.0, 0.0, 0.9], 0.25):
        got = bt.quantiles(q)
        qs = [q] if isinstance(q, float) else q
        assert tuple(got.shape) == (len(qs), H, W, 6)
        want, gen = _expected(vals, [float(v) * (B - 1) for v in qs])
        _assert_bits(to_np(got), want, gen, "q = %r" % (q,))
    one = bt.order_statistics(B - 1)
    assert tuple(one.shape) == (1, H, W, 6)


def test_on_another_stream(hip):
    import torch
    from soillib_amd import _abi
    B, H, W = 70, 37, 53
    host = _hostile(B, H, W, seed=8)
    vals = _channels(host)
    pos = _fractions(B)
    want, gen = _expected(vals, pos)
    t = [0.0] * 6
    want_x = ((vals > np.float32(0.0)).sum(axis=0).astype(np.float64) / np.float64(B)).astype(np.float32)
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        bt = _filled(host, B, H, W)
        got, got_x = bt._at_positions(pos), bt.exceedance(t)
        s.synchronize()
        _assert_bits(to_np(got), want, gen, "quantiles")
        assert np.array_equal(to_np(got_x).view(np.uint32), want_x.view(np.uint32))
        s.synchronize()
    finally:
        _abi.set_stream(0)


@pytest.mark.parametrize("B", [7, 100, 300])
def test_a_poisoned_cell_spoils_only_itself(hip, B):
    H, W = 37, 53
    r = np.random.default_rng(66)
    clean = {name: r.standard_normal((B, H, W, 2) if name == "layers" else (B, H, W)).astype(np.float32)
             for name in READ}
    dirty = {name: a.copy() for name, a in clean.items()}
    dirty["waterHeight"][3, 5, 7] = np.nan
    dirty["layers"][0, 10, 11, 0] = np.inf
    dirty["layers"][6, 36, 52] = (np.inf, -np.inf)
    dirty["debris"][2, 0, 0] = -np.inf
    spoiled = np.zeros((H, W), bool)
    for cell in [(5, 7), (10, 11), (36, 52), (0, 0)]:
        spoiled[cell] = True
    pos = _fractions(B)
    want = to_np(_filled(clean, B, H, W)._at_positions(pos))
    got = to_np(_filled(dirty, B, H, W)._at_positions(pos))
    expected, gen = _expected(_channels(dirty), pos)
    _assert_bits(got, expected, gen, "the poisoned batch")
    assert np.array_equal(got[:, ~spoiled].view(np.uint32), want[:, ~spoiled].view(np.uint32))
    assert np.isfinite(got[:, ~spoiled]).all()
    top = pos.index(float(B - 1))
    assert np.isnan(got[top][5, 7, 3]) and np.isnan(got[top][36, 52, 2]) and got[top][10, 11, 0] == np.inf
    assert got[pos.index(0.0)][0, 0, 5] == -np.inf
    assert np.isfinite(got[:, 5, 7, [0, 1, 2, 4, 5]]).all()   # its channel only


# ---------------------------------------------------------------- 5. after real steps

def test_after_real_steps(hip, oracle):
    B, H, W = 5, 48, 40
    bt = _batch(B, H, W, (20.0 / H, 20.0 / W, 4.0), _param(oracle, 48), 600, [5 + 3 * b for b in range(B)],
                _inputs(oracle, B, H, W))
    for _ in range(2):
        bt.step()
    planes = [bt.model_planes(b) for b in range(B)]
    host = {name: np.stack([p[name] for p in planes]) for name in READ}
    vals = _channels(host)
    q = [0.0, 0.1, 0.5, 0.9, 1.0]
    want, gen = _expected(vals, [v * (B - 1) for v in q])
    got = to_np(bt.quantiles(q))
    _assert_bits(got, want, gen, "quantiles")
    assert np.array_equal(to_np(bt.median()).view(np.uint32), want[2])
    assert (got[4][..., 3] > 0).any()   # the steps left water
    t = [float(np.median(vals[..., c])) for c in range(6)]
    want_x = ((vals > np.asarray(t, np.float32)).sum(axis=0).astype(np.float64) / np.float64(B)).astype(np.float32)
    assert np.array_equal(to_np(bt.exceedance(t)).view(np.uint32), want_x.view(np.uint32))


# ---------------------------------------------------------------- 6. exceedance

def _exceedance_expected(vals, t):
    with np.errstate(invalid="ignore"):
        c = (vals > np.asarray(t, np.float32)).sum(axis=0)
    return (c.astype(np.float64) / np.float64(vals.shape[0])).astype(np.float32)


# (256 x 256 stays at B <= 64, as in CASES: 393 MB of planes at B = 300)
X_CASES = [(size, B) for size in RAGGED + [(256, 256)] for B in (1, 2, 7, 64, 300) if B <= 64 or size in RAGGED]


@pytest.mark.parametrize("case", X_CASES, ids=_case_id)
def test_exceedance_bit_for_bit(hip, case):
    (H, W), B = case
    host = _hostile(B, H, W, seed=B + W)
    vals = _channels(host)
    bt = _filled(host, B, H, W)
    occurs = [float(vals[0].reshape(-1, 6)[0, c]) for c in range(6)]          # a value that occurs: strict
    occurs = [0.0 if v != v else v for v in occurs]
    for t in (occurs, [0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45], [np.inf] * 6, [-np.inf] * 6, [np.nan] * 6,
              [np.nan, 0.0, np.inf, -np.inf, 3e38, -3e38]):
        got = bt.exceedance(t)
        assert tuple(got.shape) == (H, W, 6) and got.host.name == "gpu"
        want = _exceedance_expected(vals, t)
        assert np.array_equal(to_np(got).view(np.uint32), want.view(np.uint32)), "thresholds %r" % (t,)
    assert not to_np(bt.exceedance([np.nan] * 6)).any() and not to_np(bt.exceedance([np.inf] * 6)).any()
    for name, a in host.items():
        assert np.array_equal(to_np(getattr(bt, name)).view(np.uint32), a.view(np.uint32)), "the source: " + name


# ---------------------------------------------------------------- 7. refusals

def test_a_forced_path_is_refused_where_it_cannot_hold_b(hip, monkeypatch):
    from soillib_amd import _abi
    H, W = 5, 3
    for path, top in (("reg", 64), ("lds", 256)):
        host = _hostile(top + 1, H, W, seed=top)
        bt = _filled(host, top + 1, H, W)
        want = to_np(bt.median()).view(np.uint32)
        _with_path(monkeypatch, path)
        with pytest.raises(ValueError, match="SOIL_QUANTILE_PATH=%s" % path):
            bt.median()
        assert "erode_batch_quantiles" in _abi.last_error()
        _with_path(monkeypatch, "bisect")
        assert np.array_equal(to_np(bt.median()).view(np.uint32), want)
        _with_path(monkeypatch, None)
    bt = _filled(_hostile(2, H, W, seed=2), 2, H, W)
    _with_path(monkeypatch, "sideways")
    with pytest.raises(ValueError, match="SOIL_QUANTILE_PATH"):
        bt.median()
    _with_path(monkeypatch, "auto")
    bt.median()


def test_invalid_arguments_are_refused(hip):
    from soillib_amd import _abi, silt
    lib = _abi.lib()
    B, H, W = 3, 8, 12
    host = _hostile(B, H, W, seed=1)
    bt = _filled(host, B, H, W)
    planes = bt._planes()
    out = silt.tensor(silt.float32, silt.shape(2, H, W, 6), silt.gpu)
    silt.set(out, 7.0)
    pos2 = (C.c_double * 2)(0.0, 1.5)
    thr = (C.c_float * 6)()

    def without(field):
        p = _abi.ErosionPlanes()
        for f, _ in _abi.ErosionPlanes._fields_:
            setattr(p, f, None if f == field else getattr(planes, f))
        return p

    def refused(rc, entry, naming):
        assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, (entry, naming, rc)
        assert entry in _abi.last_error() and naming in _abi.last_error(), (entry, naming, _abi.last_error())

    def quantiles(naming, p=planes, sizes=(B, H, W), pos=pos2, nq=2, o=out):
        refused(lib.soil_erode_batch_quantiles(None if p is None else C.byref(p), *sizes, pos, nq,
                                               None if o is None else o.c_ptr, None), "erode_batch_quantiles", naming)

    def exceedance(naming, p=planes, sizes=(B, H, W), t=thr, o=out):
        refused(lib.soil_erode_batch_exceedance(None if p is None else C.byref(p), *sizes, t,
                                                None if o is None else o.c_ptr, None), "erode_batch_exceedance", naming)

    for call in (quantiles, exceedance):
        call("B >= 1", sizes=(0, H, W))
        call("B >= 1", sizes=(-3, H, W))
        call("empty grid", sizes=(B, 0, W))
        call("empty grid", sizes=(B, H, -1))
        call("overflow", sizes=(B, 1 << 40, 1 << 20))
        call("overflow", sizes=(1 << 40, 1 << 12, 1 << 12))
        call("null planes", p=None)
        call("null out", o=None)
        for field in READ:
            call("null plane", p=without(field))
    quantiles("null pos", pos=None)
    exceedance("null thresholds", t=None)
    quantiles("nq must be", nq=0)
    quantiles("nq must be", nq=-1)
    quantiles("nq must be", pos=(C.c_double * 17)(), nq=17)
    for bad in (float("nan"), float("inf"), -float("inf"), -0.5, 2.0000001, 3.0):
        quantiles("pos must be finite", pos=(C.c_double * 2)(0.0, bad))
    quantiles("byte size overflows", sizes=(1, 1 << 28, 1 << 27), pos=(C.c_double * 16)(), nq=16)
    exceedance("byte size overflows", sizes=(1, 3 << 28, 1 << 29))
    assert (to_np(out) == 7.0).all()   # nothing was launched
    # what is not read may be NULL; the largest pos is B - 1
    p = _abi.ErosionPlanes()
    for f in READ:
        setattr(p, f, getattr(planes, f))
    pos_ok = (C.c_double * 2)(0.0, float(B - 1))
    assert lib.soil_erode_batch_quantiles(C.byref(p), B, H, W, pos_ok, 2, out.c_ptr, None) == _abi.SOIL_OK
    want, gen = _expected(_channels(host), [0.0, float(B - 1)])
    _assert_bits(to_np(out), want, gen, "after the refusals")
    # the Python refusals come before any device work
    for call, arg in ((bt.quantiles, []), (bt.quantiles, [1.5]), (bt.quantiles, float("nan")),
                      (bt.order_statistics, [B]), (bt.order_statistics, [0.5]), (bt.exceedance, [0.0] * 5)):
        with pytest.raises(ValueError):
            call(arg)


def test_a_row_slab_cannot_reach_the_entries(hip):
    """ErosionModel.stats() refuses a row slab with a ValueError naming it; the order statistics exist on the batch
    only, and a batch cannot be made of a row slab, by the same words."""
    from soillib_amd import _abi, soil
    from soillib_amd.erosion import ErosionBatch, ErosionModel
    m = ErosionModel(16, 8, (1.0, 1.0, 1.0), soil.param_t(), 16, dom=_abi.Domain(16, 8, 0, 8, 0, 8))
    with pytest.raises(ValueError, match="row slab"):
        ErosionBatch.from_models([m])
    for name in ("quantiles", "order_statistics", "median", "exceedance"):
        assert not hasattr(m, name)
