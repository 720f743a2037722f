"""soil_solve_uniform (soillib_amd/csrc/path.hip) against the CPU oracle: every cell of every case.

Two constructions.

EXACT.  sx sy H W is a power of two, so P = 1/(A H W) and S = source/P are exact; decay is 0, so att stays 1
(orc_expf(-0) == 1); the sources are multiples of 2^-4 in [0, 1].  Every deposit is then an integer multiple of one
quantum q = 2^-4/P, a cell's sum is (at most 16 visits) q, and while 16 visits < 2^24 every partial sum is exact in
fp32 in ANY order: the float atomics cannot round, and the plane equals the serial oracle's bit for bit.  One lost,
doubled or misplaced deposit changes bits.  The condition is asserted from the oracle's visit counts.

GENERAL.  Any scale, decay and source.  The walks are the oracle's (same fp32 statements), so each cell receives the
same fp32 products S[c]*att, in an unknown order.  With acc64 their sum in double, the exact value of a cell is
    R = (src A + acc64/count) / norm           A = fp32(sx sy), norm = fp32(|vx sy| + |vy sx|), both inputs of
                                               the last statement and computed here as that statement's operands,
and the kernel's fp32 evaluation differs from it by the k - 1 roundings of summing k same-signed terms in any order
plus the four of the normalisation (src A, /count, +, /norm):  |got - R| <= (k + 4) 2^-24 R.  No absolute term.  With
signed sources the terms may cancel and the bound is taken on the absolute sums instead.

Non-finite cells are compared by class with the fp32 oracle (NaN with NaN, the same signed infinity).
"""
import functools

import numpy as np
import pytest

from util import assert_bit_equal, philox_word0, rng_to_gpu, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (seed, offset) with which walker 0 draws u = 1.0 for px / for py (found with util.find_unit_draws)
UNIT_PX = (1, 8418514)
UNIT_PY = (1, 8418513)


# ------------------------------------------------------------------------------------------------ inputs

def _flow(oracle, kind, H, W, scale):
    x, y = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    if kind == "gradient":
        return -oracle.gradient(terrain(oracle, H, W)[..., 0].copy(), scale)
    if kind == "rotation":      # stream function sin sin (tangent to the rim, centre between the nodes) and a slight
        ax, ay = np.pi / (H - 1), np.pi / (W - 1)    # pull inwards, which keeps the coarse steps from spiralling out
        v = np.stack([ay * np.sin(ax * x) * np.cos(ay * y), -ax * np.cos(ax * x) * np.sin(ay * y)], -1)
        v += 0.25 * np.stack([ax * (0.5 * (H - 1) - x) * ay, ay * (0.5 * (W - 1) - y) * ax], -1)
        return np.ascontiguousarray(v * 8.0, np.float32)
    if kind == "sink":          # everybody converges on the cells about an off-node point
        v = np.stack([0.31 * H + 0.3 - x, 0.36 * W + 0.6 - y], -1)
        return np.ascontiguousarray(v * 0.125, np.float32)
    raise KeyError(kind)


class Case:
    def __init__(self, name, flow, source, decay, rng, scale, count, calls=1, signed=False):
        self.name, self.flow, self.source, self.decay = name, flow, source, decay
        self.rng, self.scale, self.count, self.calls, self.signed = rng, scale, int(count), calls, signed


def exact_case(oracle, name, H=64, W=32, scale=(0.5, 0.25), field="gradient", K=1, N=5000, count=None,
               source="random", rng="equal"):
    """See the module docstring.  Two consecutive calls on one rng tensor."""
    assert float(np.log2(scale[0] * scale[1] * H * W)).is_integer()
    r = np.random.default_rng(H * 131 + W + K)
    src = (r.integers(0, 17, (H, W, K)) / 16.0).astype(np.float32)
    if source == "half":        # walkers spawned in the upper half-plane carry nothing
        src[:H // 2] = 0
    elif source == "ch0_zero":  # Slen has to read the last channel
        src[..., 0] = 0
    state = oracle.rng_seed(N, 1, 0)
    if rng == "mixed":
        state["seed"] = r.integers(0, 1 << 62, N)
        state["offset"] = r.integers(0, 1 << 40, N)
        state["offset"][::7] = (1 << 32) - 1     # the counter's low word carries into the high one
    return Case(name, _flow(oracle, field, H, W, scale), src, np.zeros((H, W), np.float32), state, scale,
                N if count is None else count, calls=2)


def general_case(oracle, name, H, W, K, strong=False, signed=False, hostile=None, scale=(0.03, 0.11)):
    r = np.random.default_rng(H * 977 + W * 31 + K + 2 * strong)
    N = max(64, 2 * H * W) if H * W < 400 else 3000
    if H >= 4 and W >= 4:
        flow = -oracle.gradient(terrain(oracle, H, W)[..., 0].copy(), scale)
    else:
        flow = (r.standard_normal((H, W, 2)) * 0.5).astype(np.float32)
    src = (1e-4 + r.random((H, W, K)) * 1e-3).astype(np.float32)
    if signed:
        src *= r.choice(np.float32([-1, 1]), (H, W, K))
    decay = (r.random((H, W)) * (40.0 if strong else 0.01)).astype(np.float32)
    if hostile == "zero_block":
        flow[10:16, 20:27] = 0
    elif hostile == "nan_flow":
        flow[12, 17] = np.nan
    elif hostile == "inf_flow":
        flow[12, 17, 0] = np.inf
    elif hostile == "nan_source":
        src[12, 17, 0] = np.nan
    return Case(name, flow, src, decay, oracle.rng_seed(N, 1, 0), scale, 2 * N + 1, signed=signed)


# ------------------------------------------------------------------------------------- reference and judgement

_EXPECTED = {}


def expected(oracle, case):
    """The oracle's `calls` consecutive calls: a list of (detail dict, rng after).  Computed once per case."""
    if case.name not in _EXPECTED:
        rng, out = case.rng.copy(), []
        for _ in range(case.calls):
            d = oracle.solve_uniform_detail(case.flow, case.source, case.decay, rng, case.scale, case.count)
            out.append((d, rng.copy()))
        _EXPECTED[case.name] = out
    return _EXPECTED[case.name]


def on_gpu(case):
    """The product's `calls` consecutive calls on one rng tensor: a list of (flux, rng after)."""
    from soillib_amd import soil
    flow, src, decay, rng = to_gpu(case.flow), to_gpu(case.source), to_gpu(case.decay), rng_to_gpu(case.rng)
    out = []
    for _ in range(case.calls):
        flux = soil.solve_uniform(flow, src, decay, rng, case.scale, case.count)
        out.append((to_np(flux), to_np(rng).copy()))
    return out


def judge_rng(got, want, what):
    assert (got["seed"] == want["seed"]).all(), what + ": rng seeds"
    bad = np.flatnonzero(got["offset"] != want["offset"])
    assert bad.size == 0, "%s: rng offsets of %d walkers differ, first %d: %d vs %d" % (
        what, bad.size, bad[0], got["offset"][bad[0]], want["offset"][bad[0]])


def judge_exact(case, want, got):
    for call, ((flux, rng), (d, rng_want)) in enumerate(zip(got, want)):
        what = "%s call %d" % (case.name, call)
        assert int(d["visits"].max(initial=0)) * 16 < 1 << 24, what + ": the sums are no longer exact"
        assert_bit_equal(flux, d["flux"], what)
        judge_rng(rng, rng_want, what)


def exact_value(case, d):
    """R of the module docstring and the sum of the absolute terms, in float64."""
    sx, sy = np.float32(case.scale[0]), np.float32(case.scale[1])
    A = np.float64(sx * sy)
    norm = (np.abs(case.flow[..., 0] * sy) + np.abs(case.flow[..., 1] * sx)).astype(np.float64)[..., None]
    src = case.source.astype(np.float64)
    count = np.float64(np.float32(case.count))
    with np.errstate(all="ignore"):
        return (src * A + d["acc64"] / count) / norm, (np.abs(src * A) + d["absacc64"] / count) / norm


def judge_bound(case, want, got):
    for call, ((flux, rng), (d, rng_want)) in enumerate(zip(got, want)):
        what = "%s call %d" % (case.name, call)
        judge_rng(rng, rng_want, what)
        ref = d["flux"]
        fin = np.isfinite(ref)
        assert (np.isnan(flux) == np.isnan(ref)).all(), what + ": NaN cells"
        assert (np.isinf(flux) == np.isinf(ref)).all() and (np.sign(flux[np.isinf(ref)]) == np.sign(ref[np.isinf(ref)])).all(), \
            what + ": infinite cells"
        R, Rabs = exact_value(case, d)
        if not case.signed:
            assert (case.source[fin] >= 0).all()
            Rabs = R
        with np.errstate(invalid="ignore"):
            err = np.abs(flux.astype(np.float64) - R)[fin]
        bound = ((d["visits"] + 4) * U * Rabs)[fin]
        assert np.isfinite(bound).all(), what
        bad = err > bound
        worst = (err / np.where(bound > 0, bound, 1)).max(initial=0)
        print("%s: %d finite cells, worst error %.3f of its bound, most visits %d" % (what, fin.sum(), worst, d["visits"].max(initial=0)))
        assert not bad.any(), "%s: %d cells beyond (k + 4) 2^-24 R, worst %.3f times" % (what, bad.sum(), worst)


def reasons(d):
    return np.bincount(d["reason"], minlength=7)


# ------------------------------------------------------------------------------------------------ exact cases

G1 = dict(H=64, W=32, scale=(0.5, 0.25))
G2 = dict(H=32, W=64, scale=(0.25, 0.5))     # the axes' roles exchanged

EXACT = {}
for _g, _grid in (("64x32", G1), ("32x64", G2)):
    for _field in ("gradient", "rotation", "sink"):
        for _K in (1, 2):
            EXACT["%s-%s-K%d" % (_field, _g, _K)] = dict(_grid, field=_field, K=_K)
for _K in (1, 2):
    EXACT["half_plane_without_source-K%d" % _K] = dict(G1, K=_K, source="half")
    EXACT["per_walker_rng-K%d" % _K] = dict(G1, K=_K, rng="mixed")
    for _count in (1, 15000):
        EXACT["count_%d-K%d" % (_count, _K)] = dict(G1, K=_K, count=_count)
    for _N in (0, 1, 255, 256, 257, 4 * 64 * 32):
        EXACT["N_%d-K%d" % (_N, _K)] = dict(G1, K=_K, N=_N, count=max(_N, 1))
EXACT["first_channel_zero-K2"] = dict(G1, K=2, source="ch0_zero")
EXACT["first_channel_zero-rotation-K2"] = dict(G2, K=2, source="ch0_zero", field="rotation")


@functools.lru_cache(maxsize=None)
def _exact(oracle, name):
    return exact_case(oracle, name, **EXACT[name])


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact(hip, oracle, name):
    case = _exact(oracle, name)
    want = expected(oracle, case)
    d = want[0][0]
    r, N = reasons(d), len(case.rng)
    if "rotation" in name and "first_channel" not in name:
        # closed: nobody leaves, and whoever walks at all (a walker spawned in the far strip samples a NaN at once and
        # deposits nothing) ends at maxstep = H + W
        walked = N - r[oracle.SU_DROPPED] - r[oracle.SU_NO_SOURCE] - r[oracle.SU_NAN]
        assert r[oracle.SU_MAXSTEP] >= 0.9 * walked and r[oracle.SU_LEFT] == 0 and r[oracle.SU_NAN] < 0.06 * N, r
    if "sink" in name:
        assert r[oracle.SU_MAXSTEP] + r[oracle.SU_STALLED] >= 0.9 * (N - r[oracle.SU_NO_SOURCE] - r[oracle.SU_NAN]), r
        assert d["visits"].max() > 20 * N / 64, "no contention"
    if "half_plane" in name:
        assert r[oracle.SU_NO_SOURCE] > 0.4 * N
    if "first_channel" in name:
        assert d["visits"][..., 1].sum() > N and (d["acc64"][..., 0] == 0).all()
    judge_exact(case, want, on_gpu(case))


def test_exact_on_another_stream(hip, oracle):
    import torch
    from soillib_amd import _abi
    case = _exact(oracle, "gradient-64x32-K2")
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        got = on_gpu(case)
        s.synchronize()
    finally:
        _abi.set_stream(0)
    judge_exact(case, expected(oracle, case), got)


# ------------------------------------------------------------------------------------- a draw of exactly 1.0

def _unit_case(oracle, name, const, N):
    case = exact_case(oracle, name, N=N, K=2, **G1)
    case.rng["seed"][0], case.rng["offset"][0] = const
    return case


@pytest.mark.parametrize("axis,const", [("px", UNIT_PX), ("py", UNIT_PY)])
def test_a_draw_of_one_is_dropped(hip, oracle, axis, const):
    """The reference reads out of bounds for such a walker; kernel and oracle drop it, its two draws spent."""
    alone = _unit_case(oracle, "unit_%s_alone" % axis, const, 1)
    want = expected(oracle, alone)
    assert want[0][0]["reason"][0] == oracle.SU_DROPPED and want[0][0]["visits"].sum() == 0
    assert want[0][1]["offset"][0] == const[1] + 2
    judge_exact(alone, want, on_gpu(alone))

    among = _unit_case(oracle, "unit_%s_among_300" % axis, const, 300)
    want = expected(oracle, among)
    d = want[0][0]
    assert d["reason"][0] == oracle.SU_DROPPED and (d["reason"][1:] != oracle.SU_DROPPED).all()
    # the other 299 walk as they do beside a walker 0 that spawns on a cell without source
    other = exact_case(oracle, "unit_%s_other_299" % axis, N=300, K=2, **G1)
    empty = other.source.sum(-1) == 0
    off = np.arange(0, 1 << 14, dtype=np.uint64)
    u = ((philox_word0(1, 0, off) >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(U)
    cx, cy = (u[:-1] * np.float32(64)).astype(np.int64), (u[1:] * np.float32(32)).astype(np.int64)
    other.rng["offset"][0] = off[:-1][empty[np.minimum(cx, 63), np.minimum(cy, 31)]][0]
    d_other = oracle.solve_uniform_detail(other.flow, other.source, other.decay, other.rng.copy(), other.scale,
                                          other.count)
    assert d_other["reason"][0] == oracle.SU_NO_SOURCE
    assert_bit_equal(d["flux"], d_other["flux"], "the dropped walker changes nothing")
    judge_exact(among, want, on_gpu(among))


# ---------------------------------------------------------------------------------------------- general cases

RAGGED = [(37, 53), (96, 40), (33, 50)]
TINY = [(1, 1), (1, 9), (9, 1), (2, 2), (2, 7)]


@functools.lru_cache(maxsize=None)
def _general(oracle, name, *args, **kw):
    return general_case(oracle, name, *args, **dict(kw))


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("strong", [False, True], ids=["weak_decay", "strong_decay"])
@pytest.mark.parametrize("H,W", RAGGED + TINY)
def test_bound(hip, oracle, H, W, strong, K):
    case = _general(oracle, "general-%dx%d-%d-K%d" % (H, W, strong, K), H, W, K, strong=strong)
    want = expected(oracle, case)
    r = reasons(want[0][0])
    if strong and (H, W) in RAGGED:
        assert r[oracle.SU_SPENT] >= 0.5 * len(case.rng), r
    judge_bound(case, want, on_gpu(case))


@pytest.mark.parametrize("K", [1, 2])
def test_bound_signed_source(hip, oracle, K):
    case = _general(oracle, "signed-K%d" % K, 37, 53, K, signed=True)
    assert (case.source < 0).any() and (case.source > 0).any()
    judge_bound(case, expected(oracle, case), on_gpu(case))


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("hostile", ["zero_block", "nan_flow", "inf_flow", "nan_source"])
def test_hostile_fields(hip, oracle, hostile, K):
    case = _general(oracle, "%s-K%d" % (hostile, K), 37, 53, K, hostile=hostile)
    want = expected(oracle, case)
    d = want[0][0]
    r = reasons(d)
    if hostile == "zero_block":
        assert np.isposinf(d["flux"][10:16, 20:27]).all() and r[oracle.SU_STALLED] > 0, r
    elif hostile == "inf_flow":     # the cell's norm is infinite; a walker that samples it goes NaN (inf/inf) and ends
        assert (d["flux"][12, 17] == 0).all() and r[oracle.SU_NAN] > reasons(expected(oracle, _general(
            oracle, "general-37x53-0-K%d" % K, 37, 53, K, strong=False))[0][0])[oracle.SU_NAN], r
    else:
        assert np.isnan(d["flux"]).any()
    judge_bound(case, want, on_gpu(case))
