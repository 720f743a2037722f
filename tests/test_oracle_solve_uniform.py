"""The oracle's detailed solve_uniform (pyoracle.solve_uniform_detail) pinned without a GPU: it is what
tests/test_gpu_solve_uniform.py judges the kernel by, on that file's own cases."""
import numpy as np
import pytest

import test_gpu_solve_uniform as su
from util import assert_bit_equal, find_unit_draws, philox_word0


def _spawn_cells(case):
    """Each walker's spawn cell from the generator restated in numpy (util.philox_word0), -1 where a draw is 1.0."""
    H, W = case.source.shape[:2]
    cells = np.empty(len(case.rng), np.int64)
    for n, (seed, off) in enumerate(zip(case.rng["seed"].tolist(), case.rng["offset"].tolist())):
        w = philox_word0(seed, n, [off, off + 1])
        u = ((w >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)
        px, py = u[0] * np.float32(H), u[1] * np.float32(W)
        cells[n] = -1 if px >= H or py >= W else int(px) * W + int(py)
    return cells


def test_exp_of_zero_is_one(oracle):
    assert (oracle.expf([0.0, -0.0]) == 1.0).all()      # decay 0 leaves att == 1 exactly


@pytest.mark.parametrize("name", ["gradient-64x32-K1", "gradient-32x64-K2", "rotation-64x32-K2", "sink-32x64-K1",
                                  "half_plane_without_source-K2", "first_channel_zero-K2", "per_walker_rng-K1",
                                  "count_15000-K2", "N_0-K1", "N_257-K2"])
def test_detail_reproduces_solve_uniform_on_the_exact_construction(oracle, name):
    case = su._exact(oracle, name)
    rng_a, rng_b = case.rng.copy(), case.rng.copy()
    for call in range(2):
        want = oracle.solve_uniform(case.flow, case.source, case.decay, rng_a, case.scale, case.count)
        d = oracle.solve_uniform_detail(case.flow, case.source, case.decay, rng_b, case.scale, case.count)
        assert_bit_equal(d["flux"], want, "the detailed walk's own plane")
        assert (rng_a == rng_b).all() and (rng_a["offset"] == case.rng["offset"] + 2 * (call + 1)).all()
        # acc64 through the normalisation, every operation rounded to fp32 as path.cu:160-168 writes it
        sx, sy = np.float32(case.scale[0]), np.float32(case.scale[1])
        acc = d["acc64"].astype(np.float32)
        assert (acc.astype(np.float64) == d["acc64"]).all(), "the sums of the exact construction are fp32 numbers"
        norm = (np.abs(case.flow[..., 0] * sy) + np.abs(case.flow[..., 1] * sx))[..., None]
        with np.errstate(all="ignore"):
            flux = (case.source * (sx * sy) + acc / np.float32(case.count)) / norm
        assert flux.dtype == np.float32
        assert_bit_equal(flux, want, "acc64 rounded through the normalisation")
        assert (d["absacc64"] == d["acc64"]).all()          # non-negative sources
        assert ((d["visits"] > 0) >= (d["acc64"] > 0)).all()


@pytest.mark.parametrize("name", ["half_plane_without_source-K1", "half_plane_without_source-K2",
                                  "first_channel_zero-K2", "per_walker_rng-K2"])
def test_walkers_without_source_deposit_nothing(oracle, name):
    case = su._exact(oracle, name)
    d = su.expected(oracle, case)[0][0]
    cells = _spawn_cells(case)
    assert (cells >= 0).all()
    empty = (case.source.reshape(-1, case.source.shape[2])[cells] == 0).all(-1)
    assert ((d["reason"] == oracle.SU_NO_SOURCE) == empty).all()
    assert d["visits"].sum() > 0
    # and with no source anywhere nobody walks: nothing is deposited, every walker still spends its two draws
    only = case.rng.copy()
    none = oracle.solve_uniform_detail(case.flow, np.zeros_like(case.source), case.decay, only, case.scale, case.count)
    assert none["visits"].sum() == 0 and (none["reason"] == oracle.SU_NO_SOURCE).all()
    assert (none["acc64"] == 0).all() and (only["offset"] == case.rng["offset"] + 2).all()


def test_unit_draw_constants(oracle):
    """(seed 1, offset 8418514) makes walker 0 draw exactly 1.0; the offset before it puts the 1.0 on py."""
    for const, which in ((su.UNIT_PX, 0), (su.UNIT_PY, 1)):
        st = oracle.rng_seed(1, *const)
        u = [oracle.rng_uniform(st, [0])[0], oracle.rng_uniform(st, [0])[0]]
        assert u[which] == 1.0 and u[1 - which] < 1.0
    assert find_unit_draws(1, 0, 8418514 - 3000, 8418514 + 3000) == [8418514]
    for const in (su.UNIT_PX, su.UNIT_PY):
        case = su._unit_case(oracle, "kat_unit_%d" % const[1], const, 3)
        d, rng = su.expected(oracle, case)[0]
        assert d["reason"][0] == oracle.SU_DROPPED and (d["reason"][1:] != oracle.SU_DROPPED).all()
        assert rng["offset"][0] == const[1] + 2
        alone = su._unit_case(oracle, "kat_unit_alone_%d" % const[1], const, 1)
        d, rng = su.expected(oracle, alone)[0]
        assert d["visits"].sum() == 0 and (d["acc64"] == 0).all() and rng["offset"][0] == const[1] + 2


def test_every_end_reason_is_reached(oracle):
    """Each way a walk can end occurs in some case of the GPU file, and the counts add up to N."""
    seen = np.zeros(7, np.int64)
    cases = [su._exact(oracle, "gradient-64x32-K1"), su._exact(oracle, "sink-64x32-K1"),
             su._general(oracle, "general-37x53-1-K1", 37, 53, 1, strong=True),
             su._general(oracle, "zero_block-K1", 37, 53, 1, hostile="zero_block"),
             su._unit_case(oracle, "kat_unit_reasons", su.UNIT_PX, 2)]
    for case in cases:
        d = su.expected(oracle, case)[0][0]
        r = su.reasons(d)
        assert r.sum() == len(case.rng) and len(r) == 7
        K = case.source.shape[2]
        assert (d["visits"][..., 0] == d["visits"][..., K - 1]).all()
        assert d["visits"][..., 0].sum() <= (len(case.rng) - r[oracle.SU_DROPPED] - r[oracle.SU_NO_SOURCE]) * sum(case.source.shape[:2])
        seen += r
    assert (seen > 0).all(), seen
