"""Every entry point of include/soil_hip.h held to its bits on a reused, dirty workspace.

csrc/runtime.hip keeps one block per host thread, device and slot; it grows on demand and is never shrunk or cleared.
The parity files call each operation on allocations of its own and judge one call; here the history of a call is the
tested dimension (tests/workspace_history.py: the protocol, the plans, what a failure tells).  Every row of the guard-band
tables (tests/test_gpu_guard_bands.py, tests/test_gpu_guard_bands_erosion.py: the same Case, planes, keys and memoised
references) runs as the last step of

  1 cold       soil_workspace_release(), then the call at the row's largest key: the block is freshly allocated
  2 stale      the call on the decoy image (tests/busy_stream.py: the same layout, other valid inputs) at the same key,
               then on the real image: plausible values of another problem at exactly the addresses the call uses.  The
               rows without an input plane (workspace_history.OUTPUTS_ONLY) use another key instead
  3 shrink     the largest key, the smallest, then (1, 9) or (9, 1); batch rows (3, 65, 67), then (3, 5, 7)
  4 regrow     release, smallest, largest (the block is freed and replaced), smallest again
  5 siblings   every ordered pair of the entries that share a slot (workspace_history.SIBLING_GROUPS), back to back
  6 restless   a predecessor built not to end in a benign state: a graph without a terminal for the pointer-doubling
               entries, an all-NaN and a plateau DEM for the tile relaxations, a hostile model in the last slot of a batch
  7 refusal    the call, a refused call of the same entry, the call again (every row but workspace_history.NO_REFUSAL)
  8 shapes     the particle rows: every ordered pair of launch shapes on one pair row, one predecessor in another shape
               for each other row

Every step is judged: guards and pure inputs unchanged, and on a real image the outputs are the reference of the op's own
test file.  Where the entry has a soil_*_info call, the record after the last step is the cold call's, field by field.
tests/test_workspace_history.py shows without a GPU which history reports which class of mistake.
"""
import pytest

import test_gpu_guard_bands as grid
import workspace_history as wh
from workspace_history import COLD, REFUSAL, REGROW, RELEASE, SHRINK, STALE

ROWS = grid.all_rows()
_COLD = {}          # (entry, key) -> the info record of the call made cold


@pytest.fixture(scope="module")
def library(hip, oracle):
    return wh.SoilLibrary(hip, oracle, ROWS, grid._WANT)


def cold_record(library, entry, key):
    if entry not in wh.INFO:
        return None
    if (entry, key) not in _COLD:
        _COLD[entry, key] = wh.run_history(library, [RELEASE, wh.call(entry, key)], "the cold record")
    return _COLD[entry, key]


def through(library, steps, what):
    last = steps[-1]
    cold = cold_record(library, last.entry, last.key) if last.mode is None else None
    return wh.run_history(library, steps, what, cold)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(ROWS))
def test_cold(library, entry):
    """... twice over where the entry has an info record: two cold calls give one record, the one the other histories
    are held to."""
    steps = wh.plan(COLD, ROWS, entry)
    info = wh.run_history(library, steps, COLD)
    if entry in wh.INFO:
        again = wh.run_history(library, steps, "cold, a second time")
        assert info == again, "two cold calls, two records: %r, %r" % (info, again)
        _COLD[entry, steps[-1].key] = info


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [STALE, SHRINK, REGROW])
@pytest.mark.parametrize("entry", list(ROWS))
def test_history(library, entry, kind):
    through(library, wh.plan(kind, ROWS, entry), kind)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", [e for e in ROWS if e not in wh.NO_REFUSAL])
def test_a_refusal_in_between(library, entry):
    through(library, wh.plan(REFUSAL, ROWS, entry), REFUSAL)


@pytest.mark.gpu
@pytest.mark.parametrize("group,first,second", [pytest.param(g, a, b, id="%s-%s-%s" % (g, a, b))
                                                for g, a, b in wh.sibling_plans(ROWS)])
def test_siblings(library, group, first, second):
    through(library, wh.sibling_plan(ROWS, first, second), "siblings of %s" % group)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,image", wh.restless_plans())
def test_a_predecessor_that_does_not_end_quiet(library, entry, image):
    through(library, wh.restless_plan(ROWS, entry, image), "restless")


@pytest.mark.gpu
@pytest.mark.parametrize("entry,before,shape", [pytest.param(e, a, b, id="%s-%s-then-%s" % (e, a, b))
                                                for e, a, b in wh.shape_plans(ROWS)])
def test_launch_shapes_change_hands(library, entry, before, shape):
    through(library, wh.shape_plan(ROWS, entry, before, shape), "shapes")
