"""Every entry point of include/soil_hip.h held to its result beside a second host thread.

The header: "Several host threads may drive one device at the same time, each on its own stream: they share no scratch
(nor streams, events or pinned words of the launches, which are per thread too)."  The guard-band, busy-stream and
workspace-history files see one caller; here every row of the guard-band tables (tests/test_gpu_guard_bands.py,
tests/test_gpu_guard_bands_erosion.py: the same Case, planes, keys and memoised references) runs on a worker thread
while another worker is inside the library (tests/two_threads.py: the protocol, what a failure tells, what it cannot
see; tests/test_two_threads.py: which part reports which slip).  Per row, at the row's largest key:

  window            the partner is the same row and key on the decoy image (the same slot, sizes and kernels: whatever is
                    shared collides exactly), then the roles swap.  Rows without an input plane take their smallest key
                    as the partner
  free-running      R judged rounds beside the same partner in a loop
  siblings          the window over every ordered pair of the entries that share a slot (workspace_history.SIBLING_GROUPS)
  tiled             the particle rows again in the tiled launch shape, where the forked streams and the pinned record of
                    the tiled engine live; the mode is set before the workers start
  refusal           a refused call of the row on B inside A's window (the rows for which tests/golden/refusal_text.json
                    lists a scalar a row can pass): A's soil_last_error(), record and snapshot stay
  mixed             A walks all rows in table order and B in reverse, each judged, a barrier every 8 rows
  thread end        one row per slot group: B ends inside A's window, a fresh thread then makes B's call
  objects           what a thread made (pinned words, staging, lanes, forked streams, blocks) goes when it ends:
                    soil_host_objects_info returns to where it was, three times over

A row may end "dependent" only if its entry forks private lanes (two_threads.lane_forking_entries, read from csrc/):
their queues cannot be redrawn from outside.  Such a row is printed with the draws made; any other is a failure.
A worker that does not answer ends the whole session: nothing more is started on a device after a hang.
"""
import time

import pytest

import busy_stream as bs
import test_gpu_guard_bands as grid
import test_gpu_on_a_busy_stream as busy
import two_threads as tt
import workspace_history as wh

ROWS = grid.all_rows()
R = 32                      # free-running rounds (profiles/two_threads/checks.txt: how it was chosen)
MODES = [e for e, r in ROWS.items() if getattr(r, "modes", False)]
LANES = tt.lane_forking_entries(bs.ROOT)
DEPENDENT = {}              # row -> draws made, for the rows that ended "dependent" in this session


@pytest.fixture(scope="module")
def dev(hip):
    import torch
    flags = bs.stream_flags(torch.cuda.Stream().cuda_stream)
    assert flags & 1, "torch.cuda.Stream() is no hipStreamNonBlocking stream here (flags %#x)" % flags
    return tt.SoilTwoThreads(hip)


def end_on_stuck(e):
    if isinstance(e, tt.TwoThreadsError) and e.kind == "stuck":
        pytest.exit("a host thread hangs inside the library: %s" % e, returncode=3)


class Pair:
    """Two workers for one test (more with make()); all of them end with it."""

    def __init__(self):
        self.made = []
        self.A, self.B = self.make("A"), self.make("B")

    def make(self, name):
        self.made.append(tt.Worker(name))
        return self.made[-1]

    def close(self):
        for w in self.made:
            try:
                w.end()
            except tt.TwoThreadsError as e:
                end_on_stuck(e)
                raise
        if any(w.stuck for w in self.made):
            pytest.exit("a host thread hangs inside the library", returncode=3)


@pytest.fixture
def pair(dev):
    p = Pair()
    yield p
    p.close()


def role(hip, oracle, worker, entry, key, image="decoy", mode=None):
    """Built on the worker: a reference that is not memoised yet calls the library (the composed rows)."""
    return worker.do(lambda: tt.Role(busy.item_of(hip, oracle, entry, key, mode), entry, image), entry)


def through(entry, fn):
    """`fn()`; "stuck" ends the session; "dependent" passes for a lane-forking entry, and is written down."""
    try:
        return fn()
    except tt.TwoThreadsError as e:
        end_on_stuck(e)
        if e.kind == "dependent" and entry in LANES:
            DEPENDENT[entry] = tt.TRIES
            print("two-threads  dependent  %s: %s" % (entry, e))
            return None
        raise
    except BaseException as e:
        end_on_stuck(e)
        raise


def same_partner(hip, oracle, p, entry, mode=None):
    key = wh.largest(ROWS[entry]) if mode is None else ROWS[entry].cases[0]
    pk = key if mode is not None else tt.partner_key(ROWS, entry, busy.DECOY)
    return role(hip, oracle, p.A, entry, key, mode=mode), role(hip, oracle, p.A, entry, pk, mode=mode)


def both_ways(dev, p, entry, subject, partner, **kw):
    for A, B in ((p.A, p.B), (p.B, p.A)):
        got = through(entry, lambda: tt.window(dev, A, B, subject, partner, **kw))
        if got is None:
            return
        print("two-threads  window  %-60s subject on %s  draws %d  backlog %.1f ms" % (subject.item.what, A.name, got[0], got[1]))


def free(dev, p, entry, subject, partner):
    got = through(entry, lambda: tt.free_running(dev, p.A, p.B, subject, partner, R))
    print("two-threads  free  %-60s rounds %d  calls of the partner %d  overlap %.2f  of the call itself %.2f" % (
        subject.item.what, got["rounds"], got["calls"], got["overlap"], got["call_overlap"]))


# ------------------------------------------------------------------ the rows

@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(ROWS))
def test_window(hip, oracle, dev, pair, entry):
    subject, partner = same_partner(hip, oracle, pair, entry)
    both_ways(dev, pair, entry, subject, partner)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(ROWS))
def test_free_running(hip, oracle, dev, pair, entry):
    subject, partner = same_partner(hip, oracle, pair, entry)
    free(dev, pair, entry, subject, partner)


@pytest.mark.gpu
@pytest.mark.parametrize("group,first,second", [pytest.param(g, a, b, id="%s-%s-beside-%s" % (g, a, b))
                                                for g, a, b in tt.sibling_plans(ROWS)])
def test_window_beside_a_sibling(hip, oracle, dev, pair, group, first, second):
    subject = role(hip, oracle, pair.A, first, wh.sibling_key(ROWS[first]))
    partner = role(hip, oracle, pair.A, second, wh.sibling_key(ROWS[second]))
    got = through(first, lambda: tt.window(dev, pair.A, pair.B, subject, partner))
    if got is not None:
        print("two-threads  sibling  %-50s beside %-50s draws %d" % (subject.item.what, partner.item.what, got[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", MODES)
def test_the_particle_rows_in_the_tiled_launch_shape(hip, oracle, dev, entry):
    with wh.launch_shape(hip, "tiled"):             # (process-wide: set before the workers start)
        p = Pair()
        try:
            subject, partner = same_partner(hip, oracle, p, entry, "tiled")
            both_ways(dev, p, entry, subject, partner)
            free(dev, p, entry, subject, partner)
        finally:
            p.close()


REFUSED = [e for e in ROWS if e not in wh.NO_REFUSAL and wh.bad_scalar(e) is not None]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", REFUSED)
def test_a_refusal_next_door(hip, oracle, dev, pair, entry):
    assert wh.listed_refusals(entry)
    subject, partner = same_partner(hip, oracle, pair, entry)
    both_ways(dev, pair, entry, subject, partner, refusal=True)


@pytest.mark.gpu
def test_all_rows_in_table_order_beside_all_rows_in_reverse(hip, oracle, dev, pair):
    roles = [role(hip, oracle, pair.A, e, k, "real") for e, k in tt.subject_plans(ROWS)]
    assert through(None, lambda: tt.mixed(dev, pair.A, pair.B, roles)) == 2 * len(ROWS)


# ------------------------------------------------------------------ a thread's end

@pytest.mark.gpu
@pytest.mark.parametrize("group,entry", tt.end_plans(ROWS))
def test_a_thread_ends_next_door(hip, oracle, dev, pair, group, entry):
    key = wh.sibling_key(ROWS[entry])
    subject, partner = role(hip, oracle, pair.A, entry, key), role(hip, oracle, pair.A, entry, key, "real")
    through(entry, lambda: tt.thread_end(dev, pair.A, pair.B, lambda: pair.make("C"), subject, partner))


OWNERS = ["soil_fill_depressions", "soil_flat_distance", "soil_slope_limit", "soil_mfd_accumulate", "soil_stream_order",
          "soil_multiflow", "soil_slope_batch"]                         # five flag words, the lanes, an upload
TILED_PAIR = "soil_particles_pair_colour"                               # the forked streams and the pinned record


def settled(dev, want):
    """join() returns when the Python function has; the thread_local destructors run a moment later."""
    now = dev.host_objects()
    for _ in range(40):
        if now == want:
            break
        time.sleep(0.05)
        last, now = now, dev.host_objects()
        if want is None and now == last:
            break
    return now


@pytest.mark.gpu
def test_what_a_thread_made_goes_with_the_thread(hip, oracle, dev):
    """One call of each entry that owns per-thread objects on a thread that then ends: the live counts of streams,
    events, pinned allocations and blocks are what they were before, three lifetimes in a row."""
    assert set(OWNERS + [TILED_PAIR]) <= set(ROWS) and busy.uploads(OWNERS[-1])
    with wh.launch_shape(hip, "tiled"):
        maker = tt.Worker("references")             # (the references, made once, on a thread that ends before the count)
        try:
            roles = [role(hip, oracle, maker, e, wh.sibling_key(ROWS[e]), "real") for e in OWNERS]
            roles.append(role(hip, oracle, maker, TILED_PAIR, ROWS[TILED_PAIR].cases[0], "real", "tiled"))
        finally:
            maker.end()
        before = settled(dev, None)
        grew = None
        for life in range(3):
            w = tt.Worker("life %d" % life)
            try:
                def calls():
                    for r in roles:
                        s = tt._warm(dev, r, "thread-end", False)
                        del s
                    return dev.host_objects()
                inside = through(None, lambda: w.do(calls, "one call of each owner"))
            finally:
                w.end()
            grew = tuple(a - b for a, b in zip(inside, before))
            after = settled(dev, before)
            print("two-threads  objects  life %d: before %r, inside the thread %r, after it %r" % (life, before, inside, after))
            assert after == before, "streams, events, pinned allocations, blocks: %r before the thread, %r after it (life %d)" % (
                before, after, life)
        # ... and the count has power: the thread did hold lanes, forked streams, their events, pinned words and blocks
        # (two lanes and two forked streams; 2 * 2 + 3 and 3 events and the staging's; five words, the staging, a record
        # for either kind of tiled launch; a block per slot taken)
        assert grew[0] >= 4 and grew[1] >= 11 and grew[2] >= 8 and grew[3] >= 8, grew


# ------------------------------------------------------------------ without a GPU

def test_every_entry_point_that_takes_a_stream_is_a_subject():
    """The subjects and the exemptions of the busy-stream file (the harness's own tools, the two host counters: global
    by design, tests/two_threads.py) partition the entries of include/soil_hip.h whose prototype ends in `void* stream`."""
    entries = set(bs.stream_entries())
    subjects = {e for e, _ in tt.subject_plans(ROWS)}
    reasons = dict(busy.EXEMPT)
    assert not subjects & set(reasons)
    missing = sorted(entries - subjects - set(reasons))
    assert not missing, "entries that take a stream and are neither a subject nor listed with a reason: %s" % missing
    assert all(reasons[e] for e in reasons) and set(reasons) <= entries
    assert set(MODES) <= subjects and set(REFUSED) <= subjects and len(REFUSED) == 18


@pytest.mark.gpu
def test_only_lane_forking_rows_ended_dependent():
    """(runs last in the file)  through() has already failed every other row that ended "dependent"."""
    assert set(DEPENDENT) <= set(LANES) and len(DEPENDENT) <= len(LANES), (sorted(DEPENDENT), LANES)
    print("two-threads  dependent rows: %s" % (", ".join("%s (%d draws)" % kv for kv in sorted(DEPENDENT.items())) or "none"))
