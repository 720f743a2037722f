"""The protocol of tests/busy_stream.py against stand-ins, without a GPU: what it reports for a correct op and for
each class of ordering mistake it is there to catch.  This is the proof that tests/test_gpu_on_a_busy_stream.py would
notice such a mistake: the GPU tests run the same protocol through the same device interface.

The stand-in device: a stream is a FIFO queue of closures over numpy images; the device runs whatever can run as soon
as it is queued.  A backlog is a gate that blocks its queue until somebody synchronises; a wait blocks its queue
until its event has run.  The null stream is a queue like any other: a non-blocking stream is not ordered against it.

The op under test is out = scale * a + b on (H, W) float32 planes; `scale` is a host value (2 unless a chain says
otherwise), which the staged variants send through one shared host staging word.
"""
import numpy as np
import pytest

import busy_stream as bs
import guard_arena as ga
from guard_arena import IN, OUT, Arena

H, W = 9, 13


class Event:
    done = False


class Sim:
    NULL = "null"

    def __init__(self, lane_first=False, shared=0):
        """shared: the first `shared` streams drawn share the null stream's hardware queue, i.e. ARE its queue."""
        self.queues, self.lane_first, self.shared, self.drawn = {"null": []}, lane_first, shared, 0
        self.staging = [np.float32(0)]          # the library's one host staging word

    # ---- the queues
    def _put(self, s, kind, payload):
        self.queues[s].append((kind, payload))
        self._pump()

    def _pump(self):
        """One task at a time, always of the first queue (in priority order) whose head can run."""
        while True:
            names = list(self.queues)
            for name in (names[::-1] if self.lane_first else names):
                q = self.queues[name]
                if q and not (q[0][0] in ("gate", "wait") and not q[0][1].done):
                    kind, payload = q.pop(0)
                    if kind == "run":
                        payload()
                    elif kind == "event":
                        payload.done = True
                    break
            else:
                return

    def run_on(self, s, fn):
        self._put(s, "run", fn)

    def wait(self, s, event):
        self._put(s, "wait", event)

    def lane(self):
        name = "lane%d" % len(self.queues)
        self.queues[name] = []
        return name

    # ---- the device interface of busy_stream
    def stream(self):
        self.drawn += 1
        return "null" if self.drawn <= self.shared else self.lane()

    def image(self, host):
        return np.array(host, np.uint8)

    def read(self, image):
        return image.copy()

    def copy(self, dst, src, nbytes, s):
        self.run_on(s, lambda: dst.__setitem__(slice(0, nbytes), src[:nbytes]))

    def call(self, item, image, s):
        def view(name):
            p = item.arena.plane(name)
            return image[p.start:p.start + p.nbytes].view(p.dtype).reshape(p.shape)
        item.call(self, view, s)

    def backlog(self, s, ms):
        self._put(s, "gate", Event())

    def record(self, s):
        e = Event()
        self._put(s, "event", e)
        return e

    def done(self, event):
        return event.done

    def idle(self, s):
        return not self.queues[s]

    def overtakes(self, behind):
        e = self.record(self.NULL)
        if not e.done:                      # the host waits for the null stream, which waits for the backlog
            self.synchronize(self.NULL)
        return not behind.done

    def _open(self, names):
        for name in names:
            for kind, payload in self.queues[name]:
                if kind == "gate":
                    payload.done = True
        self._pump()

    def synchronize(self, s):
        self._open([s])
        assert not self.queues[s], "a stream that waits for something nobody will ever record"

    def synchronize_all(self):
        self._open(list(self.queues))
        assert not any(self.queues.values())


# ------------------------------------------------------------------ the stand-in "libraries"

def kernel(view, scale):
    def k():
        view("out")[:] = np.float32(scale()) * view("a") + view("b")
    return k


def good(scale=2.0):
    def call(dev, view, s):
        dev.run_on(s, kernel(view, lambda: scale))          # (the scale travels in the launch arguments)
    return call


def on_the_null_stream(dev, view, s):
    dev.run_on(dev.NULL, kernel(view, lambda: 2.0))


def lane_that_never_waits(dev, view, s):
    lane = dev.lane()
    dev.run_on(lane, kernel(view, lambda: 2.0))
    dev.wait(s, dev.record(lane))                            # joined back, but it never waited for the caller's stream


def lane_never_joined(dev, view, s):
    lane = dev.lane()
    dev.wait(lane, dev.record(s))
    dev.run_on(lane, kernel(view, lambda: 2.0))             # ... and the caller's stream goes on without it


def staged(scale, careful):
    """The scale goes through the shared staging word and one stream-ordered copy.  careful: the host waits for the
    copy before it returns (what an event per upload is for); else the next call rewrites the word before the copy ran."""
    def call(dev, view, s):
        dev.staging[0] = np.float32(scale)
        on_device = [None]
        dev.run_on(s, lambda: on_device.__setitem__(0, dev.staging[0]))
        if careful:
            dev.synchronize(s)
        dev.run_on(s, kernel(view, lambda: on_device[0]))
    return call


def synchronising(dev, view, s):
    dev.run_on(s, kernel(view, lambda: 2.0))
    dev.synchronize(s)


# ------------------------------------------------------------------ items

def item(call, scale=2.0, synchronises=None, decoy=None, seed=0):
    r = np.random.default_rng(seed)
    a, b = r.random((H, W)).astype(np.float32), r.random((H, W)).astype(np.float32)
    arena = Arena("aligned", "A").add("a", a, IN).add("out", (H, W), OUT, dtype=np.float32).add("b", b, IN).build()
    want = np.float32(scale) * a + b

    def judge(snap):
        ga.assert_bits(arena.read("out", snap), want, "out")
    return bs.Item("stand-in", arena, bs.decoy_bytes(arena) if decoy is None else decoy, call, judge, synchronises)


def reported(call, kind, lane_first=False, **kw):
    with pytest.raises(bs.BusyStreamError) as e:
        bs.run(Sim(lane_first), item(call, **kw))
    assert e.value.kind == kind, str(e.value)
    return e.value


# ------------------------------------------------------------------ the tests

def test_a_correct_op_passes():
    for lane_first in (False, True):
        rec = bs.run(Sim(lane_first), item(good()))
        assert not rec.behind_done and not rec.idle and rec.backlog_ms >= bs.FLOOR_MS


def test_the_decoy_rule():
    g = np.arange(H * W, dtype=np.int32).reshape(H, W)
    m = (g % 3 == 0).astype(np.int32)
    rng = np.zeros(5, ga.RNG)
    rng["offset"] = np.arange(5)
    a = np.arange(H * W * 2, dtype=np.float32).reshape(H, W, 2)
    arena = Arena("aligned", "A").add("a", a, IN).add("graph", g, IN, fills=(0, H * W - 1)).add("mask", m, IN, fills=(0, 1))
    arena.add("rng", rng, ga.INOUT).add("out", (H, W), OUT, dtype=np.float64).build()
    d = bs.decoy_bytes(arena)
    assert ga.bits_equal(arena.read("a", d), a.reshape(-1)[::-1].reshape(a.shape))
    assert (arena.read("graph", d) == -1).all() and ga.bits_equal(arena.read("mask", d), m)
    assert ga.bits_equal(arena.read("rng", d), rng[::-1]) and ga.bits_equal(arena.read("out", d), arena.read("out", arena.host))
    outside = np.ones(arena.size, bool)
    for p in arena.planes:
        outside[p.start:p.start + p.nbytes] = False
    assert (d[outside] == arena.host[outside]).all(), "a decoy differs from the real image inside its planes only"


def test_a_kernel_on_the_null_stream_is_reported():
    e = reported(on_the_null_stream, "mismatch")
    assert "out" in str(e)


def test_a_side_stream_that_never_waits_for_the_callers_is_reported():
    for lane_first in (False, True):
        reported(lane_that_never_waits, "mismatch", lane_first)


def test_a_side_stream_that_is_never_joined_back_is_reported():
    """Caller's stream first: the lane's result misses the snapshot (e) and is computed from the decoys of the
    clobber (f).  Lane first: it happens to finish in time, the race the protocol cannot see on a stand-in whose
    kernels are atomic; on the device the clobber is what turns a lane still running at (e) into wrong numbers."""
    dev = Sim()
    it = item(lane_never_joined)
    with pytest.raises(bs.BusyStreamError) as e:
        bs.run(dev, it)
    assert e.value.kind == "mismatch" and "out" in str(e.value)
    # through the snapshot: the plane still held the guard pattern when it was taken
    assert "nan" in str(e.value).lower()
    bs.run(Sim(lane_first=True), item(lane_never_joined))


def test_the_clobber_feeds_decoys_to_work_left_behind():
    """The same lane, looked at from the other side: what it wrote after (f) is the decoy's result, not the real one."""
    it = item(lane_never_joined)
    dev, seen = Sim(), {}
    plain_call = dev.call

    def call(item_, image, s):
        seen["live"] = image
        plain_call(item_, image, s)
    dev.call = call
    with pytest.raises(bs.BusyStreamError):
        bs.run(dev, it)
    p = it.arena.plane("a")
    a = it.arena.read("a", it.decoy)
    b = it.arena.read("b", it.decoy)
    ga.assert_bits(it.arena.read("out", seen["live"]), np.float32(2.0) * a + b, "what the lane left in the live image")
    assert p.role == IN


def test_a_staging_word_rewritten_before_its_copy_ran_is_reported_in_the_chain():
    scales = (2.0, 3.0, 0.5)
    ok = [item(staged(sc, True), sc, synchronises="stream", seed=i) for i, sc in enumerate(scales)]
    recs = bs.run_chain(Sim(), ok)
    assert len(recs) == 3
    bad = [item(staged(sc, False), sc, seed=i) for i, sc in enumerate(scales)]
    with pytest.raises(bs.BusyStreamError) as e:
        bs.run_chain(Sim(), bad)
    assert (e.value.kind, e.value.item) == ("mismatch", 0), str(e.value)       # call 0 got the scale of the last call
    # alone, each of them passes: only the chain holds the shared staging
    for it in bad:
        bs.run(Sim(), it)
    # ... and launch arguments need no staging at all
    bs.run_chain(Sim(), [item(good(sc), sc, seed=i) for i, sc in enumerate(scales)])


def test_an_op_that_synchronises_without_saying_so_is_reported():
    e = reported(synchronising, "synchronised")
    assert "backlog" in str(e) and "ms" in str(e)
    for how in ("stream", "return"):
        rec = bs.run(Sim(), item(synchronising, synchronises=how))
        assert rec.behind_done and rec.idle


def test_an_op_said_to_synchronise_that_returns_with_work_pending_is_reported():
    reported(good(), "ahead", synchronises="return")
    reported(good(), "ahead", synchronises="stream")       # it did not even wait for the work ahead of it

    def waits_then_goes_on(dev, view, s):                   # a host look in the middle, more launches after it
        dev.synchronize(s)
        dev.run_on(s, kernel(view, lambda: 2.0))
        dev.backlog(s, 1.0)
    reported(waits_then_goes_on, "pending", synchronises="return")
    rec = bs.run(Sim(), item(waits_then_goes_on, synchronises="stream"))
    assert rec.behind_done and not rec.idle


def test_a_stream_that_shares_the_null_streams_queue_is_not_used():
    """On such a stream a launch on the null stream is ordered by accident and would pass; the protocol looks whether
    the null stream overtakes the backlog, draws another stream if not, and gives up loudly if none does."""
    dev = Sim(shared=2)
    with pytest.raises(bs.BusyStreamError) as e:
        bs.run(dev, item(on_the_null_stream))
    assert e.value.kind == "mismatch" and e.value.records[0].draws == 3
    assert bs.run(Sim(shared=1), item(good())).draws == 2
    with pytest.raises(bs.BusyStreamError) as e:
        bs.run(Sim(shared=bs.TRIES), item(good()))
    assert e.value.kind == "dependent"
    # what the look is there for: without it, the shared stream hides the mistake
    blind = Sim(shared=1)
    blind.overtakes = lambda behind: True
    bs.run(blind, item(on_the_null_stream))


def test_a_chain_gets_a_fresh_backlog_behind_a_call_that_drained_the_stream():
    recs = bs.run_chain(Sim(), [item(good()), item(synchronising, synchronises="return", seed=1), item(good(), seed=2),
                                item(good(), seed=3)])
    assert [r.held for r in recs] == [True, False, True, False]
    assert [r.behind_done for r in recs] == [False, True, False, False]
    with pytest.raises(bs.BusyStreamError) as e:            # ... and the call right behind it is held to the new event
        bs.run_chain(Sim(), [item(synchronising, synchronises="stream"), item(synchronising, seed=1)])
    assert (e.value.kind, e.value.item) == ("synchronised", 1)


def test_only_the_first_call_of_a_chain_is_held_to_the_event():
    bs.run_chain(Sim(), [item(good()), item(synchronising, synchronises="stream", seed=1)])
    with pytest.raises(bs.BusyStreamError) as e:
        bs.run_chain(Sim(), [item(synchronising), item(good(), seed=1)])
    assert (e.value.kind, e.value.item) == ("synchronised", 0)


def test_a_decoy_equal_to_the_real_input_is_refused_as_powerless():
    it = item(good())
    e = reported(good(), "powerless", decoy=it.arena.host.copy())
    assert "has no power" in str(e)


def test_an_op_that_is_wrong_on_the_null_stream_already_is_a_warmup_failure():
    reported(good(2.5), "warmup")


def test_a_store_outside_the_planes_on_the_stream_is_a_guard_failure():
    def call(dev, view, s):
        good()(dev, view, s)
        dev.run_on(s, lambda: view("b").__setitem__((0, 0), 0.0) if s != dev.NULL else None)
    reported(call, "guard")


def test_the_backlog_has_a_floor_and_a_cap():
    assert bs.backlog_ms(0.01) == bs.FLOOR_MS and bs.backlog_ms(5.0) == 50.0 and bs.backlog_ms(500.0) == bs.CAP_MS


def test_the_proxy_substitutes_the_stream_and_holds_the_rows_to_none():
    class Lib:
        def soil_thing(self, a, stream):
            return (a, stream)

        def soil_other(self, a):
            return a
    p = bs.StreamProxy(Lib(), "S", ["soil_thing"])
    assert p.soil_thing(1, None) == (1, "S") and p.soil_other(2) == 2
    with pytest.raises(AssertionError):
        p.soil_thing(1, "mine")


def test_the_header_names_the_entries_that_take_a_stream():
    from soillib_amd import _abi
    entries = bs.stream_entries()
    assert "soil_erode_step_batch_models" in entries and "soil_memcpy_d2d" in entries and "soil_stream_synchronize" in entries
    assert "soil_malloc" not in entries and "soil_device_synchronize" not in entries and "soil_event_elapsed_ms" not in entries
    assert set(entries) <= set(_abi.SIGNATURES)
    import ctypes as C
    for e in entries:
        assert _abi.SIGNATURES[e][1][-1] is C.c_void_p, e
