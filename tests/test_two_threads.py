"""The protocol of tests/two_threads.py against a numpy stand-in, without a GPU: what it reports for a correct
library and for each way of sharing between host threads what belongs to one.  This is the proof that
tests/test_gpu_two_host_threads.py would notice such a slip: the GPU tests run the same protocol through the same
interface.

The stand-in device: a stream is a FIFO queue of closures over numpy images, drained by one "device" thread that takes
one closure at a time from the streams in turn; a backlog is a gate that opens after its time.  The stand-in library
keeps, per threading.get_ident(): a scratch block, a pinned staging word, a pinned flag word, an info record and an
error text.  Its two entries:

  scaled(k)   out = k * a + 1 in three queued steps: the upload of k from the staging word (read when the copy runs, as
              a pinned buffer is), scratch = k * a, out = scratch + 1.  Stream-ordered.  k < 0 is refused.
  relax       out = the running maximum of a, one cell further per pass, until a pass changes nothing: the host clears
              the flag word, queues a pass, synchronises and looks at the word, as the tile relaxations do; the number
              of passes goes into the plane `passes` and the info record.  Synchronises before it returns.
"""
import threading
import time

import numpy as np
import pytest

import busy_stream as bs
import guard_arena as ga
import two_threads as tt
from guard_arena import IN, OUT, Arena

N = 24
R = 32              # free-running rounds against the stand-in: its calls are microseconds long


class Refused(ValueError):
    pass


class Event:
    done = False


class Block:
    def __init__(self, n):
        self.data, self.k, self.live = np.zeros(n, np.float32), np.zeros(1, np.float32), True

    def free(self):
        self.data[:], self.k[:], self.live = np.nan, np.nan, False


class Sim:
    """The device and the library.  `slip`: None, "scratch", "staging", "flag", "info", "error-text" (one for all
    threads instead of one per thread) or "thread-end" (a thread's end frees every thread's blocks, at once)."""
    NULL = "null"

    def __init__(self, slip=None):
        self.slip = slip
        self.cv = threading.Condition()
        self.queues, self.running, self.turn = {"null": []}, None, 0
        self.scratch, self.staging, self.flags, self.infos, self.errors = {}, {}, {}, {}, {}
        threading.Thread(target=self._device, name="stand-in device", daemon=True).start()

    # ---- the device thread
    def _next(self):
        names = list(self.queues)
        for i in range(len(names)):
            name = names[(self.turn + i) % len(names)]
            q = self.queues[name]
            if q and not (q[0][0] == "gate" and time.monotonic() < q[0][1]):
                self.turn = (self.turn + i + 1) % len(names)
                return name, q.pop(0)
        return None

    def _device(self):
        while True:
            with self.cv:
                job = self._next()
                if job is None:
                    self.cv.wait(0.0005)
                    continue
                self.running = job[0]
            kind, payload = job[1]
            if kind == "run":
                payload()
            elif kind == "event":
                payload.done = True
            with self.cv:
                self.running = None
                self.cv.notify_all()

    def _put(self, s, kind, payload):
        with self.cv:
            self.queues[s].append((kind, payload))
            self.cv.notify_all()

    def run_on(self, s, fn):
        self._put(s, "run", fn)

    # ---- the device interface
    def stream(self):
        with self.cv:
            name = "s%d" % len(self.queues)
            self.queues[name] = []
        return name

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
        self._put(s, "gate", time.monotonic() + ms * 1e-3)

    def record(self, s):
        e = Event()
        self._put(s, "event", e)
        return e

    def done(self, event):
        return event.done

    def synchronize(self, s):
        with self.cv:
            while self.queues[s] or self.running == s:
                self.cv.wait(0.01)

    def synchronize_all(self):
        for s in list(self.queues):
            self.synchronize(s)

    # ---- the library's per-thread state
    def _key(self, what):
        return 0 if self.slip == what else threading.get_ident()

    def scratch_of(self, n):
        key = self._key("scratch")
        b = self.scratch.get(key)
        if b is None or not b.live or b.data.size < n:
            b = self.scratch[key] = Block(n)
        return b

    def staging_of(self):
        return self.staging.setdefault(self._key("staging"), np.zeros(1, np.float32))

    def flag_of(self):
        return self.flags.setdefault(self._key("flag"), np.zeros(1, np.int32))

    def set_info(self, entry, record):
        self.infos[self._key("info"), entry] = record

    def info(self, entry):
        return self.infos.get((self._key("info"), entry))

    def fail(self, text):
        self.errors[self._key("error-text")] = text
        raise Refused(text)

    def error_text(self):
        return self.errors.get(self._key("error-text"), "")

    def mark_error(self):
        try:
            self.fail("host_objects_info: null record")
        except Refused:
            return self.error_text()

    def refuse(self, role, image, s):
        try:
            role.item.refused(self, s)
        except Refused:
            return
        raise AssertionError("%s was not refused" % role.entry)

    def thread_exit(self):
        """What the library does when a host thread ends: waits for the device, then frees the thread's blocks."""
        if self.slip == "thread-end":
            for b in self.scratch.values():
                b.free()
            return
        self.synchronize_all()
        b = self.scratch.pop(threading.get_ident(), None)
        if b is not None:
            b.free()


# ------------------------------------------------------------------ the stand-in library's entries

def scaled(k):
    def call(dev, view, s):
        if k < 0:
            dev.fail("scaled: k must not be negative")
        st, b = dev.staging_of(), dev.scratch_of(N)
        st[0] = k

        def upload():
            b.k[0] = st[0]

        def first():
            if b.live:
                b.data[:N] = b.k[0] * view("a")

        def second():
            view("out")[:] = b.data[:N] + np.float32(1)
        for fn in (upload, first, second):
            dev.run_on(s, fn)
        dev.set_info("scaled", (3, int(k)))
    return call


def relax(dev, view, s):
    flag = dev.flag_of()
    dev.run_on(s, lambda: view("out").__setitem__(slice(None), view("a")))

    def one_pass():
        o = view("out")
        new = np.maximum(o, np.concatenate((o[:1], o[:-1])))
        if (new != o).any():
            flag[0] = 1
        o[:] = new
    passes = 0
    while passes < 4 * N:
        flag[0] = 0
        dev.run_on(s, one_pass)
        dev.synchronize(s)
        passes += 1
        if not flag[0]:
            break
    dev.run_on(s, lambda: view("passes").__setitem__(0, passes))
    dev.synchronize(s)
    dev.set_info("relax", (passes,))


def a_plane(seed):
    return np.random.default_rng(seed).random(N).astype(np.float32) + np.float32(0.5)


def role_scaled(k, seed=1, image="decoy"):
    a = a_plane(seed)
    arena = Arena("aligned", "A", "numpy").add("a", a, IN).add("out", (N,), OUT, dtype=np.float32).build()
    want = np.float32(k) * a + np.float32(1)

    def judge(snap):
        ga.assert_bits(arena.read("out", snap), want, "scaled(%g): out" % k)
    item = bs.Item("scaled(%g)" % k, arena, bs.decoy_bytes(arena), scaled(k), judge)
    item.refused = lambda dev, s: scaled(-1.0)(dev, None, s)
    return tt.Role(item, "scaled", image)


def role_relax(image="decoy"):
    a = np.arange(N, dtype=np.float32) + np.float32(1)             # rising: one pass; its decoy falls: N passes
    arena = Arena("aligned", "A", "numpy").add("a", a, IN).add("out", (N,), OUT, dtype=np.float32)
    arena.add("passes", (1,), OUT, dtype=np.float32).build()

    def judge(snap):
        ga.assert_bits(arena.read("out", snap), np.maximum.accumulate(a), "relax: out")
        ga.assert_bits(arena.read("passes", snap), np.array([1], np.float32), "relax: passes")
    return tt.Role(bs.Item("relax", arena, bs.decoy_bytes(arena), relax, judge, "return"), "relax", image)


@pytest.fixture
def workers():
    made = []

    def make(dev, name):
        made.append(tt.Worker(name, at_exit=dev.thread_exit, limit=20.0))
        return made[-1]
    yield make
    for w in made:
        w.end()


def both_ways(dev, A, B, subject, partner, **kw):
    tt.window(dev, A, B, subject, partner, **kw)
    tt.window(dev, B, A, subject, partner, **kw)


# ------------------------------------------------------------------ the stand-in as written passes

def test_the_stand_in_passes_every_part(workers):
    dev = Sim()
    A, B = workers(dev, "A"), workers(dev, "B")
    for subject, partner in ((role_scaled(2.0), role_scaled(2.0)), (role_scaled(2.0), role_scaled(3.0, seed=2)),
                             (role_relax(), role_relax()), (role_relax(), role_scaled(3.0)), (role_scaled(2.0), role_relax())):
        both_ways(dev, A, B, subject, partner)
        got = tt.free_running(dev, A, B, subject, partner, R)
        assert got["rounds"] == R and got["calls"] >= 1 and 0.0 < got["overlap"] <= 1.0, got
    both_ways(dev, A, B, role_scaled(2.0), role_scaled(3.0), refusal=True)
    both_ways(dev, A, B, role_relax(), role_scaled(3.0), refusal=True)
    roles = [role_scaled(k, seed=k) for k in range(1, 12)] + [role_relax()]
    assert tt.mixed(dev, A, B, roles) == 2 * len(roles)
    C = tt.thread_end(dev, A, B, lambda: workers(dev, "C"), role_scaled(2.0), role_scaled(3.0, image="real"))
    tt.window(dev, A, C, role_scaled(2.0), role_scaled(3.0))
    assert sorted(dev.scratch) == sorted(w._t.ident for w in (A, C)), "a thread's block went with it, and only its own"


# ------------------------------------------------------------------ each slip is caught, by the part and kind named

def caught(kinds, part, fn):
    with pytest.raises(tt.TwoThreadsError) as e:
        fn()
    assert e.value.kind in kinds and e.value.part == part, str(e.value)
    return e.value


def test_one_scratch_for_all_threads(workers):
    """... passes the window (the partner's call runs whole while the subject's is held back) and is a mismatch of
    the free-running part, where the two sequences interleave on the device."""
    dev = Sim("scratch")
    A, B = workers(dev, "A"), workers(dev, "B")
    both_ways(dev, A, B, role_scaled(2.0), role_scaled(2.0))
    e = caught(("mismatch",), "free-running", lambda: tt.free_running(dev, A, B, role_scaled(2.0), role_scaled(2.0), R))
    assert "scaled(2): out" in str(e)


def test_one_staging_record_for_all_threads(workers):
    """The partner rewrites the word while the subject's copy from it is queued: the window's mismatch (behind an
    event that makes the partner wait for the copy, it would be "dependent")."""
    dev = Sim("staging")
    A, B = workers(dev, "A"), workers(dev, "B")
    caught(("mismatch", "dependent"), "window", lambda: tt.window(dev, A, B, role_scaled(2.0), role_scaled(3.0, seed=2)))


def test_one_flag_word_for_all_threads(workers):
    """The partner's passes set the word the subject looks at (or its host clears it): a pass too many or too few.
    The window cannot see it: the subject sits inside its call behind the backlog while the partner runs."""
    dev = Sim("flag")
    A, B = workers(dev, "A"), workers(dev, "B")
    tt.window(dev, A, B, role_relax(), role_relax())
    caught(("mismatch",), "free-running", lambda: tt.free_running(dev, A, B, role_relax(), role_relax(), R))


def test_a_global_info_record(workers):
    dev = Sim("info")
    A, B = workers(dev, "A"), workers(dev, "B")
    e = caught(("info",), "window", lambda: tt.window(dev, A, B, role_relax(), role_relax()))
    assert "(1,)" in str(e) and "(%d,)" % N in str(e)              # the rising image's record against the falling one's


def test_a_global_error_text(workers):
    dev = Sim("error-text")
    A, B = workers(dev, "A"), workers(dev, "B")
    tt.window(dev, A, B, role_scaled(2.0), role_scaled(3.0))        # (without a refusal nothing shows)
    e = caught(("error-text",), "window", lambda: tt.window(dev, A, B, role_scaled(2.0), role_scaled(3.0), refusal=True))
    assert "host_objects_info" in str(e) and "k must not be negative" in str(e)


def test_a_threads_end_that_frees_every_threads_blocks(workers):
    dev = Sim("thread-end")
    A, B = workers(dev, "A"), workers(dev, "B")
    caught(("mismatch",), "thread-end",
           lambda: tt.thread_end(dev, A, B, lambda: workers(dev, "C"), role_scaled(2.0), role_scaled(3.0, image="real")))


def test_a_wrong_result_is_a_warmup_error_and_a_store_past_a_plane_a_guard_error(workers):
    dev = Sim()
    A, B = workers(dev, "A"), workers(dev, "B")
    wrong = role_scaled(2.0)
    wrong.item.call = scaled(2.5)
    caught(("warmup",), "window", lambda: tt.window(dev, A, B, wrong, role_scaled(2.0)))
    stray, warm = role_scaled(2.0), []

    def call(d, view, s):
        scaled(2.0)(d, view, s)
        if warm:                                    # (past the warm-up: on the stream, one element past the plane)
            o = view("out")
            past = np.lib.stride_tricks.as_strided(o, shape=(N + 1,), strides=o.strides)
            d.run_on(s, lambda: past.__setitem__(N, np.float32(7)))
        warm.append(1)
    stray.item.call = call
    e = caught(("guard",), "window", lambda: tt.window(dev, A, B, stray, role_scaled(2.0)))
    assert "'out'" in str(e) and "0 bytes past its last byte" in str(e)


def test_a_worker_that_does_not_answer_is_stuck():
    w = tt.Worker("slow", limit=0.05)
    release = threading.Event()
    with pytest.raises(tt.TwoThreadsError) as e:
        w.do(lambda: release.wait(5.0), "a closure that outlasts the limit")
    release.set()
    assert e.value.kind == "stuck" and w.stuck
    with pytest.raises(AssertionError, match="nothing more is asked"):
        w.start(lambda: None)
    w.end()                                         # (left alone: no join, no error)


def test_an_exception_on_a_worker_comes_back_as_it_is():
    w = tt.Worker("w")
    with pytest.raises(ZeroDivisionError):
        w.do(lambda: 1 // 0)
    assert w.do(lambda: threading.current_thread().name) == "two-threads-w"
    w.end()


def test_overlap_share():
    assert tt.overlap_share([[(0, 10)], [(20, 30)]], [(5, 6), (40, 50)]) == 0.5
    assert tt.overlap_share([[(0, 10)]], [(10, 20)]) == 0.0
    assert tt.overlap_share([], [(0, 1)]) == 0.0


# ------------------------------------------------------------------ the counter (include/soil_hip.h)

def test_host_objects_info_needs_no_device_and_refuses_a_null_record():
    import ctypes as C
    from soillib_amd import _abi
    lib = _abi.lib()
    assert _abi.SIGNATURES["soil_host_objects_info"] == (C.c_int, [C.POINTER(C.c_int64)])
    words = (C.c_int64 * 4)(-1, -1, -1, -1)
    seen = {}

    def on_a_thread():
        seen["rc"] = lib.soil_host_objects_info(words)
        seen["null"] = lib.soil_host_objects_info(None)
        seen["text"] = lib.soil_last_error().decode()
    t = threading.Thread(target=on_a_thread)
    t.start()
    t.join()
    assert seen["rc"] == _abi.SOIL_OK and all(w >= 0 for w in words), list(words)
    if lib.soil_device_count() == 0:
        assert list(words) == [0, 0, 0, 0]          # nothing is made without a device
    assert seen["null"] == _abi.SOIL_ERR_INVALID_ARGUMENT and seen["text"] == "host_objects_info: null record"


# ------------------------------------------------------------------ the plans of the GPU file

def test_every_row_is_a_subject_and_every_sibling_pair_an_ordered_pair():
    import test_gpu_guard_bands as grid
    import test_gpu_two_host_threads as gpu
    import workspace_history as wh
    rows = grid.all_rows()
    assert [e for e, _ in tt.subject_plans(rows)] == list(rows)
    for test in (gpu.test_window, gpu.test_free_running):
        ids = [p for m in test.pytestmark if m.name == "parametrize" for p in m.args[1]]
        assert ids == list(rows), test.__name__
    pairs = [(p.values[0], p.values[1], p.values[2]) for m in gpu.test_window_beside_a_sibling.pytestmark
             if m.name == "parametrize" for p in m.args[1]]
    assert pairs == wh.sibling_plans(rows) and len(pairs) == len(set(pairs))
    for g, names in wh.SIBLING_GROUPS.items():
        for a in names:
            for b in names:
                assert a == b or (g, a, b) in pairs
    ends = tt.end_plans(rows)
    assert [g for g, _ in ends] == list(wh.SIBLING_GROUPS) and all(e in wh.SIBLING_GROUPS[g] for g, e in ends)
    for entry, key in tt.subject_plans(rows):
        assert key == wh.largest(rows[entry])
        pk = tt.partner_key(rows, entry, gpu.busy.DECOY)
        assert pk == (wh.smallest(rows[entry]) if entry in gpu.busy.DECOY else key)


def test_the_lane_forking_entries_are_read_from_the_sources():
    import test_gpu_guard_bands as grid
    lanes = tt.lane_forking_entries(tt.bs.ROOT)
    assert "soil_multiflow" in lanes and "soil_erode_step" in lanes and "soil_particles_pair_colour" in lanes
    assert set(lanes) <= set(grid.all_rows()) and "soil_accumulate" not in lanes
