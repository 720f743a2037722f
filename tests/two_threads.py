"""A call of the library beside a second host thread: does what the thread next door does reach its result?

include/soil_hip.h: "Several host threads may drive one device at the same time, each on its own stream: they share no
scratch (nor streams, events or pinned words of the launches, which are per thread too)."  csrc/runtime.hip keys a
workspace block by (host thread, device, slot); the info records, the pinned "changed" words, the batch upload staging,
the multiflow lanes and the tiled engine's forked streams and pinned record are thread_local at their users.  The
guard-band, busy-stream and workspace-history harnesses see one caller.  Dropping one thread_local, or keying a block
without the thread id, passes all of them.

A Worker is a host thread that lives as long as its test: it takes closures from a queue and hands back the result or
the exception.  Every library call of a role is made on that role's worker, never on the thread that runs the tests
(ctypes drops the GIL inside a call, so two workers are inside the library at once).  A Role is an Item of
tests/busy_stream.py (a row of the guard-band tables, its arena layout, its decoy, its judge), the image it runs on and
the entry's name.  The protocol is written against a thin device interface (tests/busy_stream.py's, and info,
error_text, mark_error, refuse, thread_exit), which SoilTwoThreads implements on the library and
tests/test_two_threads.py on a numpy stand-in.

  window        deterministic, no timing decides the verdict.  Both workers warm up (the call once on the null stream,
                synchronised, judged where the image has a reference: this sizes each thread's blocks and makes its
                per-thread objects, so nothing below replaces a block).  A queues a backlog on its own non-blocking
                stream sA, then the event `behind`, copy live <- real, the call, copy snapshot <- live, copy live <-
                decoy.  While that is pending, B makes the partner's call on its own stream sB on the partner's image,
                synchronises sB and holds its arena to Arena.check.  `behind` must then still be pending: if it is done,
                B waited for A's stream (shared staging behind an event, a device-wide wait, or sA and sB on one
                hardware queue) and the window had no power: fresh streams are drawn, up to TRIES times, then the
                error is "dependent".  A synchronises sA; its snapshot is checked and judged; its soil_*_info record is
                the record of the same call made alone on A, and B's is B's own.  An entry that synchronises the stream
                cannot return with the backlog pending: B starts as soon as A has entered the call.
                With `refusal`, B's call is a refused call of the partner: A's soil_last_error() text (set on A before
                the window by a refusal of its own, with another message), record and snapshot stay what they were.
  free-running  timing-dependent; its power is measured.  Behind a barrier A makes R judged rounds (copy, call,
                snapshot, synchronise, check, judge, and the record is the one of the call made alone: a launch or a
                look more shows there even where the bits are right) on sA; B loops the partner's call on sB without
                pause until A is done, synchronising every 16 calls, at most 64 R calls.  Both sides take perf_counter_ns around every
                library call: a case in which no call of A intersects a call of B on the host in any round is
                "powerless".
  thread end    A opens a window; B, warm, ends (its thread exits: the library frees what the thread owned while A's
                call is pending); A's snapshot is right; a fresh worker C (whose thread id may be B's, recycled) makes
                B's call, is judged, and its record is the record of B's first call, which was a cold one too.
  mixed         A walks a list of roles in order and B in reverse, each call judged, a barrier every 8 roles.

Every wait on a worker has a time limit (LIMIT_S, or 20 x the warm-up's host time where that is longer); a worker that
does not answer is "stuck", is never joined or asked again, and whoever drives a device ends the session there.

What this cannot see: device scratch shared between threads in a stream-ordered multi-kernel entry when the two
sequences happen not to interleave (the free-running part makes it likely, not sure); process-wide modes and counters
(soil_set_particle_mode / _arith / _debris_retire, soil_particle_steps, soil_debris_retire_violations), which are global
by design and set before the workers start; soil_workspace_release beside another thread, which the header forbids;
include/soil_slab.h.
"""
import queue
import threading
import time

import busy_stream as bs
import guard_arena as ga

KINDS = ("warmup", "guard", "mismatch", "info", "error-text", "dependent", "powerless", "stuck")
TRIES = 8               # pairs of streams drawn until B's call ends while A's backlog is pending
LIMIT_S = 60.0
SYNC_EVERY, CALLS_PER_ROUND = 16, 64
BARRIER_EVERY = 8


class TwoThreadsError(AssertionError):
    """What the protocol reports.  `kind`: one of KINDS; `part`: "window", "free-running", "thread-end" or "mixed"."""

    def __init__(self, kind, part, what, detail):
        assert kind in KINDS, kind
        self.kind, self.part = kind, part
        AssertionError.__init__(self, "%s [%s in %s]: %s" % (what, kind, part, detail))


class Role:
    """`item`: a busy_stream.Item; `entry`: the entry's name (its info record, its refusal); `image`: "real" or
    "decoy", what this role's call is given when it is the partner (a subject is always judged on the real image)."""

    def __init__(self, item, entry, image="decoy"):
        assert image in ("real", "decoy")
        self.item, self.entry, self.image = item, entry, image

    def bytes(self):
        return self.item.arena.host if self.image == "real" else self.item.decoy


# ------------------------------------------------------------------ workers

class _Pending:
    def __init__(self, worker, what):
        self.worker, self.what, self.box = worker, what, queue.Queue(1)

    def wait(self, part="window"):
        w = self.worker
        try:
            ok, value = self.box.get(timeout=w.limit)
        except queue.Empty:
            w.stuck = True
            raise TwoThreadsError("stuck", part, self.what, "worker %s did not answer within %.0f s" % (w.name, w.limit))
        if not ok:
            raise value
        return value


class Worker:
    """A daemon host thread that runs closures in the order given.  `at_exit`: run on the thread as its last act (the
    stand-in's thread-local destructors; the library runs its own)."""

    def __init__(self, name, at_exit=None, limit=LIMIT_S):
        self.name, self.limit, self.stuck, self._at_exit = name, limit, False, at_exit
        self._q = queue.Queue()
        self._t = threading.Thread(target=self._main, name="two-threads-" + name, daemon=True)
        self._t.start()

    def _main(self):
        while True:
            job = self._q.get()
            if job is None:
                break
            fn, pending = job
            try:
                pending.box.put((True, fn()))
            except BaseException as e:              # (handed back, whatever it is)
                pending.box.put((False, e))
        if self._at_exit is not None:
            self._at_exit()

    def start(self, fn, what=""):
        assert not self.stuck, "worker %s is stuck: nothing more is asked of it" % self.name
        p = _Pending(self, what or self.name)
        self._q.put((fn, p))
        return p

    def do(self, fn, what="", part="window"):
        return self.start(fn, what).wait(part)

    def allow(self, host_s):
        """The time limit after a warm-up that took `host_s` on the host."""
        self.limit = max(self.limit, 20.0 * host_s)

    def end(self, part="thread-end"):
        """The thread exits (and with it what the library holds for it).  A stuck worker is left alone."""
        if self.stuck:
            return
        self._q.put(None)
        self._t.join(self.limit)
        if self._t.is_alive():
            self.stuck = True
            raise TwoThreadsError("stuck", part, self.name, "worker %s did not end within %.0f s" % (self.name, self.limit))


# ------------------------------------------------------------------ the pieces, each run on a worker

class _Side:
    """What a warm worker holds for one role: its images on the device and what its call alone left."""


def _warm(dev, role, part, judged):
    """The role's call on the null stream, synchronised; judged on the real image (`judged`), held to Arena.check on
    the partner's.  Returns the _Side."""
    it, s = role.item, _Side()
    n = it.arena.size
    s.role, s.size = role, n
    s.real, s.decoy = dev.image(it.arena.host), dev.image(it.decoy)
    s.given = s.real if (judged or role.image == "real") else s.decoy
    s.given_bytes = it.arena.host if s.given is s.real else it.decoy
    s.live, s.snap = dev.image(s.given_bytes), dev.image(it.decoy)
    t0 = time.perf_counter()
    dev.call(it, s.live, dev.NULL)
    s.host_s = time.perf_counter() - t0
    dev.synchronize(dev.NULL)
    after = dev.read(s.live)
    try:
        it.arena.check(s.given_bytes, after)
        if s.given is s.real:
            it.judge(after)
    except AssertionError as e:
        raise TwoThreadsError("warmup", part, it.what, str(e))
    s.info = dev.info(role.entry)
    return s


def _judge_snapshot(dev, side, part):
    it = side.role.item
    snap = dev.read(side.snap)
    try:
        it.arena.check(it.arena.host, snap)
    except ga.GuardError as e:
        raise TwoThreadsError("guard", part, it.what, str(e))
    try:
        it.judge(snap)
    except AssertionError as e:
        raise TwoThreadsError("mismatch", part, it.what, str(e))


def _queue_call(dev, side, s, spans=None):
    """copy live <- real, the call, copy snapshot <- live, copy live <- decoy, all on `s`."""
    it, n = side.role.item, side.size

    def timed(fn, *a):
        t0 = time.perf_counter_ns()
        fn(*a)
        if spans is not None:
            spans.append((t0, time.perf_counter_ns()))
    timed(dev.copy, side.live, side.real, n, s)
    timed(dev.call, it, side.live, s)
    timed(dev.copy, side.snap, side.live, n, s)
    timed(dev.copy, side.live, side.decoy, n, s)


def _partner_call(dev, side, s, part, refusal=False, look=None):
    """The partner's call on its image on `s`, synchronised, its arena held to Arena.check (and to the reference on
    the real image).  `refusal`: a refused call instead, after which the arena is byte for byte what it was.  Returns
    `look()`, taken as soon as `s` is idle: reading a large arena back takes longer than a short backlog."""
    it, n = side.role.item, side.size
    dev.copy(side.live, side.given, n, s)
    if refusal:
        dev.refuse(side.role, side.live, s)
    else:
        dev.call(it, side.live, s)
    dev.synchronize(s)
    seen = look() if look is not None else None
    after = dev.read(side.live)
    try:
        if refusal:
            assert ga.bits_equal(after, side.given_bytes), "the refused call changed the arena"
        it.arena.check(side.given_bytes, after)
        if side.given is side.real and not refusal:
            it.judge(after)
    except ga.GuardError as e:
        raise TwoThreadsError("guard", part, it.what + " (the partner)", str(e))
    except AssertionError as e:
        raise TwoThreadsError("mismatch", part, it.what + " (the partner)", str(e))
    return seen


def _same_record(got, want, part, what, whose):
    if got != want:
        fields = [j for j in range(len(want))] if got is None or len(got) != len(want) else [
            j for j in range(len(want)) if got[j] != want[j]]
        raise TwoThreadsError("info", part, what, "fields %s of %s record differ from the record of the call made alone "
                              "on that thread: %r, alone %r" % (fields, whose, got, want))


# ------------------------------------------------------------------ the window

class Window:
    """An open window on worker A: the subject's call queued behind a backlog on A's stream (or, for an entry that
    synchronises, A inside the call), everything before the look at `behind`."""


def _open_window(dev, A, sa, part, partner_s=0.0):
    w = Window()
    w.entered = threading.Event()
    ready = queue.Queue(1)
    length = bs.backlog_ms((sa.host_s + partner_s) * 1e3)      # (FACTOR x the host time of both calls, within floor and cap)

    def on_a():
        try:
            w.stream = dev.stream()
            dev.backlog(w.stream, length)
            w.behind = dev.record(w.stream)
        finally:
            ready.put(True)
        w.entered.set()
        _queue_call(dev, sa, w.stream)
    w.pending = A.start(on_a, sa.role.item.what)
    w.length = length
    if sa.role.item.synchronises is None:
        w.pending.wait(part)                # the whole call is queued behind the backlog
        w.pending = None
    else:                                   # the call returns only behind the backlog: B goes while A is inside it
        try:
            ready.get(timeout=A.limit)
        except queue.Empty:
            A.stuck = True
            raise TwoThreadsError("stuck", part, sa.role.item.what, "worker %s did not answer" % A.name)
        if not w.entered.is_set():          # (the closure failed before the call: its exception says why)
            w.pending.wait(part)
    return w


def _close_window(dev, A, w, part):
    if w.pending is not None:
        w.pending.wait(part)
        w.pending = None
    A.do(lambda: dev.synchronize(w.stream), part=part)


def window(dev, A, B, subject, partner, refusal=False, part="window"):
    """The window part for `subject` on worker A beside `partner` on worker B.  Returns (draws, backlog ms)."""
    what = subject.item.what
    sa = A.do(lambda: _warm(dev, subject, part, True), what, part)
    sb = B.do(lambda: _warm(dev, partner, part, False), partner.item.what, part)
    A.allow(sa.host_s), B.allow(sb.host_s)
    text = A.do(dev.mark_error, what, part) if refusal else None
    for draw in range(1, TRIES + 1):
        w = _open_window(dev, A, sa, part, sb.host_s)

        def on_b():
            return _partner_call(dev, sb, dev.stream(), part, refusal, lambda: dev.done(w.behind))
        try:
            overtaken = not B.do(on_b, partner.item.what, part)
        finally:
            if not A.stuck and not B.stuck:
                _close_window(dev, A, w, part)
        if overtaken:
            break
    else:
        raise TwoThreadsError("dependent", part, what, "in none of %d draws of two streams did the partner's call end while "
                              "the subject's backlog of %.1f ms was pending: the partner waits for the subject's stream" % (
                                  TRIES, w.length))
    A.do(lambda: _judge_snapshot(dev, sa, part), what, part)
    _same_record(A.do(lambda: dev.info(subject.entry), what, part), sa.info, part, what, "the subject's")
    if not refusal:
        _same_record(B.do(lambda: dev.info(partner.entry), what, part), sb.info, part, partner.item.what, "the partner's")
    else:
        after = A.do(dev.error_text, what, part)
        if after != text:
            raise TwoThreadsError("error-text", part, what, "a refusal on the other thread changed this thread's "
                                  "soil_last_error(): %r -> %r" % (text, after))
        _same_record(B.do(lambda: dev.info(partner.entry), what, part), sb.info, part, partner.item.what,
                     "(after its refused call) the partner's")
    return draw, w.length


# ------------------------------------------------------------------ free-running

def _intersect(a, b):
    return a[0] < b[1] and b[0] < a[1]


def overlap_share(rounds, other):
    """The share of `rounds` (lists of (t0, t1) spans) in which some span intersects some span of `other`."""
    hit = 0
    for spans in rounds:
        hit += any(_intersect(a, b) for a in spans for b in other)
    return hit / float(len(rounds)) if rounds else 0.0


def free_running(dev, A, B, subject, partner, R, part="free-running"):
    """R judged rounds of `subject` on A while B loops `partner`.  Returns a dict: rounds, calls of B, the share of
    rounds in which a library call of A intersected one of B on the host (`overlap`), and the same for the entry's own
    call alone (`call_overlap`)."""
    what = subject.item.what
    sa = A.do(lambda: _warm(dev, subject, part, True), what, part)
    sb = B.do(lambda: _warm(dev, partner, part, False), partner.item.what, part)
    A.allow(sa.host_s), B.allow(sb.host_s)
    gate, done = threading.Barrier(2), threading.Event()
    rounds, b_spans, b_calls = [], [], []

    def on_a():
        try:
            gate.wait(A.limit)
            s = dev.stream()
            for _ in range(R):
                spans = []
                _queue_call(dev, sa, s, spans)
                t0 = time.perf_counter_ns()
                dev.synchronize(s)
                spans.append((t0, time.perf_counter_ns()))
                rounds.append(spans)
                _judge_snapshot(dev, sa, part)
                _same_record(dev.info(subject.entry), sa.info, part, what, "(round %d) the subject's" % len(rounds))
        finally:
            done.set()
            gate.abort()

    def on_b():
        try:
            gate.wait(B.limit)
        except threading.BrokenBarrierError:
            return 0
        s, it, n, calls = dev.stream(), sb.role.item, sb.size, 0
        while not done.is_set() and calls < CALLS_PER_ROUND * R:
            t0 = time.perf_counter_ns()
            dev.copy(sb.live, sb.given, n, s)
            t1 = time.perf_counter_ns()
            dev.call(it, sb.live, s)
            t2 = time.perf_counter_ns()
            b_spans.extend(((t0, t1), (t1, t2)))
            b_calls.append((t1, t2))
            calls += 1
            if calls % SYNC_EVERY == 0:
                t0 = time.perf_counter_ns()
                dev.synchronize(s)
                b_spans.append((t0, time.perf_counter_ns()))
        dev.synchronize(s)
        after = dev.read(sb.live)
        try:
            it.arena.check(sb.given_bytes, after)
        except ga.GuardError as e:
            raise TwoThreadsError("guard", part, it.what + " (the partner)", str(e))
        return calls
    pa, pb = A.start(on_a, what), B.start(on_b, partner.item.what)
    try:
        pa.wait(part)
    finally:
        done.set()
        calls = pb.wait(part) if not B.stuck else 0
    share = overlap_share(rounds, b_spans)
    call_share = overlap_share([r[1:2] for r in rounds], b_calls)
    if share == 0.0:
        raise TwoThreadsError("powerless", part, what, "in none of %d rounds did a call of this thread intersect one of the "
                              "%d calls of the other on the host" % (R, calls))
    return dict(rounds=R, calls=calls, overlap=share, call_overlap=call_share)


# ------------------------------------------------------------------ a thread's end

def thread_end(dev, A, B, make_worker, subject, partner, part="thread-end"):
    """A opens a window; B, warm, ends while A's call is pending; A's snapshot is right; a fresh worker makes B's call,
    is judged on the real image, and its record is that of B's first call.  `partner.image` is "real".  Returns the
    fresh worker (the caller ends it)."""
    assert partner.image == "real"
    what = subject.item.what
    sa = A.do(lambda: _warm(dev, subject, part, True), what, part)
    sb = B.do(lambda: _warm(dev, partner, part, False), partner.item.what, part)
    A.allow(sa.host_s)
    w = _open_window(dev, A, sa, part, sb.host_s)
    try:
        B.end(part)
    finally:
        if not A.stuck and not B.stuck:
            _close_window(dev, A, w, part)
    A.do(lambda: _judge_snapshot(dev, sa, part), what, part)
    _same_record(A.do(lambda: dev.info(subject.entry), what, part), sa.info, part, what, "the subject's")
    C = make_worker()
    sc = C.do(lambda: _warm(dev, partner, part, False), partner.item.what, part)
    _same_record(sc.info, sb.info, part, partner.item.what, "a fresh thread's")
    return C


# ------------------------------------------------------------------ the mixed run

def mixed(dev, A, B, roles, part="mixed"):
    """A walks `roles` in order and B in reverse, each on a stream of its own, each call judged on the real image, with
    a barrier every BARRIER_EVERY roles.  Returns the number of calls judged."""
    gate = threading.Barrier(2)

    def walk(worker, mine):
        def run():
            n = 0
            try:
                s = dev.stream()
                for i, role in enumerate(mine):
                    if i % BARRIER_EVERY == 0:
                        gate.wait(worker.limit)
                    it = role.item
                    real, live = dev.image(it.arena.host), dev.image(it.decoy)
                    dev.copy(live, real, it.arena.size, s)
                    dev.call(it, live, s)
                    dev.synchronize(s)
                    snap = dev.read(live)
                    try:
                        it.arena.check(it.arena.host, snap)
                    except ga.GuardError as e:
                        raise TwoThreadsError("guard", part, it.what, "role %d on %s: %s" % (i, worker.name, e))
                    try:
                        it.judge(snap)
                    except AssertionError as e:
                        raise TwoThreadsError("mismatch", part, it.what, "role %d on %s: %s" % (i, worker.name, e))
                    n += 1
            except BaseException:
                gate.abort()
                raise
            return n
        return run
    pa, pb = A.start(walk(A, list(roles)), "the rows in order"), B.start(walk(B, list(roles)[::-1]), "the rows in reverse")
    errors, n = [], 0
    for p in (pa, pb):
        try:
            n += p.wait(part)
        except threading.BrokenBarrierError:
            pass                                    # (the other side's error says why)
        except TwoThreadsError as e:
            if e.kind == "stuck":
                raise
            errors.append(e)
    if errors:
        raise errors[0]
    return n


# ------------------------------------------------------------------ the plans

def partner_key(rows, entry, outputs_only):
    """The partner's key of the window and the free-running part: the subject's own (the same slot, sizes and kernels);
    a row without an input plane has no decoy and takes its smallest key, as workspace_history's stale history does."""
    import workspace_history as wh
    return wh.smallest(rows[entry]) if entry in outputs_only else wh.largest(rows[entry])


def subject_plans(rows):
    """(entry, key): every row at its largest key."""
    import workspace_history as wh
    return [(e, wh.largest(rows[e])) for e in rows]


def sibling_plans(rows):
    """(group, subject, partner): every ordered pair of every sibling group of workspace_history's slot table."""
    import workspace_history as wh
    return wh.sibling_plans(rows)


def end_plans(rows):
    """(group, entry): one row per workspace slot group, the group's first entry that is a row."""
    import workspace_history as wh
    return [(g, next(e for e in names if e in rows)) for g, names in wh.SIBLING_GROUPS.items()]


def lane_forking_entries(root):
    """The entries whose call forks private lanes of the library, whose queues cannot be redrawn from outside: read
    from csrc/ (the users of t_flow / FlowLanes in graph.hip, of t_fork in erosion_particles_tiled.hip, which every
    overlapped pair and every step of one model reaches)."""
    import os
    import re
    import workspace_history as wh
    src = lambda name: open(os.path.join(root, "soillib_amd", "csrc", name)).read()          # noqa: E731
    graph, tiled = src("graph.hip"), src("erosion_particles_tiled.hip")
    out = set()
    m = re.search(r"FlowLanes\s*>?\s*t_flow\s*;(.*)", graph, flags=re.S)
    assert m, "graph.hip has no t_flow"
    after = m.group(1)
    for fn in re.finditer(r"\nint (soil_[a-z0-9_]+)\(", after):
        body = after[fn.end():]
        nxt = re.search(r"\nint soil_[a-z0-9_]+\(", body)
        if "t_flow" in (body[:nxt.start()] if nxt else body):
            out.add(fn.group(1))
    assert out == {"soil_multiflow"}, out
    assert re.search(r"ThreadOwned<Fork>\s+t_fork|std::map<int, Fork>\s+t_fork", tiled) and "launch_pair_tiled" in tiled
    out.update(wh.SLOTS["WS_PAIR_GATE"])            # every caller of launch_pair_tiled takes the pair's gate slot
    return sorted(out)


# ------------------------------------------------------------------ the device: the library

class SoilTwoThreads(bs.SoilDevice):
    """busy_stream.SoilDevice, used from the workers, with what the two-thread protocol adds: the info records, the
    error text, a refused call.  Nothing here synchronises the device: a device-wide wait on one worker would close the
    other's window."""

    def image(self, host):
        import numpy as np
        from soillib_amd import silt
        return silt.tensor.from_numpy(np.ascontiguousarray(host).view(np.float32)).gpu()

    def info(self, entry):
        import ctypes as C
        import workspace_history as wh
        if entry not in wh.INFO:
            return None
        fn, n = wh.INFO[entry]
        words = (C.c_int64 * n)()
        self._check(getattr(self.lib, fn)(words))
        return tuple(int(w) for w in words)

    def error_text(self):
        return self.lib.soil_last_error().decode("utf-8", "replace")

    def mark_error(self):
        """A refusal of this thread's own, with a message no row's refusal has."""
        rc = self.lib.soil_host_objects_info(None)
        assert rc == self._abi.SOIL_ERR_INVALID_ARGUMENT, rc
        text = self.error_text()
        assert "host_objects_info" in text, text
        return text

    def refuse(self, role, image, s):
        import workspace_history as wh
        arena, base, entry = role.item.arena, image.ptr, role.entry
        bad = wh.bad_scalar(entry)
        if bad is None:
            ptr = lambda name: None                                                             # noqa: E731
        else:
            ptr = lambda name: None if name is None else base + arena.plane(name).start        # noqa: E731
        try:
            role.item.call(bs.StreamProxy(wh._Refusing(self.lib, entry), self._handle(s), self.entries), ptr)
        except ValueError as e:                     # _abi.check: SOIL_ERR_INVALID_ARGUMENT
            msg = str(e)
        except self._abi.SoilError as e:
            ga.end_session_on_fault(e, role.item.what)
            raise AssertionError("%s with %s: %s" % (entry, bad or "null planes", e))
        else:
            raise AssertionError("%s with %s was not refused" % (entry, "%s invalid" % bad if bad else "null planes"))
        listed = wh.listed_refusals(entry)
        assert not listed or (self._abi.SOIL_ERR_INVALID_ARGUMENT, msg) in listed, (
            "%s: %r is no refusal that tests/golden/refusal_text.json lists" % (entry, msg))

    def thread_exit(self):
        pass                                        # (the library's own thread_local destructors)

    def host_objects(self):
        import ctypes as C
        words = (C.c_int64 * 4)()
        self._check(self.lib.soil_host_objects_info(words))
        return tuple(int(w) for w in words)
