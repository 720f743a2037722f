"""A call of the library on a busy, non-blocking stream: is it ordered on the caller's stream, all of it?

include/soil_hip.h: `stream` is the caller's hipStream_t, and "all functions are asynchronous on that stream unless
stated otherwise".  On the null stream the legacy stream's implicit ordering hides a launch, memset or copy issued on
the wrong stream, a side stream that never waits for the caller's, a lane that is never joined back and a staging
buffer rewritten before its copy ran; on an idle stream with finished inputs, timing hides them.  The protocol below
makes them visible.  It is written against a thin device interface (copy, call, record, query, synchronise), which
SoilDevice implements on the library and tests/test_busy_stream.py on queues of closures over numpy arrays.

For one Item (a call, its guard_arena.Arena layout, its judge) three images of the arena exist on the device:
`real` (the planes as built), `decoy` (the same layout, different valid inputs: decoy_bytes) and `live`, which the
call is given; a fourth buffer takes the snapshot.

  1. warm-up     the call on the null stream on the real image, synchronised, timed on the host, and judged as
                 guard_arena.run_case judges it (Arena.check and guard_arena.judge_outputs).  It also sizes the
                 library's workspace, so the run below replaces no block (which would synchronise the device).
  2. power       the call on the decoy image, judged against the real reference: the judgement must FAIL, else the
                 decoy has no power and the run could hide nothing ("powerless").  An Item without any input plane
                 (power == "outputs") is judged on the untouched decoy image instead: its power lies in the output
                 planes, which hold the guard pattern before copy (b) and after copy (f).
  3. the run     on s, a fresh non-blocking stream, with live = decoy:
                   (a) a backlog of device work on s, then the event `behind` on s; then a no-op on the null stream,
                       waited for on the host: it must end while `behind` is pending.  Streams outnumber hardware
                       queues, and streams that share a queue run in the order of submission: on a stream that
                       shares the null stream's queue a launch on the null stream is ordered by accident, and the
                       run would have no power against it.  Such a stream is drained and another one drawn
                   (b) copy live <- real on s
                   (c) the call, with s as its stream
                   (d) behind done?  s idle?   (looked at at once)
                   (e) copy snapshot <- live on s
                   (f) copy live <- decoy on s: inputs and outputs are clobbered behind the call
                   (g) synchronise s; Arena.check of the snapshot against the real image; judge the outputs
                 Work that does not wait for s reads decoys at (c); work that s does not wait for misses the snapshot
                 (e) or reads the decoys of (f).  Either way the snapshot is not the reference.
     A chain is several Items behind ONE backlog, (b) .. (f) each with its own images, nothing between them; only
     behind an Item that synchronises, which drains the stream, a fresh backlog and a fresh `behind` are queued.
  4. the contract  an Item that does not synchronise must return with `behind` still pending: the whole call was
                 enqueued behind unfinished work ("synchronised" otherwise; the message carries the backlog and the
                 host time).  This is also what decides that the backlog was long enough.  An Item that the header
                 says synchronises must return with `behind` done ("ahead" otherwise), and one that synchronises
                 before it returns must also leave s idle ("pending" otherwise).  In a chain the first Item and every
                 Item right behind a fresh backlog are held to `behind`; the others are not: a later upload may wait
                 for the event of the previous one, which lets the host run one call ahead of the device, not more.

What this cannot see: a race narrower than the backlog that happens to order itself; a private lane of the library
that shares its hardware queue with s (a lane that does not wait for s is then ordered by accident: only the null
stream's queue is looked at, a lane's cannot be from outside; with several lanes the others still show); the
library's internal workspace; two streams of one host thread that share a workspace slot (excluded by
csrc/common.hpp's own rule); a second host thread: the protocol sees one caller (tests/two_threads.py and
tests/test_gpu_two_host_threads.py put a second one beside every row).
"""
import ctypes as C
import os
import re
import time

import numpy as np

import guard_arena as ga
from guard_arena import IN, INOUT, OUT, SCRATCH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FACTOR, FLOOR_MS, CAP_MS = 10.0, 20.0, 1000.0       # the backlog: FACTOR x the warm-up's host time, within [floor, cap]


class BusyStreamError(AssertionError):
    """What the protocol reports.  `kind`: "warmup" (wrong on the null stream already), "powerless", "guard" (a guard
    band or pure input of the snapshot is not the real image's), "mismatch" (an output of the snapshot is not the
    reference), "synchronised", "ahead" (said to synchronise, returned with the backlog pending), "pending", "dependent"
    (no stream was found that the null stream overtakes); `item`: its index in the chain."""

    def __init__(self, kind, item, what, detail):
        self.kind, self.item = kind, item
        AssertionError.__init__(self, "%s [%s]: %s" % (what, kind, detail))


class Item:
    """One call under the protocol.  `arena`: a built numpy-backend Arena (the layout, and in arena.host the real
    image); `decoy`: the decoy image's bytes; `call`: what Device.call is given; `judge(snapshot bytes)`: raises an
    AssertionError where an output is not the reference; `synchronises`: None (stream-ordered), "stream" (the header
    says it synchronises) or "return" (... before it returns); `power`: "call" or "outputs"."""

    def __init__(self, what, arena, decoy, call, judge, synchronises=None, power="call"):
        assert synchronises in (None, "stream", "return") and power in ("call", "outputs")
        assert decoy.shape == arena.host.shape and decoy.dtype == np.uint8
        self.what, self.arena, self.decoy, self.call, self.judge = what, arena, decoy, call, judge
        self.synchronises, self.power = synchronises, power


class Record:
    """What the run of one Item measured: for profiles/busy_stream/checks.txt."""

    def __init__(self, what, synchronises, host_ms, backlog_ms, behind_done, idle, capped, held=True, draws=1):
        self.what, self.synchronises, self.host_ms, self.backlog_ms = what, synchronises, host_ms, backlog_ms
        self.behind_done, self.idle, self.capped, self.held, self.draws = behind_done, idle, capped, held, draws

    def line(self):
        return "busy-stream  %-60s %-11s host %9.3f ms  backlog %8.1f ms  behind %-7s%s idle %-3s stream %d%s" % (
            self.what, self.synchronises or "ordered", self.host_ms, self.backlog_ms,
            "done" if self.behind_done else "pending", " " if self.held else "-", "yes" if self.idle else "no", self.draws,
            "  [x%g of the host time is above the cap]" % FACTOR if self.capped else "")


# ------------------------------------------------------------------ decoys

def decoy_bytes(arena, special=None):
    """The decoy image of a built arena.  float32 / float64 planes that hold data: the elements in reverse flat order
    (a grid turned by 180 degrees, the models of a batch in reverse: range and meaning are kept); int32 planes whose
    guard fills are indices (graphs): all -1, every cell terminal; int32 planes with (0, 1) fills (masks, distances):
    unchanged; soil_rng planes: the records in reverse order.  `special`: plane name -> fn(real plane) -> decoy."""
    out = arena.host.copy()
    for p in arena.planes:
        if not (p.role in (IN, INOUT) or (p.role == SCRATCH and p.data is not None)):
            continue
        real = p.data.reshape(-1)
        if special and p.name in special:
            new = np.ascontiguousarray(special[p.name](p.data), p.dtype).reshape(-1)
        elif p.dtype == np.int32:
            new = real if tuple(p.fills) == (0, 1) else np.full(real.shape, -1, np.int32)
        else:
            new = real[::-1]
        assert new.shape == real.shape
        out[p.start:p.start + p.nbytes] = np.ascontiguousarray(new).view(np.uint8)
    return out


# ------------------------------------------------------------------ the protocol

def backlog_ms(host_ms):
    return min(CAP_MS, max(FLOOR_MS, FACTOR * host_ms))


def _judged(dev, item, i, image, kind):
    """Steps 1 and (g): the image against the real image (guards, pure inputs) and the reference."""
    snap = dev.read(image)
    try:
        item.arena.check(item.arena.host, snap)
    except ga.GuardError as e:
        raise BusyStreamError("warmup" if kind == "warmup" else "guard", i, item.what, str(e))
    try:
        item.judge(snap)
    except AssertionError as e:
        raise BusyStreamError(kind, i, item.what, str(e))


TRIES = 8           # streams drawn until one is found that the null stream overtakes


def _contract(dev, items, looks, held, snap, lengths, host_ms, wanted):
    for i, it in enumerate(items):
        if not held[i]:
            continue
        if it.synchronises is None and looks[i][0]:
            raise BusyStreamError("synchronised", i, it.what, "the call returned after the work queued ahead of it had finished: "
                                  "it synchronised, or a backlog of %.1f ms was too short for a call of %.3f ms on the host (x%g "
                                  "would be %.1f ms, the cap %.0f ms)" % (lengths[i], host_ms[i], FACTOR, wanted, CAP_MS))
        if it.synchronises is not None and not looks[i][0]:
            raise BusyStreamError("ahead", i, it.what, "the header says the call synchronises the stream, and it returned while "
                                  "the work queued ahead of it was still running")
    for i, it in enumerate(items):
        if it.synchronises == "return" and not looks[i][1]:
            raise BusyStreamError("pending", i, it.what, "the header says the call synchronises the stream before it returns, "
                                  "and it returned with work pending on it")
    for i, it in enumerate(items):
        _judged(dev, it, i, snap[i], "mismatch")


def busy_stream(dev, length, what):
    """(a): a stream with `length` ms of backlog and the event `behind` on it, which the null stream OVERTAKES: a no-op
    on the null stream, waited for on the host, ends while `behind` is pending.  Streams outnumber hardware queues, and
    the runtime runs streams that share a queue in the order of submission: on such a stream work on the null stream
    (or on a private lane of the library that shares the queue) is ordered by accident, and a run has no power against
    it.  A stream that fails the look is drained and another is drawn.  Returns (stream, behind, streams drawn)."""
    for draw in range(1, TRIES + 1):
        s = dev.stream()
        dev.backlog(s, length)
        behind = dev.record(s)
        if dev.overtakes(behind):
            return s, behind, draw
        dev.synchronize(s)
    raise BusyStreamError("dependent", 0, what, "none of %d streams drawn is independent of the null stream: the run "
                          "would have no power" % TRIES)


def run_chain(dev, items):
    """The protocol for a chain of Items (one Item: a chain of one).  Returns one Record per Item; raises
    BusyStreamError for the first thing found, in the order warm-up, power, contract, snapshots.  In a chain an Item
    that synchronises drains the stream, so a fresh backlog and a fresh `behind` are queued after it: the Items held to
    `behind` are the first one and every one right after such a backlog."""
    size = [it.arena.size for it in items]
    real = [dev.image(it.arena.host) for it in items]
    decoy = [dev.image(it.decoy) for it in items]
    live = [dev.image(it.arena.host) for it in items]
    snap = [dev.image(np.zeros(n, np.uint8)) for n in size]
    host_ms = []
    # 1. the warm-up, in the chain's order
    for i, it in enumerate(items):
        t0 = time.perf_counter()
        dev.call(it, live[i], dev.NULL)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    dev.synchronize_all()
    for i, it in enumerate(items):
        _judged(dev, it, i, live[i], "warmup")
    # 2. the decoys have power
    for i, it in enumerate(items):
        dev.copy(live[i], decoy[i], size[i], dev.NULL)
        if it.power == "call":
            dev.call(it, live[i], dev.NULL)
    dev.synchronize_all()
    for i, it in enumerate(items):
        try:
            it.judge(dev.read(live[i]))
        except AssertionError:
            pass
        else:
            raise BusyStreamError("powerless", i, it.what, "the decoy of %s has no power" % it.what)
        dev.copy(live[i], decoy[i], size[i], dev.NULL)
    dev.synchronize_all()
    # 3. the run
    wanted = FACTOR * sum(host_ms)
    length = backlog_ms(sum(host_ms))
    s, behind, draws = busy_stream(dev, length, items[0].what)
    looks, held, fresh, behind_ms = [], [], True, length
    lengths = []
    for i, it in enumerate(items):
        lengths.append(behind_ms)
        dev.copy(live[i], real[i], size[i], s)
        dev.call(it, live[i], s)
        looks.append((dev.done(behind), dev.idle(s)))
        held.append(fresh)
        dev.copy(snap[i], live[i], size[i], s)
        dev.copy(live[i], decoy[i], size[i], s)
        fresh = it.synchronises is not None and i + 1 < len(items)
        if fresh:                       # (as long as the calls still to come need, not as the whole chain did)
            behind_ms = backlog_ms(sum(host_ms[i + 1:]))
            dev.backlog(s, behind_ms)
            behind = dev.record(s)
    dev.synchronize(s)
    dev.synchronize_all()           # (whatever a mis-ordered call left on another stream ends before the images go)
    records = [Record(it.what, it.synchronises, host_ms[i], lengths[i], looks[i][0], looks[i][1],
                      it.synchronises is None and wanted > CAP_MS, held[i], draws) for i, it in enumerate(items)]
    # 4. the contract
    try:
        _contract(dev, items, looks, held, snap, lengths, host_ms, wanted)
    except BusyStreamError as e:
        e.records = records           # (what was measured, for whoever reports the failure)
        raise
    return records


def run(dev, item):
    return run_chain(dev, [item])[0]


# ------------------------------------------------------------------ the header: which entries take a stream

def stream_entries():
    """The entries of include/soil_hip.h whose prototype ends in `void* stream`."""
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(soil_[a-z0-9_]+)\s*\([^;{]*?\bvoid\s*\*\s*stream\s*\)\s*;", text)))


def header_near(entry, before=2500, after=600):
    """The header's text around the prototype of `entry`: its own comment, above it or beside it."""
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    m = re.search(r"\b%s\s*\(" % re.escape(entry), re.sub(r"/\*.*?\*/", lambda c: " " * len(c.group(0)), text, flags=re.S))
    assert m, "%s is not declared in include/soil_hip.h" % entry
    return text[max(0, m.start() - before):m.end() + after]


class StreamProxy:
    """`lib` with `stream` in place of the last argument of every entry that takes a stream; the rows of the
    guard-band tables pass None there, which is asserted.  Everything else is the library's."""

    def __init__(self, lib, stream, entries):
        self._lib, self._stream, self._entries = lib, stream, frozenset(entries)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._entries:
            return fn

        def on_stream(*args):
            assert args and args[-1] is None, "%s: the row passes the null stream in the last place" % name
            return fn(*(args[:-1] + (self._stream,)))
        return on_stream


# ------------------------------------------------------------------ the device: the library, torch's streams and events

_HIP_STREAM_NON_BLOCKING = 1


def hip_runtime():
    """The libamdhip64 this process has loaded already: the one torch brought (the library binds to it as well), else
    the only one mapped."""
    import torch
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no libamdhip64 is loaded"
    own = [p for p in paths if p.startswith(os.path.dirname(os.path.abspath(torch.__file__)) + os.sep)]
    assert own or len(paths) == 1, "which of %s owns torch's streams?" % paths
    return C.CDLL((own or paths)[0])


def stream_flags(handle):
    hip = hip_runtime()
    hip.hipStreamGetFlags.restype = C.c_int
    hip.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    flags = C.c_uint(0)
    rc = hip.hipStreamGetFlags(C.c_void_p(handle), C.byref(flags))
    assert rc == 0, "hipStreamGetFlags: %d" % rc
    return flags.value


class SoilDevice:
    """The device interface on libsoil_hip and torch: images are silt tensors, streams torch.cuda.Stream() (non-blocking:
    stream_flags), events torch events, the backlog torch.cuda._sleep (repeated soil_gaussian_blur calls without it),
    calibrated once with two events."""
    NULL = None

    def __init__(self, lib):
        import torch
        from soillib_amd import _abi
        self.torch, self.lib, self._abi = torch, lib, _abi
        self.entries = stream_entries()
        self.what = ""
        self._blur = self._word = None
        self.unit_per_ms = self._calibrate()

    # ---- the backlog
    def _work(self, s, units):
        if hasattr(self.torch.cuda, "_sleep"):
            with self.torch.cuda.stream(s):
                self.torch.cuda._sleep(int(units))
            return
        H = W = 2048
        if self._blur is None:
            self._blur = (self.image(np.zeros(H * W * 4, np.uint8)), self.image(np.zeros(H * W * 4, np.uint8)))
        for _ in range(max(1, int(units))):
            self._abi.check(self.lib.soil_gaussian_blur(self._blur[0].ptr, self._blur[1].ptr, H, W, 1, 2.0, self._handle(s)))

    def _calibrate(self):
        """Units (cycles of torch.cuda._sleep, or blur calls) per millisecond, from two events around a probe."""
        torch = self.torch
        self.kind = "cycles of torch.cuda._sleep" if hasattr(torch.cuda, "_sleep") else "soil_gaussian_blur calls of 2048 x 2048"
        probe = 10000000 if hasattr(torch.cuda, "_sleep") else 50
        s = torch.cuda.Stream()
        self._work(s, probe // 10)              # (the first launch of the kernel: its load is not timed)
        s.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(s)
        self._work(s, probe)
        stop.record(s)
        stop.synchronize()
        return probe / start.elapsed_time(stop)

    def backlog(self, s, ms):
        self._work(s, ms * self.unit_per_ms)

    # ---- the interface
    def _handle(self, s):
        return None if s is None else C.c_void_p(s.cuda_stream)

    def _check(self, rc):
        try:
            self._abi.check(rc)
        except self._abi.SoilError as e:
            ga.end_session_on_fault(e, self.what)
            raise

    def stream(self):
        return self.torch.cuda.Stream()

    def image(self, host):
        from soillib_amd import silt
        t = silt.tensor.from_numpy(np.ascontiguousarray(host).view(np.float32)).gpu()
        self._check(self.lib.soil_device_synchronize())
        return t

    def read(self, image):
        return image.cpu().numpy().view(np.uint8).copy()

    def copy(self, dst, src, nbytes, s):
        self._check(self.lib.soil_memcpy_d2d(dst.ptr, src.ptr, nbytes, self._handle(s)))

    def call(self, item, image, s):
        arena, base = item.arena, image.ptr
        self.what = item.what
        try:
            item.call(StreamProxy(self.lib, self._handle(s), self.entries),
                      lambda name: None if name is None else base + arena.plane(name).start)
        except self._abi.SoilError as e:
            ga.end_session_on_fault(e, item.what)
            raise

    def record(self, s):
        e = self.torch.cuda.Event()
        e.record(s)
        return e

    def done(self, event):
        return bool(event.query())

    def overtakes(self, behind):
        """A one-word fill on the null stream and an event behind it, waited for on the host: did they end while
        `behind` was pending?"""
        if self._word is None:
            self._word = self.image(np.zeros(256, np.uint8))
        self._check(self.lib.soil_set_f32(self._word.ptr, 1.0, 1, None))
        e = self.torch.cuda.Event()
        e.record(self.torch.cuda.default_stream())
        e.synchronize()
        return not behind.query()

    def idle(self, s):
        return bool(s.query())

    def synchronize(self, s):
        self._check(self.lib.soil_stream_synchronize(self._handle(s)))

    def synchronize_all(self):
        self._check(self.lib.soil_device_synchronize())


def case_item(case, want, what, synchronises=None, decoy=None):
    """The Item of a guard_arena.Case: "aligned" placement, fill A.  `decoy`: None (the rule of decoy_bytes), "outputs"
    (a row without input planes) or plane name -> fn for the planes the rule does not fit."""
    arena = ga.Arena("aligned", "A", "numpy")
    for name, role, data, dtype, fills in case.planes:
        arena.add(name, data, role, dtype=dtype, fills=fills)
    arena.build()
    special = decoy if isinstance(decoy, dict) else None
    return Item(what, arena, decoy_bytes(arena, special), case.call,
                lambda snap: ga.judge_outputs(case, arena, snap, want, what), synchronises,
                "outputs" if decoy == "outputs" else "call")
