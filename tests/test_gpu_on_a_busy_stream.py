"""Every entry point of include/soil_hip.h that takes a stream, held to its result on a busy, non-blocking stream.

The header: `stream` is the caller's hipStream_t, "all functions are asynchronous on that stream unless stated
otherwise".  The rest of the suite passes the null stream, whose implicit ordering hides a launch, memset or copy on
the wrong stream, a side stream that never waits for the caller's, a lane never joined back and a staging buffer
rewritten before its copy ran.  Here every row of the guard-band tables (tests/test_gpu_guard_bands.py,
tests/test_gpu_guard_bands_erosion.py: the same Case, planes and reference) runs through the protocol of
tests/busy_stream.py on a torch.cuda.Stream(), which is a hipStreamNonBlocking stream: behind a backlog of device work,
its inputs copied in on the stream just before the call, its planes snapshotted and clobbered with decoys on the
stream right after it; every run first makes sure that the null stream overtakes its stream (streams share hardware
queues: busy_stream.busy_stream).  tests/test_busy_stream.py shows without a GPU what the protocol reports for each class of
mistake; test_the_harness_sees_a_launch_on_the_null_stream shows on the device that it has power there.

Keys: grid rows at (65, 70), batch rows at (3, 65, 67), the particle rows at PARTICLE_SIZE under every launch shape,
the batch particle rows at (3, 65, 67) with 200 and 1100 walkers (the direct and the staged shape): the smallest
shapes at which a call is more than one launch.

The rows pass None as their stream; StreamProxy puts the stream in its place for every entry whose prototype ends in
`void* stream`.  The references keep the real library and the null stream.

Out of scope, as in the guard-band tests: include/soil_slab.h and the library's internal workspace.
"""
import ctypes as C
import re

import numpy as np
import pytest

import busy_stream as bs
import guard_arena as ga
import test_gpu_guard_bands as grid
import test_gpu_guard_bands_erosion as erosion
from guard_arena import IN, INOUT, Case, P
from test_gpu_guard_bands import F32, key_id, ok, rs
from test_gpu_parity import particle_mode  # noqa: F401  (a fixture: every launch shape of the particle kernels)

ROWS = grid.all_rows()

# ------------------------------------------------------------------ the header's synchronisation sentences

# entry -> ("return": the header says the call synchronises the stream before it returns, so it leaves the stream idle;
#           "stream": it says that the call synchronises, not when), and the header's words near the prototype
SYNCHRONISES = {
    # soil::accumulate: "Synchronises the stream before returning, like the reference (graph.cu:564)."
    "soil_accumulate": ("return", "Synchronises the stream before returning, like the reference"),
    # the realisation loop: "Synchronises the stream before returning, like soil_accumulate: ..."
    "soil_multiflow": ("return", "Synchronises the stream before returning, like soil_accumulate"),
    # path-integral MC: "flux is zeroed, filled and normalised; synchronises."
    "soil_solve_uniform": ("stream", "flux is zeroed, filled and normalised; synchronises."),
    # the fill: "(csrc/conditioning.hip); synchronises the stream." and, at the batch form, "both calls synchronise
    # the stream before they return, so neither finds the other's data in use"
    "soil_fill_depressions": ("return", "both calls synchronise the stream before they return"),
    "soil_fill_depressions_batch": ("return", "both calls synchronise the stream before they return"),
    # flats: "soil_flat_distance and soil_flat_distance_batch synchronise the stream before they return, as
    # soil_fill_depressions does"
    "soil_flat_distance": ("return", "soil_flat_distance and soil_flat_distance_batch synchronise the stream before they return"),
    "soil_flat_distance_batch": ("return", "soil_flat_distance and soil_flat_distance_batch synchronise the stream before they return"),
    # threshold hillslopes: "Both calls synchronise the stream before they return, as soil_fill_depressions does."
    "soil_slope_limit": ("return", "Both calls synchronise the stream before they return, as soil_fill_depressions does."),
    "soil_slope_limit_batch": ("return", "Both calls synchronise the stream before they return, as soil_fill_depressions does."),
    # exact multiple flow: "soil_mfd_accumulate(_batch) synchronise the stream before they return, as soil_slope_limit does."
    "soil_mfd_accumulate": ("return", "soil_mfd_accumulate(_batch) synchronise the stream before they return"),
    "soil_mfd_accumulate_batch": ("return", "soil_mfd_accumulate(_batch) synchronise the stream before they return"),
    # stream order: "the host looks at one pinned word per level, so BOTH ENTRIES SYNCHRONISE THE STREAM, once per level"
    "soil_stream_order": ("stream", "BOTH ENTRIES SYNCHRONISE THE STREAM, once per level"),
    "soil_stream_order_batch": ("stream", "BOTH ENTRIES SYNCHRONISE THE STREAM, once per level"),
}

# The particle launches of one model are stream-ordered in the direct and the staged shape.  In the tiled shape the host
# follows the rounds through a pinned word and queues them as the device gets on, which the header says at
# soil_set_particle_mode: under the tiled modes of `particle_mode` the rows of MODES are held to the opposite, as every
# entry that synchronises is: they return after the backlog has run.
TILED_FOLLOWS = "In the tiled shape the host follows the device"

# rows without any input plane: nothing a decoy could differ in.  Their power lies in the output planes alone, which
# hold the guard pattern before the inputs are copied in and after the clobber (busy_stream: power == "outputs")
DECOY = {e: "outputs" for e in ("soil_set_f32", "soil_set_i32", "soil_rng_seed", "soil_noise", "soil_noise_window")}

# the harness's own tools, and the two host counters (no device plane; test_the_counters_are_read_behind_the_stream)
EXEMPT = {
    "soil_memcpy_h2d": "the harness's own tool (uploads the images)",
    "soil_memcpy_d2h": "the harness's own tool (reads the snapshot)",
    "soil_memcpy_d2d": "the harness's own tool (the copies on the stream)",
    "soil_stream_synchronize": "the harness's own tool",
    "soil_event_record": "the harness's own tool (torch's events stand in for it)",
    "soil_particle_steps": "a host counter without a device plane: test_the_counters_are_read_behind_the_stream",
    "soil_debris_retire_violations": "a host counter without a device plane: test_the_counters_are_read_behind_the_stream",
}


def keys_of(entry):
    cases = ROWS[entry].cases
    for key in ((65, 70), (3, 65, 67)):
        if key in cases:
            return [key]
    both = [k for k in ((3, 65, 67, "N1100"), (3, 65, 67, "N200")) if k in cases]
    if both:
        return both
    if cases == [erosion.PARTICLE_SIZE]:
        return [erosion.PARTICLE_SIZE]
    spanning = [k for k in cases if max(grid.dims(k)[1:]) > 64]          # more than one 64-cell tile
    assert spanning, entry
    return spanning[:1]


def params(rows):
    return [pytest.param(e, k, id="%s-%s" % (e, key_id(k))) for e in rows for k in keys_of(e)]


def sync_of(entry, mode=None):
    if entry in SYNCHRONISES:
        return SYNCHRONISES[entry][0]
    if mode is not None and mode.startswith("tiled"):
        return "stream"
    return None


def item_of(lib, oracle, entry, key, mode=None):
    case = ROWS[entry].build(key, oracle)
    if (entry, key) not in grid._WANT:                  # the reference is made once, and shared with the guard-band tests
        grid._WANT[entry, key] = case.want(lib, oracle)
    what = "%s %s%s" % (entry, key_id(key), " " + mode if mode else "")
    return bs.case_item(case, grid._WANT[entry, key], what, sync_of(entry, mode), DECOY.get(entry))


@pytest.fixture(scope="module")
def dev(hip):
    import torch
    flags = bs.stream_flags(torch.cuda.Stream().cuda_stream)
    if not flags & 1:                                   # hipStreamNonBlocking
        pytest.skip("torch.cuda.Stream() is no hipStreamNonBlocking stream here (flags %#x)" % flags)
    d = bs.SoilDevice(hip)
    print("busy-stream  calibration: %.1f %s per millisecond" % (d.unit_per_ms, d.kind))
    return d


def through(dev, items):
    try:
        records = bs.run_chain(dev, items)
    except bs.BusyStreamError as e:
        for r in getattr(e, "records", []):
            print(r.line())
        raise
    for r in records:
        print(r.line())
    return records


# ------------------------------------------------------------------ the rows

PLAIN = [e for e, r in ROWS.items() if not getattr(r, "modes", False)]
MODES = [e for e, r in ROWS.items() if getattr(r, "modes", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,key", params(PLAIN))
def test_row_on_a_busy_stream(hip, oracle, dev, entry, key):
    through(dev, [item_of(hip, oracle, entry, key)])


@pytest.mark.gpu
@pytest.mark.parametrize("entry,key", params(MODES))
def test_row_on_a_busy_stream_in_every_particle_launch_shape(hip, oracle, dev, particle_mode, entry, key):   # noqa: F811
    through(dev, [item_of(hip, oracle, entry, key, particle_mode)])


# The batch rows that upload host records: scale pairs (n_scales == B), seeds, a param or a whole record per model.  They
# go through the host thread's one pinned staging buffer (csrc/erosion_particles.hip: upload_seeds / batch_upload,
# csrc/flow_host.hpp) and share the thread's workspace slots.
def uploads(entry):
    if entry.endswith("_batch"):
        return entry[:-len("_batch")] in (
            "soil_random_weighted", "soil_slope", "soil_slope_limit", "soil_mfd_weights", "soil_mfd_accumulate", "soil_flow_paths",
            "soil_downstream", "soil_stream_power", "soil_stream_power_deposit", "soil_stream_power_deposit_n",
            "soil_stream_power_n", "soil_diffuse", "soil_particles", "soil_erode_step")
    # (soil_erode_cells_fused_batch_colour has one param and one scale: launch arguments)
    return bool(re.search(r"_batch_(colour|params|models)$", entry)) and entry != "soil_erode_cells_fused_batch_colour"


UPLOADS = [e for e in ROWS if uploads(e)]           # in table order


def chain_key(entry):
    keys = keys_of(entry)
    # the batch particle rows: the launches alone in the direct shape, the whole steps in the staged one
    return keys[-1] if entry.startswith("soil_particles_batch") else keys[0]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["table", "reversed"])
def test_chain_on_a_busy_stream(hip, oracle, dev, order):
    """All of UPLOADS behind one backlog, each with its own images, nothing between them but what the library does
    itself: a staging buffer rewritten before its copy ran gives call i the records of call i + 1, a workspace slot
    reused too early another call's scratch.  A row that synchronises drains the stream: a fresh backlog follows it.  The
    first call and every call right behind a fresh backlog are held to the event (a later upload may wait for the copy
    before it: the host runs one upload ahead of the device, not more)."""
    entries = UPLOADS if order == "table" else UPLOADS[::-1]
    assert len(entries) >= 20
    through(dev, [item_of(hip, oracle, e, chain_key(e)) for e in entries])


@pytest.mark.gpu
def test_the_harness_sees_a_launch_on_the_null_stream(hip, dev):
    """soil_multiply_f32 on the stream, then soil_add_f32 on the null stream on purpose: the add runs ahead of the
    backlog on the decoys, and the snapshot holds t * 0.3 alone.  A wrong number, not a fault."""
    key = (65, 70)
    t, other = rs(key, 1), rs(key, 2, lo=-1.0)

    def call(lib, p):
        ok(lib.soil_multiply_f32(p("t"), 0.3, t.size, None))
        ok(hip.soil_add_f32(p("t"), p("other"), t.size, None))          # (the library itself, not the proxy)
    case = Case([P("t", INOUT, t), P("other", IN, other)], call, None)
    want = dict(t=t * F32(0.3) + other)
    with pytest.raises(bs.BusyStreamError) as e:
        through(dev, [bs.case_item(case, want, "multiply on the stream, add on the null stream")])
    assert e.value.kind == "mismatch" and ": t" in str(e.value), str(e.value)
    assert not e.value.records[0].behind_done, "the composite was queued behind the backlog"


@pytest.mark.gpu
def test_the_counters_are_read_behind_the_stream(hip, oracle, dev):
    """soil_particle_steps and soil_debris_retire_violations take a stream and no device plane.  Behind a backlog and a
    particle launch on the stream, soil_particle_steps gives that launch's steps, and both return only after the
    backlog: they read behind the stream's work (the header: "synchronises `stream`")."""
    from soillib_amd import _abi
    assert hip.soil_set_particle_mode(1) == 0
    try:
        it = item_of(hip, oracle, "soil_transport_fluvial", erosion.PARTICLE_SIZE)
        real, live = dev.image(it.arena.host), dev.image(it.arena.host)
        total = C.c_uint64(0)
        ok(hip.soil_particle_steps(C.byref(total), 1, None))
        dev.call(it, live, None)
        ok(hip.soil_particle_steps(C.byref(total), 1, None))
        steps = total.value
        assert steps > 0
        # (any stream will do, one that shares the null stream's hardware queue too: nothing here runs on the null stream
        # while the backlog is pending, and both assertions are about this stream's own order)
        s = dev.stream()
        h = C.c_void_p(s.cuda_stream)
        dev.backlog(s, bs.FLOOR_MS)
        behind = dev.record(s)
        dev.copy(live, real, it.arena.size, s)
        dev.call(it, live, s)
        assert not dev.done(behind), "the launch was queued behind the backlog"
        ok(hip.soil_particle_steps(C.byref(total), 1, h))
        assert dev.done(behind) and total.value == steps, (total.value, steps)
        dev.backlog(s, bs.FLOOR_MS)
        behind = dev.record(s)
        ok(hip.soil_debris_retire_violations(C.byref(total), 0, h))
        assert dev.done(behind) and total.value == 0
        _abi.check(hip.soil_device_synchronize())
    finally:
        hip.soil_set_particle_mode(0)


# ------------------------------------------------------------------ without a GPU

def _normal(text):
    return re.sub(r"\s+", " ", re.sub(r"(?m)^\s*/?\*+/?", " ", text)).strip()


def test_the_header_says_that_every_entry_of_the_set_synchronises():
    from soillib_amd import _abi
    for entry, (when, words) in SYNCHRONISES.items():
        assert entry in _abi.SIGNATURES and entry in bs.stream_entries(), entry
        assert when in ("return", "stream") and "synchronis" in words.lower(), entry
        near = _normal(bs.header_near(entry, before=4500, after=1500))
        assert words in near, "%s: the header near its prototype does not say %r" % (entry, words)
        if when == "return":
            assert re.search(r"before (they |it )?return", words), entry
    near = _normal(bs.header_near("soil_set_particle_mode", before=1500))
    assert TILED_FOLLOWS in near and "synchronis" in near.lower()


def test_every_entry_point_that_takes_a_stream_runs_here():
    """The rows this file runs and EXEMPT partition the entries of include/soil_hip.h whose prototype ends in
    `void* stream` (include/soil_slab.h stays out of scope, as in the guard-band tests)."""
    from soillib_amd import _abi
    entries = set(bs.stream_entries())
    assert entries <= set(_abi.SIGNATURES)
    run_here = {e for e in PLAIN + MODES}
    assert {p.values[0] for p in params(PLAIN) + params(MODES)} == run_here
    assert not run_here & set(EXEMPT)
    missing = sorted(entries - run_here - set(EXEMPT))
    assert not missing, "entries that take a stream and are neither run here nor exempt: %s" % missing
    unknown = sorted((run_here | set(EXEMPT)) - entries)
    assert not unknown, "rows or exemptions that take no stream: %s" % unknown
    assert set(SYNCHRONISES) <= run_here and set(DECOY) <= run_here and set(UPLOADS) <= run_here
    for e in DECOY:                         # "outputs" only where there is no input plane at all
        case = ROWS[e].build(keys_of(e)[0], None)
        assert all(role == ga.OUT for _, role, *_ in case.planes), e
