"""tests/workspace_history.py without a GPU: the slot table against csrc/common.hpp, the protocol against a numpy
stand-in "library" with a persistent scratch array into which each class of mistake is built, and the inputs of the
non-quiescent predecessors against the properties they are built for."""
import numpy as np
import pytest

import busy_stream as bs
import flats_ref
import guard_arena as ga
import test_gpu_guard_bands as grid
import workspace_history as wh
from guard_arena import IN, INOUT, OUT, Case, P
from workspace_history import COLD, REFUSAL, REGROW, RELEASE, SHRINK, STALE

ROWS = grid.all_rows()


# ------------------------------------------------------------------ slot coverage

def _params(fn):
    """The argument tuples a test function of tests/test_gpu_workspace_history.py is parametrised with, as pytest will
    run them: the product of its parametrize marks, by argument name."""
    import itertools
    marks = [m for m in fn.pytestmark if m.name == "parametrize"]
    names = [[n.strip() for n in m.args[0].split(",")] for m in marks]
    values = [[getattr(v, "values", v if len(n) > 1 else (v,)) for v in m.args[1]] for m, n in zip(marks, names)]
    return [dict(kv for n, v in zip(names, combo) for kv in zip(n, v)) for combo in itertools.product(*values)]


def histories_2_to_5():
    """entry -> the kinds of histories 2 to 5 that tests/test_gpu_workspace_history.py runs it under, read from that
    file's own parametrisation: a row or kind dropped there is missing here."""
    import test_gpu_workspace_history as gpu
    out = {}
    for a in _params(gpu.test_history):
        assert a["kind"] in (STALE, SHRINK, REGROW)
        out.setdefault(a["entry"], set()).add(a["kind"])
    for a in _params(gpu.test_siblings):
        assert (a["group"], a["first"], a["second"]) in wh.sibling_plans(ROWS)
        out.setdefault(a["first"], set()).add(wh.SIBLINGS)
        out.setdefault(a["second"], set()).add(wh.SIBLINGS)
    return out


def check_slots(enumerators, slots, rows, histories):
    assert set(slots) == set(enumerators), "SLOTS and WorkspaceSlot differ in %s" % sorted(set(slots) ^ set(enumerators))
    for slot, entries in slots.items():
        assert entries, slot
        for e in entries:
            assert e in rows, "%s: %s is no row of the guard-band tables" % (slot, e)
        assert any(histories.get(e) for e in entries), "%s appears in no history" % slot


def test_every_slot_has_its_entries_and_a_history():
    enumerators = wh.slot_enumerators()
    assert len(enumerators) == len(set(enumerators)) >= 27
    check_slots(enumerators, wh.SLOTS, ROWS, histories_2_to_5())


def test_the_gpu_file_runs_every_plan():
    """Every row under histories 1 to 4 and (but for NO_REFUSAL) 7, every pair of history 5, every image of history 6
    and every plan of history 8: read from the parametrisation of tests/test_gpu_workspace_history.py."""
    import test_gpu_workspace_history as gpu
    assert [a["entry"] for a in _params(gpu.test_cold)] == list(ROWS)
    assert {(a["entry"], a["kind"]) for a in _params(gpu.test_history)} == {(e, k) for e in ROWS for k in (STALE, SHRINK, REGROW)}
    assert {a["entry"] for a in _params(gpu.test_a_refusal_in_between)} == set(ROWS) - set(wh.NO_REFUSAL)
    assert [(a["group"], a["first"], a["second"]) for a in _params(gpu.test_siblings)] == wh.sibling_plans(ROWS)
    assert [(a["entry"], a["image"]) for a in _params(gpu.test_a_predecessor_that_does_not_end_quiet)] == wh.restless_plans()
    assert [(a["entry"], a["before"], a["shape"]) for a in _params(gpu.test_launch_shapes_change_hands)] == wh.shape_plans(ROWS)
    histories = histories_2_to_5()
    assert set(histories) == set(ROWS) and all({STALE, SHRINK, REGROW} <= k for k in histories.values())


# slot -> the sources of csrc/ that name it outside a comment.  A slot taken in another file, or no longer taken in one
# of these, fails here and sends its author to SLOTS, whose entries are read from these files by hand.
SLOT_SOURCES = {
    "WS_ACCUMULATE_0": ["graph.hip"], "WS_ACCUMULATE_1": ["graph.hip"], "WS_MULTIFLOW": ["graph.hip"],
    "WS_FLOW_BATCH": ["graph.hip"], "WS_ACCUMULATE_BATCH": ["graph.hip"],
    "WS_SMALL_LAUNCH": ["erosion_particles.hip"], "WS_BATCH": ["erosion_particles.hip"],
    "WS_TILED_FLUVIAL": ["erosion_particles_tiled.hip"], "WS_TILED_DEBRIS": ["erosion_particles_tiled.hip"],
    "WS_PAIR_GATE": ["erosion_particles_tiled.hip"],
    "WS_CONDITIONING": ["conditioning.hip"], "WS_ERODE": ["erosion_step.hip"], "WS_STEP_RNG": ["erosion_step.hip"],
    "WS_STATS": ["erosion_stats.hip"], "WS_FLOW_PATHS": ["flow_paths.hip"], "WS_FLATS": ["flats.hip"],
    "WS_DOWNSTREAM": ["downstream.hip"], "WS_DEPOSIT": ["downstream.hip"], "WS_DEPOSIT_RAKE": ["downstream.hip"],
    "WS_DEPOSIT_PLANES": ["downstream.hip"], "WS_POWER_N": ["downstream.hip"], "WS_POWER_N_ITERATE": ["downstream.hip"],
    "WS_DIFFUSE": ["diffuse.hip"], "WS_SLOPE_LIMIT": ["slope_limit.hip"], "WS_UPSTREAM": ["upstream.hip"],
    "WS_STREAM_ORDER": ["stream_order.hip"], "WS_MFD": ["mfd.hip"],
}
# ... and the source that defines each C entry of a slot reaches the slot's source: itself, or through these calls
REACHES = {
    "erosion_batch.hip": ["erosion_particles.hip"],                                      # particles_batch, batch_models_to_device
    "erosion_step.hip": ["erosion_particles.hip", "erosion_particles_tiled.hip"],        # the step's launches
    "erosion_particles.hip": ["erosion_particles_tiled.hip"],                            # the tiled shape of a launch
}


def _code(text):
    import re
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def test_the_slot_table_follows_the_sources():
    import os
    import re
    csrc = os.path.join(wh.ROOT, "soillib_amd", "csrc")
    code = {f: _code(open(os.path.join(csrc, f)).read()) for f in sorted(os.listdir(csrc)) if f != "common.hpp"}
    named = {}
    for f, text in code.items():
        for slot in set(re.findall(r"\bWS_[A-Z0-9_]+\b", text)):
            named.setdefault(slot, []).append(f)
    assert named == SLOT_SOURCES, {s: (named.get(s), SLOT_SOURCES.get(s)) for s in set(named) | set(SLOT_SOURCES)
                                   if named.get(s) != SLOT_SOURCES.get(s)}
    defined = {}
    for f, text in code.items():
        for entry in re.findall(r"^int (soil_[a-z0-9_]+)\(", text, flags=re.M):
            defined[entry] = f
    for slot, entries in wh.SLOTS.items():
        for e in entries:
            home = defined[e]
            assert any(src == home or src in REACHES.get(home, ()) for src in SLOT_SOURCES[slot]), (slot, e, home)


def test_an_enumerator_without_a_history_fails():
    with pytest.raises(AssertionError, match="WS_NEW"):
        check_slots(wh.slot_enumerators() + ["WS_NEW"], wh.SLOTS, ROWS, histories_2_to_5())
    with pytest.raises(AssertionError, match="no row"):
        check_slots(wh.slot_enumerators() + ["WS_NEW"], dict(wh.SLOTS, WS_NEW=["soil_new_entry"]), ROWS, histories_2_to_5())
    with pytest.raises(AssertionError, match="no history"):
        check_slots(wh.slot_enumerators(), wh.SLOTS, ROWS, {})


def test_every_shared_slot_has_a_sibling_group():
    """A slot that several entries take is covered by a group of history 5 that holds all of them (the particle slots
    change hands in history 8, the launch shapes; the accumulate lanes share one group)."""
    by_shape = {"WS_SMALL_LAUNCH", "WS_TILED_FLUVIAL", "WS_TILED_DEBRIS", "WS_PAIR_GATE"}
    groups = [set(g) for g in wh.SIBLING_GROUPS.values()]
    for slot, entries in wh.SLOTS.items():
        if len(entries) > 1 and slot not in by_shape:
            assert any(set(entries) <= g for g in groups), slot
    for g in wh.SIBLING_GROUPS.values():
        assert len(g) == len(set(g)) >= 2 and set(g) <= set(ROWS)
    modes = {e for e, r in ROWS.items() if getattr(r, "modes", False)}
    for slot in by_shape:
        assert set(wh.SLOTS[slot]) <= modes


def test_the_plans_use_the_tables_own_keys():
    for entry, row in ROWS.items():
        kinds = [COLD, STALE, SHRINK, REGROW] + ([] if entry in wh.NO_REFUSAL else [REFUSAL])
        for kind in kinds:
            steps = wh.plan(kind, ROWS, entry)
            calls = [s for s in steps if s.op != "release"]
            assert 1 <= len(calls) <= 4 and steps[-1].op == "call" and steps[-1].image == "real", (entry, kind)
            assert all(s.entry == entry and s.key in row.cases for s in calls), (entry, kind)
        assert wh.plan(COLD, ROWS, entry)[0] is RELEASE and wh.plan(COLD, ROWS, entry)[1].key == wh.largest(row)
        shrink = [s.key for s in wh.plan(SHRINK, ROWS, entry)]
        assert [wh.cells_of(k) for k in shrink] == sorted((wh.cells_of(k) for k in shrink), reverse=True), (entry, shrink)
        regrow = wh.plan(REGROW, ROWS, entry)
        assert regrow[0] is RELEASE and regrow[-1].key == wh.smallest(row)
    assert wh.plan(SHRINK, ROWS, "soil_flow_paths_batch")[0].key == (3, 65, 67)
    assert [s.key for s in wh.plan(SHRINK, ROWS, "soil_fill_depressions")][-1] in ((1, 9), (9, 1))
    for e in wh.OUTPUTS_ONLY:                   # no input plane at all: another key in place of a decoy
        case = ROWS[e].build(wh.largest(ROWS[e]), None)
        assert all(role == OUT for _, role, *_ in case.planes), e
        a, b = wh.plan(STALE, ROWS, e)
        assert a.key != b.key and a.image == b.image == "real"
    for e in wh.NO_REFUSAL:                     # and the rows without a refusal take no workspace slot
        assert not any(e in entries for entries in wh.SLOTS.values()), e
    assert set(wh.INFO) <= set(ROWS) and set(wh.RESTLESS_IMAGES) <= set(ROWS)


def test_every_launch_shape_changes_hands():
    plans = wh.shape_plans(ROWS)
    modes = {e for e, r in ROWS.items() if getattr(r, "modes", False)}
    assert {e for e, _, _ in plans} == modes and wh.PAIR_ROW in modes
    pairs = {(a, b) for e, a, b in plans if e == wh.PAIR_ROW}
    assert pairs == {(a, b) for a in wh.LAUNCH_SHAPES for b in wh.LAUNCH_SHAPES if a != b}
    for e in modes - {wh.PAIR_ROW}:
        own = [(a, b) for x, a, b in plans if x == e]
        assert len(own) == 1 and own[0][0] != own[0][1], e
    rest = [(a, b) for e, a, b in plans if e != wh.PAIR_ROW]
    assert {a for a, _ in rest} == {b for _, b in rest} == set(wh.LAUNCH_SHAPES)    # every shape before and under test
    import inspect
    import test_gpu_parity
    assert all('"%s"' % m in inspect.getsource(test_gpu_parity) for m in wh.LAUNCH_SHAPES)


# ------------------------------------------------------------------ the protocol against stand-ins

TILE = 8
KEYS = [(5, 7), (9, 11), (1, 9)]           # 35, 99 and 9 cells: none a multiple of the tile
MISTAKES = ("marks", "count", "extent", "reuse", "regrow", "info")


def _x(key):
    return np.random.default_rng(list(key)).random(key).astype(np.float32)


def _reference(x):
    return (x + np.float32((x > 0.5).sum())).astype(np.float32)


def _build(key, oracle):
    x = _x(key)
    return Case([P("x", IN, x), P("y", OUT, key, np.float32)], None, lambda lib, oracle: dict(y=_reference(x)))


class _Row:
    cases, build = KEYS, staticmethod(_build)


STAND_IN_ROWS = {"relax": _Row}


class StandIn:
    """One op, y = x + the number of cells above 0.5, counted the way a tile relaxation would: a mark per cell over the
    tile-padded extent of the grid and a count word, in a block that grows on demand and is never cleared; an info record
    (tiles, count).  Fresh memory is zero, which is what hides most of the mistakes from a cold call.  `mistake`:
      marks    the marks are set where a cell is above 0.5 and never cleared
      count    the count word is added to, not reset
      extent   the marks are cleared over the cells of the grid, not over the tiles that are summed
      reuse    the result of the last call is given back when the shape matches
      regrow   a block too small for the call is kept (the extents are cut to it: a wrong number, not a fault)
      info     the record is that of the call before"""

    def __init__(self, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.mistake, self.block, self.record, self.last, self.cache = mistake, None, (0, 0), (0, 0), None

    def release(self):
        self.block = None

    def prepare(self, step):
        case = STAND_IN_ROWS[step.entry].build(step.key, None)
        arena = ga.Arena("aligned", "A", "numpy")
        for name, role, data, dtype, fills in case.planes:
            arena.add(name, data, role, dtype=dtype, fills=fills)
        arena.build()
        if step.image == "real":
            want = case.want(None, None)
            return wh.Prepared(arena, arena.host.copy(), lambda snap: ga.judge_outputs(case, arena, snap, want, repr(step)))
        return wh.Prepared(arena, bs.decoy_bytes(arena), None)

    def run(self, prep, step):
        arena = prep.arena
        arena.host[:] = prep.image
        x, y = arena.view("x"), arena.view("y")
        n = x.size
        padded = -(-n // TILE) * TILE
        if self.block is None or (self.block.size < 1 + padded and self.mistake != "regrow"):
            self.block = np.zeros(1 + padded, np.int64)
        held = min(padded, self.block.size - 1)
        marks = self.block[1:1 + held]
        if self.mistake != "marks":
            marks[:min(n, held) if self.mistake == "extent" else held] = 0
        at = np.flatnonzero(x.reshape(-1) > 0.5)
        marks[at[at < held]] = 1
        if self.mistake != "count":
            self.block[0] = 0
        self.block[0] += marks.sum()
        if self.mistake == "reuse" and self.cache is not None and self.cache.shape == x.shape:
            y[:] = self.cache
        else:
            y[:] = x + np.float32(self.block[0])
        self.cache = y.copy()
        self.last, self.record = self.record, (padded // TILE, int(self.block[0]))
        return arena.host.copy()

    def refuse(self, prep, step):
        return prep.image.copy()

    def info(self, entry):
        return self.last if self.mistake == "info" else self.record


def caught_by(mistake):
    """The kinds of history that report `mistake`, each on a stand-in of its own (fresh, zeroed memory)."""
    cold = wh.run_history(StandIn(mistake), wh.plan(COLD, STAND_IN_ROWS, "relax"))
    caught = {}
    for kind in (COLD, STALE, SHRINK, REGROW, REFUSAL):
        steps = wh.plan(kind, STAND_IN_ROWS, "relax")
        own_cold = cold if steps[-1].key == (9, 11) else wh.run_history(
            StandIn(mistake), [RELEASE, wh.call("relax", steps[-1].key)])
        try:
            wh.run_history(StandIn(mistake), steps, kind, own_cold)
        except wh.HistoryError as e:
            caught[kind] = (e.kind, e.step)
    return caught


def test_the_correct_stand_in_passes_every_history():
    assert caught_by(None) == {}


def test_the_stand_in_data_can_show_each_mistake():
    big, small = _x((9, 11)).reshape(-1) > 0.5, _x((5, 7)).reshape(-1) > 0.5
    assert big[35:40].any(), "the larger grid leaves a mark in the smaller grid's last tile, past its cells"
    assert (big[:35] & ~small).any(), "... and marks inside it where the smaller grid has none"
    assert (small[::-1] & ~small).any(), "the decoy leaves marks where the real image has none"
    assert not np.array_equal(_reference(_x((9, 11))), _reference(_x((9, 11))[::-1, ::-1]))


@pytest.mark.parametrize("mistake,kinds", [
    ("marks", {STALE: ("mismatch", 1), SHRINK: ("mismatch", 1), REGROW: ("mismatch", 3)}),
    ("count", {STALE: ("mismatch", 1), SHRINK: ("mismatch", 1), REGROW: ("mismatch", 3), REFUSAL: ("mismatch", 2)}),
    ("extent", {SHRINK: ("mismatch", 1), REGROW: ("mismatch", 3)}),
    ("reuse", {STALE: ("mismatch", 1)}),
    ("regrow", {REGROW: ("mismatch", 2)}),
    ("info", {STALE: ("info", 1), SHRINK: ("info", 2), REGROW: ("info", 3), REFUSAL: ("info", 2)}),
])
def test_which_history_catches_which_mistake(mistake, kinds):
    """The cold call catches none of them: on fresh, zeroed memory each of these stand-ins is right.  A repeat of the
    identical call (the refusal history without its refusal) sees only the count and the record."""
    assert caught_by(mistake) == kinds


def test_a_failure_names_the_step_and_what_preceded_it():
    with pytest.raises(wh.HistoryError) as e:
        wh.run_history(StandIn("marks"), wh.plan(REGROW, STAND_IN_ROWS, "relax"), "regrow")
    msg = str(e.value)
    assert e.value.kind == "mismatch" and e.value.step == 3
    assert "regrow: relax 5x7 on real, after [release; relax 5x7 on real; relax 9x11 on real]" in msg, msg


def test_a_refusal_that_touches_a_plane_or_the_record_is_reported():
    class Touches(StandIn):
        def refuse(self, prep, step):
            snap = prep.image.copy()
            snap[prep.arena.plane("y").start] ^= 1
            return snap

    class Resets(StandIn):
        def refuse(self, prep, step):
            self.record = (0, 0)
            return prep.image.copy()

    class Accepts(StandIn):
        def refuse(self, prep, step):
            raise AssertionError("relax with null planes was not refused")
    for lib, kind in ((Touches(), "refusal"), (Resets(), "info"), (Accepts(), "refusal")):
        with pytest.raises(wh.HistoryError) as e:
            wh.run_history(lib, wh.plan(REFUSAL, STAND_IN_ROWS, "relax"))
        assert (e.value.kind, e.value.step) == (kind, 1)


def test_a_store_outside_a_plane_is_reported_at_its_step():
    class Overruns(StandIn):
        def run(self, prep, step):
            snap = StandIn.run(self, prep, step)
            if step.image == "decoy":
                p = prep.arena.plane("y")
                snap[p.start + p.nbytes] ^= 1
            return snap
    with pytest.raises(wh.HistoryError) as e:
        wh.run_history(Overruns(), wh.plan(STALE, STAND_IN_ROWS, "relax"))
    assert (e.value.kind, e.value.step) == ("guard", 0)


# ------------------------------------------------------------------ the inputs of history 6

def _arena(entry, key, oracle):
    case = ROWS[entry].build(key, oracle)
    arena = ga.Arena("aligned", "A", "numpy")
    for name, role, data, dtype, fills in case.planes:
        arena.add(name, data, role, dtype=dtype, fills=fills)
    return arena.build()


@pytest.mark.parametrize("shape", [(5, 7), (65, 70), (33, 260), (1, 9), (9, 1), (3, 65, 67), (3, 9, 1)])
def test_the_cyclic_graph_has_no_terminal(shape):
    g = wh.cyclic_graph(shape)
    assert g.shape == shape and g.dtype == np.int32 and wh.never_ends(g)
    H, W = shape[-2:]
    flat = g.reshape(-1, H * W)
    own = np.arange(H * W)
    dy, dx = np.abs(flat // W - own // W), np.abs(flat % W - own % W)
    assert (dy + dx == 1).all(), "every receiver is a D4 neighbour"
    hops = flat.copy()
    for _ in range(int(np.ceil(np.log2(H * W))) + 2):      # pointer doubling: no walk has ended after any round
        hops = np.take_along_axis(hops, hops, 1)
        assert ((hops >= 0) & (hops != -1)).all()
    assert not wh.never_ends(grid.gs(shape if len(shape) == 2 else shape, grid.D8)), "the rows' own graphs do end"


@pytest.mark.parametrize("entry", wh.CYCLES)
def test_the_cyclic_predecessor_of_every_pointer_doubling_entry(oracle, entry):
    key = wh.sibling_key(ROWS[entry])
    arena = _arena(entry, key, oracle)
    image = wh.restless_image(arena, entry, "cycles")
    assert wh.never_ends(arena.read("graph", image))
    if "stop" in [p.name for p in arena.planes]:            # (the deposit steps take none)
        assert not arena.read("stop", image).any()
    for p in arena.planes:                      # nothing else differs from the real image
        if p.name not in ("graph", "stop"):
            assert ga.bits_equal(arena.read(p.name, image), arena.read(p.name, arena.host)), p.name


@pytest.mark.parametrize("entry", wh.RELAXATIONS)
def test_the_relaxations_predecessors_leave_the_marks_extreme(oracle, entry):
    key = wh.sibling_key(ROWS[entry])
    arena = _arena(entry, key, oracle)
    nan = arena.read("height", wh.restless_image(arena, entry, "nan"))
    flat = arena.read("height", wh.restless_image(arena, entry, "plateau"))
    assert np.isnan(nan).all() and (flat == 5.0).all()
    H, W = key[-2:]
    # all NaN: no cell can drain, so nothing ever relaxes and no tile is ever marked as moved
    assert not flats_ref.seeds(nan.reshape(-1, H, W)[0], grid.D8).any()
    # a plateau: one flat over the whole grid, drained from the border alone; the relaxation has to carry every ring
    # inwards through every tile, the most a grid of this size can ask for
    dist = flats_ref.distance_bfs(flat.reshape(-1, H, W)[0], grid.D8)
    seeds = flats_ref.seeds(flat.reshape(-1, H, W)[0], grid.D8)
    border = np.zeros((H, W), bool)
    border[[0, -1], :] = border[:, [0, -1]] = True
    assert np.array_equal(seeds, border)
    assert len(np.unique(dist)) == (min(H, W) + 1) // 2


@pytest.mark.parametrize("entry", wh.HOSTILE_LAST)
def test_the_hostile_model_sits_in_the_last_slot(oracle, entry):
    key = wh.sibling_key(ROWS[entry])
    arena = _arena(entry, key, oracle)
    image = wh.restless_image(arena, entry, "hostile_last", oracle)
    B = key[0]
    odd = 0
    for p in arena.planes:
        real, got = arena.read(p.name, arena.host), arena.read(p.name, image)
        assert ga.bits_equal(real[:B - 1], got[:B - 1]), p.name
        if not ga.bits_equal(real[B - 1], got[B - 1]):
            assert p.role in (IN, INOUT)
            odd += int(not np.isfinite(got[B - 1]).all())
    assert odd >= 3, "the last model holds non-finite cells in several planes"


@pytest.mark.parametrize("entry", sorted(ROWS))
def test_the_decoy_differs_from_the_real_image_in_every_input_plane(oracle, entry):
    """... in every input plane the rule of busy_stream.decoy_bytes changes: (0, 1) masks and distances stay by that
    rule, and a plane that is one value throughout (a flux plane of zeros) is its own mirror image."""
    arena = _arena(entry, wh.largest(ROWS[entry]), oracle)         # the key of history 2
    decoy = bs.decoy_bytes(arena)
    differs = 0
    for p in arena.planes:
        if p.data is None or p.role not in (IN, INOUT):
            assert ga.bits_equal(arena.read(p.name, decoy), arena.read(p.name, arena.host))
            continue
        real = p.data.reshape(-1)
        mirror = ga.bits_equal(real, real[::-1])
        stays = (p.dtype == np.int32 and tuple(p.fills) == (0, 1)) or (p.dtype != np.int32 and mirror) or \
            (p.dtype == np.int32 and tuple(p.fills) != (0, 1) and bool((real == -1).all()))
        assert ga.bits_equal(arena.read(p.name, decoy), p.data) == stays, p.name
        differs += not stays
    assert differs or entry in wh.OUTPUTS_ONLY, entry
