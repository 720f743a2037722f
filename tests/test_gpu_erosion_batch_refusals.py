"""What the twelve batch entry points refuse, and in which order (include/soil_hip.h: soil_erode_step_batch,
soil_particles_batch, soil_erode_cells_fused_batch, each plain, _colour, _params and _models).  Every entry checks
null arguments, then the colour planes, then the sizes, then the physics planes, then (step and cells) that layers
and layers_next are distinct buffers.  For each class of bad call: SOIL_ERR_INVALID_ARGUMENT, a message that starts
with the entry's own name and holds the text below; with two faults at once, the earlier check is the one that
reports.  The texts are written out here, not taken from the library.  B = 2, 8 x 8, N = 16; a refused call launches
nothing."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

B, H, W, N = 2, 8, 8, 16
NULL_ARG = ": null argument"
NULL_MODELS = ": null models"
COLOUR = ": every colour plane is required"
NO_MODEL = ": a batch needs at least one model (B >= 1)"
EMPTY = ": empty grid (H and W must be >= 1)"
NEGATIVE = ": negative particle count"
NEGATIVE_MODEL = ": models[1].N outside [0, 2^31)"
PLANE = {"step": ": every plane but `height` is required", "cells": ": null plane (only `height` is optional)",
         "particles": ": null plane"}
DISTINCT = ": layers and layers_next must be distinct buffers"

PHASES = {"step": "soil_erode_step_batch", "particles": "soil_particles_batch", "cells": "soil_erode_cells_fused_batch"}
ENTRIES = [(phase, kind) for kind in ("", "_colour", "_params", "_models") for phase in PHASES]


def _cases(phase, kind):
    """(label, overrides of the good call, the text the message must hold), one fault first, then two at once."""
    models, coloured, walkers = kind == "_models", kind != "", phase != "cells" or kind == "_models"
    null_arg = [("models", NULL_MODELS)] if models else [("scale", NULL_ARG), ("param", NULL_ARG)]
    negative = dict(N_1=-1) if models else dict(N=-1)
    cases = [("null planes", dict(planes=None), NULL_ARG)]
    cases += [("null " + name, {name: None}, text) for name, text in null_arg]
    if coloured:
        cases += [("colour without %s" % f, dict(colour_without=f), COLOUR) for f in ("albedo_bedrock", "albedo_debris")]
    cases += [("B = 0", dict(B=0), NO_MODEL), ("H = 0", dict(H=0), EMPTY)]
    if walkers:
        cases.append(("N < 0", negative, NEGATIVE_MODEL if models else NEGATIVE))
    cases.append(("no waterFlux", dict(without="waterFlux"), PLANE[phase]))
    if phase != "particles":
        cases += [("no uplift", dict(without="uplift"), PLANE[phase]), ("layers twice", dict(same_layers=True), DISTINCT)]
    # two faults: the earlier check reports
    first = "planes" if models else "scale"
    if coloured:
        cases.append(("null %s and a colour plane" % first, {first: None, "colour_without": "albedo_surface"}, NULL_ARG))
        cases.append(("a colour plane and B = 0", dict(colour_without="albedo_fluvial", B=0), COLOUR))
    else:
        cases.append(("null param and B = 0", dict(param=None, B=0), NULL_ARG))
    if models:
        cases.append(("a colour plane and null models", dict(colour_without="albedo_fluvial", models=None), COLOUR))
        cases.append(("null models and no waterFlux", dict(models=None, without="waterFlux"), NULL_MODELS))
    cases.append(("B = 0 and H = 0", dict(B=0, H=0), NO_MODEL))
    if walkers:
        cases.append(("H = 0 and N < 0", dict(H=0, **negative), NEGATIVE_MODEL if models else EMPTY))
    cases.append(("H = 0 and no waterFlux", dict(H=0, without="waterFlux"), EMPTY))
    if phase != "particles":
        cases.append(("no waterFlux and layers twice", dict(without="waterFlux", same_layers=True), PLANE[phase]))
    return cases


@pytest.fixture(scope="module")
def batch(hip):
    """A coloured batch whose planes every call below points at (none is read or written: every call is refused)."""
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    return ErosionBatch(B, H, W, (1.0, 1.0, 1.0), soil.param_t(), N, seeds=[1, 2], colour=True)


def _call(lib, batch, phase, kind, bad):
    from soillib_amd import _abi
    planes, colour = batch._planes(), batch._colour()
    if "without" in bad:
        setattr(planes, bad["without"], None)
    if bad.get("same_layers"):
        planes.layers_next = planes.layers
    if "colour_without" in bad:
        setattr(colour, bad["colour_without"], None)
    models = (_abi.BatchModel * B)()
    for b, m in enumerate(models):
        m.param, m.N, m.seed, m.step_index = batch.param._c, N, b + 1, 0
        m.scale[:] = [1.0, 1.0, 1.0]
    models[1].N = bad.get("N_1", N)
    seeds = (C.c_uint64 * B)(1, 2)
    params = (_abi.Param * B)(batch.param._c, batch.param._c)
    good = dict(planes=C.byref(planes), scale=_abi.vec((1.0, 1.0, 1.0), 3), models=models, B=B, H=H, N=N,
                param=params if kind == "_params" else batch.param._ref())
    a = {**good, **{k: v for k, v in bad.items() if k in good}}
    args = [a["planes"]] + ([C.byref(colour)] if kind else []) + [a["B"], a["H"], W]
    if kind == "_models":
        args.append(a["models"])
    else:
        args += ([a["N"], seeds, 0] if phase != "cells" else []) + [a["scale"], a["param"]]
    args += ([0] if phase == "cells" else []) + [None]
    return getattr(lib, PHASES[phase] + kind)(*args)


@pytest.mark.parametrize("phase, kind", ENTRIES, ids=[PHASES[phase] + kind for phase, kind in ENTRIES])
def test_a_bad_call_is_refused_by_the_first_check_it_fails(hip, batch, phase, kind):
    from soillib_amd import _abi
    name = PHASES[phase][len("soil_"):] + kind
    for label, bad, text in _cases(phase, kind):
        assert _call(hip, batch, phase, kind, bad) == _abi.SOIL_ERR_INVALID_ARGUMENT, label
        message = _abi.last_error()
        assert message.startswith(name + ": "), (label, message)
        assert text in message, (label, message)
