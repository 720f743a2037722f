"""One erosion step on one GPU: the build's definition of the legacy `soil.erode`.

The reference snapshot no longer contains `soil::erode` (only its commented-out
binding, python/source/model.cpp:142); what remains are the kernels it was
composed of.  SURVEY.md §3.1 fixes the composition of one step as

    silt.seed(rng, seed, step*N)                       (example/dem_process.py:81)
    transport_fluvial -> transport_debris              (erosion.cu:189-239, :395-436)
    delta = 0; mass_transfer; mass_creep               (erosion.cu:576-611, :712-727)
    layers += delta; layer_merge                       (dem_process.py:47, erosion.cu:747-757)

`ErosionModel.step()` runs exactly that, as two particle kernels followed by
ONE fused cell kernel (soil_erode_cells_fused) that also re-zeroes the flux
planes; `step_unfused()` runs the same step through the individual reference
ops (one launch each) and exists so that tests can show both are bit-identical.
The model may be a row slab of a larger grid (see soillib_amd.parallel).

`ErosionModel(..., colour=True)` carries the four colour planes of the coloured
step (include/soil_hip.h, soil_colour_planes) through every phase:
`step()` is soil_erode_step_colour, `step_unfused()` the same step through the
reference ops with their albedo arguments.  Whole grids on one GPU only.

`ErosionBatch(B, H, W, scale, param, n_particles, seeds)` holds B independent
models of one shape with one seed each, the planes of `ErosionModel` as
(B, H, W[, C]) tensors, model-major.  `step()` (soil_erode_step_batch) steps every
model at once and leaves model b where `ErosionModel(..., seed=seeds[b]).step()`
leaves that model alone, up to the fp32 summation order of the flux planes: a
few launches for the whole batch where B models take B times their own handful
(DESIGN.md 3.5).  `particles()` and `cells_fused()` run the two phases
separately; `model_planes(b)` copies one model's planes to the host.  Whole
grids, one shared param.  `ErosionBatch(..., colour=True)` carries the four colour
planes of the coloured step too (soil_erode_step_batch_colour): model b ends where
`ErosionModel(..., seed=seeds[b], colour=True).step()` leaves it.  A sequence of B
param_t in place of `param` makes the batch a parameter sweep (soil_erode_step_batch_params):
model b steps with params[b], as `ErosionModel(..., params[b], ..., seed=seeds[b])` would.
B scale triples in place of `scale`, or B walker counts in place of `n_particles`, make
a batch of different models (soil_erode_step_batch_models): model b steps as
`ErosionModel(H, W, scales[b], params[b], Ns[b], seed=seeds[b])` would.
`ErosionBatch.from_models(models)` copies B whole-grid `ErosionModel`s into such a batch,
each at its own step index, and `to_models()` copies them back out.

`ErosionModel.resized(H, W)` and `ErosionBatch.resized(H, W)` return a new model or batch of another resolution
holding the resampled state (soil_erode_resize_batch: every plane of every model in one launch, `height` rebuilt,
flux planes zero), with the seeds, params, step indices and walker counts carried over and each scale rescaled to
the same world extent: the multiscale schedule (erode coarse, resample, erode finer) for whole models and batches
(DESIGN.md 3.5).

`ErosionBatch.stats()` and `ErosionModel.stats()` reduce every model on the device to one small record
(soil_erode_batch_stats: sum, sum of squares, min, max and the count of non-finite cells of the ten STAT_CHANNELS), and
`ErosionBatch.ensemble()` reduces the batch to per-cell mean and variance maps of the six ENSEMBLE_CHANNELS
(soil_erode_batch_ensemble): what a sweep or an ensemble wants to know without copying a plane to the host.
`ErosionBatch.quantiles(q)`, `order_statistics(ranks)` and `median()` give per-cell order statistics across the models
(soil_erode_batch_quantiles), and `exceedance(thresholds)` the share of the models above a threshold per cell
(soil_erode_batch_exceedance): the summaries of a heavy-tailed ensemble.
"""
import ctypes as C
import numbers
import os

import numpy as np

from . import _abi, _check, silt

# the channels of a soil_model_stats record and of the ensemble maps, in the order of include/soil_hip.h
STAT_CHANNELS = ("bedrock", "sediment", "height", "waterHeight", "mass", "debris", "velocity.x", "velocity.y",
                 "debrisVelocity.x", "debrisVelocity.y")
ENSEMBLE_CHANNELS = ("bedrock", "sediment", "height", "waterHeight", "mass", "debris")
# soil_channel_stats as a numpy record (32 bytes)
STATS_DTYPE = np.dtype([("sum", "<f8"), ("sumsq", "<f8"), ("nonfinite", "<i8"), ("min", "<f4"), ("max", "<f4")])


def _stats(planes, B, H, W):
    """The (B, 10) records of B models: one soil_erode_batch_stats into a device buffer of B x 320 bytes, then one
    copy of that buffer to the host (the only synchronisation)."""
    words = C.sizeof(_abi.ModelStats) // 4
    out = silt.tensor(silt.float32, silt.shape(B, words), silt.gpu)
    _abi.check(_abi.lib().soil_erode_batch_stats(C.byref(planes), B, H, W, out.c_ptr, _abi.stream()))
    return out.cpu().numpy().view(STATS_DTYPE).reshape(B, len(STAT_CHANNELS))


def _check_size(who, H, W):
    for v in (H, W):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool) or v < 1:
            raise ValueError("%s.resized: H and W must be integers >= 1, got %r x %r" % (who, H, W))


def _rescaled(scale, Ho, Wo, H, W):
    """The scale of the same world at (H, W) cells: the cell size times old / new, sz as it is."""
    return [float(scale[0]) * Ho / H, float(scale[1]) * Wo / W, float(scale[2])]


def _resize_into(new, old, B):
    """Every plane of `old` (B models) resampled into `new` by one soil_erode_resize_batch; `new` was allocated with
    every plane the entry point writes in full left unzeroed."""
    dst, src = new._planes(), old._planes()
    dst_c = src_c = None
    if old.colour:
        dst_colour, src_colour = new._colour(), old._colour()
        dst_c, src_c = C.byref(dst_colour), C.byref(src_colour)
    _abi.check(_abi.lib().soil_erode_resize_batch(C.byref(dst), C.byref(src), dst_c, src_c, B, new.H, new.W, old.H,
                                                  old.W, _abi.stream()))


class ErosionModel:
    """Planes of one erosion model (or one row slab of it), resident in HBM.

    rows    local rows held (owned + ghost), W columns
    dom     _abi.Domain describing where the slab sits in the global grid

    `resized(H, W)` returns a new whole-grid model of (H, W) with the state resampled (soil_erode_resize_batch).
    """

    PLANES_1 = ("height", "uplift", "rainfall", "waterHeight", "waterFlux", "mass", "massFlux",
                "debris", "debrisFlux")
    PLANES_2 = ("velocity", "velocityFlux", "debrisVelocity", "debrisVelocityFlux")
    # soil_colour_planes, in its order: (rows, W, 3) each
    PLANES_3 = ("albedoBedrock", "albedoSurface", "albedoFluvial", "albedoDebris")

    # what soil_erode_resize_batch writes in full: every plane but layers_next
    RESIZED = ("layers",) + PLANES_1 + PLANES_2 + PLANES_3

    def __init__(self, H, W, scale, param, n_particles, seed=0, dom=None, alloc=None, colour=False, _written=()):
        """`_written`: planes the caller is about to write in full, not zeroed here (resized())."""
        self.H, self.W = int(H), int(W)
        self.scale = [float(v) for v in scale]
        self.param = param
        self.N = int(n_particles)
        self.seed = int(seed)
        self.dom = dom if dom is not None else _abi.Domain(self.H, self.W, 0, self.H, 0, self.H)
        self.rows = int(self.dom.rows)
        self.colour = bool(colour)
        if self.colour and self.rows != self.H:
            raise ValueError("a coloured model needs the whole grid on one GPU (no slabs)")
        self.step_index = 0
        alloc = alloc or (lambda dtype, shape: silt.tensor(dtype, silt.shape(*shape), silt.gpu))
        self._alloc = alloc
        r, w = self.rows, self.W
        self.layers = alloc(silt.float32, (r, w, 2))
        self.layers_next = alloc(silt.float32, (r, w, 2))
        for name in self.PLANES_1:
            setattr(self, name, alloc(silt.float32, (r, w)))
        for name in self.PLANES_2:
            setattr(self, name, alloc(silt.float32, (r, w, 2)))
        self.rng = alloc(silt.rng, (self.N,))
        self.rng_debris = alloc(silt.rng, (self.N,))   # the fluvial launch's state two draws on
        for name in self.PLANES_3 if self.colour else ():
            setattr(self, name, alloc(silt.float32, (r, w, 3)))
        for name in ("layers", "layers_next") + self.PLANES_1 + self.PLANES_2 + (self.PLANES_3 if self.colour else ()):
            if name not in _written:
                silt.set(getattr(self, name), 0.0)
        silt.seed(self.rng, self.seed, 0)

    # -- helpers -------------------------------------------------------------
    def _planes(self):
        p = _abi.ErosionPlanes()
        for name in _abi._PLANES:
            setattr(p, name, getattr(self, name).ptr)
        return p

    def _colour(self):
        c = _abi.ColourPlanes()
        for field, name in zip(_abi.COLOUR_PLANES, self.PLANES_3):
            setattr(c, field, getattr(self, name).ptr)
        return c

    def _scale(self):
        return _abi.vec(self.scale, 3)

    def set_layers(self, layers_tensor):
        """Copy an (rows, W, 2) tensor of (bedrock, sediment) into the model."""
        silt.set(self.layers, layers_tensor)

    def resized(self, H, W, scale=None, n_particles=None):
        """A new ErosionModel of (H, W) holding this model's state resampled (soil_erode_resize_batch, one launch:
        every persistent plane bilinear as soil_resize, `height` = the new layers merged, flux planes zero); this
        model is left as it is.  The new model has the same param object, seed and colour setting and continues
        at this model's step index.  `scale` defaults to the same world with more (or fewer) cells,
        [sx * Ho / H, sy * Wo / W, sz]; `n_particles` to this model's.  A row slab, H or W < 1, a scale that is not
        3 numbers or a negative walker count raise ValueError before any device work."""
        if self.rows != self.H:
            raise ValueError("ErosionModel.resized: the model is a row slab (%d of %d rows)" % (self.rows, self.H))
        _check_size("ErosionModel", H, W)
        if scale is None:
            scale = _rescaled(self.scale, self.H, self.W, H, W)
        else:
            try:
                scale = list(scale)
                ok = len(scale) == 3 and all(isinstance(v, numbers.Real) for v in scale)
            except TypeError:
                ok = False
            if not ok:
                raise ValueError("ErosionModel.resized: scale is not 3 numbers: %r" % (scale,))
        N = self.N if n_particles is None else n_particles
        if not isinstance(N, numbers.Integral) or isinstance(N, bool) or N < 0:
            raise ValueError("ErosionModel.resized: n_particles = %r is not a walker count >= 0" % (N,))
        new = ErosionModel(H, W, scale, self.param, N, seed=self.seed, colour=self.colour, _written=self.RESIZED)
        new.step_index = self.step_index
        _resize_into(new, self, 1)
        return new

    def stats(self):
        """This model reduced on the device (soil_erode_batch_stats with B = 1): a numpy structured array of shape
        (10,), one element per channel of STAT_CHANNELS, with the fields sum, sumsq (fp64, over the finite cells),
        nonfinite (cells holding NaN or an infinity), min and max (over the finite cells; +inf / -inf when there
        is none).  The bytes are those of this model's row of ErosionBatch.stats().  One copy of 320 bytes to the
        host, the only synchronisation.  A row slab raises ValueError before any device work."""
        if self.rows != self.H:
            raise ValueError("ErosionModel.stats: the model is a row slab (%d of %d rows)" % (self.rows, self.H))
        return _stats(self._planes(), 1, self.H, self.W)[0]

    # -- the three phases ------------------------------------------------------
    def seed_step(self):
        silt.seed(self.rng, self.seed, self.step_index * self.N)

    def particles_pair(self, overwrite=False):
        """Both particle launches of the step, overlapped (soil_particles_pair_slab).  The
        debris launch draws from its own tensor, seeded where the fluvial launch leaves
        the shared one in the sequential order (two draws per particle further).
        `overwrite`: the flux planes were left as they were by cells_fused(keep_flux=True)
        (SOIL_FLUX_OVERWRITE: the launches' first rounds store instead of adding)."""
        silt.seed(self.rng_debris, self.seed, self.step_index * self.N + 2)
        planes = self._planes()
        if self.colour:   # soil_particles_pair_colour: the two colour flux planes cleared first
            colour = self._colour()
            _abi.check(_abi.lib().soil_particles_pair_colour(
                C.byref(planes), C.byref(colour), self.rng.c_ptr, self.rng_debris.c_ptr, self.N, self.H,
                self.W, self._scale(), self.param._ref(), _abi.SOIL_FLUX_OVERWRITE if overwrite else 0,
                _abi.stream()))
            return
        _abi.check(_abi.lib().soil_particles_pair_slab_ex(
            C.byref(planes), self.rng.c_ptr, self.rng_debris.c_ptr, self.N, None,
            C.byref(self.dom), self._scale(), self.param._ref(),
            _abi.SOIL_FLUX_OVERWRITE if overwrite else 0, _abi.stream()))

    def particles_fluvial(self):
        """The fluvial launch; a coloured model clears albedoFluvial first and adds this launch's
        colour flux to it (spawn colours from albedoSurface)."""
        L = _abi.lib()
        flux_a = src_a = None
        if self.colour:
            silt.set(self.albedoFluvial, 0.0)
            flux_a, src_a = self.albedoFluvial.c_ptr, self.albedoSurface.c_ptr
        _abi.check(L.soil_particles_fluvial_slab(
            self.waterFlux.c_ptr, self.massFlux.c_ptr, self.velocityFlux.c_ptr, flux_a,
            self.rng.c_ptr, self.N, self.layers.c_ptr, self.rainfall.c_ptr,
            self.waterHeight.c_ptr, self.velocity.c_ptr, src_a, None, C.byref(self.dom),
            self._scale(), self.param._ref(), _abi.stream()))

    def particles_debris(self):
        """The debris launch; with colour as particles_fluvial, into albedoDebris (every walker
        walked to the end, as soil_particles_debris_slab with colour planes does)."""
        L = _abi.lib()
        flux_a = src_a = None
        if self.colour:
            silt.set(self.albedoDebris, 0.0)
            flux_a, src_a = self.albedoDebris.c_ptr, self.albedoSurface.c_ptr
        _abi.check(L.soil_particles_debris_slab(
            self.debrisFlux.c_ptr, self.debrisVelocityFlux.c_ptr, flux_a, self.rng.c_ptr, self.N,
            self.layers.c_ptr, self.debrisVelocity.c_ptr, src_a, None, C.byref(self.dom),
            self._scale(), self.param._ref(), _abi.stream()))

    def cells_fused(self, r0=None, r1=None, keep_flux=False):
        """Fused cell phase on local rows [r0, r1) (default: the owned rows).  `keep_flux`: the
        flux planes are not re-zeroed (SOIL_CELLS_KEEP_FLUX) — the next particles_pair must then
        be told to overwrite them."""
        d = self.dom
        dom = _abi.Domain(d.H, d.W, d.x0, d.rows, d.r0 if r0 is None else r0,
                          d.r1 if r1 is None else r1)
        planes = self._planes()
        flags = _abi.SOIL_CELLS_KEEP_FLUX if keep_flux else 0
        if self.colour:
            colour = self._colour()
            _abi.check(_abi.lib().soil_erode_cells_fused_colour(
                C.byref(planes), C.byref(colour), C.byref(dom), self._scale(), self.param._ref(), flags,
                _abi.stream()))
            return
        _abi.check(_abi.lib().soil_erode_cells_fused_ex(
            C.byref(planes), C.byref(dom), self._scale(), self.param._ref(), flags, _abi.stream()))

    def swap_layers(self):
        self.layers, self.layers_next = self.layers_next, self.layers

    # -- whole steps -----------------------------------------------------------
    def step(self):
        """One erosion step: 2 particle launches + 1 fused cell launch.  With the whole grid on
        this device it is the library's own step driver (soil_erode_step, csrc/erosion_step.hip:
        seed, both particle launches overlapped on two streams, fused cell phase;
        SOIL_STEP_PAIR=0 in the environment makes it run them one after the other).  A coloured
        model runs soil_erode_step_colour."""
        if self.colour:
            planes, colour = self._planes(), self._colour()
            _abi.check(_abi.lib().soil_erode_step_colour(
                C.byref(planes), C.byref(colour), self.rng.c_ptr, self.N, self.seed, self.step_index, self.H,
                self.W, self._scale(), self.param._ref(), 0, _abi.stream()))
            self.swap_layers()
            self.step_index += 1
            return
        if self.rows == self.H:
            planes = self._planes()
            _abi.check(_abi.lib().soil_erode_step(
                C.byref(planes), self.rng.c_ptr, self.N, self.seed, self.step_index, self.H, self.W,
                self._scale(), self.param._ref(), _abi.stream()))
            self.swap_layers()
            self.step_index += 1
            return
        self.seed_step()                       # a slab of a larger grid (soillib_amd.parallel)
        if os.environ.get("SOIL_STEP_PAIR") != "0":
            self.particles_pair()
        else:
            self.particles_fluvial()
            self.particles_debris()
        self.cells_fused()
        self.swap_layers()
        self.step_index += 1

    def step_unfused(self):
        """The same step through the stand-alone reference ops (single GPU only); with colour the
        contract of soil_colour_planes (include/soil_hip.h), colour flux planes zeroed first."""
        from . import soil
        if self.rows != self.H:
            raise ValueError("step_unfused needs the whole grid on one GPU")
        self.seed_step()
        bed = surf = fl = db = None
        if self.colour:
            bed, surf, fl, db = self.albedoBedrock, self.albedoSurface, self.albedoFluvial, self.albedoDebris
            silt.set(fl, 0.0)
            silt.set(db, 0.0)
        soil.transport_fluvial(self.layers, self.rainfall, self.waterHeight, self.waterFlux,
                               self.mass, self.massFlux, self.velocity, self.velocityFlux, bed,
                               fl, surf, self.rng, self.scale, self.param)
        soil.transport_debris(self.layers, self.debrisVelocity, self.debrisVelocityFlux,
                              self.debris, self.debrisFlux, bed, db, surf, self.rng, self.scale,
                              self.param)
        delta = self.layers_next  # reuse the spare layer buffer as the delta plane
        silt.set(delta, 0.0)
        soil.mass_transfer(delta, self.layers, self.uplift, self.waterHeight, self.mass,
                           self.velocity, self.debris, self.debrisVelocity, bed, fl, db, surf,
                           self.scale, self.param)
        soil.mass_creep(delta, self.layers, self.scale, self.param)
        silt.add(self.layers, delta)
        soil.layer_merge(self.height, self.layers)
        for name in ("waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux"):
            silt.set(getattr(self, name), 0.0)  # silt.set(track.*, 0)
        self.step_index += 1


class ErosionBatch:
    """B independent whole-grid erosion models of one (H, W) shape, stepped together (include/soil_hip.h:
    soil_erode_step_batch).  Every plane of ErosionModel is a (B, H, W[, C]) GPU tensor, zeroed here; model b
    has its own terrain, rainfall, uplift and seed, and shares N and scale with the others.  `colour`: the four
    colour planes of ErosionModel(colour=True) too, (B, H, W, 3) each, and the coloured entry points
    (soil_erode_step_batch_colour).

    `param` is one param_t shared by every model, or a sequence of B param_t: a parameter sweep, in which model b
    steps with params[b] (soil_erode_step_batch_params, with or without colour).  A sweep holds them as
    `self.params` (`self.param` is None) and reads them at every call of particles(), cells_fused() and step(): a
    change to one of the objects, or a replaced element, takes effect at the next call.  A wrong count or an
    element that is not a param_t raises ValueError before any device work.

    `scale` is one (sx, sy, sz) triple, or a sequence of B triples held as `self.scales` (`self.scale` is None)
    and read at every call as a sweep's params are.  `n_particles` is one walker count, or a sequence of B counts
    fixed at construction as `self.Ns` (`self.N` is None).  Either makes the batch one of different models
    (soil_erode_step_batch_models): model b steps with its own param, scale, walker count, seed and step index
    `first_step[b] + step_index`, where `first_step` is 0 unless the batch came from from_models().  A wrong
    count, an element that is not 3 numbers or a negative walker count raises ValueError before any device
    work.

    `resized(H, W)` returns a new batch of (H, W) with every plane of every model resampled in one launch
    (soil_erode_resize_batch) and the seeds, params, step indices, walker counts and rescaled scales carried
    over."""

    PLANES_1 = ErosionModel.PLANES_1
    PLANES_2 = ErosionModel.PLANES_2
    PLANES_3 = ErosionModel.PLANES_3

    def __init__(self, B, H, W, scale, param, n_particles, seeds, colour=False, _written=()):
        """`_written`: planes the caller is about to write in full, not zeroed here (resized())."""
        self.B, self.H, self.W = int(B), int(H), int(W)
        self.seeds = [int(v) for v in seeds]
        if len(self.seeds) != self.B:
            raise ValueError("ErosionBatch: %d seeds for %d models" % (len(self.seeds), self.B))
        if self.B < 1 or self.H < 1 or self.W < 1:
            raise ValueError("ErosionBatch: B, H and W must be >= 1")
        self.scale, self.scales = self._scale_arg(scale)
        from .soil import param_t
        if isinstance(param, param_t):
            self.param, self.params = param, None
        else:
            try:
                self.params = list(param)
            except TypeError:
                raise ValueError("ErosionBatch: param must be a param_t or a sequence of %d param_t" % self.B)
            self.param = None
            self._check_params()
        self.N, self.Ns = self._n_arg(n_particles)
        self.colour = bool(colour)
        self.step_index = 0
        self.first_step = [0] * self.B
        shape = (self.B, self.H, self.W)
        alloc = lambda *dims: silt.tensor(silt.float32, silt.shape(*dims), silt.gpu)
        self.layers = alloc(*shape, 2)
        self.layers_next = alloc(*shape, 2)
        for name in self.PLANES_1:
            setattr(self, name, alloc(*shape))
        for name in self.PLANES_2:
            setattr(self, name, alloc(*shape, 2))
        for name in self._colour_names():
            setattr(self, name, alloc(*shape, 3))
        for name in self._names():
            if name not in _written:
                silt.set(getattr(self, name), 0.0)
        self._seeds = (C.c_uint64 * self.B)(*self.seeds)

    def _colour_names(self):
        return self.PLANES_3 if self.colour else ()

    def _names(self):
        return ("layers", "layers_next") + self.PLANES_1 + self.PLANES_2 + self._colour_names()

    _planes = ErosionModel._planes
    _colour = ErosionModel._colour
    _scale = ErosionModel._scale

    def _scale_arg(self, scale):
        """(scale, None) for one triple, (None, scales) for a sequence of B triples."""
        try:
            items = list(scale)
        except TypeError:
            raise ValueError("ErosionBatch: scale must be a triple or a sequence of %d triples" % self.B)
        if len(items) == 3 and all(isinstance(v, numbers.Real) for v in items):
            return [float(v) for v in items], None
        self.scales = items
        self._check_scales()
        return None, items

    def _check_scales(self):
        if len(self.scales) != self.B:
            raise ValueError("ErosionBatch: %d scales for %d models" % (len(self.scales), self.B))
        for b, s in enumerate(self.scales):
            try:
                ok = len(s) == 3 and all(isinstance(v, numbers.Real) for v in s)
            except TypeError:
                ok = False
            if not ok:
                raise ValueError("ErosionBatch: scales[%d] is not 3 numbers: %r" % (b, s))

    def _n_arg(self, n_particles):
        """(N, None) for one walker count, (None, Ns) for a sequence of B counts."""
        try:
            items = list(n_particles)
        except TypeError:
            return int(n_particles), None
        if len(items) != self.B:
            raise ValueError("ErosionBatch: %d walker counts for %d models" % (len(items), self.B))
        Ns = []
        for b, n in enumerate(items):
            if not isinstance(n, numbers.Integral) or isinstance(n, bool) or n < 0:
                raise ValueError("ErosionBatch: Ns[%d] = %r is not a walker count >= 0" % (b, n))
            Ns.append(int(n))
        return None, Ns

    def _per_model(self):
        """True when the models differ in more than their param: the soil_*_batch_models entries."""
        return self.scales is not None or self.Ns is not None or any(self.first_step)

    def _models(self):
        """The B records as they are now, a C array of soil_batch_model (copied by the entry points)."""
        if self.params is not None:
            self._check_params()
        if self.scales is not None:
            self._check_scales()
        models = (_abi.BatchModel * self.B)()
        for b, m in enumerate(models):
            m.param = (self.params[b] if self.params is not None else self.param)._c
            m.scale[:] = [float(v) for v in (self.scales[b] if self.scales is not None else self.scale)]
            m.N = self.Ns[b] if self.Ns is not None else self.N
            m.seed = self.seeds[b]
            m.step_index = self.first_step[b] + self.step_index
        return models

    def _check_params(self):
        from .soil import param_t
        if len(self.params) != self.B:
            raise ValueError("ErosionBatch: %d params for %d models" % (len(self.params), self.B))
        for b, p in enumerate(self.params):
            if not isinstance(p, param_t):
                raise ValueError("ErosionBatch: params[%d] is a %s, not a param_t" % (b, type(p).__name__))

    def _params(self):
        """The sweep's params as they are now, a C array of B soil_param (copied by the entry points)."""
        self._check_params()
        return (_abi.Param * self.B).from_buffer_copy(b"".join(bytes(p._c) for p in self.params))

    @classmethod
    def from_models(cls, models):
        """A new batch holding copies (device to device) of the planes of B whole-grid ErosionModels of one (H, W)
        and one colour setting, model b with the param, scale, walker count, seed and step index of models[b].  An
        empty list, mixed shapes or colour settings, or a row slab raise ValueError before any device work."""
        models = list(models)
        if not models:
            raise ValueError("ErosionBatch.from_models: no models")
        m0 = models[0]
        for b, m in enumerate(models):
            if not isinstance(m, ErosionModel):
                raise ValueError("ErosionBatch.from_models: models[%d] is a %s, not an ErosionModel" % (
                    b, type(m).__name__))
            if m.rows != m.H:
                raise ValueError("ErosionBatch.from_models: models[%d] is a row slab (%d of %d rows)" % (
                    b, m.rows, m.H))
            if (m.H, m.W) != (m0.H, m0.W):
                raise ValueError("ErosionBatch.from_models: models[%d] is %dx%d, models[0] %dx%d" % (
                    b, m.H, m.W, m0.H, m0.W))
            if m.colour != m0.colour:
                raise ValueError("ErosionBatch.from_models: models[%d] has colour=%s, models[0] colour=%s" % (
                    b, m.colour, m0.colour))
        batch = cls(len(models), m0.H, m0.W, [list(m.scale) for m in models], [m.param for m in models],
                    [m.N for m in models], [m.seed for m in models], colour=m0.colour)
        batch.first_step = [int(m.step_index) for m in models]
        for b, m in enumerate(models):
            for name in batch._names():
                batch._copy(name, b, m, into_batch=True)
        return batch

    def to_models(self):
        """B new ErosionModels holding copies of the planes, model b at step index first_step[b] + step_index
        with its own param, scale, walker count and seed."""
        out = []
        for b in range(self.B):
            m = ErosionModel(self.H, self.W, list(self.scales[b]) if self.scales is not None else list(self.scale),
                             self.params[b] if self.params is not None else self.param,
                             self.Ns[b] if self.Ns is not None else self.N, seed=self.seeds[b], colour=self.colour)
            for name in self._names():
                self._copy(name, b, m, into_batch=False)
            m.step_index = self.first_step[b] + self.step_index
            out.append(m)
        return out

    def resized(self, H, W, scale=None, n_particles=None):
        """A new ErosionBatch of the same B and colour setting at (H, W), every plane of every model resampled by
        one launch whatever B is (soil_erode_resize_batch; `height` = the new layers merged, flux planes zero); this
        batch is left as it is.  Carried over: seeds, the param or the params (the same objects), step_index and
        first_step, and whichever of scale / scales and N / Ns the batch uses, so the new batch steps through the
        entry points this one would.  Each scale defaults to the same world with more (or fewer) cells,
        [sx * Ho / H, sy * Wo / W, sz]; `scale` (one triple or B triples) and `n_particles` (one count or B counts)
        replace them, under the constructor's checks.  Raises ValueError before any device work, as the
        constructor does."""
        _check_size("ErosionBatch", H, W)
        if scale is None:
            if self.scales is not None:
                self._check_scales()
                scale = [_rescaled(s, self.H, self.W, H, W) for s in self.scales]
            else:
                scale = _rescaled(self.scale, self.H, self.W, H, W)
        if n_particles is None:
            n_particles = list(self.Ns) if self.Ns is not None else self.N
        elif isinstance(n_particles, numbers.Integral) and not isinstance(n_particles, bool) and n_particles < 0:
            raise ValueError("ErosionBatch.resized: n_particles = %r is not a walker count >= 0" % (n_particles,))
        new = ErosionBatch(self.B, H, W, scale, self.param if self.params is None else list(self.params), n_particles,
                           self.seeds, colour=self.colour, _written=ErosionModel.RESIZED)
        new.step_index = self.step_index
        new.first_step = list(self.first_step)
        _resize_into(new, self, self.B)
        return new

    def stats(self):
        """Every model reduced on the device by two launches whatever B is (soil_erode_batch_stats): a numpy
        structured array of shape (B, 10), element [b, c] channel STAT_CHANNELS[c] of model b, with the fields sum,
        sumsq (fp64, over the finite cells), nonfinite (cells holding NaN or an infinity), min and max (over the
        finite cells; +inf / -inf when there is none); the dtype mirrors soil_channel_stats.  Deterministic: row b
        carries the bytes of ErosionModel.stats() of that model alone.  One entry-point call into a device buffer
        of B x 320 bytes, then one copy of that buffer to the host, the only synchronisation."""
        return _stats(self._planes(), self.B, self.H, self.W)

    def ensemble(self, var=True):
        """(mean, var): per cell, the mean and the population variance across the B models of the six
        ENSEMBLE_CHANNELS, two silt GPU tensors of (H, W, 6) written by one launch whatever B is
        (soil_erode_batch_ensemble: fp64 sums over b in order, var = max(q / B - m * m, 0)).  `var=False`: mean
        only, and the second element is None.  The batch is left as it is; nothing synchronises."""
        mean = silt.tensor(silt.float32, silt.shape(self.H, self.W, len(ENSEMBLE_CHANNELS)), silt.gpu)
        variance = silt.tensor(silt.float32, silt.shape(self.H, self.W, len(ENSEMBLE_CHANNELS)), silt.gpu) if var else None
        _abi.check(_abi.lib().soil_erode_batch_ensemble(C.byref(self._planes()), self.B, self.H, self.W, mean.c_ptr,
                                                        variance.c_ptr if var else None, _abi.stream()))
        return mean, variance

    def _positions(self, who, values, what, top):
        """`values` (one number or a sequence) as a list of floats in [0, top], or ValueError."""
        if isinstance(values, numbers.Real) and not isinstance(values, bool):
            values = [values]
        try:
            items = list(values)
        except TypeError:
            raise ValueError("ErosionBatch.%s: %s must be a number or a sequence of numbers" % (who, what))
        if not items:
            raise ValueError("ErosionBatch.%s: no %s given" % (who, what))
        out = []
        for v in items:
            if not isinstance(v, numbers.Real) or isinstance(v, bool):
                raise ValueError("ErosionBatch.%s: %r is not a number" % (who, v))
            f = float(v)
            if f != f or not 0.0 <= f <= top:
                raise ValueError("ErosionBatch.%s: %r is outside [0, %r]" % (who, v, top))
            out.append(f)
        return out

    def _at_positions(self, pos):
        """(len(pos), H, W, 6): the values at the fractional ranks `pos`, SOIL_QUANTILES_MAX to a call of
        soil_erode_batch_quantiles, each call into its slice of the one tensor."""
        out = silt.tensor(silt.float32, silt.shape(len(pos), self.H, self.W, len(ENSEMBLE_CHANNELS)), silt.gpu)
        per = self.H * self.W * len(ENSEMBLE_CHANNELS) * 4
        planes = self._planes()
        for j0 in range(0, len(pos), _abi.SOIL_QUANTILES_MAX):
            chunk = pos[j0:j0 + _abi.SOIL_QUANTILES_MAX]
            _abi.check(_abi.lib().soil_erode_batch_quantiles(
                C.byref(planes), self.B, self.H, self.W, (C.c_double * len(chunk))(*chunk), len(chunk),
                C.c_void_p(out.ptr + j0 * per), _abi.stream()))
        return out

    def quantiles(self, q):
        """Per cell, the quantiles `q` (one number or a sequence, each in [0, 1]) across the B models of the six
        ENSEMBLE_CHANNELS: a silt GPU tensor of (len(q), H, W, 6) (soil_erode_batch_quantiles).  q[j] is the value
        at fractional rank q[j] * (B - 1) of the cell's B values in the total order of the header (by bit
        pattern: -inf < ... < -0 < +0 < ... < +inf < NaN), interpolated linearly in fp64 between the two order
        statistics around it.  One launch per 16 quantiles whatever B is; q may be unsorted and may repeat.  An
        empty q, a NaN or a value outside [0, 1] raises ValueError before any device work.  The batch is left as
        it is; nothing synchronises."""
        return self._at_positions([v * (self.B - 1) for v in self._positions("quantiles", q, "q", 1.0)])

    def order_statistics(self, ranks):
        """Per cell, the order statistics `ranks` (one integer or a sequence, each in [0, B - 1]; 0 the minimum)
        across the B models: (len(ranks), H, W, 6), each value the bit pattern of one of the models
        (soil_erode_batch_quantiles at exact positions).  A rank that is not an integer or lies outside
        [0, B - 1], or no rank at all, raises ValueError before any device work.  Nothing synchronises."""
        if isinstance(ranks, numbers.Real) and not isinstance(ranks, bool):
            ranks = [ranks]
        try:
            items = list(ranks)
        except TypeError:
            raise ValueError("ErosionBatch.order_statistics: ranks must be an integer or a sequence of integers")
        for r in items:
            if not isinstance(r, numbers.Integral) or isinstance(r, bool):
                raise ValueError("ErosionBatch.order_statistics: rank %r is not an integer" % (r,))
        return self._at_positions(self._positions("order_statistics", [int(r) for r in items], "ranks",
                                                  float(self.B - 1)))

    def median(self):
        """Per cell, the median across the B models, an (H, W, 6) view: position (B - 1) / 2 of
        soil_erode_batch_quantiles (the middle model's value for odd B, the fp64 midpoint of the middle two for
        even B).  Nothing synchronises."""
        out = self._at_positions([(self.B - 1) / 2])
        return silt.tensor.from_device(out.ptr, out.type, tuple(out.shape)[1:], keepalive=out)

    def exceedance(self, thresholds):
        """Per cell and channel, the share of the B models whose value exceeds `thresholds` (six numbers in the
        order of ENSEMBLE_CHANNELS; the comparison is strict, and false with a NaN on either side): an (H, W, 6)
        float32 silt GPU tensor written by one launch whatever B is (soil_erode_batch_exceedance).  Anything but
        six numbers raises ValueError before any device work.  Nothing synchronises."""
        try:
            items = list(thresholds)
        except TypeError:
            raise ValueError("ErosionBatch.exceedance: thresholds must be six numbers (%s)" % ", ".join(ENSEMBLE_CHANNELS))
        if len(items) != len(ENSEMBLE_CHANNELS) or not all(
                isinstance(v, numbers.Real) and not isinstance(v, bool) for v in items):
            raise ValueError("ErosionBatch.exceedance: thresholds must be six numbers (%s), got %r" % (
                ", ".join(ENSEMBLE_CHANNELS), thresholds))
        out = silt.tensor(silt.float32, silt.shape(self.H, self.W, len(ENSEMBLE_CHANNELS)), silt.gpu)
        _abi.check(_abi.lib().soil_erode_batch_exceedance(
            C.byref(self._planes()), self.B, self.H, self.W, (C.c_float * 6)(*[float(v) for v in items]), out.c_ptr,
            _abi.stream()))
        return out

    # ---- flow routing of every model (soil_hip.h: "flow graphs: batches of models") ----

    def _edge(self, who, edge):
        return _check.edge("ErosionBatch.%s" % who, _abi.D8 if edge is None else edge)

    def _flow_tensor(self, who, what, t, dtype):
        """`t` must be a (B, H, W) silt tensor of `dtype`, or ValueError."""
        shape = (self.B, self.H, self.W)
        if not isinstance(t, silt.tensor) or tuple(t.shape) != shape or t.type is not dtype:
            got = "%s %r" % (t.type.name, tuple(t.shape)) if isinstance(t, silt.tensor) else type(t).__name__
            raise ValueError("ErosionBatch.%s: %s must be a %s tensor of shape %r, got %s" % (
                who, what, dtype.name, shape, got))
        return t

    def _optional(self, who, dtype, **tensors):
        """Each of `tensors` (by the argument's name) is None or a (B, H, W) tensor of `dtype`, or ValueError."""
        for what, t in tensors.items():
            if t is not None:
                self._flow_tensor(who, what, t, dtype)

    def _routing(self, who, kind, edge, T, offset, uplift):
        """The arguments that stream_power(), stream_power_deposit() and evolve() route by, or ValueError: the edge
        and the batch's path scale(s)."""
        _check.kind("ErosionBatch.%s" % who, kind, ("steepest", "random_weighted"))
        e = self._edge(who, edge)
        if kind == "random_weighted":
            _check.draw("ErosionBatch.%s" % who, T, offset)
        self._optional(who, silt.float32, uplift=uplift)
        return e, self._path_scale(who)

    def flow(self, kind="steepest", edge=None, T=None, offset=0):
        """The receiver graph of each model's `height` plane: a (B, H, W) int32 silt GPU tensor whose entries are
        cell indices within their model (or -1), written by one launch whatever B is.  `kind`: "steepest"
        (soil_steepest_batch), "direction" (soil_direction_batch: the neighbour's number k instead of its index)
        or "random_weighted" (soil_random_weighted_batch: model b draws with self.seeds[b] at `offset`, and `T`,
        the temperature, is required: 0 or a normal positive float32, soil.valid_temperature).  `edge` defaults to
        d8.  An unknown kind, a missing or refused T or a bad edge raises ValueError before any device work.  Nothing
        synchronises."""
        from . import soil
        _check.kind("ErosionBatch.flow", kind, ("steepest", "direction", "random_weighted"))
        e = self._edge("flow", edge)
        if kind == "random_weighted":
            _check.draw("ErosionBatch.flow", T, offset)
            return soil.random_weighted_batch(self.height, e, self.seeds, int(offset), float(T))
        return (soil.steepest_batch if kind == "steepest" else soil.direction_batch)(self.height, e)

    def drainage(self, graph=None, source=None, decay=None, edge=None):
        """What drains through each cell of each model: `source` accumulated down `graph` (soil_accumulate_batch),
        a (B, H, W) float32 silt GPU tensor.  `graph` defaults to flow(edge=edge); `source` to a plane of ones —
        the number of upstream cells, the cell itself included —, `source=batch.rainfall` gives a discharge;
        `decay`: the per-cell factors of accumulate_decay.  A tensor of the wrong shape or dtype raises ValueError
        before any device work.  Nothing synchronises."""
        from . import soil
        e = self._edge("drainage", edge)
        self._optional("drainage", silt.int32, graph=graph)
        self._optional("drainage", silt.float32, source=source, decay=decay)
        if graph is None:
            graph = self.flow(edge=e)
        if source is None:
            source = silt.tensor(silt.float32, silt.shape(self.B, self.H, self.W), silt.gpu)
            silt.set(source, 1.0)
        return soil.accumulate_batch(graph, source, e, decay)

    def drainage_mfd(self, T=None, p=None, source=None, edge=None, conditioned=True):
        """What drains through each cell of each model under multiple flow directions, exactly
        (soil.mfd_accumulate_batch): a (B, H, W) float32 silt GPU tensor.  Exactly one of `T` and `p` is given: with
        `T` the limit of the mean of drainage() over random_weighted graphs at that temperature, with `p` the
        multiple-flow accumulation with shares proportional to (drop / length) ** p and the batch's scale(s).  `source`
        defaults to ones.  With `conditioned` it runs on filled() with soil.flat_distance_batch routing the flats and
        filled lakes, so that every cell drains off the grid; otherwise on the raw heights, where every pit is a
        terminal.  The batch's planes are not touched.  A wrong argument raises ValueError before any device work.
        Synchronises the stream."""
        from . import soil
        who = "ErosionBatch.drainage_mfd"
        e = self._edge("drainage_mfd", edge)
        if (T is None) == (p is None):
            raise ValueError("%s: exactly one of T and p must be given" % who)
        self._optional("drainage_mfd", silt.float32, source=source)
        scale = None if p is None else self._path_scale("drainage_mfd")
        if T is not None and (isinstance(T, bool) or not isinstance(T, numbers.Real) or not soil.valid_temperature(T)):
            raise ValueError("%s: T must be 0 or a normal positive float32, got %r" % (who, T))
        if p is not None and (_check.number(who, "p", p) > 16):
            raise ValueError("%s: p must be a finite number in 0 .. 16, got %r" % (who, p))
        height, dist = self.height, None
        if conditioned:
            height = soil.fill_depressions_batch(self.height, e)
            dist = soil.flat_distance_batch(height, e)
        return soil.mfd_accumulate_batch(height, source, e, T=T, p=p, scale=scale, dist=dist)

    def flow_slope(self, graph=None):
        """The slope of each model's `height` along `graph` (default: flow()), a (B, H, W) float32 silt GPU tensor
        (soil_slope_batch), with the batch's one scale or model b's own (x, y) of `scales`.  A graph of the wrong
        shape or dtype, or a wrong count of scales, raises ValueError before any device work."""
        from . import soil
        self._optional("flow_slope", silt.int32, graph=graph)
        scale = self._path_scale("flow_slope")
        if graph is None:
            graph = self.flow()
        return soil.slope_batch(self.height, graph, scale)

    def _path_scale(self, who):
        """The batch's one (x, y) scale pair, or model b's own of `scales` (flow_slope's rule)."""
        if self.scales is not None:
            try:
                self._check_scales()
            except ValueError as e:
                raise ValueError("ErosionBatch.%s: %s" % (who, e))
            return [[float(s[0]), float(s[1])] for s in self.scales]
        return [float(self.scale[0]), float(self.scale[1])]

    def basins(self, graph=None, stop=None, edge=None):
        """Where each cell of each model drains to along `graph` (default: flow()): a (B, H, W) int32 silt GPU tensor
        of terminal cells, indices within their model, -1 for a cell on a cycle or draining into one
        (soil_flow_paths_batch).  `stop`: an optional (B, H, W) int32 plane of pour points.  `edge` as in drainage():
        the edges a walk takes, d8 by default, which covers every graph flow() makes; with d4 a diagonal entry of
        `graph` is no edge, and the default graph is flow(edge=d4).  A tensor of the wrong shape or dtype or a bad
        edge raises ValueError before any device work.  Nothing synchronises."""
        from . import soil
        e = self._edge("basins", edge)
        self._optional("basins", silt.int32, graph=graph, stop=stop)
        if graph is None:
            graph = self.flow(edge=e)
        return soil.basins_batch(graph, e, stop)

    def flow_length(self, graph=None, stop=None, edge=None):
        """The length of each cell's way down `graph` (default: flow()) to its terminal, a (B, H, W) float32 silt GPU
        tensor (soil_flow_paths_batch; NaN for a cell on a cycle or draining into one), with the batch's one scale or
        model b's own (x, y) of `scales`, exactly as flow_slope() takes them.  `stop` and `edge` as in basins()."""
        from . import soil
        e = self._edge("flow_length", edge)
        self._optional("flow_length", silt.int32, graph=graph, stop=stop)
        scale = self._path_scale("flow_length")
        if graph is None:
            graph = self.flow(edge=e)
        return soil.flow_length_batch(graph, e, scale, stop)

    def downstream(self, graph=None, a=None, b=None, terminal=None, stop=None, edge=None, scaled=True, double=False):
        """A value carried down `graph` (default: flow()) in every model: x[n] = a[n] L(n) + b[n] x[r(n)], x = terminal
        on the cells without an edge (soil_downstream_batch), a (B, H, W) float32 silt GPU tensor (float64 with
        `double`).  `a`, `b`, `terminal`: (B, H, W) float32 tensors or None (1, 1, 0); L is the edge's length under the
        batch's scale(s), as flow_length() takes them, or 1 with scaled=False.  `stop` and `edge` as in basins().  A
        tensor of the wrong shape or dtype or a bad edge raises ValueError before any device work.  Nothing
        synchronises."""
        from . import soil
        e = self._edge("downstream", edge)
        self._optional("downstream", silt.int32, graph=graph)
        self._optional("downstream", silt.float32, a=a, b=b, terminal=terminal)
        self._optional("downstream", silt.int32, stop=stop)
        scale = self._path_scale("downstream") if scaled else None
        if graph is None:
            graph = self.flow(edge=e)
        return soil.downstream_batch(graph, e, a, b, terminal, scale, stop, double)

    def stream_power(self, dt, K, m=0.5, kind="steepest", edge=None, T=None, offset=0, uplift=None, n=1.0, iters=12,
                     residual=False):
        """One implicit stream-power step of every model, on its conditioned surface: conditioned() ->
        drainage(graph=g) -> soil.erosivity(area, K, m) -> soil.stream_power_batch on the filled surface with the
        batch's scale(s).  Returns the (B, H, W) float32 heights after the step; the batch's own planes are not
        touched.  `uplift`: a (B, H, W) float32 tensor or None; `kind`, `edge`, `T`, `offset` as in conditioned().
        `n`: the slope exponent, 1 .. 16; with n != 1 the last link is soil.stream_power_n_batch with `iters` Newton
        steps, and `residual` returns (heights, residual) as it does (with n == 1 the residual is a tensor of zeros).
        A bad argument raises ValueError before any device work.  Synchronises the stream (the fill does)."""
        from . import soil
        who = "ErosionBatch.stream_power"
        _check.number(who, "dt", dt)
        _check.number(who, "K", K)
        _check.number(who, "m", m, lo=None)
        n = _check.exponent(who, n)
        _check.count(who, "iters", iters)
        e, scale = self._routing("stream_power", kind, edge, T, offset, uplift)
        filled, graph = self.conditioned(kind, e, T, offset)
        area = self.drainage(graph=graph, edge=e)
        if n == 1.0 and not residual:
            return soil.stream_power_batch(filled, graph, soil.erosivity(area, K, m), e, scale, dt, uplift)
        return soil.stream_power_n_batch(filled, graph, soil.erosivity(area, K, m), e, scale, dt, n, uplift, None,
                                         int(iters), False, residual)

    def stream_power_deposit(self, dt, K, m=0.5, G=1.0, iters=8, kind="steepest", edge=None, T=None, offset=0,
                             uplift=None, flux=False, residual=False):
        """One implicit stream-power step with sediment deposition of every model, on its conditioned surface:
        conditioned() -> drainage(graph=g) -> soil.erosivity(area, K, m) and soil.deposition(area, G, cell) ->
        soil.stream_power_deposit_batch with `iters` iterations and the batch's scale(s); `cell` is the product of a
        model's scale pair.  Returns the (B, H, W) float32 heights after the step, or with `flux` / `residual` a tuple
        with those as soil.stream_power_deposit_batch returns them; the batch's own planes are not touched.  `G`: the
        deposition coefficient, a finite number >= 0; the rest as in stream_power().  A bad argument raises ValueError
        before any device work.  Synchronises the stream (the fill does)."""
        from . import soil
        who = "ErosionBatch.stream_power_deposit"
        _check.number(who, "dt", dt)
        _check.number(who, "K", K)
        _check.number(who, "m", m, lo=None)
        _check.number(who, "G", G)
        _check.count(who, "iters", iters)
        e, scale = self._routing("stream_power_deposit", kind, edge, T, offset, uplift)
        filled, graph = self.conditioned(kind, e, T, offset)
        area = self.drainage(graph=graph, edge=e)
        # a cell's area, model by model: float32 of the product of its pair, one value a model either way
        pairs = scale if self.scales is not None else [scale] * self.B
        cell = silt.tensor.from_numpy(np.array([s[0] * s[1] for s in pairs], np.float32).reshape(self.B, 1, 1)).gpu()
        return soil.stream_power_deposit_batch(filled, graph, soil.erosivity(area, K, m), soil.deposition(area, G, cell),
                                               e, scale, dt, uplift, int(iters), False, flux, residual)

    def stream_power_deposit_n(self, dt, K, m=0.5, G=1.0, n=2.0, iters=None, kind="steepest", edge=None, T=None,
                               offset=0, uplift=None, flux=False, residual=False):
        """stream_power_deposit() at a slope exponent `n` in 1 .. 16, dh/dt = u - K A^m S^n + (G / A) Qs: the same
        chain, conditioned() -> drainage(graph=g) -> soil.erosivity(area, K, m) and soil.deposition(area, G, cell) ->
        soil.stream_power_deposit_n_batch with `iters` iterations (None: its default) and the batch's scale(s).
        Returns what stream_power_deposit() returns; the batch's own planes are not touched.  The iteration has a
        domain (soil.stream_power_deposit_n): ask for the residual where K dt / L is large and G is above 1.  A bad
        argument raises ValueError before any device work.  Synchronises the stream (the fill does)."""
        from . import soil
        who = "ErosionBatch.stream_power_deposit_n"
        _check.number(who, "dt", dt)
        _check.number(who, "K", K)
        _check.number(who, "m", m, lo=None)
        _check.number(who, "G", G)
        n = _check.exponent(who, n)
        iters = _check.count(who, "iters", soil.DEPOSIT_N_ITERS if iters is None else iters)
        e, scale = self._routing("stream_power_deposit_n", kind, edge, T, offset, uplift)
        filled, graph = self.conditioned(kind, e, T, offset)
        area = self.drainage(graph=graph, edge=e)
        pairs = scale if self.scales is not None else [scale] * self.B  # (a cell's area: stream_power_deposit's)
        cell = silt.tensor.from_numpy(np.array([s[0] * s[1] for s in pairs], np.float32).reshape(self.B, 1, 1)).gpu()
        return soil.stream_power_deposit_n_batch(filled, graph, soil.erosivity(area, K, m),
                                                 soil.deposition(area, G, cell), e, scale, dt, n, uplift, int(iters),
                                                 False, flux, residual)

    def evolve_deposit(self, dt, K, G, n, m=0.5, kappa=None, critical_slope=None, uplift=None, iters=None,
                       kind="steepest", edge=None, T=None, offset=0, first_axis=0):
        """The landscape-evolution step with every term the library has: stream_power_deposit_n(dt, K, m, G, n, iters,
        ...), then with `critical_slope` (as in slope_limited()) the collapse to the threshold, soil.slope_limit_batch
        with the step's `edge`, then soil.diffuse_batch over the same `dt` with the diffusivity `kappa` and
        border="fixed", as in evolve().  The uplift is applied once, in the first step.  Returns the (B, H, W) float32
        heights; the batch's own planes are not touched.  A bad argument raises ValueError before any device work.
        Synchronises the stream (the fill does)."""
        from . import soil
        who = "ErosionBatch.evolve_deposit"
        self._check_diffuse("evolve_deposit", dt, kappa, None, None, None, "fixed", first_axis)
        e = self._edge("evolve_deposit", edge)
        if critical_slope is not None:
            critical_slope = self._critical_slope("evolve_deposit", critical_slope)
        _check.number(who, "K", K)
        _check.number(who, "m", m, lo=None)
        _check.number(who, "G", G)
        _check.exponent(who, n)
        if iters is not None:
            _check.count(who, "iters", iters)
        _, scale = self._routing("evolve_deposit", kind, edge, T, offset, uplift)
        carved = self.stream_power_deposit_n(dt, K, m, G, n, iters, kind, edge, T, offset, uplift)
        if critical_slope is not None:
            carved = soil.slope_limit_batch(carved, scale, critical_slope, e)
        return soil.diffuse_batch(carved, scale, dt, kappa, border="fixed", first_axis=first_axis)

    def _check_diffuse(self, who, dt, kappa, diffusivity, uplift, fixed, border, first_axis):
        """The arguments of diffuse() and of the diffusion half of evolve(), or ValueError."""
        full = "ErosionBatch.%s" % who
        _check.number(full, "dt", dt)
        _check.kappa_or_diffusivity(full, kappa, diffusivity)
        self._optional(who, silt.float32, diffusivity=diffusivity, uplift=uplift)
        self._optional(who, silt.int32, fixed=fixed)
        _check.border(full, border)
        _check.first_axis(full, first_axis)

    def diffuse(self, dt, kappa=None, diffusivity=None, uplift=None, fixed=None, border="fixed", first_axis=0,
                double=False):
        """One implicit step of hillslope diffusion of every model's `height` over `dt` (soil.diffuse_batch) with the
        batch's scale(s), as flow_length() takes them: a (B, H, W) float32 silt GPU tensor (float64 with `double`).
        Exactly one of `kappa` (a number) and `diffusivity` (a (B, H, W) float32 tensor); `uplift`, `fixed`, `border`
        and `first_axis` as in soil.diffuse.  The batch's own planes are not touched.  A bad argument raises
        ValueError before any device work.  Nothing synchronises."""
        from . import soil
        self._check_diffuse("diffuse", dt, kappa, diffusivity, uplift, fixed, border, first_axis)
        scale = self._path_scale("diffuse")
        return soil.diffuse_batch(self.height, scale, dt, kappa, diffusivity, uplift, fixed, border, first_axis, double)

    def evolve(self, dt, K, m=0.5, kappa=None, uplift=None, kind="steepest", edge=None, T=None, offset=0,
               first_axis=0, G=None, iters=8, n=1.0):
        """One landscape-evolution step of every model, uplift + stream power + linear diffusion: stream_power(dt, K,
        m, kind, edge, T, offset, uplift) and then soil.diffuse_batch of its result over the same `dt` with the
        diffusivity `kappa` and border="fixed" — the outermost cells, the base level of the conditioned graph, keep
        what the stream-power step left them.  The uplift is applied once, in the stream-power step.  With `G` (a
        finite number >= 0) the first half is stream_power_deposit(dt, K, m, G, iters, ...) instead: the eroded
        material is deposited on its way down.  With `n` != 1 (a slope exponent in 1 .. 16) the first half is
        stream_power(..., n=n, iters=iters); `G` together with n != 1 raises ValueError here: that step is
        evolve_deposit(), on stream_power_deposit_n().  Returns the (B, H, W) float32 heights; the batch's own planes
        are not touched.  A bad argument raises ValueError before any device work.  Synchronises the stream (the fill
        does)."""
        from . import soil
        carved, scale = self._carved("evolve", dt, K, m, kappa, uplift, kind, edge, T, offset, first_axis, G, iters, n)
        return soil.diffuse_batch(carved, scale, dt, kappa, border="fixed", first_axis=first_axis)

    def _carved(self, name, dt, K, m, kappa, uplift, kind, edge, T, offset, first_axis, G, iters, n):
        """The checks of evolve() under the method's `name` and its first half: (the carved surface, the scale(s))."""
        who = "ErosionBatch.%s" % name
        self._check_diffuse(name, dt, kappa, None, None, None, "fixed", first_axis)
        n = _check.exponent(who, n)
        if G is not None:
            _check.number(who, "G", G)
            _check.count(who, "iters", iters)
            if n != 1.0:
                raise ValueError("%s: G (deposition) takes the slope exponent n = 1 only, got n = %r" % (who, n))
        elif n != 1.0:
            _check.count(who, "iters", iters)
        _check.number(who, "K", K)
        _check.number(who, "m", m, lo=None)
        _, scale = self._routing(name, kind, edge, T, offset, uplift)
        if G is None and n != 1.0:
            carved = self.stream_power(dt, K, m, kind, edge, T, offset, uplift, n, iters)
        elif G is None:
            carved = self.stream_power(dt, K, m, kind, edge, T, offset, uplift)
        else:
            carved = self.stream_power_deposit(dt, K, m, G, iters, kind, edge, T, offset, uplift)
        return carved, scale

    def _critical_slope(self, who, slope):
        """`slope` of slope_limited() and evolve_limited(): a finite number >= 0 or a (B, H, W) float32 tensor."""
        if isinstance(slope, silt.tensor):
            return self._flow_tensor(who, "slope", slope, silt.float32)
        return _check.number("ErosionBatch.%s" % who, "slope", slope)

    def slope_limited(self, slope, edge=None, excess=False):
        """The slope-limited surface of every model's `height` (soil.slope_limit_batch) with the batch's scale(s), as
        diffuse() takes them: the greatest surface below the heights on which no cell stands higher above a neighbour
        than `slope` times the distance allows — a (B, H, W) float32 silt GPU tensor, or with `excess` the tuple
        (surface, excess), excess = height - surface, the mass above the threshold.  `slope`: a finite number >= 0 or
        a (B, H, W) float32 tensor (an entry that is NaN or negative: no limit at that cell); `edge` defaults to d8.
        The batch's own planes are not touched.  A bad argument raises ValueError before any device work.
        Synchronises the stream."""
        from . import soil
        e = self._edge("slope_limited", edge)
        slope = self._critical_slope("slope_limited", slope)
        scale = self._path_scale("slope_limited")
        return soil.slope_limit_batch(self.height, scale, slope, e, excess)

    def evolve_limited(self, dt, K, critical_slope, m=0.5, kappa=None, uplift=None, kind="steepest", edge=None, T=None,
                       offset=0, first_axis=0, G=None, iters=8, n=1.0):
        """evolve() with threshold hillslopes: incision, then collapse to the threshold, then diffusion.  The carved
        surface of evolve()'s first half goes through soil.slope_limit_batch with `critical_slope` (a finite number
        >= 0 or a (B, H, W) float32 tensor, as in slope_limited()) and the step's `edge` before soil.diffuse_batch
        relaxes it.  What collapses is removed, not deposited: slope_limited(..., excess=True) on a surface gives
        the collapsed mass to a caller who wants to route it.  Everything else as in evolve(), whose own calls are
        what they were."""
        from . import soil
        e = self._edge("evolve_limited", edge)
        critical_slope = self._critical_slope("evolve_limited", critical_slope)
        carved, scale = self._carved("evolve_limited", dt, K, m, kappa, uplift, kind, edge, T, offset, first_axis, G,
                                     iters, n)
        limited = soil.slope_limit_batch(carved, scale, critical_slope, e)
        return soil.diffuse_batch(limited, scale, dt, kappa, border="fixed", first_axis=first_axis)

    def filled(self, edge=None):
        """The depression-filled surface of every model's `height`: a (B, H, W) float32 silt GPU tensor, model b's
        plane what soil.fill_depressions gives for it alone (soil_fill_depressions_batch: one call for the batch,
        launches that do not grow with B).  `edge` defaults to d8.  Synchronises the stream."""
        from . import soil
        e = self._edge("filled", edge)
        return soil.fill_depressions_batch(self.height, e)

    def conditioned(self, kind="steepest", edge=None, T=None, offset=0):
        """(filled, graph): filled() and the receiver graph of that surface with its flats and lakes routed
        (soil.resolve_flats_batch), a (B, H, W) int32 tensor of cell indices within their model whose only terminals
        are cells on the border or beside NaN cells.  `kind`: "steepest" or "random_weighted" — drawn on the filled
        surface with self.seeds, `T` and `offset` checked as flow() checks them; "direction" is refused, its entries
        are no indices.  drainage(graph=g), basins(graph=g) and flow_length(graph=g) take this graph as it is: where
        flow() stops at every closed pit of an eroded model, every cell then drains off the grid.  A bad kind, edge,
        T or offset raises ValueError before any device work.  Synchronises the stream."""
        from . import soil
        _check.kind("ErosionBatch.conditioned", kind, ("steepest", "random_weighted"),
                    " (the entries of 'direction' are not indices)")
        e = self._edge("conditioned", edge)
        if kind == "random_weighted":
            _check.draw("ErosionBatch.conditioned", T, offset)
        filled = soil.fill_depressions_batch(self.height, e)
        graph = None
        if kind == "random_weighted":
            graph = soil.random_weighted_batch(filled, e, self.seeds, int(offset), float(T))
        return filled, soil.resolve_flats_batch(filled, e, graph)

    # ---- upstream extrema and breaching (soil_hip.h: "flow graphs: upstream extrema") ----

    def _upstream(self, who, batch_call, value, graph, stop, edge, arg):
        e = self._edge(who, edge)
        self._flow_tensor(who, "value", value, silt.float32)
        self._optional(who, silt.int32, graph=graph, stop=stop)
        if graph is None:
            graph = self.flow(edge=e)
        return batch_call(graph, value, e, stop, arg)

    def upstream_min(self, value, graph=None, stop=None, edge=None, arg=False):
        """For every cell of every model the least of `value`, a (B, H, W) float32 tensor, over all the cells that
        drain through it along `graph` (default: flow()), the cell itself included (soil_upstream_extreme_batch): a
        (B, H, W) float32 silt GPU tensor, with `arg` the pair (out, arg), arg the int32 index within its model of the
        cell that holds the value (the smallest among equals, -1 where out is NaN).  NaN is ignored wherever a number
        reaches the cell; cycles are allowed.  `stop` and `edge` as in basins().  A tensor of the wrong shape or dtype
        or a bad edge raises ValueError before any device work.  Nothing synchronises."""
        from . import soil
        return self._upstream("upstream_min", soil.upstream_min_batch, value, graph, stop, edge, arg)

    def upstream_max(self, value, graph=None, stop=None, edge=None, arg=False):
        """The greatest of `value` over all the cells that drain through each cell: -upstream_min(-value), as
        soil.upstream_max_batch states it."""
        from . import soil
        return self._upstream("upstream_max", soil.upstream_max_batch, value, graph, stop, edge, arg)

    def breached(self, kind="steepest", edge=None, T=None, offset=0):
        """(surface, graph): the graph of conditioned() and every model's ORIGINAL `height` carved along it
        (soil.breach_batch) — each cell lowered to the lowest height of anything that drains through it.  The surface
        never stands above `height` and never rises along the graph, where filled() raises every lake to its rim.
        soil.stream_power_batch(surface, graph, ...) on this pair is the step that adds no mass: the solver methods
        of the batch run on the filled surface and turn every lake into land at each step.  `kind`, `edge`, `T`,
        `offset` as in conditioned().  Synchronises the stream (the fill does)."""
        from . import soil
        e = self._edge("breached", edge)
        _, graph = self.conditioned(kind, e, T, offset)
        return soil.breach_batch(self.height, graph, e), graph

    def upstream_length(self, graph=None, stop=None, edge=None):
        """The length of the longest way down to each cell along `graph` (default: flow()), a (B, H, W) float32 silt
        GPU tensor (soil.upstream_length_batch): the greatest flow_length() in the cell's catchment less the cell's
        own, with the batch's scale(s) as flow_length() takes them.  NaN for a cell on a cycle or draining into one.
        `stop` and `edge` as in basins()."""
        from . import soil
        e = self._edge("upstream_length", edge)
        self._optional("upstream_length", silt.int32, graph=graph, stop=stop)
        scale = self._path_scale("upstream_length")
        if graph is None:
            graph = self.flow(edge=e)
        return soil.upstream_length_batch(graph, e, scale, stop)

    # ---- stream order and channel segments (soil_hip.h: "flow graphs: stream order") ----

    def _network(self, who, threshold, kind, edge, graph, area):
        """The (graph, area, edge) a channel network is cut from: those given, or conditioned() -> drainage() as the
        solver methods route."""
        _check.number("ErosionBatch.%s" % who, "threshold", threshold, lo=None)
        _check.kind("ErosionBatch.%s" % who, kind, ("steepest", "random_weighted"))
        e = self._edge(who, edge)
        self._optional(who, silt.int32, graph=graph)
        self._optional(who, silt.float32, area=area)
        if graph is None:
            _, graph = self.conditioned(kind, e)
        if area is None:
            area = self.drainage(graph=graph, edge=e)
        return graph, area, e

    def stream_order(self, threshold, kind="steepest", edge=None, graph=None, area=None, donors=False):
        """The Strahler order of every cell of every model, a (B, H, W) int32 silt GPU tensor, 0 off the channels
        (soil.stream_order_batch): the channels are the cells whose drainage area is >= `threshold`.  `graph=None`:
        the graph of conditioned(kind, edge); `area=None`: drainage() along the graph, the count of upstream cells.
        With `donors` returns (order, donors).  The batch's own planes are not touched.  A tensor of the wrong shape
        or dtype, a bad kind, edge or threshold raises ValueError before any device work.  Synchronises the stream."""
        from . import soil
        g, a, e = self._network("stream_order", threshold, kind, edge, graph, area)
        return soil.stream_order_batch(g, e, None, a, float(threshold), None, donors)

    def stream_segments(self, threshold, kind="steepest", edge=None, graph=None, area=None, by="link"):
        """(order, segment, steps, length) of every model's channel network (soil.stream_segments_batch), the
        channels, `graph` and `area` as in stream_order(), lengths with the batch's scale(s); `by` is "link" or
        "order".  A non-channel cell is its own segment at distance 0 with order 0."""
        from . import soil
        scale = self._path_scale("stream_segments")
        g, a, e = self._network("stream_segments", threshold, kind, edge, graph, area)
        return soil.stream_segments_batch(g, e, None, a, float(threshold), None, scale, by)

    def _copy(self, name, b, model, into_batch):
        """Plane `name` of model b of the batch from (into_batch) or to ErosionModel `model`, on the stream."""
        t, single = getattr(self, name), getattr(model, name)
        per = t.nbytes() // self.B
        if single.nbytes() != per:
            raise ValueError("plane %s: %d bytes per model, the single model holds %d" % (name, per, single.nbytes()))
        here = t.ptr + b * per
        dst, src = (here, single.ptr) if into_batch else (single.ptr, here)
        _abi.check(_abi.lib().soil_memcpy_d2d(C.c_void_p(dst), C.c_void_p(src), per, _abi.stream()))

    def _call(self, entry, walkers, *flags):
        """The batch's form of `entry` (soil_erode_step_batch, soil_particles_batch, soil_erode_cells_fused_batch):
        _models for different models, _params for a sweep, _colour with colour planes, else `entry` itself, with
        the arguments that form takes.  `walkers`: the entry takes N, the seeds and the step index; `flags`: what
        goes before the stream."""
        args = (self.B, self.H, self.W)
        if self._per_model():
            suffix, args = "_models", args + (self._models(),)
        else:
            suffix = "_params" if self.params is not None else "_colour" if self.colour else ""
            if walkers:
                args += (self.N, self._seeds, self.step_index)
            args += (self._scale(), self._params() if self.params is not None else self.param._ref())
        # the plain entries take no colour planes, _colour needs them, _params and _models take them or NULL
        colour = (C.byref(self._colour()) if self.colour else None,) if suffix else ()
        _abi.check(getattr(_abi.lib(), entry + suffix)(C.byref(self._planes()), *colour, *args, *flags, _abi.stream()))

    def set_layers(self, layers_tensor):
        """Copy a (B, H, W, 2) tensor of (bedrock, sediment) into the batch."""
        if tuple(layers_tensor.shape) != (self.B, self.H, self.W, 2):
            raise ValueError("set_layers needs a (%d, %d, %d, 2) tensor, got %s" % (
                self.B, self.H, self.W, tuple(layers_tensor.shape)))
        silt.set(self.layers, layers_tensor)

    def set_colour(self, name, tensor):
        """Copy a (B, H, W, 3) tensor into colour plane `name` (one of PLANES_3) of a coloured batch."""
        if not self.colour:
            raise ValueError("set_colour: the batch was made without colour planes (colour=False)")
        if name not in self.PLANES_3:
            raise ValueError("set_colour: %r is not a colour plane (%s)" % (name, ", ".join(self.PLANES_3)))
        if tuple(tensor.shape) != (self.B, self.H, self.W, 3):
            raise ValueError("set_colour needs a (%d, %d, %d, 3) tensor, got %s" % (
                self.B, self.H, self.W, tuple(tensor.shape)))
        silt.set(getattr(self, name), tensor)

    def particles(self):
        """Both particle launches of this step for every model, adding into the flux planes
        (soil_particles_batch); with colour the two colour flux planes are cleared first and receive this
        step's colour flux (soil_particles_batch_colour).  A sweep: soil_particles_batch_params; different
        models: soil_particles_batch_models."""
        self._call("soil_particles_batch", True)

    def cells_fused(self, keep_flux=False):
        """Fused cell phase of every model (soil_erode_cells_fused_batch[_colour]); `keep_flux`: the flux
        planes are left as they are (SOIL_CELLS_KEEP_FLUX).  A sweep: soil_erode_cells_fused_batch_params;
        different models: soil_erode_cells_fused_batch_models."""
        self._call("soil_erode_cells_fused_batch", False, _abi.SOIL_CELLS_KEEP_FLUX if keep_flux else 0)

    def swap_layers(self):
        self.layers, self.layers_next = self.layers_next, self.layers

    def step(self):
        """One erosion step of every model (soil_erode_step_batch, with colour soil_erode_step_batch_colour);
        swaps the layer buffers.  A sweep: soil_erode_step_batch_params; different models:
        soil_erode_step_batch_models."""
        self._call("soil_erode_step_batch", True)
        self.swap_layers()
        self.step_index += 1

    def model_plane(self, name, b):
        """Plane `name` of model b as a host numpy array, (H, W[, C])."""
        if not 0 <= b < self.B:
            raise IndexError("model %d of a batch of %d" % (b, self.B))
        t = getattr(self, name)
        dims = tuple(t.shape)[1:]
        per = t.nbytes() // self.B
        view = silt.tensor.from_device(t.ptr + b * per, t.type, dims, keepalive=t)
        return view.cpu().numpy()

    def model_planes(self, b):
        """Every plane of model b as host numpy arrays, by name (the colour planes too, with colour)."""
        return {name: self.model_plane(name, b) for name in self._names()}
