"""Row-slab sharding of the erosion step across the GPUs of one node — Python face of the
library's slab runner (include/soil_slab.h, csrc/slab_runner.hip).

One process per GPU.  Rank r owns global rows [r*S, (r+1)*S) of a (world*S, W) grid plus
G = soil_ghost_rows(param) = ceil(sqrt(2)*maxage)+2 ghost rows per interior side: one particle
step moves at most sqrt(2) cells (erosion_map.cu:61-76), so no trajectory born in the owned
rows can leave the slab and the sharded step is EXACT (same trajectories, same deposits as the
single-GPU run; only the fp32 summation order of the flux differs).  The step — exchange
schedule, halos trimmed to the measured reach of the walks, repeat-launch fallback, RCCL
send/recv groups on the runner's own HIP streams — is C++ inside libsoil_hip.so; what is left
here is construction:

  SlabRunner      forwards to soil_slab_create / soil_slab_step / soil_slab_plane
  RcclComm        the library's RCCL communicator (soil_comm_rccl_*); the 128-byte id travels
                  through torch.distributed's store (gloo), which is all torch is used for
  CallbackComm    a soil_comm made of Python callables: gloo on staged host buffers (several
                  ranks sharing one GPU, or no GPU at all) and the in-process wire of the tests
  CallbackOps     a soil_slab_ops made of Python callables: the CPU tests plug the oracle in
                  here, so that world-size-2/3 gloo runs exercise the library's own host logic

SlabRunner(..., colour=True) is the sharded coloured step (soil_slab_create_colour): the four colour
planes of ErosionModel(colour=True) ride through every step, their owned rows ending as the
whole-grid soil_erode_step_colour leaves them ("Colour on slabs").
"""
import ctypes as C
import os

from . import _abi

FIELD_PLANES = ("layers", "velocity", "waterHeight", "debrisVelocity")
FLUX_FLUVIAL = ("waterFlux", "massFlux", "velocityFlux")      # final after the fluvial launch
FLUX_DEBRIS = ("debrisFlux", "debrisVelocityFlux")            # final after the debris launch
FLUX_PLANES = FLUX_FLUVIAL + FLUX_DEBRIS
PLANE_CHANNELS = {
    "layers": 2, "layers_next": 2, "height": 1, "uplift": 1, "rainfall": 1, "waterHeight": 1,
    "waterFlux": 1, "mass": 1, "massFlux": 1, "velocity": 2, "velocityFlux": 2, "debris": 1,
    "debrisFlux": 1, "debrisVelocity": 2, "debrisVelocityFlux": 2,
    "albedo_bedrock": 3, "albedo_surface": 3, "albedo_fluvial": 3, "albedo_debris": 3,
}
# the planes a coloured runner adds (soil_colour_planes; soil_slab_plane refuses them on a physics runner)
COLOUR_PLANES = ("albedo_bedrock", "albedo_surface", "albedo_fluvial", "albedo_debris")


def slab_layout(rank, world, S, G):
    """Rows a rank holds: (x0, rows, r0, r1) — global row of local row 0, local
    row count, owned local row range (soil_slab_layout)."""
    out = (C.c_int64 * 4)()
    _abi.lib().soil_slab_layout(rank, world, S, G, out)
    return tuple(int(v) for v in out)


# ---- the wire -------------------------------------------------------------------------

class SelfComm:
    """A world of one (soil_comm_self_create)."""

    def __init__(self):
        self.rank, self.world = 0, 1
        self._c = C.POINTER(_abi.Comm)()
        _abi.check(_abi.lib().soil_comm_self_create(C.byref(self._c)))

    def c_comm(self):
        return self._c

    def barrier(self):
        pass

    def max_over_ranks(self, value):
        return float(value)

    def describe(self):
        return {"backend": "self", "world_size": 1}

    def close(self):
        if self._c:
            _abi.lib().soil_comm_self_destroy(self._c)
            self._c = None


class WedgedComm:
    """A wire whose every operation blocks like a transfer whose peer never shows up, under the
    library's watchdog (soil_comm_wedged_create): the tests' proof that a dead wire surfaces as
    CommError within its timeout instead of hanging the host."""

    def __init__(self, rank=0, world=2, timeout_s=1.0):
        self.rank, self.world = rank, world
        self._c = C.POINTER(_abi.Comm)()
        _abi.check(_abi.lib().soil_comm_wedged_create(C.byref(self._c), rank, world, float(timeout_s)))

    def c_comm(self):
        return self._c

    def describe(self):
        return {"backend": "wedged (test)", "world_size": self.world}

    def close(self):
        if self._c:
            _abi.lib().soil_comm_wedged_destroy(self._c)
            self._c = None


def _dist_env():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def _init_gloo():
    """torch.distributed over gloo: the bootstrap channel (ids, timings), never the data path of a
    GPU run."""
    import torch.distributed as dist
    if not dist.is_initialized():
        for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29671"), ("RANK", "0"),
                     ("WORLD_SIZE", "1")):
            os.environ.setdefault(k, v)
        dist.init_process_group(backend="gloo")
    return dist


def rccl_library():
    """Which librccl the library bound and its version (soil_comm_rccl_library)."""
    path, v = C.create_string_buffer(1024), C.c_int32()
    _abi.check(_abi.lib().soil_comm_rccl_library(path, 1024, C.byref(v)))
    return {"librccl": path.value.decode(), "rccl_version": "%d.%d.%d" % (v.value // 10000, v.value // 100 % 100,
                                                                          v.value % 100)}


class RcclComm:
    """RCCL communicator owned by libsoil_hip.so (soil_comm_rccl_create).  Rank 0 makes the id,
    torch.distributed (gloo) broadcasts its 128 bytes."""

    def __init__(self):
        import torch
        dist = self.dist = _init_gloo()
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        lib = _abi.lib()
        uid = (C.c_uint8 * 128)()
        failed, why = 0, None
        if self.rank == 0:
            try:
                _abi.check(lib.soil_comm_rccl_unique_id(uid))
            except Exception as e:      # noqa: BLE001  (the broadcast below must still take place)
                failed, why = 1, e
        else:
            # Every rank proves that it can load librccl and call into it BEFORE anybody enters the
            # collective ncclCommInitRank: a rank that cannot would leave the others blocked in there, and
            # the fallback to gloo could never be agreed on (advisor finding of round 3).  The probe binds
            # the library and asks for its version — no thread, no socket (round 4's probe made a unique
            # id on every rank, which starts a bootstrap root per call).  (What is left uncovered: a
            # failure INSIDE the collective on a subset of ranks — RCCL's own bootstrap time-out ends that.)
            try:
                _abi.check(lib.soil_comm_rccl_probe(None))
            except Exception as e:      # noqa: BLE001
                failed, why = 1, e
        bad = torch.tensor([failed])
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        t = torch.tensor(list(uid) + [failed], dtype=torch.uint8)
        dist.broadcast(t, 0)
        if int(bad.item()):
            raise RuntimeError("librccl is not usable on %s: %s" % ("this rank" if failed else "another rank", why))
        uid = (C.c_uint8 * 128)(*t[:128].tolist())
        self._c = C.POINTER(_abi.Comm)()
        _abi.check(lib.soil_comm_rccl_create(C.byref(self._c), uid, self.rank, self.world))

    def c_comm(self):
        return self._c

    def barrier(self):
        self.dist.barrier()

    def max_over_ranks(self, value):
        import torch
        t = torch.tensor([float(value)], dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def describe(self):
        n, r, d = C.c_int32(), C.c_int32(), C.c_int32()
        _abi.check(_abi.lib().soil_comm_rccl_info(self._c, C.byref(n), C.byref(r), C.byref(d)))
        return dict(rccl_library(), backend="rccl (libsoil_hip: ncclSend/ncclRecv groups)",
                    world_size=int(n.value), rank=int(r.value), device=int(d.value))

    def close(self, keep_group=False):
        if self._c:
            _abi.lib().soil_comm_rccl_destroy(self._c)
            self._c = None
        if not keep_group and self.dist.is_initialized():
            self.dist.barrier()
            self.dist.destroy_process_group()


class CallbackComm:
    """soil_comm whose three entry points are Python callables (SOIL_COMM_HOST_ORDERED: the runner
    synchronises its back-end before every call and the call blocks until the data have landed).

    impl.exchange(sends, recvs)   lists of (address, bytes, peer)
    impl.all_reduce(address, n)   in-place float32 sum over the ranks
    impl.barrier()
    """

    def __init__(self, rank, world, impl):
        self.rank, self.world, self.impl = int(rank), int(world), impl
        self.error = None

        def guard(fn):
            def run(*a):
                try:
                    fn(*a)
                    return 0
                except BaseException as e:      # an exception cannot cross the C frames
                    self.error = e
                    return _abi.SOIL_ERR_HIP
            return run

        def xfers(p, n):
            return [(int(p[i].ptr or 0), int(p[i].bytes), int(p[i].peer)) for i in range(n)]

        self._ex = _abi.EXCHANGE_FN(guard(lambda ctx, s, ns, r, nr, st: impl.exchange(xfers(s, ns), xfers(r, nr))))
        self._ar = _abi.ALLREDUCE_FN(guard(lambda ctx, buf, n, st: impl.all_reduce(int(buf), int(n))))
        self._ba = _abi.BARRIER_FN(guard(lambda ctx: impl.barrier()))
        self._comm = _abi.Comm(None, self.rank, self.world, _abi.SOIL_COMM_HOST_ORDERED, self._ex, self._ar,
                               self._ba)

    def c_comm(self):
        return C.pointer(self._comm)

    def barrier(self):
        self.impl.barrier()

    def max_over_ranks(self, value):
        return self.impl.max_over_ranks(value)

    def describe(self):
        note = getattr(self, "note", None)
        return {"backend": note or type(self.impl).__name__, "world_size": self.world}

    def close(self):
        if hasattr(self.impl, "close"):
            self.impl.close()


class GlooWire:
    """torch.distributed (gloo) as the wire of a CallbackComm.  `device` memory is staged through
    host buffers (soil_memcpy_d2h / h2d) — functional only, tens of MB/s: several ranks sharing one
    GPU in tests; with `device=False` the addresses are host memory (CPU back-end)."""

    def __init__(self, device):
        self.dist = _init_gloo()
        self.device = device

    def _view(self, addr, nbytes):
        import numpy as np
        return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(addr))

    def _to_host(self, addr, nbytes):
        import numpy as np
        if not self.device:
            return self._view(addr, nbytes)
        h = np.empty(nbytes, np.uint8)
        _abi.check(_abi.lib().soil_memcpy_d2h(h.ctypes.data, C.c_void_p(addr), nbytes, None))
        return h

    def exchange(self, sends, recvs):
        import numpy as np
        import torch
        dist = self.dist
        keep, ops = [], []
        for addr, n, peer in sends:
            t = torch.from_numpy(np.ascontiguousarray(self._to_host(addr, n)))
            keep.append(t)
            ops.append(dist.P2POp(dist.isend, t, peer))
        landed = []
        for addr, n, peer in recvs:
            t = torch.empty(n, dtype=torch.uint8)
            landed.append((addr, n, t))
            ops.append(dist.P2POp(dist.irecv, t, peer))
        for r in dist.batch_isend_irecv(ops) if ops else ():
            r.wait()
        for addr, n, t in landed:
            if self.device:
                _abi.check(_abi.lib().soil_memcpy_h2d(C.c_void_p(addr), t.numpy().ctypes.data, n, None))
            else:
                self._view(addr, n)[:] = t.numpy()

    def all_reduce(self, addr, n):
        import numpy as np
        import torch
        h = self._to_host(addr, 4 * n).view(np.float32)
        t = torch.from_numpy(np.ascontiguousarray(h).copy())
        self.dist.all_reduce(t)
        if self.device:
            _abi.check(_abi.lib().soil_memcpy_h2d(C.c_void_p(addr), t.numpy().ctypes.data, 4 * n, None))
        else:
            self._view(addr, 4 * n).view(np.float32)[:] = t.numpy()

    def barrier(self):
        self.dist.barrier()

    def max_over_ranks(self, value):
        import torch
        t = torch.tensor([float(value)], dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def close(self):
        if self.dist.is_initialized():
            self.dist.barrier()
            self.dist.destroy_process_group()


def default_comm(device=True):
    """The communicator of a job launched by torch.distributed.run: RCCL in the library; gloo on
    staged buffers when SOIL_DIST_BACKEND=gloo (ranks that share a GPU) or without a device."""
    rank, world = _dist_env()
    backend = os.environ.get("SOIL_DIST_BACKEND") or ("nccl" if device else "gloo")
    if backend == "gloo":
        wire = GlooWire(device)
        return CallbackComm(wire.dist.get_rank(), wire.dist.get_world_size(), wire)
    if world == 1 and os.environ.get("SOIL_RCCL_WORLD1") != "1":
        return SelfComm()
    # RCCL inside the library.  Should its bootstrap fail on any rank (library not found, IPC
    # refused by the host driver, ...) every rank falls back to gloo on staged buffers — slow, and
    # said so loudly in describe() / the bench line — rather than the job dying without a number.
    import sys
    import torch
    comm, err = None, None
    try:
        comm = RcclComm()
    except Exception as e:      # noqa: BLE001
        err = e
    dist = _init_gloo()
    ok = torch.tensor([0 if comm is None else 1])
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok.item()) == 1:
        return comm
    if comm is not None:
        comm.close(keep_group=True)
    print("soillib_amd.parallel: RCCL bootstrap failed on %s (%s): FALLING BACK to gloo on staged "
          "host buffers — the exchange times of this run are not RCCL's" %
          ("this rank" if err is not None else "another rank", err), file=sys.stderr)
    wire = GlooWire(device)
    fallback = CallbackComm(wire.dist.get_rank(), wire.dist.get_world_size(), wire)
    fallback.note = "gloo on staged host buffers — FALLBACK, the RCCL bootstrap failed: %s" % (err,)
    return fallback


# ---- the compute back-end ---------------------------------------------------------------

class CallbackOps:
    """soil_slab_ops whose entries are methods of a Python object (tests/parallel_worker.py: the
    oracle on host memory).  Methods take raw addresses and the ctypes structs of _abi.

    The colour table (soil_slab_colour_ops) is made of the methods colour_particles_fluvial,
    colour_particles_debris, colour_particles_pair, colour_cells and colour_particles_pass (the
    soil_slab_colour_ops entries with that prefix); a back-end without colour_cells has none, and a
    coloured runner refuses it."""

    def __init__(self, backend):
        self.backend = backend
        self.error = None
        self._keep = []
        fields = {}

        def wrap(name, proto, attr=None):
            fn = getattr(backend, attr or name, None)
            if fn is None:
                return proto()          # NULL entry
            if name == "stream":
                cb = proto(lambda ctx, lane: None)
            else:
                def run(ctx, *a, _fn=fn):
                    try:
                        _fn(*a)
                        return 0
                    except BaseException as e:
                        self.error = e
                        return _abi.SOIL_ERR_HIP
                cb = proto(run)
            self._keep.append(cb)
            return cb
        for name, proto in _abi.OPS_FIELDS:
            fields[name] = wrap(name, proto)
        self._ops = _abi.SlabOps(None, *[fields[n] for n, _ in _abi.OPS_FIELDS])
        self._cops = None
        if getattr(backend, "colour_cells", None) is not None:
            cf = {name: wrap(name, proto, "colour_" + name) for name, proto in _abi.COLOUR_OPS_FIELDS}
            self._cops = _abi.SlabColourOps(None, *[cf[n] for n, _ in _abi.COLOUR_OPS_FIELDS])

    def c_ops(self):
        return C.pointer(self._ops)

    def c_colour_ops(self):
        """The colour table, or None when the back-end has no colour entries."""
        return C.pointer(self._cops) if self._cops is not None else None


# ---- the runner -----------------------------------------------------------------------------

class SlabRunner:
    """The sharded erosion model; `step()` advances the global grid by one step
    (soil_slab_step)."""

    def __init__(self, rows_per_rank, W, param, particles_div=8, seed=0, ops=None, scale=None,
                 noise_seed=3.0, init=True, comm=None, noise_rows=None, trim=None, pair=None,
                 halo_need=0, device=None, mode=None, colour=False):
        """comm: SelfComm / RcclComm / CallbackComm (default: default_comm()); ops: CallbackOps or
        None for the HIP back-end on device `device` (default: SOIL_DEVICE or LOCAL_RANK).
        colour: carry the four colour planes (COLOUR_PLANES, zero until set_plane fills them) through
        every step (soil_slab_create_colour); a CallbackOps back-end must then have a colour table."""
        lib = self.lib = _abi.lib()
        self.cb_ops = ops
        if ops is None:
            if device is None:
                device = int(os.environ.get("SOIL_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            _abi.check(lib.soil_set_device(int(device)))
        self.comm = comm if comm is not None else default_comm(device=ops is None)
        self.param = param
        cfg = _abi.SlabConfig()
        cfg.rows_per_rank, cfg.W, cfg.particles_div, cfg.seed = int(rows_per_rank), int(W), int(particles_div), int(seed)
        if scale is not None:
            cfg.scale[0], cfg.scale[1], cfg.scale[2] = [float(v) for v in scale]
        cfg.noise_seed = float(noise_seed)
        cfg.noise_rows = int(noise_rows or 0)
        cfg.init = 1 if init else 0
        cfg.trim = -1 if trim is None else int(bool(trim))
        cfg.pair = -1 if pair is None else int(bool(pair))
        cfg.halo_need = int(halo_need)
        # how a walk that crosses a slab's edge is served (soil_slab.h): "deep" halos or "migrate"; None: the
        # library's default (SOIL_SLAB_MODE in the environment, else deep halos)
        cfg.mode = -1 if mode is None else {"deep": 0, "migrate": 1}[mode]
        self._h = C.c_void_p()
        pref = param._ref() if hasattr(param, "_ref") else C.byref(param)
        self.colour = bool(colour)
        if self.colour:
            self._check(lib.soil_slab_create_colour(C.byref(self._h), C.byref(cfg), pref, self.comm.c_comm(),
                                                    ops.c_ops() if ops is not None else None,
                                                    ops.c_colour_ops() if ops is not None else None))
        else:
            self._check(lib.soil_slab_create(C.byref(self._h), C.byref(cfg), pref, self.comm.c_comm(),
                                             ops.c_ops() if ops is not None else None))
        i = self.info()
        self.rank, self.world = i.rank, i.world
        self.S, self.W, self.H, self.G, self.N = i.S, i.W, i.H, i.G, i.N
        self.x0, self.rows, self.r0, self.r1 = i.x0, i.rows, i.r0, i.r1
        self.trim, self.pair = bool(i.trim), bool(i.pair)
        self.mode = "migrate" if i.mode == 1 else "deep"
        self.scale = list(scale) if scale is not None else [20.0 / self.H, 20.0 / self.W, 4.0]
        self._mark = None

    def _check(self, rc):
        if rc != 0:
            for src in (self.cb_ops, self.comm):
                err = getattr(src, "error", None)
                if err is not None:
                    src.error = None
                    raise err
        _abi.check(rc)

    def info(self):
        i = _abi.SlabInfo()
        _abi.check(self.lib.soil_slab_get_info(self._h, C.byref(i)))
        return i

    def step(self, ev=None):
        """One step of the global grid.  `ev`: an object with record(i) — bench.py's HIP events —
        called at the marks of soil_slab_step on the runner's main stream."""
        if ev is not None:
            if self._mark is None or self._mark[0] is not ev:
                self._mark = (ev, _abi.MARK_FN(lambda ctx, i: ev.record(int(i), self.stream())))
            self._check(self.lib.soil_slab_step(self._h, self._mark[1], None))
        else:
            self._check(self.lib.soil_slab_step(self._h, _abi.MARK_FN(), None))

    def stream(self, lane=0):
        """The runner's main (lane 0) / communication (1) HIP stream as a c_void_p."""
        st = C.c_void_p()
        _abi.check(self.lib.soil_slab_stream(self._h, lane, C.byref(st)))
        return st

    def plane_ptr(self, name):
        p, rows, ch = C.c_void_p(), C.c_int64(), C.c_int64()
        _abi.check(self.lib.soil_slab_plane(self._h, name.encode(), C.byref(p), C.byref(rows), C.byref(ch)))
        return p, int(rows.value), int(ch.value)

    def plane(self, name, owned=False):
        """A plane of the slab as a numpy array (a copy for the HIP back-end, a view of the
        back-end's memory otherwise): local rows incl. ghost rows, or the owned rows only."""
        import numpy as np
        p, rows, ch = self.plane_ptr(name)
        shape = (rows, self.W, ch) if ch > 1 else (rows, self.W)
        n = rows * self.W * ch
        if self.cb_ops is None:
            self.sync()
            a = np.empty(shape, np.float32)
            _abi.check(self.lib.soil_memcpy_d2h(a.ctypes.data, p, 4 * n, None))
        else:
            a = np.ctypeslib.as_array((C.c_float * n).from_address(p.value)).reshape(shape)
        return a[self.r0:self.r1] if owned else a

    def set_plane(self, name, array):
        import numpy as np
        p, rows, ch = self.plane_ptr(name)
        a = np.ascontiguousarray(array, np.float32)
        assert a.size == rows * self.W * ch, (a.shape, rows, self.W, ch)
        if self.cb_ops is None:
            self.sync()  # nothing of the runner's own lanes may still be writing the plane
            _abi.check(self.lib.soil_memcpy_h2d(p, a.ctypes.data, 4 * a.size, None))
            _abi.check(self.lib.soil_device_synchronize())
        else:
            C.memmove(p.value, a.ctypes.data, 4 * a.size)

    @property
    def halo_rows(self):
        i = self.info()
        return {"flux": int(i.rows_flux), "field": int(i.rows_field), "full": int(i.rows_full),
                "window": int(i.rows_window), "window_full": int(i.rows_window_full)}

    @property
    def migration(self):
        i = self.info()
        return {"passes": int(i.passes), "walkers_handed": int(i.walkers_handed)}

    @property
    def fallbacks(self):
        return int(self.info().repeated_launches)

    @property
    def reach_hist(self):
        i = self.info()
        return [int(i.reach_hist[k]) for k in range(i.n_reach)]

    @property
    def step_index(self):
        return int(self.info().step_index)

    # -- bench plumbing ----------------------------------------------------------
    def sync(self):
        self._check(self.lib.soil_slab_sync(self._h))

    def barrier(self):
        self.comm.barrier()

    def max_over_ranks(self, value):
        return self.comm.max_over_ranks(value)

    def close(self):
        if self._h:
            self.lib.soil_slab_destroy(self._h)
            self._h = C.c_void_p()

    def shutdown(self):
        """Free the slab and tear the communicator down."""
        self.close()
        self.comm.close()


# ---- flow accumulation: replicas, realisations sharded ------------------------------

def multiflow(height, source, K, T, edge=1, seed=0, comm=None, rank=None, world=None,
              local_sum=None):
    """Stochastic multiple-flow accumulation (example/dem_multiflow.py:43-49) over all
    ranks.  `accumulate` does not shard — its pointer jumps span the whole grid
     — so every rank holds the full DEM and computes the realisations
    k = rank, rank + world, ... < K; one all-reduce(sum) of the float64 mean plane
    (128 MiB at 4096^2) combines them.

    `height`, `source`: silt.gpu float32 tensors (H, W), the same on every rank.
    Returns a torch float64 tensor (H, W) holding the mean on every rank.
    `local_sum(first, stride) -> torch tensor` replaces the HIP back-end in the
    CPU (gloo) tests."""
    if comm is None:
        import torch.distributed as comm
    if world is None:
        live = comm.is_available() and comm.is_initialized()
        rank, world = (comm.get_rank(), comm.get_world_size()) if live else (0, 1)
    if local_sum is None:
        from . import soil

        def local_sum(first, stride):
            out = soil.multiflow(height, source, K, T, edge, seed, first=first, stride=stride)
            return out.view_torch()
    total = local_sum(rank, world)
    if world > 1:
        comm.all_reduce(total, op=comm.ReduceOp.SUM)
    return total
