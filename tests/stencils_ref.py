"""The constructions the hostile stencil tests share (not a test module): planes whose values, central-difference
quotients and normal lengths sit on either side of the thresholds that pick between the fast and the written-out
form of the stencil kernels (csrc/stencil.hip, csrc/window.hpp: win_row_plain, csrc/soil_math.hpp: QuotWatch), the
scales, z scales and sigmas off and at the ends of the plain range, the list of cases the GPU file compares, and a
few lines of numpy that restate lerp5, the normal map and the laplacian in float32 (numpy's + - * / and sqrt are the
IEEE operations) for the census of tests/test_stencils_hostile.py.  Pure numpy, every plane deterministic from a seed."""
import numpy as np

f32 = np.float32
NAN, INF = f32(np.nan), f32(np.inf)


def p2(e):
    return f32(np.ldexp(1.0, int(e)))


def _below(v):
    return float(np.nextafter(f32(v), f32(0.0)))


def _above(v):
    return float(np.nextafter(f32(v), INF))


# ---- shapes ------------------------------------------------------------------------------------------------------
WINDOW_SHAPES = [(37, 260), (9, 1028), (70, 264), (5, 8), (4, 4), (2, 8), (1, 4)]      # W a multiple of four
SCALAR_SHAPES = [(37, 53), (3, 5), (1, 1)]
SHAPES = WINDOW_SHAPES + SCALAR_SHAPES
CHILD_SHAPES = [(37, 260), (70, 264)]                                                    # what the child processes run
BLUR_SHAPES = [(1, 1), (1, 40), (40, 1), (5, 3), (17, 15), (20, 50), (33, 1030), (40, 515)]

# ---- scales ------------------------------------------------------------------------------------------------------
PLAIN = (0.4, 1.7)
SCALES_OFF_PLAIN = (_below(p2(-40)), float(p2(-41)), _above(p2(40)), float(p2(41)), float(f32(1e-40)), float(f32(3e38)),
                    -1.5, 0.0, -0.0, float("inf"), float("nan"))
SCALES_AT_ENDS = (float(p2(-40)), float(p2(40)))
Z_SCALES = (3.0, -3.0, 0.0, -0.0, float(f32(1e-30)), float(p2(-130)), float(f32(1e30)), float("inf"), float("nan"))
SIGMAS = (1e-3, 0.05, 0.3, 1.0, 2.5, 16.0, 1e4, float("inf"), -2.0)
SIGMAS_DEGENERATE = (0.0, float("nan"))


def name_of(v):
    """A scale as a word of a case's name: the float's hex form tells +0 from -0 and the neighbours of 2^-40."""
    v = float(v)
    return repr(v) if v != v or v in (float("inf"), -float("inf")) or v == 0 else float(v).hex()


def three_ways(s):
    """A scale on x with y plain, on y with x plain, on both."""
    return [("x", (s, PLAIN[1])), ("y", (PLAIN[0], s)), ("both", (s, s))]


def end_pairs():
    """The four combinations of SCALES_AT_ENDS, and the suite's everyday scale."""
    lo, hi = SCALES_AT_ENDS
    return [(lo, lo), (lo, hi), (hi, lo), (hi, hi), PLAIN]


# ---- planes ------------------------------------------------------------------------------------------------------

def exponent_plane(H, W, e, seed):
    """Random signs and mantissas, exponents drawn from {e - 1, e, e + 1}."""
    r = np.random.default_rng(seed)
    exps = (int(e) + 127 + r.integers(-1, 2, (H, W))).astype(np.uint32)
    mant = r.integers(0, 1 << 23, (H, W)).astype(np.uint32)
    sign = r.integers(0, 2, (H, W)).astype(np.uint32)
    return ((sign << np.uint32(31)) | (exps << np.uint32(23)) | mant).view(np.float32)


def sites(H, W):
    """Cells where one value decides for more than its own thread: the first and last lanes of a wave and of a
    work-group (columns 0, 3, 4, 255, 256, 259, 1023, 1024), the first rows, either side of the band boundaries 4, 8,
    16, 32, the last two rows and columns — every such row and every such column carries at least one site."""
    cols = sorted({c for c in (0, 3, 4, 255, 256, 259, 1023, 1024, W - 2, W - 1) if 0 <= c < W})
    rows = sorted({r for r in (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, H - 2, H - 1) if 0 <= r < H})
    out = []
    for i, x in enumerate(rows):
        for j in range(3):
            out.append((x, cols[(3 * i + j) % len(cols)]))
    for j, y in enumerate(cols):
        out.append((rows[(5 * j + 2) % len(rows)], y))
    return sorted(set(out))


THRESHOLD_EXPONENTS = (-55, -54, -53, 47, 48, 49)


def threshold_cells():
    """The six magnitudes around win_row_plain's range 2^-54 .. 2^48 (both ends inside it)."""
    return [p2(-55), f32(_below(p2(-54))), p2(-54), p2(48), f32(_above(p2(48))), p2(49)]


def threshold_planes(H, W):
    """name -> plane: exponent planes around the two ends of the plain range of a loaded value, and a mid-range
    plane carrying single cells on either side of each end at `sites`."""
    out = {"e%+d" % e: exponent_plane(H, W, e, 100 + e) for e in THRESHOLD_EXPONENTS}
    mixed = exponent_plane(H, W, 0, 7)
    mags = threshold_cells()
    for i, (x, y) in enumerate(sites(H, W)):
        mixed[x, y] = mags[i % 6] * f32(-1.0 if (i // 6) % 2 else 1.0)
    out["mixed"] = mixed
    return out


def _clip_e(e):
    return max(-124, min(125, int(e)))          # e - 1 .. e + 1 stay normal numbers


def quotient_planes(H, W, scale):
    """name -> plane whose central differences over `scale` have exponents around QuotWatch's range 2^-60 .. 2^90:
    exponent planes chosen for each of the two cell sizes (a difference of two values of exponent e has exponent e
    give or take two; where 2^90 times the cell size is no float the plane stops at the top of the range), and a
    mid-range plane with isolated such differences: a zero and a value of that exponent either side of a site."""
    out = {}
    for axis, s in enumerate(scale):
        lg = int(np.round(np.log2(float(s))))
        for side, q in (("lo", -60), ("hi", 90)):
            e = _clip_e(q + lg + 1)                 # (the central difference halves)
            out["%s over %s" % (side, "xy"[axis])] = exponent_plane(H, W, e, 300 + 10 * axis + (q > 0))
    iso = exponent_plane(H, W, 0, 11)
    r = np.random.default_rng(12)
    for i, (x, y) in enumerate(sites(H, W)):
        axis = i % 2
        lg = int(np.round(np.log2(float(scale[axis]))))
        q = (-62, 88, -61, 89, -60, 90, -59, 91, -58, 92)[i % 10]
        v = f32(1.0 + r.random()) * p2(_clip_e(q + lg + 1)) * f32(-1.0 if r.random() < 0.5 else 1.0)
        a, b = ((x - 1, y), (x + 1, y)) if axis == 0 else ((x, y - 1), (x, y + 1))
        if 0 <= a[0] and b[0] < H and 0 <= a[1] and b[1] < W:
            iso[a], iso[b] = f32(0.0), v
    out["isolated"] = iso
    return out


def nonfinite_sites(H, W):
    """(x, y, value) of the NaN, +inf and -inf cells of `normal_planes`: each alone in the interior; in adjacent pairs
    along each axis (so that fm1 and fp1 of the cell between, or f0, are non-finite); in each of the two rows and
    columns next to every border; in columns 254 .. 257 (lanes 63 and 0 of two waves); two rows either side of rows 8
    and 16 (band boundaries).  Grids under 64 cells get one NaN in the last cell, under 8 cells nothing."""
    bad = (NAN, INF, -INF)
    if H * W < 8:
        return []
    if H * W < 64:
        return [(H - 1, W - 1, NAN)]
    out = []

    def put(x, y, v, dy=0, column=False):
        """`y` is a column of a grid 230 wide or wider; narrower grids fold it into theirs (`column`: taken as it is)"""
        if not column and W < 230:
            y = 2 + (7 * y) % (W - 6)
        if 0 <= y + dy < W:
            out.append((x % H, y + dy, v))                           # (a short grid folds the rows into its own)
    xm = H // 2
    for k, v in enumerate(bad):
        put(xm + 3, 20 + 12 * k, v)                                  # alone
        put(xm - 3, 22 + 12 * k, v), put(xm - 2, 22 + 12 * k, v)     # a pair along x
        put(xm - 8, 24 + 12 * k, v), put(xm - 8, 24 + 12 * k, v, 1)  # a pair along y
        put(xm + 8, 26 + 12 * k, v), put(xm + 10, 26 + 12 * k, v)    # fm1 and fp1 of the cell between, along x
        put(xm + 6, 60 + 12 * k, v), put(xm + 6, 60 + 12 * k, v, 2)  # ... along y
        for j, x in enumerate((0, 1, H - 2, H - 1)):                 # the rows next to the borders
            put(x, 70 + 30 * k + 7 * j, v)
        for j, y in enumerate((0, 1, W - 2, W - 1)):                 # the columns next to the borders
            put(11 + 6 * k + (j % 2) * 3 if H > 30 else (2 + k + j) % H, y, v, column=True)
        for j, y in enumerate((254, 255, 256, 257)):                 # lanes 63 | 0
            put((20 + 5 * k + (j // 2) * 2) % H, y, v, column=True)
        for j, x in enumerate((6, 7, 8, 9, 14, 15, 16, 17)):         # either side of rows 8 and 16
            put(x, 130 + 30 * k + 3 * j, v)
    put(0, 0, NAN), put(H - 1, W - 1, INF), put(0, W - 1, -INF)       # corners
    return out


def with_nonfinite(plane):
    h = plane.copy()
    for x, y, v in nonfinite_sites(*h.shape):
        h[x, y] = v
    return h


def flat_patches(H, W):
    """(x0, x1, y0, y1, value): patches of 5 x 5 or more, one each of +0, -0 and a nonzero constant, across columns
    255 | 256 (or the next wave boundaries) and a band boundary where the grid reaches them, else wherever the grid
    has room."""
    vals = (f32(0.0), f32(-0.0), f32(0.8125))
    if W >= 260 and H >= 28:                    # rows 8, 16 and 24 inside: a boundary of the bands of 4 and 8, 16 and 32
        return [(5 + 8 * k, 11 + 8 * k, 250 - k, 260 - k, v) for k, v in enumerate(vals)]
    if W > 774 and H >= 8:                      # a short wide grid: one patch on each of three wave boundaries, row 4 inside
        return [(2, 7, 256 * (k + 1) - 5, 256 * (k + 1) + 5, v) for k, v in enumerate(vals)]
    if H >= 28 and W >= 8:
        return [(5 + 8 * k, 11 + 8 * k, max(0, W // 2 - 4), min(W, W // 2 + 4), v) for k, v in enumerate(vals)]
    if H >= 5 and W >= 5:
        return [(0, 5, 0, 5, vals[1])]
    return [(0, H, 0, min(W, 3), vals[1])] if W >= 2 else []


def normal_planes(H, W):
    """name -> plane for soil_normal: `flats` (a mid-range plane with patches of +0, -0 and a constant: a -0
    numerator under a negative z scale), `steep` (exponents around 37: with z = 3 over a cell size of 0.4 the normal's
    length straddles 2^40; the mid-range planes straddle it over a cell size of 2^-40), `nonfinite` (the mid-range
    plane with the cells of `nonfinite_sites`)."""
    base = exponent_plane(H, W, 0, 21)
    flats = base.copy()
    for x0, x1, y0, y1, v in flat_patches(H, W):
        flats[x0:x1, y0:y1] = v
    return {"flats": flats, "steep": exponent_plane(H, W, 37, 22), "nonfinite": with_nonfinite(base)}


def blur_planes(H, W, C):
    """name -> (H, W, C) plane: standard normal draws, and the same with single NaN, +inf and -inf cells at a corner,
    mid-edge, in the interior and within 16 cells of the end of a 1024-float segment (each value in the same
    columns, so that what a bad cell spreads over stays a small share of a wide grid)."""
    r = np.random.default_rng(1000 * H + W + C)
    t = r.standard_normal((H, W, C)).astype(np.float32)
    bad = t.copy()
    if W >= 500:
        seg = 1024 // C
        for k, v in enumerate((NAN, INF, -INF)):
            corner = ((0, 0), (H - 1, 0), (H - 1, W - 1))[k]
            edge = ((H - 1, W // 2), (0, W // 2), (H // 2, 0))[k]
            for x, y in (corner, edge, (H // 2 + 2 * k - 2, W // 4), (3 + 5 * k, seg - 5 if seg < W else W - 5),
                         (4 + 5 * k, seg + 3 if seg + 3 < W else W - 3)):
                bad[x, y, (k + y) % C] = v
    else:
        bad = None
    return {"normal": t, "nonfinite": bad} if bad is not None else {"normal": t}


# ---- numpy restatements (float32, statement for statement) ----------------------------------------------------------

def _shift(h, k, axis):
    """h[i + k] along `axis`, NaN where that is outside the grid."""
    out = np.full(h.shape, NAN, np.float32)
    n = h.shape[axis]
    if abs(k) >= n:
        return out
    src = [slice(None)] * 2
    dst = [slice(None)] * 2
    src[axis] = slice(max(0, k), n + min(0, k))
    dst[axis] = slice(max(0, -k), n - max(0, k))
    out[tuple(dst)] = h[tuple(src)]
    return out


def lerp5(h, axis):
    """(derivative, branch) of lerp5_axis along `axis`: branch 0 the fourth-order formula, 1 central, 2 forward,
    3 backward, 4 the final 0.0."""
    h = np.asarray(h, np.float32)
    fm2, fm1, fp1, fp2 = (_shift(h, k, axis) for k in (-2, -1, 1, 2))
    fin = np.isfinite
    with np.errstate(all="ignore"):
        c = [fin(fm2) & fin(fm1) & fin(fp1) & fin(fp2), fin(fm1) & fin(fp1), fin(fp1) & fin(h), fin(fm1) & fin(h)]
        v = [((fm2 - f32(8) * fm1) + (f32(8) * fp1 - fp2)) / f32(12), f32(0.5) * (fp1 - fm1), fp1 - h, h - fm1]
    branch = np.full(h.shape, 4, np.int8)
    d = np.zeros(h.shape, np.float32)
    for k in (3, 2, 1, 0):
        branch[c[k]] = k
        d[c[k]] = v[k][c[k]]
    return d, branch


def normal(h, scale):
    """soil::op::normal in numpy: (out (H, W, 3), the two numerators d * s.z, the length)."""
    sx, sy, sz = (f32(v) for v in scale)
    with np.errstate(all="ignore"):
        ax, ay = lerp5(h, 0)[0] * sz, lerp5(h, 1)[0] * sz
        vx, vy, vz = -(ax / sx), -(ay / sy), np.ones(ax.shape, np.float32)
        length = np.sqrt(vx * vx + vy * vy + vz * vz)
        inv = f32(1.0) / length
        return np.stack([vx * inv, vy * inv, vz * inv], -1).astype(np.float32), (ax, ay), length


def laplacian(t, scale):
    """__laplacian<D> in numpy (clamp-to-self)."""
    t = np.asarray(t, np.float32)
    H, W = t.shape[:2]
    with np.errstate(all="ignore"):
        hx = f32(1.0) / f32(scale[0]) / f32(scale[0])
        hy = f32(1.0) / f32(scale[1]) / f32(scale[1])
        xs, ys = np.arange(H)[:, None], np.arange(W)[None, :]

        def at(dx, dy):
            nx, ny = xs + dx, ys + dy
            ok = (nx >= 0) & (nx < H) & (ny >= 0) & (ny < W)
            nb = t[np.clip(nx, 0, H - 1), np.clip(ny, 0, W - 1)]
            return np.where(ok[..., None], nb, t)
        half = f32(0.5)
        LH = (at(-1, 0) - t) * hx + (at(1, 0) - t) * hx + (at(0, -1) - t) * hy + (at(0, 1) - t) * hy
        LD = half * (at(-1, -1) - t) * hx + half * (at(1, 1) - t) * hx + half * (at(1, -1) - t) * hy + half * (at(-1, 1) - t) * hy
        return (half * LH + half * LD).astype(np.float32)


def central_quotients(h, scale):
    """The watched quotients of k_gradient4 inside the grid: 0.5 (h[x + 1] - h[x - 1]) / s.x and the same along y."""
    h = np.asarray(h, np.float32)
    with np.errstate(all="ignore"):
        qx = f32(0.5) * (h[2:, 1:-1] - h[:-2, 1:-1]) / f32(scale[0])
        qy = f32(0.5) * (h[1:-1, 2:] - h[1:-1, :-2]) / f32(scale[1])
    return np.concatenate([qx.ravel(), qy.ravel()])


def classes(v, lo, hi):
    """How many of the magnitudes |v| (NaN left out) lie below lo (and are not zero), in [lo, hi], above hi."""
    a = np.abs(np.asarray(v, np.float32).ravel())
    a = a[~np.isnan(a)]
    return int(((a > 0) & (a < lo)).sum()), int(((a >= lo) & (a <= hi)).sum()), int((a > hi).sum())


def informative(out):
    """(NaN share, distinct words, the distinct words wanted) of an oracle output."""
    out = np.ascontiguousarray(out, np.float32)
    cells = out.shape[0] * out.shape[1]
    words = out.view(np.uint32).ravel()
    need = 1000 if cells >= 2000 else (cells + 1) // 2
    return float(np.isnan(out).mean()), int(len(np.unique(words))), need


# ---- the cases the GPU file compares (and the CPU file holds to the informative-output cap) -------------------------
#
# A case is (name, operator, plane, arguments); `select` leaves out the ones whose oracle output says too little.

OPS3 = ("gradient", "negslope", "normal")
Z_PLAIN = 3.0


def mid_plane(H, W):
    return exponent_plane(H, W, 0, 5)


def lap_planes(H, W, D, seed=31):
    """(H, W, D): a different plane in each channel."""
    return np.stack([exponent_plane(H, W, 0, seed + c) for c in range(D)], -1)


def run(api, op, plane, args):
    """One operator of `api` (the oracle module, or the device front-end of the GPU file) on a case."""
    if op == "gradient":
        return api.gradient(plane, args)
    if op == "negslope":
        return api.negslope(plane, args)
    if op == "normal":
        return api.normal(plane, args)
    if op == "laplacian":
        return api.laplacian(plane, args)
    if op == "blur":
        return api.gaussian_blur(plane, args)
    raise ValueError(op)


def off_plain_cases(H, W):
    """Scales off the plain range, three ways each: gradient, negslope and normal (z = 3) on a mid-range plane and
    on the mixed threshold plane; laplacian D = 1 and D = 2 on mid-range planes."""
    planes = {"mid": mid_plane(H, W), "mixed": threshold_planes(H, W)["mixed"]}
    out = []
    for s in SCALES_OFF_PLAIN:
        for way, sc in three_ways(s):
            for op in OPS3:
                for pname, plane in planes.items():
                    args = sc + (Z_PLAIN,) if op == "normal" else sc
                    out.append(("%s, %s, %s = %s" % (op, pname, way, name_of(s)), op, plane, args))
            for D in (1, 2):
                out.append(("laplacian D=%d, %s = %s" % (D, way, name_of(s)), "laplacian", lap_planes(H, W, D), sc))
    return out


def ends_cases(H, W):
    """Scales at the ends of the plain range (the fast form) on values and quotients either side of every threshold.
    (Where the negslope or the normal of a high-exponent plane overflows throughout, `select` leaves the case out;
    the gradient stays on every plane.)"""
    out = []
    for sc in end_pairs():
        planes = dict(threshold_planes(H, W))
        planes.update(quotient_planes(H, W, sc))
        for pname, plane in planes.items():
            for op in OPS3:
                args = sc + (Z_PLAIN,) if op == "normal" else sc
                out.append(("%s, %s, (%s, %s)" % (op, pname, name_of(sc[0]), name_of(sc[1])), op, plane, args))
    return out


def normal_cases(H, W):
    """normal_planes under every z scale, over (0.4, 1.7) and over (2^-40, 2^40); 1e30 goes with the low-exponent
    threshold planes (over anything larger the squares overflow)."""
    out = []
    low = {k: v for k, v in threshold_planes(H, W).items() if k in ("e-55", "e-54", "e-53")}
    for sc in (PLAIN, SCALES_AT_ENDS):
        for z in Z_SCALES:
            planes = low if z == float(f32(1e30)) else normal_planes(H, W)
            for pname, plane in planes.items():
                out.append(("normal, %s, (%s, %s, %s)" % (pname, name_of(sc[0]), name_of(sc[1]), name_of(z)), "normal", plane,
                            tuple(sc) + (z,)))
    return out


def laplacian_cases(H, W, D):
    """The non-finite cell placements of normal_planes in every channel (a different base plane in each, and the
    placements shifted by a column in the second), over the everyday scale and over the ends."""
    t = lap_planes(H, W, D, seed=41)
    for c in range(D):
        for x, y, v in nonfinite_sites(H, W):
            t[x, (y + c) % W, c] = v
    return [("laplacian D=%d, nonfinite, (%s, %s)" % (D, name_of(sc[0]), name_of(sc[1])), "laplacian", t, sc)
            for sc in (PLAIN, (SCALES_AT_ENDS[0], SCALES_AT_ENDS[1]), (2.0, 0.5))]


def blur_cases(H, W, C):
    out = []
    for pname, plane in blur_planes(H, W, C).items():
        for sigma in SIGMAS + SIGMAS_DEGENERATE:
            if pname == "nonfinite" and (sigma in SIGMAS_DEGENERATE or sigma == float("inf")):
                continue                                    # (the closed forms are stated for finite planes)
            out.append(("blur C=%d, %s, sigma %s" % (C, pname, name_of(sigma)), "blur", plane, sigma))
    return out


# ---- closed forms: the degenerate cases that are compared although they break the cap -------------------------------

def closed_form(name, op, plane, args):
    """The whole expected output of a degenerate case, or None when the case is no such case."""
    if op == "blur":
        if args != args or args == 0:
            return np.full(plane.shape, NAN, np.float32)             # 0 / 0 in the centre tap's exponent: NaN weights
        if args == float("inf") and np.isfinite(plane).all():
            return np.zeros(plane.shape, np.float32)                 # weights of +0: fma(x, +0, +0) = +0 for every finite x
    if op == "normal" and args[2] == 0 and plain_pair(args[:2]):
        with np.errstate(all="ignore"):
            out = np.empty(plane.shape + (3,), np.float32)
            out[..., 0] = -((lerp5(plane, 0)[0] * f32(args[2])) / f32(args[0]))    # a zero of the sign the reference's
            out[..., 1] = -((lerp5(plane, 1)[0] * f32(args[2])) / f32(args[1]))    # statements give it
            out[..., 2] = 1.0
        return out if (out[..., :2] == 0).all() else None
    if op == "laplacian" and lap_overflows(args):
        return laplacian(plane, args)
    return None


def plain_pair(sc):
    return all(float(p2(-40)) <= float(s) <= float(p2(40)) for s in sc)


def lap_overflows(sc):
    with np.errstate(all="ignore"):
        return any(np.isinf(f32(1.0) / f32(s) / f32(s)) for s in sc)


def select(oracle, cases):
    """The cases that are compared, each with the oracle's output: those that keep the informative-output cap (at most
    half NaN, at least the distinct words `informative` wants) and the degenerate ones whose whole output has a closed
    form.  Anything else is left out of both files; tests/test_stencils_hostile.py pins what that is."""
    kept, left_out = [], []
    for name, op, plane, args in cases:
        with np.errstate(all="ignore"):
            want = run(oracle, op, plane, args)
        share, distinct, need = informative(want)
        if (share <= 0.5 and distinct >= need) or closed_form(name, op, plane, args) is not None:
            kept.append((name, op, plane, args, want))
        else:
            left_out.append((name, share, distinct, need))
    return kept, left_out
