"""Designed edge inputs of the grid-sample family (cs_gridwarp.hip, cs_inpaintprep.hip, cs_gridsample.h) and their expected outputs,
shared by tests/test_grid_edges_surface.py (which holds the reference side to its conditions) and tests/test_gpu_grid_edges.py
(which compares the kernels with it bit for bit).  Nothing in the package imports it.

Every construction is made of integers and exactly representable float32 values (dyadic fractions, nextafter neighbours), so
every machine builds the same bits.  A builder returns a Case: the inputs, the expected arrays (tools/grid_oracle.py,
tools/inpaint_oracle.py) and a reach record -- counts, each of which must be above zero, of the output pixels that sit on the edge
the case was built for.  A seeded fuzz essentially never lands there: a coordinate of fraction exactly 0.5, a difference exactly
on its threshold, a masked run across a 2048-column chunk of the bit-row scans.
"""
import numpy as np

import grid_oracle as go
import inpaint_oracle as io

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
SIZES = (1, 2, 3, 5, 33, 64, 257)
EXACT_WIDTHS = (2, 3, 5, 33, 257)        # w - 1 a power of two: linspace(-1, 1, w) and a shift of c * w / (w - 1) pixels are exact
OPS = ("warp", "fill", "mask", "stretch")
SPECIALS = (INF, -INF, NAN, F32(-0.0), np.finfo(F32).max, F32(1e-45), F32(-3e-39))


class Case:
    def __init__(self, name, inputs, expected, reach, **params):
        self.name, self.inputs, self.expected, self.reach, self.params = name, inputs, expected, reach, params

    def line(self):
        return f"{self.name}: " + ", ".join(f"{k}={v}" for k, v in self.reach.items())


def up(v):
    return np.nextafter(F32(v), INF)


def down(v):
    return np.nextafter(F32(v), -INF)


def image(c, h, w, salt=0):
    """float32 [c,h,w] of values k / 256, neighbours all different."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([((x * 37 + y * 11 + k * 101 + salt * 13) % 256) for k in range(c)]).astype(F32) / F32(256.0)


def distinct_depth(h, w):
    """float32 [h,w] of values k / 64 whose 8 neighbours all differ from the pixel (a nearest sample one column or row off shows),
    with differences of exactly 0.25 among them."""
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 37 + y * 11) % 64).astype(F32) / F32(64.0)


def with_specials(img, every=7, salt=0):
    """A copy of `img` with every `every`-th element (in flat order, from `salt`) one of SPECIALS in turn."""
    out = np.array(img, dtype=F32)
    flat = out.reshape(-1)
    idx = np.arange(salt % every, flat.size, every)
    flat[idx] = np.array(SPECIALS, dtype=F32)[np.arange(idx.size) % len(SPECIALS)]
    return out


# ---- coordinates ---------------------------------------------------------------------------------------------------------------
def grid_value(c, size):
    """The float32 grid value whose unnormalised coordinate (g + 1) * ((size - 1) / 2) is exactly c, searched among the floats
    around 2 c / (size - 1) - 1; None when there is none."""
    if size == 1:
        return None
    half = F32(size - 1) / F32(2.0)
    g = F32(2.0 * c / (size - 1) - 1.0)
    cand, lo, hi = [g], g, g
    for _ in range(4):
        lo, hi = down(lo), up(hi)
        cand += [lo, hi]
    for v in cand:
        if (v + F32(1.0)) * half == F32(c):
            return F32(v)
    return None


def designed_coordinates(size):
    """The source coordinates of one axis: every integer and half-integer from -3 to size + 3, the padding edges, whole spans of
    the reflection and points many spans away."""
    cs = set(np.arange(-3.0, size + 3.5, 0.5).tolist())
    cs |= {-1.0, -0.5, size - 0.5, float(size), 2.0 * (size - 1), -2.0 * (size - 1), 4.0 * (size - 1) + 0.5, 1e6, -1e6,
           6.0 * (size - 1), 1e6 + 0.5}
    return sorted(cs)


def axis_values(size):
    """(grid values, the coordinates they reproduce exactly) of one axis; an axis of size 1 takes any grid value to 0."""
    if size == 1:
        g = np.array([-1.0, 0.0, 1.0, 0.5, 1e6, -3.0], dtype=F32)
        return g, np.zeros_like(g)
    pairs = [(grid_value(c, size), c) for c in designed_coordinates(size)]
    pairs = [(g, c) for g, c in pairs if g is not None]
    return np.array([p[0] for p in pairs], dtype=F32), np.array([p[1] for p in pairs], dtype=F32)


def coordinate_table(h, w, shape=None):
    """gx, gy [1,Ho,Wo] over the designed coordinates of a w x h image and the reach record.  shape None: the full cross product;
    (Ho, Wo): the two lists cycled against each other over that many points."""
    xs, cx = axis_values(w)
    ys, cy = axis_values(h)
    if shape is None:
        ix, iy = np.meshgrid(np.arange(xs.size), np.arange(ys.size))
    else:
        i = np.arange(shape[0] * shape[1]).reshape(shape)
        ix, iy = i % xs.size, (i // xs.size + i) % ys.size
    gx, gy, x, y = xs[ix][None], ys[iy][None], cx[ix], cy[iy]
    half = lambda v: int((v - np.floor(v) == 0.5).sum())   # noqa: E731
    reach = dict(x_values=int(xs.size), y_values=int(ys.size))
    if w > 1:
        reach.update(x_half=half(x), x_integer=int((x == np.floor(x)).sum()), x_outside=int(((x < 0) | (x > w - 1)).sum()),
                     x_on_pad_edge=int(((x == -1) | (x == w)).sum()))
    if h > 1:
        reach.update(y_half=half(y), y_outside=int(((y < 0) | (y > h - 1)).sum()))
    return gx.astype(F32), gy.astype(F32), reach


def nonfinite_grid(gx, gy):
    """Copies of a grid with NaN, inf and -inf in x, in y and in both, every 5th point."""
    gx, gy = gx.copy(), gy.copy()
    fx, fy = gx.reshape(-1), gy.reshape(-1)
    vals = np.array([NAN, INF, -INF], dtype=F32)
    i = np.arange(0, fx.size, 5)
    fx[i[0::3]] = vals[np.arange(i[0::3].size) % 3]
    fy[i[1::3]] = vals[np.arange(i[1::3].size) % 3]
    fx[i[2::3]] = vals[np.arange(i[2::3].size) % 3]
    fy[i[2::3]] = vals[(np.arange(i[2::3].size) + 1) % 3]
    return gx, gy


SAMPLER_SHAPES = ((1, 1), (1, 2), (3, 1), (2, 3), (3, 5), (5, 2), (33, 64), (64, 33), (5, 257), (257, 3))


# ---- detect_disocclusions_gpu on a caller's grid ---------------------------------------------------------------------------
DETECT_SHAPES = ((1, 2), (2, 3), (3, 5), (5, 2), (33, 64), (64, 33), (7, 257), (257, 2))
DETECT_THRESHOLD = 0.25


def detect_case(h, w, nonfinite=False):
    """depth, grid, grid_x_warped of detect_disocclusions_gpu: a depth whose neighbours all differ (by multiples of 1 / 64, some
    exactly the threshold 0.25 above the pixel), sampled at the designed coordinates, and a grid_x_warped whose horizontal steps are
    the step threshold 3 * 2 / w itself and the floats either side of it."""
    depth = distinct_depth(h, w)
    gx, gy, reach = coordinate_table(h, w, (h, w))
    step = F32(2.0 / w * 3.0)
    v = np.array([step, up(step), down(step), F32(0.0)], dtype=F32)
    y, x = np.mgrid[0:h, 0:w]
    gxw = np.where(x % 2 == 1, v[(x // 2 + y) % 4], F32(0.0)).astype(F32)
    if nonfinite:
        gx, gy = nonfinite_grid(gx, gy)
        depth = with_specials(depth, every=11, salt=3)
        gxw = with_specials(gxw, every=13, salt=5)
        reach = dict(grid_nan=int(np.isnan(gx).sum() + np.isnan(gy).sum()), grid_inf=int(np.isinf(gx).sum() + np.isinf(gy).sum()))
    grid = np.stack([gx[0], gy[0]], -1)[None].astype(F32)
    with np.errstate(invalid="ignore"):
        wd = go.sample_nearest(depth[None, None], gx, gy, "border")[0, 0]
        grad = np.abs(gxw[:, 1:] - gxw[:, :-1])
        reach.update(depth_step_on_threshold=int((wd - depth == F32(DETECT_THRESHOLD)).sum()), grid_step_on_threshold=int((grad == step).sum()),
                     grid_step_above=int((grad == up(step)).sum()))
        want = go.detect_disocclusions_gpu(depth, grid, gxw, DETECT_THRESHOLD)
    if h * w < 16 or nonfinite:   # (too few points for every edge: the larger shapes carry the counts)
        reach = {k: v for k, v in reach.items() if v > 0}
    return Case(f"detect {h}x{w}" + (" non-finite" if nonfinite else ""), dict(depth=depth, grid=grid, gxw=gxw), dict(mask=want), reach,
                threshold=DETECT_THRESHOLD)


# ---- the four k_gridwarp operations -------------------------------------------------------------------------------------------
def run_ops(img, depth, args, fill_modes=("border",)):
    """The expected outputs of the four operations on image [B,C,H,W], depth [B,H,W]: keys warp, stretch, stretch_mask, mask and
    fill:<mode> / valid:<mode> (the fill operation on every frame by itself, stacked)."""
    with np.errstate(all="ignore"):
        out = dict(warp=go.apply_stereo_divergence_gpu(img, depth, *args), mask=go.compute_forward_mask_gpu(depth, *args))
        out["stretch"], out["stretch_mask"] = go.warp_and_fill_gpu(img, depth, *args)
        for mode in fill_modes:
            fr = [go.apply_stereo_divergence_gpu_with_fill(img[k], depth[k], *args, fill_mode=mode) for k in range(img.shape[0])]
            out["fill:" + mode] = np.stack([f[0] for f in fr])
            out["valid:" + mode] = np.stack([f[1] for f in fr])
    return out


SHIFT_SHAPES = ((1, 1), (3, 1), (1, 2), (2, 3), (3, 5), (5, 33), (64, 33), (2, 257), (7, 257))
FILL_MODES = ("border", "zeros", "reflection", "other")


def shifts(w):
    """The uniform shifts, in source columns, of a width: integers and half-integers around 0 and w, whole reflection spans."""
    s = {0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 2.5, -2.0, w - 1.0, w - 0.5, float(w), w + 0.5, -float(w), 2.0 * (w - 1), -2.0 * (w - 1),
         4.0 * (w - 1) + 0.5, 1e6, -1e6}
    return sorted(s)


def shift_case(h, w, c, specials=False, forward=False):
    """A flat depth (no range: every offset is the separation) and a separation of c * w / (w - 1) pixels: every source x is the
    column minus c exactly, so the bilinear x taps sit on weights 0, 1 and 0.5, the forward destinations col + offset on integers
    and the source x on -1 and 1 away from column 0.  forward: the separation is c pixels itself, so that the forward destinations
    col + offset are integers, -1 and w (outside by the strict comparisons) among them."""
    img = image(3, h, w, salt=int(c * 2) % 7)[None]
    if specials:
        img = with_specials(img, every=5, salt=int(c * 2) % 5)
    depth = np.full((1, h, w), 0.5, dtype=F32)
    sep = F32(c) if forward else F32(c) * F32(w) / F32(max(w - 1, 1))
    assert forward or w == 1 or float(sep) * (w - 1) == c * w, (w, c)
    args = (0.0, float(sep), 1.0, 0.0)
    want = run_ops(img, depth, args, FILL_MODES)
    with np.errstate(all="ignore"):
        gx = go.grid_x(go.pixel_offset(depth, *args))
        x = go.source_coord(gx, w, "zeros")
        dest = np.arange(w, dtype=F32) + go.pixel_offset(depth, *args)
    if forward:
        reach = dict(dest_integer=int((dest == np.floor(dest)).sum()), dest_on_edge=int(((dest == -1) | (dest == w)).sum()))
        return Case(f"offset {h}x{w} by {c:g}", dict(image=img, depth=depth), want, reach, args=args)
    reach = dict(exact=int((x == np.arange(w, dtype=F32) - F32(c)).all()) if w > 1 else 1)
    if w > 1 and c != np.floor(c):
        reach["x_half"] = int((x - np.floor(x) == 0.5).sum())
    if w > 1 and c == np.floor(c):
        reach["x_integer"] = int((x == np.floor(x)).sum())
    if w > 2 and 0 < abs(c) <= w - 1 and c == np.floor(c):
        reach["grid_on_one_away_from_its_column"] = int((np.abs(gx) == 1).sum())
    if specials:
        o = want["fill:zeros"]
        reach.update(out_nan=int(np.isnan(o).sum()), out_finite=int(np.isfinite(o).sum()))
        if h * w < 8:
            reach = {k: v for k, v in reach.items() if v > 0}
    return Case(f"shift {h}x{w} by {c:g}" + (" specials" if specials else ""), dict(image=img, depth=depth), want, reach, args=args)


def levels(h, w, n):
    """int [h,w] of levels 0 .. n-1 in runs of one to six columns, the rows different."""
    y, x = np.mgrid[0:h, 0:w]
    return ((x + 3 * y) // 3 + (x * 7) // 11 + (x // 17) * (y + 1)) % n


TIE_DIVERGENCES = {"sample ties": 257.0 / 256.0, "integer destinations": 2.0, "steps of 1.5": 3.0, "steps above 1.5": float(up(3.0)),
                   "steps below 1.5": float(down(3.0))}


def tie_case(kind, h=5, w=257):
    """Two or three depth levels (0, 0.5, 1) with exponent 1 and convergence 0.5: offsets of +- divergence / 2.  257 / 256 makes
    every source x a half column (bilinear weights 0.5 between different colours), 2 lands every col + offset on an integer, 3 makes
    adjacent offsets differ by exactly 1.5 and by 3; its float neighbours by the floats either side of 1.5."""
    n = 2 if kind in ("sample ties", "integer destinations") else 3
    depth = (levels(h, w, n).astype(F32) / F32(n - 1))[None]
    img = image(3, h, w)[None]
    args = (TIE_DIVERGENCES[kind], 0.0, 1.0, 0.5)
    want = run_ops(img, depth, args)
    po = go.pixel_offset(depth, *args)
    x = go.source_coord(go.grid_x(po), w, "zeros")
    dpo = np.abs(po[..., 1:] - po[..., :-1])
    dest = np.arange(w, dtype=F32) + po
    reach = {"sample ties": dict(x_half=int((x - np.floor(x) == 0.5).sum())),
             "integer destinations": dict(dest_integer=int((dest == np.floor(dest)).sum()), dest_on_edge=int(((dest == -1) | (dest == w)).sum())),
             "steps of 1.5": dict(step_on_threshold=int((dpo == 1.5).sum()), step_of_3=int((dpo == 3.0).sum())),
             "steps above 1.5": dict(step_just_above=int((dpo == up(1.5)).sum())),
             "steps below 1.5": dict(step_just_below=int((dpo == down(1.5)).sum()))}[kind]
    reach["gaps"] = int(want["mask"].sum())
    return Case(f"gridwarp {kind}", dict(image=img, depth=depth), want, reach, args=args)


# ---- inpaint_prepare ---------------------------------------------------------------------------------------------------------------
def prepare_expected(img, depth, sf, thr):
    with np.errstate(all="ignore"):
        wr, fl, m = io.prepare(img, depth, sf, thr)
    return dict(warped=wr, filled=fl, mask=m, warped_u8=io.codes(wr), filled_u8=io.codes(fl))


PREPARE_TIE_SF = 100.0 / 256.0   # divergence_px = w / 256: at w = 257 the levels 0 and 1 sample half a column to either side


def prepare_tie_case(kind, h=5, w=257):
    """inpaint_prepare on level depths at a divergence of 257 / 256 pixels: every nearest sample of the depth is a tie between two
    columns (half to even decides), every bilinear tap pair has weights 0.5.  "two": levels 0 and 1 at the reference's threshold;
    "three": levels 0, 0.5 and 1 with the threshold 0.5, so that warped depth minus depth is exactly the threshold."""
    n, thr = (2, 0.05) if kind == "two" else (3, 0.5)
    depth = (levels(h, w, n).astype(F32) / F32(n - 1))[None]
    img = image(3, h, w)[None]
    want = prepare_expected(img, depth, PREPARE_TIE_SF, thr)
    d = io.depth_chain(depth[0])
    gxw = (go.linspace(w) - (d * F32(-(PREPARE_TIE_SF / 100.0) * w)) / F32(w / 2)).astype(F32)[None]
    x = go.source_coord(gxw, w, "zeros")[0]
    gy = np.broadcast_to(go.linspace(h)[None, :, None], (1, h, w))
    d2 = d + F32(0.5)
    wd = go.sample_nearest(d2[None, None], gxw, gy, "border")[0, 0]
    ties = x - np.floor(x) == 0.5
    lo, hi = np.clip(np.floor(x), 0, w - 1).astype(int), np.clip(np.floor(x) + 1, 0, w - 1).astype(int)
    rows = np.arange(h)[:, None]
    reach = dict(nearest_ties=int(ties.sum()), ties_between_levels=int((ties & (d2[rows, lo] != d2[rows, hi])).sum()),
                 masked=int(want["mask"].sum()), unmasked=int((~want["mask"]).sum()))
    if kind == "three":
        reach["difference_on_threshold"] = int((wd - d2 == F32(thr)).sum())
    return Case(f"prepare ties, {kind} levels", dict(image=img, depth=depth), want, reach, sf=PREPARE_TIE_SF, thr=thr)


# ---- normalisation edges ------------------------------------------------------------------------------------------------------------
NORM_FRAMES = {
    "max 1": (1.0 - 2.0 ** -19, 1.0),   # (a range of 1.9e-6: above 1e-6 as it stands, far below it once divided by 255)
    "max above 1": (0.25, float(up(1.0))), "max 255": (0.0, 255.0),
    "range 1e-6": (0.0, float(F32(1e-6))), "range above 1e-6": (0.0, float(up(1e-6))), "range below 1e-6": (0.0, float(down(1e-6))),
    "range 0": (0.5, 0.5),
}
NORM_BATCHES = {"one frame above 1": ("max 1", "max 255", "range above 1e-6"), "ranges": ("range 1e-6", "range above 1e-6", "range below 1e-6", "range 0")}


def norm_depth(name, h=3, w=33):
    lo, hi = NORM_FRAMES[name]
    lv = levels(h, w, 3)
    mid = F32((lo + hi) / 2) if name.startswith("max") else F32(lo)
    return np.where(lv == 0, F32(lo), np.where(lv == 1, mid, F32(hi))).astype(F32)


def norm_case(name):
    """One frame, or a batch, whose maximum sits on `> 1` (1, the float above it, 255) or whose range sits on `> 1e-6`.  The
    k_gridwarp chain divides the whole batch by 255 when any frame is above 1, the inpaint chain each frame on its own."""
    frames = NORM_BATCHES.get(name, (name,))
    depth = np.stack([norm_depth(f) for f in frames])
    b, h, w = depth.shape
    img = np.stack([image(3, h, w, salt=k) for k in range(b)])
    args = (6.0, 0.5, 2.0, 0.5)
    want = run_ops(img, depth, args)
    want.update({"prepare/" + k: v for k, v in prepare_expected(img, depth, 12.0, 0.05).items()})
    mx = depth.reshape(b, -1).max(1)
    batch255 = bool((mx > 1).any())
    d = depth / F32(255.0) if batch255 else depth
    rng = d.reshape(b, -1).max(1) - d.reshape(b, -1).min(1)
    own = np.array([(f / F32(255.0) if f.max() > 1 else f).max() - (f / F32(255.0) if f.max() > 1 else f).min() for f in depth])
    reach = dict(frames=b)
    if "max" in name or "above 1" in name:
        reach[{True: "frames_divided", False: "frames_not_divided"}[batch255]] = b
    if name == "one frame above 1":
        reach["frames_the_inpaint_chain_leaves"] = int((mx <= 1).sum())
    if "range" in name or name == "ranges":
        reach["ranges_on_threshold"] = int((rng == F32(1e-6)).sum() + (own == F32(1e-6)).sum() + (rng == up(1e-6)).sum() + (rng == down(1e-6)).sum() + (rng == 0).sum())
    return Case(f"normalisation: {name}", dict(image=img, depth=depth), want, reach, args=args, sf=12.0, thr=0.05)


# ---- bit-row layouts -----------------------------------------------------------------------------------------------------------------
BITROW_WIDTHS = (4097, 6200)


def layouts(w):
    """(name, unmasked bool [w]) of the designed rows: nothing unmasked, one unmasked pixel, and masked runs."""
    out = [("all masked", np.zeros(w, dtype=bool))]
    for c in (0, 31, 32, 2047, 2048, 4095, 4096, w - 1):
        u = np.zeros(w, dtype=bool)
        u[c] = True
        out.append((f"only {c}", u))
    for a, b in ((2040, 2100), (1, w - 1), (0, 33), (w - 33, w)):
        u = np.ones(w, dtype=bool)
        u[a:b] = False
        out.append((f"run {a}..{b}", u))
    return out


def layout_reach(mask):
    """Counts over the rows of a mask [.., w]: rows with nothing unmasked, rows with one unmasked pixel, rows whose masked run
    covers more than a word on both sides of a multiple of 2048 (the 64-word chunks of the bit-row scans carry a value there)."""
    m = mask.reshape(-1, mask.shape[-1])
    w = m.shape[-1]
    crossing = 0
    for k in range(2048, w - 33, 2048):
        crossing += int(m[:, k - 33:k + 33].all(1).sum())
    return dict(rows_all_masked=int(m.all(1).sum()), rows_one_unmasked=int(((~m).sum(1) == 1).sum()), rows_crossing_a_chunk=crossing)


def interp_case(w):
    """interpolate_fill_gpu on the designed rows: 13 layouts in three frames of five rows (the two rows left over repeat)."""
    rows = [~u for _, u in layouts(w)]
    rows += rows[9:11]
    mask = np.stack(rows).reshape(3, 5, w)
    img = np.stack([image(2, 5, w, salt=k) for k in range(3)])
    want = dict(filled=go.interpolate_fill_gpu(img, mask))
    return Case(f"interpolate_fill {w}", dict(image=img, mask=mask), want, layout_reach(mask))


STRETCH_DIV = 16384.0


def stretch_bitrow_case(w, first):
    """warp_and_fill_gpu / compute_forward_mask_gpu whose gap mask is four designed layouts (from `first`) of one frame of five rows,
    induced through depth: with exponent 1, convergence 0, divergence 16384 and separation -w a depth of (t + w - x) / 16384 sends
    source column x exactly onto column t.  Unmasked columns keep their place, every other source column lands on the row's first
    unmasked column, or on -1 (outside by the strict comparison) in a row with none.  Row 0 holds the frame's 0 and 1."""
    lay = layouts(w)[first:first + 4]
    depth = np.zeros((1, 5, w), dtype=F32)
    x = np.arange(w)
    depth[0, 0] = (x + w - x).astype(F32) / F32(STRETCH_DIV)
    depth[0, 0, 0], depth[0, 0, 1] = 0.0, 1.0
    for r, (_, u) in enumerate(lay, start=1):
        t = np.where(u, x, np.flatnonzero(u)[0] if u.any() else -1)
        depth[0, r] = (t + w - x).astype(F32) / F32(STRETCH_DIV)
    img = image(1, 5, w)[None]
    args = (STRETCH_DIV, -float(w), 1.0, 0.0)
    want = run_ops(img, depth, args)
    po = go.pixel_offset(depth, *args)
    dest = np.arange(w, dtype=F32) + po
    reach = layout_reach(want["mask"][0, 1:])
    reach = {k: v for k, v in reach.items() if v > 0}
    reach.update(rows=len(lay), dest_exact=int((dest == np.floor(dest)).all()), dest_on_minus_one=int((dest == -1).sum()))
    if not reach["dest_on_minus_one"]:
        del reach["dest_on_minus_one"]
    return Case(f"stretch layouts {w} from {first}", dict(image=img, depth=depth), want, reach, args=args, names=[n for n, _ in lay])


PREPARE_LAYOUT_SF, PREPARE_LAYOUT_THR = 1000.0, 2.0


def prepare_bitrow_case(w, first):
    """inpaint_prepare whose mask is four designed layouts, one per frame of five equal rows: depth 0.5 (no offset: the source x
    stays inside [-1, 1]) on the unmasked columns and their neighbours, 0 and 1 in turn (ten widths away at this divergence)
    everywhere else; the threshold 2 keeps the disocclusion test out of it."""
    lay = layouts(w)[first:first + 4]
    x = np.arange(w)
    frames = []
    for _, u in lay:
        mid = u.copy()
        mid[1:] |= u[:-1]
        mid[:-1] |= u[1:]
        row = np.where(mid, F32(0.5), (x % 2).astype(F32))
        if mid.all() or not (row == 0).any() or not (row == 1).any():
            raise AssertionError("layout without both outer levels")
        frames.append(np.broadcast_to(row, (5, w)))
    depth = np.stack(frames).astype(F32)
    img = np.stack([image(3, 5, w, salt=k) for k in range(len(lay))])
    want = prepare_expected(img, depth, PREPARE_LAYOUT_SF, PREPARE_LAYOUT_THR)
    induced = sum(int(np.array_equal(want["mask"][k], np.broadcast_to(~u, (5, w)))) for k, (_, u) in enumerate(lay))
    reach = {k: v for k, v in layout_reach(want["mask"]).items() if v > 0}
    reach["layouts_induced"] = induced   # (a single unmasked pixel one column inside the right edge cannot be induced: the edge column joins it)
    return Case(f"prepare layouts {w} from {first}", dict(image=img, depth=depth), want, reach, sf=PREPARE_LAYOUT_SF, thr=PREPARE_LAYOUT_THR)


DILATION_HEIGHTS = (1, 2, 3, 5, 7)


def dilation_case(h, w=70):
    """inpaint_prepare on a far frame with single near pixels: the background samples the column to its left, so the pixel right
    of a near one, and only it, is a disocclusion; the two dilations make it a 5 x 5 block.  The near pixels sit so that the blocks
    cross the word boundaries 31 | 32 and 63 | 64 and the frame's top and bottom rows.  Four frames, two near pixels each."""
    cols = (30, 31, 32, 33, 62, 63, 64, 65)
    rows = [r for r in (0, 1, 2, h - 3, h - 2, h - 1) if 0 <= r < h]
    depth = np.zeros((4, h, w), dtype=F32)
    for k, c in enumerate(cols):
        depth[k % 4, rows[(k * 5 + k // 4) % len(rows)], c - 1] = 1.0
    img = np.stack([image(3, h, w, salt=k) for k in range(4)])
    sf = 200.0 / w * 1.0   # divergence_px = 2: the background's source x is (w - 1) / w columns to the left
    want = prepare_expected(img, depth, sf, 0.05)
    m = want["mask"]
    reach = dict(blocks_across_31_32=int((m[..., 31] & m[..., 32]).sum()), blocks_across_63_64=int((m[..., 63] & m[..., 64]).sum()),
                 top_row=int(m[:, 0, 28:68].sum()), bottom_row=int(m[:, h - 1, 28:68].sum()), unmasked=int((~m).sum()))
    return Case(f"prepare dilation h={h}", dict(image=img, depth=depth), want, reach, sf=sf, thr=0.05)


# ---- non-finite depth ----------------------------------------------------------------------------------------------------------------
NONFINITE_DEPTHS = ("nan", "inf", "-inf", "both inf", "all nan", "nan above 1", "inf and nan")


def nonfinite_depth(kind, h=3, w=33):
    d = (levels(h, w, 3).astype(F32) / F32(2.0)) * F32(0.75) + F32(0.125)
    if kind == "all nan":
        return np.full((h, w), NAN, dtype=F32)
    if kind == "nan above 1":
        d = d * F32(200.0)
    put = {"nan": (NAN,), "inf": (INF,), "-inf": (-INF,), "both inf": (INF, -INF), "nan above 1": (NAN,), "inf and nan": (INF, NAN)}[kind]
    for k, v in enumerate(put):
        d[(1 + k) % h, 5 + 9 * k] = v
    return d.astype(F32)


def nonfinite_depth_case(kinds):
    """A batch of frames with NaN / infinite depth values beside a clean frame.  A NaN makes the frame's min and max NaN: the frame
    is flat (every offset that of depth 0) and takes no part in the batch's `> 1`; an infinite value makes the range infinite:
    finite depths normalise to 0 (or NaN under -inf), the infinite one to NaN, and a NaN source x samples column 0."""
    depth = np.stack([nonfinite_depth(k) for k in kinds] + [levels(3, 33, 3).astype(F32) / F32(2.0)])
    b, h, w = depth.shape
    img = np.stack([image(3, h, w, salt=k) for k in range(b)])
    args = (6.0, 0.5, 2.0, 0.5)
    want = run_ops(img, depth, args)
    want.update({"prepare/" + k: v for k, v in prepare_expected(img, depth, 12.0, 0.05).items()})
    reach = dict(depth_nan=int(np.isnan(depth).sum()), depth_inf=int(np.isinf(depth).sum()), out_finite=int(np.isfinite(want["warp"]).sum()))
    reach = {k: v for k, v in reach.items() if v > 0 or k == "out_finite"}
    return Case("non-finite depth: " + ", ".join(kinds), dict(image=img, depth=depth), want, reach, args=args, sf=12.0, thr=0.05)


NONFINITE_BATCHES = (("nan", "inf", "-inf"), ("both inf", "all nan", "nan above 1"), ("inf and nan",))


# ---- every case ---------------------------------------------------------------------------------------------------------------------
def gridwarp_cases():
    """The cases of the four k_gridwarp operations (inputs image [B,C,H,W], depth [B,H,W]; params args)."""
    for h, w in SHIFT_SHAPES:
        for c in (shifts(w) if w > 1 else (0.0, 1.0)):
            if w in EXACT_WIDTHS or w == 1:
                yield shift_case(h, w, c)
    for h, w, c in ((3, 5, 1.0), (3, 5, 0.5), (2, 257, 2.5), (2, 257, -1.0), (5, 33, 0.0), (3, 1, 0.0), (1, 2, 0.5)):
        yield shift_case(h, w, c, specials=True)
    for h, w, c in ((1, 2, 1.0), (2, 3, -1.0), (3, 5, 1.0), (5, 33, -1.0), (5, 64, 1.0), (5, 64, -64.0), (2, 257, 257.0), (2, 257, -1.0), (3, 1, 1.0)):
        yield shift_case(h, w, c, forward=True)
    for kind in TIE_DIVERGENCES:
        yield tie_case(kind)


def prepare_cases():
    for kind in ("two", "three"):
        yield prepare_tie_case(kind)
    for h in DILATION_HEIGHTS:
        yield dilation_case(h)
    for w in BITROW_WIDTHS:
        for first in (0, 4, 8, 9):
            yield prepare_bitrow_case(w, first)


def both_chain_cases():
    """Cases that run the four operations and inpaint_prepare (expected keys prepare/...)."""
    for name in list(NORM_FRAMES) + list(NORM_BATCHES):
        yield norm_case(name)
    for kinds in NONFINITE_BATCHES:
        yield nonfinite_depth_case(kinds)
