"""The depth blur (cs_blur.hip) over its parameter range -- box width, mask radius, vertical smoothing and falloff away from the
20 / 20 / 2.0 / 6 every neighbouring test uses -- and over the plan branches those parameters select, on the non-node path
(engine.directional_blur against oracle.blur) and the node path (engine.generate against node_oracle.generate).  Every comparison is
bit for bit on float32 patterns; only gpu_warp's colours keep the 2e-6 of test_gpu_warp_reads_the_tile_map.  -m gpu.

The branch each case is meant to take is written next to it together with the rule of blur_plan / blur_fast_ok / blur_fused_lds
that sends it there, and asserted through cs_test_blur_plan -- the library's own plan for the call, not a restatement:
    two-pass   radius = int(mask width) < 1, or blur_fused_lds(vert, radius, bs) > 64 KB, or the forced switch
    per tile   fused, but w % 4 != 0 or the worklist does not fit behind the bit rows
    fast       worklist, k_blur_fused<true>: 1 <= radius <= 31, at most 32 float4 chunks per tile row (bs <= 64), 16-byte aligned
    slow       worklist, k_blur_fused<false>: any of those three missed (vert never decides: (32 + 2 vert) * 2 <= 256 holds up to
               vert 48, and by blur_fused_lds no call with vert >= 36 is fused at all)
"""
import numpy as np
import pytest
import torch

import synth
from oracle import node_oracle, oracle

pytestmark = pytest.mark.gpu

FUSED, LISTED, LAZY, PRE_EDGES, FAST, REFUSED = 1, 2, 4, 8, 16, 32   # cs_test_blur_plan's bits
TILEMAP, NODE, RGB, ALIGNED = 1, 2, 4, 8                             # ... and its flags


@pytest.fixture(scope="module")
def engine():
    from comfystereo_amd import engine as e
    assert torch.cuda.is_available()
    return e


def plan_bits(strength, mask_width, falloff, vert, n, h, w, flags=ALIGNED):
    from comfystereo_amd import _native
    return _native.lib().cs_test_blur_plan(float(strength), float(strength if mask_width is None else mask_width), int(vert),
                                           float(falloff), n, h, w, flags)


def fall_mode(bits):
    return (bits >> 8) & 7


def same(got, want, what, nan_ok=False):
    """The same float32 patterns.  nan_ok: where the oracle has a NaN the kernel has one too, of any sign and payload (the default NaN
    of 0 / 0 and of 0 * inf has the sign bit set on x86 and clear on the GPU; IEEE 754 leaves it open); elsewhere, the same bits."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    nan = np.isnan(want)
    assert nan_ok or not nan.any(), what
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the non-node path
# ---------------------------------------------------------------------------------------------------------------------------
# (n, h, w), depth kind: what the SHAPE decides (test_gpu_blur_plan.py names the rules)
FRAMES = {
    "listed": ((1, 40, 128), "blobs"),      # two tile rows of two tiles, the worklist fits -> k_blur_copy + worklist
    "per_tile": ((1, 40, 130), "stepped"),  # w % 4 != 0 -> k_blur_edges (scalar), one workgroup per tile
    "wide": ((1, 70, 1284), "stepped"),     # more than 1024 columns, 21 tile columns, the last one 4 columns wide -> listed
    "tiny": ((1, 5, 8), "blobs"),           # smaller than a tile: the worklist does not fit -> one workgroup per tile
    "batch": ((2, 33, 192), "blobs"),       # two frames, the second tile row one image row high -> listed
}
SHAPE_LISTED = {"listed": True, "per_tile": False, "wide": True, "tiny": False, "batch": True}

# (strength, mask width or None = the strength, falloff, vert): branch on the frames the shape lets be listed, and why.
# bs = round-half-even(strength), radius = int(mask width).  Every strength, mask width, vert and falloff of the issue's table is
# in some row, and every row runs on every frame.
ROWS = [
    ((0.6, 0.5, 1.0, 0), "two-pass"),    # bs 1; radius 0 < 1.  falloff 1.0: x
    ((1, 1, 0.5, 1), "fast"),            # bs 1, radius 1: the smallest of both.  falloff 0.5: sqrt
    ((1.5, 32, 2.0, 6), "slow"),         # bs 2 (half to even, up); radius 32 > 31 alone.  falloff 2.0: x * x
    ((2.5, 64, 3.0, 15), "slow"),        # bs 2 (half to even, down); radius 64: three words per bit-row window.  falloff 3.0
    ((3.5, 130, 0.0, 0), "slow"),        # bs 4 (up, even box); radius 130 beyond most frames' width.  falloff 0: ones, every tile listed
    ((7.5, 5, 0.1, 1), "fast"),          # bs 8 (up) / radius 5.  falloff 0.1: powf
    ((20.6, 33.7, 0.7, 6), "slow"),      # bs 21 (odd box); radius 33 > 31.  powf
    ((63.4, 31.9, 1.3, 15), "fast"),     # bs 63: 32 chunks; radius int(31.9) = 31; LDS 51.5 KB.  powf
    ((64, 31, 2.9, 0), "fast"),          # bs 64: (32 + 64 + 31 + 3) >> 2 = 32 chunks, the last box that passes; radius 31, the last too
    ((66, 300, 4.0, 1), "slow"),         # bs 66: 33 chunks, and radius 300: 11 words per window, beyond every frame's width
    ((66, 31, 2.0, 6), "slow"),          # bs 66 alone: pad4 36, (36 + 64 + 32 + 3) >> 2 = 33 > 32
    ((100, 20, 1.0, 6), "slow"),         # bs 100: 42 chunks -- the vector loader's second round (qb = 32)
    ((200, 5, 0.5, 0), "slow"),          # bs 200, wider than most frames; fused: 34.3 KB depth tile + 16 KB weights
    ((200, None, 2.0, 15), "two-pass"),  # bs 200 / radius 200 / vert 15: 34.3 + 31.7 KB > 64 KB; k_blur_apply's LDS 65 408 bytes
    ((5, None, 2.0, 35), "fast"),        # vert 35: 512 * 102 + 9 216 + 3 264 + 636 = 65 340 <= 65 536, the last vert that is fused
    ((5, None, 2.0, 36), "two-pass"),    # vert 36: 66 428 > 65 536
    ((20.6, None, 2.0, 47), "two-pass"),  # vert 47, 48, 49 around (32 + 2 vert) * 2 <= 256: never reached fused, two-pass by LDS
    ((7.5, 31, 1.0, 48), "two-pass"),
    ((2.5, 5, 0.7, 49), "two-pass"),
    ((64, 33.7, 3.0, 100), "two-pass"),  # vert 100, taller than every frame: k_blur_apply's LDS 118 784 + 16 256 of 163 840 bytes
]
FALL_MODE = {1.0: 0, 0.5: 1, 2.0: 2, 3.0: 3, 0.0: 5}   # everything else: 4, csm::powf_exact


def codes(kind, n, h, w):
    """`kind` of tools/synth.py rounded to 0..255 codes, [n, h, w] (one seed / centre per frame)"""
    return np.round(synth.depth_batch(kind, n, h, w, channels=1)[..., 0] * 255).astype(np.float32)


def blur_gpu(engine, depth, prm):
    s, mw, f, v = prm
    return [t.cpu().numpy() for t in engine.directional_blur(depth, s, 20, f, v, blur_mask_width=mw)]


def blur_want(depth, prm):
    s, mw, f, v = prm
    return oracle.blur(depth, s, 20, f, v, mask_width=mw)


@pytest.mark.parametrize("fname", list(FRAMES))
@pytest.mark.parametrize("prm,branch", ROWS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else v)
def test_parameter_rows_equal_the_oracle(engine, fname, prm, branch):
    (n, h, w), kind = FRAMES[fname]
    bits = plan_bits(*prm, n, h, w)
    assert bits >= 0 and not bits & REFUSED
    assert bool(bits & FUSED) == (branch != "two-pass"), "fused / two-pass"
    assert bool(bits & LISTED) == (branch != "two-pass" and SHAPE_LISTED[fname]), "worklist / one workgroup per tile"
    assert bool(bits & FAST) == (branch == "fast" and SHAPE_LISTED[fname]), "k_blur_fused<true> / <false>"
    assert fall_mode(bits) == FALL_MODE.get(prm[2], 4)
    depth = codes(kind, n, h, w)
    got = blur_gpu(engine, cuda(depth), prm)
    # (mask radius 0: the weight of an edge pixel is clamp(1 - 0 / 0) = NaN in the reference, :1168)
    for g, o, eye in zip(got, blur_want(depth, prm), "LR"):
        same(g, o, (fname, prm, eye), nan_ok=prm[1] is not None and prm[1] < 1)


def test_listed_slow_by_alignment_alone(engine):
    """(7.5, 5, 0.1, 1) is `fast` on (40, 128); 4 bytes off the 16-byte grid the same call runs k_blur_fused<false>"""
    prm, (n, h, w) = (7.5, 5, 0.1, 1), (1, 40, 128)
    assert plan_bits(*prm, n, h, w, ALIGNED) & FAST and not plan_bits(*prm, n, h, w, 0) & FAST
    assert plan_bits(*prm, n, h, w, 0) & LISTED
    frame = codes("blobs", n, h, w)
    store = torch.zeros(h * w + 8, dtype=torch.float32, device="cuda")
    depth = store[1:1 + h * w].view(n, h, w)
    depth.copy_(torch.from_numpy(frame))
    assert depth.data_ptr() % 16 == 4 and depth.is_contiguous()
    for g, o, eye in zip(blur_gpu(engine, depth, prm), blur_want(frame, prm), "LR"):
        same(g, o, eye)


@pytest.mark.parametrize("strength", [0.4, 0.5])
def test_a_box_of_no_columns_is_refused(engine, strength):
    """round(0.4) = round-half-even(0.5) = 0: torch raises on the zero-width kernel (:1236); CS_EINVAL before any launch"""
    from comfystereo_amd import _native
    assert plan_bits(strength, None, 1.0, 0, 1, 40, 128) == _native.CS_EINVAL
    with pytest.raises(_native.NativeError) as err:
        engine.directional_blur(cuda(codes("blobs", 1, 40, 128)), strength, 20, 1.0, 0)
    assert err.value.code == _native.CS_EINVAL


@pytest.mark.parametrize("strength", [0.0, -3.0])
def test_no_strength_returns_the_input_twice(engine, strength):
    depth = codes("blobs", 2, 33, 192)
    for g in blur_gpu(engine, cuda(depth), (strength, None, 2.0, 6)):
        same(g, depth, strength)


# widths: one column (the bit rows do not fit either), three tile columns with w % 4 != 0, 300 (k_blur_weights: 512 threads),
# 1284 and 2052 (1024 threads, two and three columns per thread)
@pytest.mark.parametrize("w", [1, 130, 300, 1284, 2052])
def test_two_pass_forced_and_by_radius_zero(engine, dev_switch, w):
    """k_blur_weights + k_blur_apply at widths where the row's threads loop, forced by the switch (same bits as the fused form of the
    same call, where the shape has one) and chosen by mask width 0.5 -> radius 0"""
    n, h = 1, 37
    prm, prm0 = (20, None, 2.0, 6), (20, 0.5, 2.0, 6)
    depth = codes("blobs", n, h, w)
    dev = cuda(depth)
    assert bool(plan_bits(*prm, n, h, w) & FUSED) == (w != 1)   # (one column, 37 rows: the bit rows outgrow the scratch)
    fused = blur_gpu(engine, dev, prm)
    assert not plan_bits(*prm0, n, h, w) & (FUSED | REFUSED)
    zero = blur_gpu(engine, dev, prm0)
    dev_switch("blur_two_pass", 1)
    assert not plan_bits(*prm, n, h, w) & (FUSED | REFUSED)
    forced = blur_gpu(engine, dev, prm)
    want, want0 = blur_want(depth, prm), blur_want(depth, prm0)
    for k, eye in enumerate("LR"):
        same(forced[k], want[k], (w, eye, "forced"))
        same(fused[k], want[k], (w, eye, "fused"))
        same(zero[k], want0[k], (w, eye, "radius 0"), nan_ok=True)


# strength 200 / vert 15 is two-pass at any width; k_blur_weights keeps 16 w + 704 bytes of LDS, of 163 840 (CS_LDS_BYTES)
@pytest.mark.parametrize("h,w", [(8, 3840), (8, 4056), (3, 10196)])
def test_two_pass_wide_rows(engine, h, w):
    """a 4K row (62 144 bytes), the first width beyond 64 KB (65 600) and the last one that fits (163 840 exactly)"""
    prm = (200, None, 2.0, 15)
    assert not plan_bits(*prm, 1, h, w) & (FUSED | REFUSED)
    depth = codes("stepped", 1, h, w)
    for g, o, eye in zip(blur_gpu(engine, cuda(depth), prm), blur_want(depth, prm), "LR"):
        same(g, o, (w, eye))


def test_two_pass_refuses_rows_beyond_its_lds(engine):
    """16 * 10200 + 704 > 163 840: CS_ELIMIT from the host, before any launch"""
    from comfystereo_amd import _native
    prm = (200, None, 2.0, 15)
    assert plan_bits(*prm, 1, 3, 10200) & REFUSED and not plan_bits(*prm, 1, 3, 10200) & FUSED
    with pytest.raises(_native.NativeError) as err:
        engine.directional_blur(torch.zeros(1, 3, 10200, device="cuda"), 200, 20, 2.0, 15)
    assert err.value.code == _native.CS_ELIMIT


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the node path: RGB depth at the frames' size, so that k_gray_edges makes the edge bit rows
# ---------------------------------------------------------------------------------------------------------------------------
UI = {"none": "No fill", "polylines_soft": "Fill - Polylines Soft", "hybrid_edge": "Imperfect fill - Hybrid Edge",
      "gpu_warp": "GPU Warp (Fast)"}
WARP = (6.0, 0.0, "left-right", 0.1, 0.5, 2.0)   # divergence, separation, mode, balance, convergence, exponent: the neighbours'

# (strength = mask width, edge threshold, falloff, vert): lazy = k_gray_edges + k_blur_classify + tile map
NODE_ROWS = [
    ((7.5, 6, 1.0, 0), "fast"),        # bs 8 / radius 7, no vertical reach
    ((20.6, 20, 1.3, 6), "fast"),      # bs 21 / radius 20, powf
    ((64, 20, 2.0, 15), "slow"),       # radius 64 > 31: the classification's reach is three words wide, its last compact form
    ((66, 20, 3.0, 15), "slow"),       # radius 66: four words -> the classification's plain walk; bs 66: 33 chunks
    ((120, 20, 2.0, 15), "slow"),      # 24 064 + 31 744 + 4 960 + 1 096 = 61 864 <= 65 536: still fused
    ((150, 20, 2.0, 15), "two-pass"),  # 28 160 + 31 744 + 5 952 + 1 216 = 67 072 > 65 536, under a caller with a tile map
    ((200, 10, 0.5, 15), "two-pass"),  # the widgets' maximum
    ((1, 20, 2.0, 0), "fast"),         # bs 1 / radius 1: the box is the pixel
    ((2.5, 0.5, 4.0, 3), "fast"),      # bs 2 / radius 2, threshold 0.5: edges nearly everywhere
]
NODE_IDS = ["-".join(map(str, p)) for p, _ in NODE_ROWS]
NODE_FRAMES = [((2, 72, 1284), "blobs"), ((1, 40, 256), "stepped")]


def node_plan(prm, branch, n, h, w):
    """the plan of cs_generate's blur for these parameters, checked against the row's branch -> lazy"""
    s, _, f, v = prm
    bits = plan_bits(s, None, f, v, n, h, w, TILEMAP | NODE | RGB | ALIGNED)
    assert bits >= 0 and not bits & REFUSED
    two_pass = branch == "two-pass"
    assert bool(bits & FUSED) == (not two_pass)
    assert bool(bits & LAZY) == bool(bits & PRE_EDGES) == bool(bits & LISTED) == (not two_pass)
    assert bool(bits & FAST) == (branch == "fast")
    return not two_pass


def node_gpu(engine, img, depth, fill, prm, **kw):
    s, thr, f, v = prm
    out = engine.generate(cuda(img), cuda(depth), *WARP, fill, thr, s, True, depth_blur_falloff=f, depth_blur_vert_smooth=v, **kw)
    return [o.cpu().numpy() for o in out]


_NODE_WANT = {}


def node_want(fi, fill, prm):
    """node_oracle.generate for NODE_FRAMES[fi], once per fill and parameters"""
    key = (fi, fill, prm)
    if key not in _NODE_WANT:
        s, thr, f, v = prm
        img, depth = node_inputs(fi)
        _NODE_WANT[key] = node_oracle.generate(img, depth, *WARP, UI[fill], thr, s, True, depth_blur_falloff=f, depth_blur_vert_smooth=v)
        for a in _NODE_WANT[key]:
            a.setflags(write=False)
    return _NODE_WANT[key]


_NODE_IN = {}


def node_inputs(fi):
    if fi not in _NODE_IN:
        (n, h, w), kind = NODE_FRAMES[fi]
        _NODE_IN[fi] = (synth.image_f32(n, h, w, seed=31 + fi), synth.depth_batch(kind, n, h, w, channels=3))
    return _NODE_IN[fi]


@pytest.mark.parametrize("fi", [0, 1])
@pytest.mark.parametrize("prm,branch", NODE_ROWS, ids=NODE_IDS)
def test_node_polylines_soft_lazy_equals_full_copy_and_oracle(engine, dev_switch, fi, prm, branch):
    n, h, w = NODE_FRAMES[fi][0]
    node_plan(prm, branch, n, h, w)
    img, depth = node_inputs(fi)
    lazy = node_gpu(engine, img, depth, "polylines_soft", prm)
    dev_switch("blur_full_copy", 1)
    assert not plan_bits(prm[0], None, prm[2], prm[3], n, h, w, NODE | RGB | ALIGNED) & (LAZY | PRE_EDGES)   # (no tile map: never lazy)
    full = node_gpu(engine, img, depth, "polylines_soft", prm)
    want = node_want(fi, "polylines_soft", prm)
    for k in range(4):
        same(lazy[k], full[k], (prm, k, "lazy / full copy"))
        same(lazy[k], want[k], (prm, k))


@pytest.mark.parametrize("fi", [0, 1])
@pytest.mark.parametrize("fill", ["none", "hybrid_edge", "gpu_warp"])
@pytest.mark.parametrize("prm,branch", NODE_ROWS, ids=NODE_IDS)
def test_node_other_readers_of_the_tile_map(engine, fill, fi, prm, branch):
    """cs_fwdtile.hip (none), the hybrid splat (complete maps through k_blur_copy_tiles where its fused form does not take the call)
    and gpu_warp on the same parameters"""
    n, h, w = NODE_FRAMES[fi][0]
    node_plan(prm, branch, n, h, w)
    img, depth = node_inputs(fi)
    got = node_gpu(engine, img, depth, fill, prm)
    want = node_want(fi, fill, prm)
    for k in (1, 2, 3):
        same(got[k], want[k], (fill, prm, k))
    if fill == "gpu_warp":
        assert np.abs(got[0] - want[0]).max() <= 2e-6
    else:
        same(got[0], want[0], (fill, prm, 0))


@pytest.mark.parametrize("fill", ["polylines_soft", "gpu_warp"])
@pytest.mark.parametrize("prm", [(150, 20, 2.0, 15), (200, 10, 0.5, 15)], ids=["150", "200"])
def test_node_two_pass_writes_complete_maps(engine, fill, prm):
    """The caller asked for a tile map and the plan is two-pass: no tile may be left to a reader.  Workspace and outputs start as
    0xff bytes (NaN patterns): a tile of the blurred maps that nobody wrote would reach the outputs as NaN."""
    n, h, w = NODE_FRAMES[0][0]
    assert not node_plan(prm, "two-pass", n, h, w)
    img, depth = node_inputs(0)
    s, thr, f, v = prm
    p = engine.make_params(n, h, w, h, w, 3, fill, WARP[2], WARP[0], WARP[1], WARP[3], WARP[4], WARP[5], True, s, thr, f, v, 4)
    plan = engine.Plan(p, torch.device("cuda"))
    for t in (plan.ws, plan.stereo, plan.depth_l, plan.depth_r, plan.mask):
        t.view(torch.uint8).fill_(0xff)
    got = [o.cpu().numpy() for o in plan.run(cuda(img), cuda(depth))]
    want = node_want(0, fill, prm)
    for k in (1, 2, 3):
        assert not np.isnan(got[k]).any(), k
        same(got[k], want[k], (fill, prm, k))
    assert not np.isnan(got[0]).any()
    if fill == "gpu_warp":
        assert np.abs(got[0] - want[0]).max() <= 2e-6
    else:
        same(got[0], want[0], (fill, prm, 0))


def test_node_unit_range_frame_beside_a_0_255_frame(engine, dev_switch):
    """(66, 20, 3.0, 15): the x255 plane of the bit rows and the summaries' scale under a reach of 66 columns and 15 rows"""
    prm, (n, h, w) = (66, 20, 3.0, 15), NODE_FRAMES[0][0]
    assert node_plan(prm, "slow", n, h, w)
    img = node_inputs(0)[0]
    depth = node_inputs(0)[1].copy()
    depth[1] *= 255.0
    s, thr, f, v = prm
    lazy = node_gpu(engine, img, depth, "polylines_soft", prm)
    dev_switch("blur_full_copy", 1)
    full = node_gpu(engine, img, depth, "polylines_soft", prm)
    want = node_oracle.generate(img, depth, *WARP, UI["polylines_soft"], thr, s, True, depth_blur_falloff=f, depth_blur_vert_smooth=v)
    for k in range(4):
        same(lazy[k], full[k], (k, "lazy / full copy"))
        same(lazy[k], want[k], k)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. designed inputs for the reach of the lazy classification
# ---------------------------------------------------------------------------------------------------------------------------
DH, DW, BASE = 96, 384, 100   # three tile rows of six tiles


def textured(h=DH, w=DW):
    """BASE + 0 .. 4 codes: Sobel-x stays below 4 * 4 = 16 (no edge at threshold 20, decision value 100), but the box blur of a tile
    differs from the tile -- on a flat depth a tile blended with a small weight and a copied one have the same bits"""
    y, x = np.mgrid[0:h, 0:w]
    return (BASE + (x * 7 + y * 3) % 5).astype(np.float32)


def step_frame(c, rows=None, step=26):
    """+`step` codes from column `c` on (in `rows` only, or everywhere); flat within two columns of the step, so that Sobel-x at the
    step is exactly 4 * step where the step runs through all three rows: 104 > 100 for 26 codes, 100 for 25"""
    d = textured()
    d[:, max(c - 2, 0):c + 2] = BASE
    r = slice(None) if rows is None else slice(*rows)
    d[r, c:] += step
    return d


def designed_frames(radius, vert):
    """Edge columns at a tile boundary and `radius` columns left and right of one, each one column early, on the spot and one late;
    edge rows ending / starting `vert` rows above / below a tile-row boundary, likewise.  A weight at distance `radius` is 0 and one
    at `radius - 1` is not; a row `vert` away is inside the vertical box and one at `vert + 1` is not."""
    frames = []
    for s in sorted({0, radius, -radius}):
        for d in (-1, 0, 1):
            frames.append(step_frame(192 + s + d))
    for d in (-1, 0, 1):
        last = 64 - vert - 1 + d    # the last edge row: tile row 2 (rows 64 ..) has it in reach iff 64 - last <= vert
        frames.append(step_frame(96, rows=(last - 4, last + 2)))
        first = 31 + vert + 1 + d   # the first edge row: tile row 0 (rows .. 31) has it in reach iff first - 31 <= vert
        frames.append(step_frame(288, rows=(first - 1, first + 5)))
    return np.stack(frames)


@pytest.mark.parametrize("radius,bs,vert", [(1, 1, 0), (7, 8, 0), (20, 21, 6), (31, 31, 15), (32, 32, 15), (64, 64, 15)])
def test_lazy_reach_on_designed_edges(engine, dev_switch, radius, bs, vert):
    """One step edge per frame, placed so that a neighbouring tile is just inside, at, and just outside the reach of the blur: the
    oracle says which tiles are blended, lazy (k_blur_classify's reach) must equal the full copy and the oracle."""
    strength = {1: 1.0, 7: 7.5, 20: 20.6, 31: 31.0, 32: 32.0, 64: 64.0}[radius]   # bs = round(strength), radius = int(strength)
    codes_ = designed_frames(radius, vert)
    n = len(codes_)
    assert plan_bits(strength, None, 2.0, vert, n, DH, DW, TILEMAP | NODE | RGB | ALIGNED) & LAZY
    # the designed property, on the oracle's blur of the codes: the set of tiles the blur changes moves with the placement
    # (a box of one column is the pixel itself: blended and copied tiles have the same bits, the case only runs the reach of 1)
    tiles = []
    for k in range(n if bs > 1 else 0):
        L, R = oracle.blur(codes_[k], strength, 20, 2.0, vert)
        changed = (L != codes_[k]) | (R != codes_[k])
        tiles.append(changed.reshape(DH // 32, 32, DW // 64, 64).any(axis=(1, 3)))
        assert tiles[-1].any() and not tiles[-1].all()
    assert bs == 1 or any(not np.array_equal(tiles[k], tiles[k + 2]) for k in range(0, len(tiles) - 2))
    img = synth.image_f32(n, DH, DW, seed=41)
    depth = np.repeat(codes_[..., None], 3, axis=3)
    prm = (strength, 20, 2.0, vert)
    lazy = node_gpu(engine, img, depth, "polylines_soft", prm)
    dev_switch("blur_full_copy", 1)
    full = node_gpu(engine, img, depth, "polylines_soft", prm)
    s, thr, f, v = prm
    want = node_oracle.generate(img, depth, *WARP, UI["polylines_soft"], thr, s, True, depth_blur_falloff=f, depth_blur_vert_smooth=v)
    for k in range(4):
        same(lazy[k], full[k], (radius, k, "lazy / full copy"))
        same(lazy[k], want[k], (radius, k))


@pytest.mark.parametrize("c", [63, 64, 65])
def test_a_sobel_of_exactly_the_decision_value_is_no_edge(engine, c):
    """Integer codes, flat: a step of 25 codes gives Sobel-x 100 and 100 / 200 = 0.5 is not > 0.5 -- away from the frame's borders
    (edges themselves, by the zero padding) the blur returns its input; 26 codes give 104 and an edge.  Single-channel depth on the
    node path (the gray conversion of RGB rounds the codes)."""
    h, w = 40, 128
    flat25, flat26 = np.full((h, w), BASE, np.float32), np.full((h, w), BASE, np.float32)
    flat25[:, c:] += 25
    flat26[:, c:] += 26
    prm = (20, None, 2.0, 6)
    want = blur_want(flat25, prm)
    for g, o, eye in zip(blur_gpu(engine, cuda(flat25), prm), want, "LR"):
        assert np.array_equal(o[:, 32:96], flat25[:, 32:96])   # (the borders' reach ends at columns 20 and 107)
        same(g, o, (c, eye, 25))
    want = blur_want(flat26, prm)
    assert (want[0][:, 32:96] != flat26[:, 32:96]).any()
    for g, o, eye in zip(blur_gpu(engine, cuda(flat26), prm), want, "LR"):
        same(g, o, (c, eye))
    depth = np.stack([flat25, flat26])[..., None]
    img = synth.image_f32(2, h, w, seed=43)
    nprm = (20, 20, 2.0, 6)
    got = node_gpu(engine, img, depth, "polylines_soft", nprm)
    want = node_oracle.generate(img, depth, *WARP, UI["polylines_soft"], 20, 20, True, depth_blur_falloff=2.0, depth_blur_vert_smooth=6)
    for k in range(4):
        same(got[k], want[k], (c, k))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. one non-finite sample in a tile without an edge in reach
# ---------------------------------------------------------------------------------------------------------------------------
# (sample, its column, mask width): the tile of the sample is (1, 2), columns 128 .. 191
@pytest.mark.parametrize("bad,col,mw", [(np.inf, 160, None), (np.inf, 185, 5), (np.nan, 160, None)], ids=["inf", "inf-box-crosses", "nan"])
def test_non_finite_sample_in_an_edge_free_tile(engine, bad, col, mw):
    """The reference blends w * blur + (1 - w) * depth everywhere (:1243): where w == 0 and the box holds the sample, 0 * inf or
    0 * NaN makes the output NaN over the box's columns.  The kernels copy a tile that no edge reaches (deviation D2), so
    there the sample stays in its pixel:
      inf, box inside its tile     its neighbours are edges (|Sobel| = inf), the tile is blended: the oracle's bits everywhere
      inf, box crossing into the next tile (mask width 5 < half the box)   that tile has no edge in reach and stays finite
      NaN                          no comparison with a NaN is true, so there is no edge: the tile is copied, one NaN instead of 20
    Pinned in the listed form and with one workgroup per tile: the oracle's values in the tiles an edge reaches, the input elsewhere."""
    prm = (20, mw, 2.0, 6)
    radius = int(prm[1] or prm[0])
    for w in (320, 322):   # listed / one workgroup per tile (w % 4 != 0)
        depth = np.full((1, 96, w), BASE, np.float32)
        depth[0, :, 40:] += 60.0    # edge pixels at columns 39 and 40 of every row: tile column 0 is blended, 64 - 20 > 40
        depth[0, 48, col] = bad
        assert bool(plan_bits(*prm, 1, 96, w) & LISTED) == (w == 320)
        want = blur_want(depth, prm)
        blended = np.zeros((96, w), bool)
        blended[:, :64] = True
        blended[:, 256:] = True     # the frame's last column is an edge (zero padding): its reach stays right of column 256
        if np.isinf(bad):           # edge pixels at columns col - 1 and col + 1, rows 47 .. 49: within tile (1, 2) with their reach
            assert 128 <= col - 1 - radius and col + 1 + radius <= 191
            blended[32:64, 128:192] = True
        pinned = [np.where(blended, o[0], depth[0])[None] for o in want]
        departs = sum(int((np.isnan(o) != np.isnan(q)).sum()) for o, q in zip(want, pinned))
        assert (departs > 0) == (mw is not None or np.isnan(bad)), departs   # (the first case has nothing to depart in)
        for g, q, eye in zip(blur_gpu(engine, cuda(depth), prm), pinned, "LR"):
            same(g, q, (w, eye), nan_ok=True)
