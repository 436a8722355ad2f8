"""The reference side of the grid-sample edge sweep (tools/grid_edge_inputs.py), held to its conditions on the CPU so that
tests/test_gpu_grid_edges.py cannot pass vacuously:
  - the restated grid_sample (tools/grid_oracle.py) equals CPU torch's bit for bit on every designed coordinate, on images with
    infinite, NaN and subnormal pixels, and on grids with NaN and infinite values;
  - every builder reaches the edge it was built for (the reach counts, printed one line per builder, are all above zero);
  - the restatement equals the reference's own CPU outputs on NaN / infinite depth (tests/golden/grid_edges_nonfinite.npz);
  - the designed cases tell right from wrong: a restatement that rounds half away from zero, that takes a threshold as `>=`, or
    that takes the nearest valid column for the right border, gives other outputs on them."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grid_edge_inputs as ge
import grid_oracle as go

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits_differ(a, b):
    """The number of elements of two float32 arrays whose bits differ, every NaN counting as the same value."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(((a.view(np.int32) != b.view(np.int32)) & ~(np.isnan(a) & np.isnan(b))).sum())


def torch_sample(img, gx, gy, mode, padding):
    grid = torch.from_numpy(np.stack([gx, gy], -1))
    return F.grid_sample(torch.from_numpy(img), grid, mode=mode, padding_mode=padding, align_corners=True).numpy()


def check_samplers(img, gx, gy, where):
    with np.errstate(all="ignore"):
        for padding in go.PADDINGS:
            assert bits_differ(go.sample_bilinear(img, gx, gy, padding), torch_sample(img, gx, gy, "bilinear", padding)) == 0, (where, padding)
            assert bits_differ(go.sample_nearest(img, gx, gy, padding), torch_sample(img, gx, gy, "nearest", padding)) == 0, (where, padding, "nearest")


@pytest.mark.parametrize("h,w", ge.SAMPLER_SHAPES)
def test_restated_grid_sample_equals_cpu_torch_on_the_designed_coordinates(h, w):
    gx, gy, reach = ge.coordinate_table(h, w)
    print(f"coordinates {h}x{w}:", reach)
    assert all(v > 0 for v in reach.values()) or h * w < 4, reach
    img = np.stack([ge.image(2, h, w), ge.distinct_depth(h, w)[None].repeat(2, 0)])[:, :2]
    check_samplers(np.ascontiguousarray(img[:1]), gx, gy, (h, w))
    # pixels of inf, -inf, NaN, -0, the largest float and subnormals: under a weight of exactly 0 (integer coordinates), of
    # exactly 1, and between finite neighbours
    sp = ge.with_specials(img[:1], every=3 if h * w < 16 else 7)
    check_samplers(sp, gx, gy, (h, w, "specials"))
    # NaN and infinite grid values (border and reflection: the sample of column / row 0; zeros: NaN)
    nx, ny = ge.nonfinite_grid(gx, gy)
    assert np.isnan(nx).any() and (np.isinf(nx).any() or nx.size < 10)
    check_samplers(np.ascontiguousarray(img[:1]), nx, ny, (h, w, "non-finite grid"))
    check_samplers(sp, nx, ny, (h, w, "specials, non-finite grid"))


def test_fma32_is_a_fused_multiply_add_on_infinite_and_nan_operands():
    inf, nan, big = F32(np.inf), F32(np.nan), np.finfo(F32).max
    rows = [(inf, 0.5, 1.0, inf), (-inf, 0.5, 1.0, -inf), (inf, 0.0, 1.0, nan), (1.0, 1.0, inf, inf), (inf, 1.0, -inf, nan),
            (big, 2.0, 0.0, inf), (big, 1.0, big, inf), (nan, 0.0, 0.0, nan), (big, 0.5, 0.0, big * F32(0.5)), (-big, 2.0, big, -big)]
    a, b, c, want = (np.array(v, dtype=F32) for v in zip(*rows))
    assert bits_differ(go.fma32(a, b, c), want) == 0
    t = torch.addcmul(torch.from_numpy(c).double(), torch.from_numpy(a).double(), torch.from_numpy(b).double()).float().numpy()
    assert bits_differ(want, t) == 0   # (none of these rows rounds twice: the float64 evaluation is the fused one)


def all_cases():
    yield from (ge.detect_case(h, w, nf) for h, w in ge.DETECT_SHAPES for nf in (False, True))
    yield from ge.gridwarp_cases()
    yield from (ge.stretch_bitrow_case(w, first) for w in ge.BITROW_WIDTHS for first in (0, 4, 8, 9))
    yield from (ge.interp_case(w) for w in ge.BITROW_WIDTHS)
    yield from ge.prepare_cases()
    yield from ge.both_chain_cases()


def test_every_builder_reaches_its_edge():
    n = 0
    for c in all_cases():
        print(c.line())
        assert c.reach and all(v > 0 for v in c.reach.values()), c.line()
        n += 1
    assert n > 150


def test_nonfinite_depth_equals_the_reference_fixture():
    z = np.load(os.path.join(GOLDEN, "grid_edges_nonfinite.npz"))
    for k, kinds in enumerate(ge.NONFINITE_BATCHES):
        c = ge.nonfinite_depth_case(kinds)
        for key in ("warp", "stretch", "stretch_mask", "mask", "fill:border", "valid:border"):
            want, got = c.expected[key], z[f"b{k}/{key}"]
            if want.dtype == bool:
                assert np.array_equal(np.unpackbits(got, count=want.size).reshape(want.shape).astype(bool), want), (kinds, key)
            else:
                assert bits_differ(got, want) == 0, (kinds, key)
        # a frame with a NaN is flat: every offset is that of depth 0, whatever its other values
        depth = c.inputs["depth"]
        po = go.pixel_offset(depth, *c.params["args"])
        for f in range(depth.shape[0]):
            if np.isnan(depth[f]).any():
                assert (po[f] == po[f].flat[0]).all() and np.isfinite(po[f]).all(), (kinds, f)


# ---- the designed cases tell right from wrong -----------------------------------------------------------------------------------
@contextlib.contextmanager
def mutated(**names):
    old = {k: getattr(go, k) for k in names}
    try:
        for k, v in names.items():
            setattr(go, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(go, k, v)


def half_away(v):
    with np.errstate(invalid="ignore"):
        return (np.sign(v) * np.floor(np.abs(v) + F32(0.5))).astype(F32)


def at_or_above(threshold):
    """`>=` in place of `>` for the comparisons against `threshold`, every other one as it is."""
    def cmp(a, b):
        return np.where(np.asarray(b, dtype=F32) == F32(threshold), np.greater_equal(a, b), np.greater(a, b))
    return cmp


def nearest_borders(valid):
    """borders() with the right border the NEAREST valid column at or after c (the reference takes the row's last)."""
    w = valid.shape[-1]
    cols = np.arange(w, dtype=np.int64)
    left = np.maximum.accumulate(np.where(valid, cols, -1), axis=-1)
    right = np.minimum.accumulate(np.where(valid, cols, w)[..., ::-1], axis=-1)[..., ::-1]
    return left, np.where(right < w, right, -1)


def differing(build, keys, **mutation):
    right = build()
    with mutated(**mutation):
        wrong = build()
    n = 0
    for k in keys:
        a, b = right.expected[k], wrong.expected[k]
        n += int((a != b).sum()) if a.dtype != F32 else bits_differ(a, b)
    return n


MUTATIONS = [
    ("half away in the nearest sample of inpaint_prepare", lambda: ge.prepare_tie_case("two"), ("mask",), dict(rint=half_away)),
    ("half away in detect_disocclusions", lambda: ge.detect_case(33, 64), ("mask",), dict(rint=half_away)),
    (">= 1.5 in the gap dilation", lambda: ge.tie_case("steps of 1.5"), ("mask", "stretch_mask"), dict(above=at_or_above(1.5))),
    (">= threshold in detect_disocclusions", lambda: ge.detect_case(33, 64), ("mask",), dict(above=at_or_above(ge.DETECT_THRESHOLD))),
    (">= step threshold in detect_disocclusions", lambda: ge.detect_case(33, 64), ("mask",), dict(above=at_or_above(F32(2.0 / 64 * 3.0)))),
    (">= threshold in inpaint_prepare", lambda: ge.prepare_tie_case("three"), ("mask",), dict(above=at_or_above(0.5))),
    (">= 1 in the k_gridwarp chain", lambda: ge.norm_case("max 1"), ("mask",), dict(above=at_or_above(1.0))),
    (">= 1 in the inpaint chain", lambda: ge.norm_case("max 1"), ("prepare/mask",), dict(above=at_or_above(1.0))),
    (">= 1e-6 in the k_gridwarp chain", lambda: ge.norm_case("range 1e-6"), ("mask",), dict(above=at_or_above(1e-6))),
    (">= 1e-6 in the inpaint chain", lambda: ge.norm_case("range 1e-6"), ("prepare/mask",), dict(above=at_or_above(1e-6))),
    ("nearest right border in interpolate_fill", lambda: ge.interp_case(4097), ("filled",), dict(borders=nearest_borders)),
    ("nearest right border in the edge stretch", lambda: ge.stretch_bitrow_case(4097, 8), ("stretch",), dict(borders=nearest_borders)),
]


@pytest.mark.parametrize("name,build,keys,mutation", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_wrong_restatement_differs_on_the_designed_cases(name, build, keys, mutation):
    n = differing(build, keys, **mutation)
    print(f"{name}: {n} differing output pixels")
    assert n > 0, name
