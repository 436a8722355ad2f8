"""The Gaussian depth blurs on the MI355X (cs_gaussblur.hip through stereoimage_generation, engine.gaussian_blur and the C
ABI).  Every comparison is exact on the float32 bit patterns: the reference's fixtures (tests/golden/gauss_blur.npz) and the
numpy restatement (tools/gauss_oracle.py), which tests/test_gauss_surface.py holds bit-equal to those fixtures and to
np.convolve.  No tolerance, no share of values left out."""
import ctypes

import numpy as np
import pytest
import torch

import gauss_oracle as go
from comfystereo_amd import _native, engine
from comfystereo_amd import stereoimage_generation as sig
from test_gauss_surface import case_args, load

pytestmark = pytest.mark.gpu
OPS = ["plain", "edge_selective", "left", "right"]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_bits(got, want, where):
    if isinstance(got, torch.Tensor):
        assert got.is_cuda and got.dtype == torch.float32, where
        got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (where, got.dtype, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (where, int(bad.sum()), "first at", tuple(int(i) for i in np.argwhere(bad)[0]))


def test_the_drop_ins_equal_every_fixture():
    z, meta = load()
    for c in meta["cases"]:
        args = case_args(z, c)
        got = getattr(sig, c["fn"])(*args)
        assert isinstance(got, np.ndarray), c["id"]
        assert_bits(got, z[f"{c['id']}/out"], c["id"])


def test_the_drop_ins_take_lists_and_other_dtypes_as_float32():
    d = go.depth_map("codes", 9, 14, 5)
    want = go.edge_selective_blur_depth_map(d, 1, 6)
    assert_bits(sig.edge_selective_blur_depth_map(d.astype(np.float64), 1, 6), want, "float64")
    assert_bits(sig.edge_selective_blur_depth_map(d.astype(np.uint8).tolist(), 1, 6), want, "list")
    assert_bits(sig.blur_depth_map(np.asfortranarray(d), 2.5), go.blur_depth_map(d, 2.5), "fortran order")
    with pytest.raises(ValueError):
        sig.blur_depth_map(np.zeros((2, 3, 4), dtype=np.float32), 1.0)
    with pytest.raises(ValueError):
        sig.left_direction_aware_blur_depth_map(np.zeros(5, dtype=np.float32), 1.0, 6)


# sizes 1, 2, 3, 63, 64, 65, 257, 1920, 4099 as heights and as widths, never large in both
SHAPES = [(1, 1), (1, 4099), (4099, 1), (2, 1920), (1920, 3), (3, 2), (63, 257), (257, 64), (65, 63), (64, 4099), (4099, 65),
          (1920, 2), (3, 1920), (257, 257)]
# sigma -> radius int(3 * sigma): 0, 1, 7, 60, 600
SIGMAS = [(0.2, 0), (0.4, 1), (2.5, 7), (20, 60), (200, 600)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_engine_equals_the_restatement_over_sizes_and_radii(shape):
    h, w = shape
    rng = np.random.default_rng(h * 10007 + w)
    kinds = ["codes", "unit", "noise", "ellipse"]
    for i, (sigma, radius) in enumerate(SIGMAS):
        assert int(3 * sigma) == radius
        d = go.depth_map(kinds[(i + h + w) % 4], h, w, int(rng.integers(1 << 30)))
        op = OPS[(i + h) % 4]
        thr = [0.5, 6, 40][(i + w) % 3]
        got = engine.gaussian_blur(cuda(d), sigma, op, thr)
        assert_bits(got, go.gaussian_blur(d, sigma, op, thr), (shape, sigma, op, thr))
    # every operation at one radius, and sigma <= 0 (the blends blend the depth with itself)
    d = go.depth_map("codes", h, w, 99)
    for op in OPS:
        assert_bits(engine.gaussian_blur(cuda(d), 2.5, op, 6), go.gaussian_blur(d, 2.5, op, 6), (shape, op))
        assert_bits(engine.gaussian_blur(cuda(d), 0, op, 0.5), go.gaussian_blur(d, 0, op, 0.5), (shape, op, "sigma 0"))


def test_radius_above_width_and_height():
    for h, w, sigma in ((3, 2, 2.5), (63, 257, 200), (5, 7, 70), (1, 1, 200)):
        assert int(3 * sigma) > max(h, w)
        d = go.depth_map("noise", h, w, h + w)
        for op in OPS:
            assert_bits(engine.gaussian_blur(cuda(d), sigma, op, 6), go.gaussian_blur(d, sigma, op, 6), (h, w, sigma, op))


def test_a_batch_equals_its_frames_one_by_one_and_two_runs_are_identical():
    frames = np.stack([go.depth_map(k, 70, 300, 40 + i) for i, k in enumerate(["codes", "unit", "noise", "ellipse", "flat"])])
    D = cuda(frames)
    for op in OPS:
        for sigma in (1, 7):
            a = engine.gaussian_blur(D, sigma, op, 6)
            b = engine.gaussian_blur(D, sigma, op, 6)
            assert a.shape == D.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (op, sigma, "two runs")
            for i in range(frames.shape[0]):
                one = engine.gaussian_blur(D[i], sigma, op, 6)
                assert one.shape == D[i].shape
                assert torch.equal(one.view(torch.int32), a[i].view(torch.int32)), (op, sigma, i)
            assert_bits(a, go.gaussian_blur(frames, sigma, op, 6), (op, sigma, "batch against the restatement"))
    # a non-contiguous view is taken as its values
    v = cuda(frames.transpose(0, 2, 1)).transpose(1, 2)
    assert not v.is_contiguous()
    assert_bits(engine.gaussian_blur(v, 2.5, "left", 6), go.gaussian_blur(frames, 2.5, "left", 6), "view")


# ---- straight through the C ABI -------------------------------------------------------------------------------------------------
def abi_blur(op, d, taps, thr, off=0, toff=0, ws_short=0, n_taps=None, alias=False):
    """cs_gaussian_blur on numpy depth [n, h, w] with depth, out and workspace `off` float32 elements into their allocations
    (4-byte aligned only when off is odd) and the taps `toff` doubles into theirs -> (status, out numpy)."""
    L = _native.lib()
    n, h, w = d.shape
    nt = len(taps) if n_taps is None else n_taps
    cnt = n * h * w
    D = torch.zeros(cnt + off + 8, dtype=torch.float32, device="cuda")
    D[off:off + cnt] = cuda(d).reshape(-1)
    O = torch.full((cnt + off + 8,), -7.0, dtype=torch.float32, device="cuda")
    T = torch.zeros(len(taps) + toff, dtype=torch.float64, device="cuda")
    T[toff:] = cuda(np.asarray(taps, dtype=np.float64))
    nb = L.cs_gaussian_blur_workspace_bytes(n, h, w, nt)
    WS = torch.zeros(nb // 4 + off + 8, dtype=torch.float32, device="cuda")
    p = lambda t, o: ctypes.c_void_p(t.data_ptr() + o * t.element_size())
    st = L.cs_gaussian_blur(_native.GAUSS_OP[op], p(D, off), p(T, toff), nt, float(thr), n, h, w, p(D, off) if alias else p(O, off),
                            p(WS, off), nb - ws_short, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if st == _native.CS_OK and not alias:
        assert (O[:off] == -7.0).all() and (O[off + cnt:] == -7.0).all(), "wrote outside the output"
    return st, O[off:off + cnt].reshape(n, h, w).cpu().numpy()


def asymmetric_taps(n, seed):
    t = np.random.default_rng(seed).random(n) + 0.01
    return t / t.sum()


@pytest.mark.parametrize("n_taps", [3, 9, 41, 203])
def test_asymmetric_taps_through_the_c_abi(n_taps):
    """The Gaussian is symmetric, so a kernel that ran its taps backwards would pass every test above; this one it fails.
    np.convolve semantics: tests/test_gauss_surface.py holds the restatement to np.convolve on such taps."""
    taps = asymmetric_taps(n_taps, n_taps)
    d = np.stack([go.depth_map("noise", 37, 1100, 1), go.depth_map("codes", 37, 1100, 2)])
    for op in OPS:
        st, got = abi_blur(op, d, taps, 6)
        assert st == _native.CS_OK
        assert_bits(got, go.gaussian_blur_taps(d, taps, op, 6), (n_taps, op))
        assert not np.array_equal(got, go.gaussian_blur_taps(d, taps[::-1].copy(), op, 6)), "the tap order must matter here"


def test_unaligned_and_offset_views_through_the_c_abi():
    taps = go.gaussian_taps(2.5)
    d = np.stack([go.depth_map("codes", 33, 131, 8), go.depth_map("unit", 33, 131, 9)])
    for off, toff in ((1, 0), (3, 1), (2, 5), (64, 0)):
        for op in ("plain", "edge_selective"):
            st, got = abi_blur(op, d, taps, 6, off=off, toff=toff)
            assert st == _native.CS_OK, (off, toff)
            assert_bits(got, go.gaussian_blur_taps(d, taps, op, 6), (off, toff, op))


def test_error_codes_and_the_tap_cap():
    L = _native.lib()
    cap = L.cs_gaussian_blur_max_taps()
    d = go.depth_map("codes", 6, 40, 1)[None]
    taps = go.gaussian_taps(1)
    assert abi_blur("plain", d, taps, 6, alias=True)[0] == _native.CS_EINVAL       # out must not alias depth
    assert abi_blur("plain", d, taps, 6, ws_short=1)[0] == _native.CS_EWORKSPACE
    assert abi_blur("plain", d, taps, 6, n_taps=6)[0] == _native.CS_EINVAL
    assert abi_blur("plain", d, taps, 6, n_taps=0)[0] == _native.CS_EINVAL
    # at the cap: accepted and exact; one odd count above: CS_ELIMIT
    big = asymmetric_taps(cap, 7)
    st, got = abi_blur("right", d, big, 6)
    assert st == _native.CS_OK
    assert_bits(got, go.gaussian_blur_taps(d, big, "right", 6), "at the cap")
    assert abi_blur("right", d, np.ones(cap + 2), 6)[0] == _native.CS_ELIMIT
    # the engine wrapper: ValueError on shape, dtype, device and a missing threshold; CS_ELIMIT surfaces as NativeError
    D = cuda(d[0])
    for bad in (lambda: engine.gaussian_blur(D[0], 1.0), lambda: engine.gaussian_blur(D[None, None], 1.0),
                lambda: engine.gaussian_blur(D.double(), 1.0), lambda: engine.gaussian_blur(D.cpu(), 1.0),
                lambda: engine.gaussian_blur(d[0], 1.0), lambda: engine.gaussian_blur(D, 1.0, "left"),
                lambda: engine.gaussian_blur(D, 1.0, "sideways", 6), lambda: engine.gaussian_blur(D[:0], 1.0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_native.NativeError) as ei:
        engine.gaussian_blur(D, (cap // 2 + 1) / 3 + 0.01)
    assert ei.value.code == _native.CS_ELIMIT
    # the output is a new tensor and the input is left alone
    before = D.clone()
    out = engine.gaussian_blur(D, 2.5, "edge_selective", 6)
    assert out.data_ptr() != D.data_ptr() and torch.equal(D, before)


_BLUR_4K = {}


@pytest.mark.parametrize("op", OPS)
def test_one_4k_map_per_operation(op):
    h, w, sigma, thr = 2160, 3840, 7, 6
    if "d" not in _BLUR_4K:
        d = go.depth_map("codes", h, w, 2160)
        _BLUR_4K.update(d=d, blurred=go.blur_taps(d, go.gaussian_taps(sigma)))
    d, blurred = _BLUR_4K["d"], _BLUR_4K["blurred"]
    want = blurred if op == "plain" else go.blend(d, blurred, go.weight(d, op, thr)).astype(np.float32)
    assert_bits(engine.gaussian_blur(cuda(d), sigma, op, thr), want, ("4K", op))


def test_a_fused_multiply_add_anywhere_in_a_pass_would_show():
    """Rounded to float32, a float64 sum hides a last-bit change of one of its steps from every test above (the float32
    rounding point lies 29 bits higher).  Here it cannot hide: all taps are zero but a pair -1, 1 + 2^-40 on equal neighbouring
    samples x, so the sum is round(x * (1 + 2^-40)) - x -- the rounding error of that one product IS the result (12 significant
    bits), while a fused multiply-add would keep all 24.  The pair visits every tap position of the unrolled loops; a map
    with constant rows exposes the row pass, one with constant columns (its row pass gives full-mantissa values) the column pass."""
    rng = np.random.default_rng(21)
    h, w, n = 40, 70, 21
    const_rows = np.repeat((rng.random((h, 1), dtype=np.float32) * np.float32(200) + np.float32(20)), w, 1)
    const_cols = np.repeat((rng.random((1, w), dtype=np.float32) * np.float32(200) + np.float32(20)), h, 0)
    for pos in range(1, n):
        flipped = np.zeros(n)
        flipped[pos - 1], flipped[pos] = -1.0, 1.0 + 2.0 ** -40
        taps = flipped[::-1].copy()
        for name, d in (("constant rows", const_rows), ("constant columns", const_cols)):
            st, got = abi_blur("plain", d[None], taps, 0)
            assert st == _native.CS_OK
            want = go.gaussian_blur_taps(d[None], taps)
            assert_bits(got, want, (name, pos))
            if name == "constant rows":   # what a fused row pass would have stored: x * 2^-40 with all its bits
                fused = (d.astype(np.float64) * 2.0 ** -40).astype(np.float32)
                rows_only = go.convolve_axis(d, taps, 1)
                assert not np.array_equal(rows_only, fused), "the case must tell fused from unfused"
