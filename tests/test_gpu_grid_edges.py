"""The grid-sample family on the MI355X (cs_gridwarp.hip, cs_inpaintprep.hip, cs_gridsample.h) over the designed edge inputs of
tools/grid_edge_inputs.py: rounding ties of the nearest and bilinear samples, strict comparisons at equality, the padding edges,
the bit-row scans across their 2048-column chunks and word boundaries, the 5-row dilation at the frame's top and bottom, the
normalisation thresholds, and NaN / infinite pixels, grid values and depths.

Contract: EVERY output bit for bit -- masks, float32 colours (all NaN patterns count as one value), uint8 codes of finite colours.
Exponents 2, 1 and 0.5 only.  tests/test_grid_edges_surface.py holds the expected side to CPU torch and to its reach counts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import grid_edge_inputs as ge
from comfystereo_amd import _native, engine
from comfystereo_amd import stereoimage_generation as sig
from test_grid_edges_surface import bits_differ

pytestmark = pytest.mark.gpu
F32 = np.float32


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, where):
    """A device tensor against an expected array: zero differing bits."""
    g = got.cpu().numpy().reshape(want.shape)
    if want.dtype == F32:
        assert g.dtype == F32, where
        n = bits_differ(g, want)
    else:
        assert g.dtype == want.dtype, (where, g.dtype)
        n = int((g != want).sum())
    assert n == 0, (where, n, "differing elements")


def run_gridwarp(c):
    """The four operations of one case through the module functions, every expected key compared."""
    img, depth, args = c.inputs["image"], c.inputs["depth"], c.params["args"]
    I, D = cuda(img), cuda(depth)
    w = img.shape[-1]
    same(sig.apply_stereo_divergence_gpu(I, D, *args), c.expected["warp"], (c.name, "warp"))
    wr, m = sig.warp_and_fill_gpu(I, D, *args)
    same(wr, c.expected["stretch"], (c.name, "stretch"))
    same(m, c.expected["stretch_mask"], (c.name, "stretch mask"))
    same(sig.compute_forward_mask_gpu(D, *args, "cuda"), c.expected["mask"], (c.name, "mask"))
    for key in c.expected:
        if key.startswith("fill:"):
            mode = key[5:]
            for f in range(img.shape[0]):
                im1 = I[f].permute(1, 2, 0) if w in (1, 3, 4) else I[f]   # (a CHW image of width 1, 3 or 4 reads as HWC, as in the reference)
                wr, v = sig.apply_stereo_divergence_gpu_with_fill(im1, D[f], *args, fill_mode=mode)
                same(wr, c.expected[key][f], (c.name, key, f))
                same(v, c.expected["valid:" + mode][f], (c.name, "valid", mode, f))
            # the engine entry, frame by frame as the expected arrays are: a batch is normalised as a whole ("other" is the
            # module function's word for border)
            for f in range(img.shape[0]):
                wr, v = engine.grid_warp(I[f:f + 1], D[f:f + 1], *args, op="fill", padding=mode if mode in _native.GRID_PADDING else "border")
                same(wr, c.expected[key][f:f + 1], (c.name, key, "engine", f))
                same(v, c.expected["valid:" + mode][f:f + 1], (c.name, "valid", mode, "engine", f))


def run_prepare(c, prefix=""):
    img, depth = c.inputs["image"], c.inputs["depth"]
    got = engine.inpaint_prepare(cuda(img), cuda(depth), c.params["sf"], c.params["thr"], codes=True)
    for k, g in zip(("warped", "filled", "mask"), got[:3]):
        same(g, c.expected[prefix + k], (c.name, k))
    for k, g, fl in (("warped_u8", got[3], got[0]), ("filled_u8", got[4], got[1])):
        ok = np.isfinite(np.moveaxis(fl.cpu().numpy(), -3, -1))   # (the codes are defined for finite colours)
        assert np.array_equal(g.cpu().numpy()[ok], c.expected[prefix + k][ok]), (c.name, k)
    return got


@functools.lru_cache(maxsize=None)
def gridwarp_cases():
    return list(ge.gridwarp_cases())


@pytest.mark.parametrize("family", ["shift", "offset", "gridwarp"])
def test_the_four_operations_on_designed_shifts_and_ties(family):
    """shift: uniform shifts by integers and half columns under every padding, finite and special pixels (a non-finite pixel under a
    weight of exactly 0 makes the sum NaN, as in CPU torch); offset: forward destinations on -1 and w; gridwarp: level depths on the
    sample ties, on integer destinations and on offset steps of 1.5 and its neighbours."""
    mine = [c for c in gridwarp_cases() if c.name.split()[0] == family]
    assert len(mine) >= 5
    for c in mine:
        run_gridwarp(c)


@pytest.mark.parametrize("w", ge.BITROW_WIDTHS)
def test_bit_row_layouts(w):
    """Rows with nothing unmasked, with one unmasked pixel at a word or chunk edge, and masked runs across column 2048 k:
    interpolate_fill_gpu on the masks themselves, the edge stretch and the inpaint pre-fill on the same layouts induced through
    depth."""
    c = ge.interp_case(w)
    same(sig.interpolate_fill_gpu(cuda(c.inputs["image"]), cuda(c.inputs["mask"]), "cuda"), c.expected["filled"], c.name)
    for first in (0, 4, 8, 9):
        run_gridwarp(ge.stretch_bitrow_case(w, first))
        run_prepare(ge.prepare_bitrow_case(w, first))


def test_inpaint_prepare_on_ties_and_dilation_edges():
    for kind in ("two", "three"):
        run_prepare(ge.prepare_tie_case(kind))
    for h in ge.DILATION_HEIGHTS:
        run_prepare(ge.dilation_case(h))


@pytest.mark.parametrize("nonfinite", [False, True])
def test_detect_disocclusions_on_designed_grids(nonfinite):
    for h, w in ge.DETECT_SHAPES:
        c = ge.detect_case(h, w, nonfinite)
        got = sig.detect_disocclusions_gpu(cuda(c.inputs["depth"]), cuda(c.inputs["grid"]), cuda(c.inputs["gxw"]), "cuda", threshold=c.params["threshold"])
        same(got, c.expected["mask"], c.name)


def test_normalisation_edges_in_both_chains():
    """Frame maxima of 1, the float above it and 255; ranges of 1e-6, its neighbours and 0; a batch of which one frame is above 1
    (the k_gridwarp chain divides the whole batch by 255, the inpaint chain that frame alone)."""
    for name in list(ge.NORM_FRAMES) + list(ge.NORM_BATCHES):
        c = ge.norm_case(name)
        run_gridwarp(c)
        run_prepare(c, "prepare/")


def test_nonfinite_depth_in_both_chains_batches_and_reruns():
    """NaN / infinite depth: a frame with a NaN is flat, an infinite value makes the range infinite.  The batch equals its frames
    (in the inpaint chain, whose frames are on their own) and two runs are identical."""
    for kinds in ge.NONFINITE_BATCHES:
        c = ge.nonfinite_depth_case(kinds)
        run_gridwarp(c)
        first = run_prepare(c, "prepare/")
        again = run_prepare(c, "prepare/")
        for a, b in zip(first, again):
            assert bits_differ(a.float().cpu().numpy(), b.float().cpu().numpy()) == 0, (c.name, "second run")
        I, D = cuda(c.inputs["image"]), cuda(c.inputs["depth"])
        for f in range(I.shape[0]):
            one = engine.inpaint_prepare(I[f:f + 1], D[f:f + 1], c.params["sf"], c.params["thr"], codes=True)
            for a, b in zip(first, one):
                assert bits_differ(a[f].float().cpu().numpy(), b[0].float().cpu().numpy()) == 0, (c.name, "frame", f)
        args = c.params["args"]
        a, b = sig.warp_and_fill_gpu(I, D, *args), sig.warp_and_fill_gpu(I, D, *args)
        assert bits_differ(a[0].cpu().numpy(), b[0].cpu().numpy()) == 0 and torch.equal(a[1], b[1]), c.name


# ---- through the C ABI: optional outputs, and every tensor one element off its natural alignment ---------------------------------
F_GUARD, B_GUARD = -7.0, 0xA5


class Buf:
    """A device allocation holding `n` elements `off` elements into it, guard values before and after."""

    def __init__(self, dtype, n, off, data=None):
        guard = F_GUARD if dtype == torch.float32 else B_GUARD if dtype == torch.uint8 else 0x5A5A5A5A
        self.t = torch.full((n + off + 8,), guard, dtype=dtype, device="cuda")
        self.n, self.off, self.guard = n, off, guard
        if data is not None:
            d = np.ascontiguousarray(data)
            self.t[off:off + n] = cuda(d.astype(np.uint8) if d.dtype == bool else d).reshape(-1)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + self.off * self.t.element_size())

    def get(self, shape):
        assert (self.t[:self.off] == self.guard).all() and (self.t[self.off + self.n:] == self.guard).all(), "wrote outside the output"
        return self.t[self.off:self.off + self.n].reshape(shape)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, off):
    return Buf(torch.int32, nbytes // 4 + 1, off)


def abi_grid_warp(c, op, off):
    L = _native.lib()
    img, depth, args = c.inputs["image"], c.inputs["depth"], c.params["args"]
    b, ch, h, w = img.shape
    I, D = Buf(torch.float32, img.size, off, img), Buf(torch.float32, depth.size, off, depth)
    O, M = Buf(torch.float32, img.size, off), Buf(torch.uint8, depth.size, off)
    nb = L.cs_grid_warp_workspace_bytes(b, h, w)
    W = workspace(nb, off)
    st = L.cs_grid_warp(I.ptr, D.ptr, b, ch, h, w, *[float(a) for a in args], _native.GRID_OP[op], 0, O.ptr, M.ptr, W.ptr, nb, stream())
    torch.cuda.synchronize()
    assert st == _native.CS_OK, (op, off, st)
    return O.get(img.shape), M.get(depth.shape)


@pytest.mark.parametrize("off", [0, 1, 3])
def test_unaligned_tensors_through_the_c_abi(off):
    L = _native.lib()
    c = ge.tie_case("steps of 1.5")
    for op, ok, mk in (("warp", "warp", None), ("fill", "fill:border", "valid:border"), ("mask", None, "mask"), ("stretch", "stretch", "stretch_mask")):
        O, M = abi_grid_warp(c, op, off)
        if ok:
            same(O, c.expected[ok], (op, off))
        else:
            assert (O == F_GUARD).all()
        if mk:
            same(M.bool(), c.expected[mk], (op, off, "mask"))
        else:
            assert (M == B_GUARD).all()
    # cs_interpolate_fill
    c = ge.interp_case(4097)
    img, mask = c.inputs["image"], c.inputs["mask"]
    b, ch, h, w = img.shape
    I, Mi, O = Buf(torch.float32, img.size, off, img), Buf(torch.uint8, mask.size, off, mask), Buf(torch.float32, img.size, off)
    assert L.cs_interpolate_fill(I.ptr, Mi.ptr, b, ch, h, w, O.ptr, stream()) == _native.CS_OK
    torch.cuda.synchronize()
    same(O.get(img.shape), c.expected["filled"], ("interpolate_fill", off))
    # cs_detect_disocclusions
    c = ge.detect_case(33, 64)
    d, g, x = c.inputs["depth"], c.inputs["grid"], c.inputs["gxw"]
    Dd, G, X, O = Buf(torch.float32, d.size, off, d), Buf(torch.float32, g.size, off, g), Buf(torch.float32, x.size, off, x), Buf(torch.uint8, d.size, off)
    assert L.cs_detect_disocclusions(Dd.ptr, G.ptr, X.ptr, 33, 64, c.params["threshold"], O.ptr, stream()) == _native.CS_OK
    torch.cuda.synchronize()
    same(O.get(d.shape).bool(), c.expected["mask"], ("detect", off))
    # cs_inpaint_prepare, all outputs
    got = abi_prepare(ge.prepare_tie_case("three"), off, range(5))
    check_prepare_abi(ge.prepare_tie_case("three"), got, range(5))


PREPARE_OUTPUTS = ("warped", "filled", "mask", "warped_u8", "filled_u8")


def abi_prepare(c, off, wanted):
    """cs_inpaint_prepare with the outputs of indices `wanted` (PREPARE_OUTPUTS) and null pointers for the others."""
    L = _native.lib()
    img, depth = c.inputs["image"], c.inputs["depth"]
    b, _, h, w = img.shape
    I, D = Buf(torch.float32, img.size, off, img), Buf(torch.float32, depth.size, off, depth)
    outs = [Buf(torch.float32, img.size, off), Buf(torch.float32, img.size, off), Buf(torch.uint8, depth.size, off),
            Buf(torch.uint8, img.size, off), Buf(torch.uint8, img.size, off)]
    nb = L.cs_inpaint_prepare_workspace_bytes(b, h, w)
    W = workspace(nb, off)
    ptrs = [o.ptr if k in wanted else None for k, o in enumerate(outs)]
    st = L.cs_inpaint_prepare(I.ptr, D.ptr, b, h, w, (c.params["sf"] / 100.0) * w, c.params["thr"], *ptrs, W.ptr, nb, stream())
    torch.cuda.synchronize()
    assert st == _native.CS_OK
    shapes = (img.shape, img.shape, depth.shape, depth.shape + (3,), depth.shape + (3,))
    res = [o.get(s) for o, s in zip(outs, shapes)]
    for k, (o, r) in enumerate(zip(outs, res)):
        if k not in wanted:
            assert (r == o.guard).all(), ("an output that was not asked for was written", PREPARE_OUTPUTS[k])
    return res


def check_prepare_abi(c, res, wanted):
    for k in wanted:
        name = PREPARE_OUTPUTS[k]
        same(res[k].bool() if name == "mask" else res[k], c.expected[name], (c.name, name))


def test_each_optional_output_of_inpaint_prepare_alone():
    """Every single output requested alone, and the floats with the codes on and off, equal the all-outputs call."""
    c = ge.prepare_tie_case("two")
    for wanted in ([0], [1], [2], [3], [4], [0, 1, 2], [3, 4], [1, 4]):
        check_prepare_abi(c, abi_prepare(c, 0, wanted), wanted)
    c = ge.dilation_case(5)
    for wanted in ([1], [2], [4]):
        check_prepare_abi(c, abi_prepare(c, 1, wanted), wanted)
