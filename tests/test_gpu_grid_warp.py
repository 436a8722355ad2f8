"""The grid-sample warps on the MI355X (cs_gridwarp.hip through stereoimage_generation): every fixture case of
tests/golden/grid_warp*.npz, a seeded fuzz against the restatement (tools/grid_oracle.py) over widths 1 .. 16 384 and the row
kernel's workgroup and LDS cuts, non-contiguous and host inputs, and the refusal of a frame wider than the LDS row.

Contract: masks and colours bit-exact for the exponents torch.pow special-cases (2, 1, 0.5) -- the kernel evaluates the vectorised
CPU grid_sample's fused sums; interpolate_fill_gpu bit-exact.  For a general exponent the
kernel's powf is correctly rounded and CPU torch's vectorised pow is not everywhere: an offset one ulp apart can move a forward
destination across a column or a grid x by an ulp, so those pixels are counted and bounded instead (TOL is that test's alone)."""
import numpy as np
import pytest
import torch

import grid_oracle as go
from comfystereo_amd import _native
from comfystereo_amd import stereoimage_generation as sig
from test_grid_surface import expected_case, load

pytestmark = pytest.mark.gpu
TOL = 1e-6


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_case(z, c):
    cid, fn = c["id"], c["fn"]
    if fn == "interpolate_fill_gpu":
        b, ch, h, w = c["shape"]
        m = np.unpackbits(z[f"{cid}/mask"], count=b * h * w).reshape(b, h, w).astype(bool)
        return dict(filled=sig.interpolate_fill_gpu(cuda(z[f"{cid}/image"]), cuda(m), "cuda"))
    if fn == "detect_disocclusions_gpu":
        m = sig.detect_disocclusions_gpu(cuda(z[f"{cid}/depth"]), cuda(z[f"{cid}/grid"]), cuda(z[f"{cid}/gxw"]), "cuda",
                                         threshold=c["threshold"])
        return dict(mask=m)
    args = (c["divergence_px"], c["separation_px"], c["exponent"], c["convergence"])
    if fn == "compute_forward_mask_gpu":
        return dict(mask=sig.compute_forward_mask_gpu(cuda(z[f"{cid}/depth"]), *args, "cuda"))
    if fn == "apply_stereo_divergence_gpu":
        return dict(warped=sig.apply_stereo_divergence_gpu(cuda(z[f"{cid}/image"]), cuda(z[f"{cid}/depth"]), *args))
    if fn == "warp_and_fill_gpu":
        wr, m = sig.warp_and_fill_gpu(cuda(z[f"{cid}/image"]), cuda(z[f"{cid}/depth"]), *args)
        return dict(warped=wr, mask=m)
    wr, v = sig.apply_stereo_divergence_gpu_with_fill(cuda(z[f"{cid}/image"]), cuda(z[f"{cid}/depth"]), *args,
                                                      fill_mode=c["fill_mode"])
    return dict(warped=wr, valid=v)


def check(got, want, where, exact_colours=True):
    """Masks and colours bit for bit; exact_colours=False (a general exponent only): colours within TOL."""
    for k, v in want.items():
        g = got[k]
        assert g.is_cuda, (where, k)
        g = g.cpu().numpy().reshape(v.shape)
        if v.dtype == bool:
            assert g.dtype == bool and np.array_equal(g, v), (where, k, int((g != v).sum()))
        elif exact_colours:
            assert g.dtype == v.dtype and np.array_equal(g.view(np.int32), v.view(np.int32)), (where, k, int((g != v).sum()), float(np.abs(g - v).max()))
        else:
            assert np.abs(g - v).max() <= TOL, (where, k, float(np.abs(g - v).max()))


def test_every_small_fixture_case():
    z, meta = load("grid_warp.npz")
    for c in meta["cases"]:
        got, want = run_case(z, c), expected_case(z, c)
        check(got, want, c["id"], exact_colours=c.get("exponent", 2.0) in (2.0, 1.0, 0.5))   # (1.3: the module docstring)


def test_the_1080p_fixture():
    import make_grid_goldens as mg
    z, meta = load("grid_warp_1080p.npz")
    img, depth = mg.inputs_1080p()
    rows, p = meta["rows"], meta["warp"]
    args = (p["divergence_px"], p["separation_px"], p["exponent"], p["convergence"])
    I, D = cuda(img), cuda(depth)
    assert np.array_equal(sig.apply_stereo_divergence_gpu(I, D, *args).cpu().numpy()[:, :, rows], z["asd/rows"])
    wr, m = sig.warp_and_fill_gpu(I, D, *args)
    assert np.array_equal(np.packbits(m.cpu().numpy()), z["waf/mask"])
    assert np.array_equal(wr.cpu().numpy()[:, :, rows], z["waf/rows"])
    m = sig.compute_forward_mask_gpu(D, meta["mask"]["divergence_px"], meta["mask"]["separation_px"], p["exponent"], p["convergence"], "cuda")
    assert np.array_equal(np.packbits(m.cpu().numpy()), z["cfm/mask"])
    f = meta["fill"]
    wr, v = sig.apply_stereo_divergence_gpu_with_fill(I[0], D[0], f["divergence_px"], f["separation_px"], p["exponent"],
                                                      p["convergence"], f["fill_mode"])
    assert np.array_equal(np.packbits(v.cpu().numpy()), z["wf/valid"])
    assert np.array_equal(wr.cpu().numpy()[:, rows], z["wf/rows"])
    mi = go.block_depth_u8(1080, 1920, meta["interp_mask"]["seed"])[None] > meta["interp_mask"]["above"]
    assert np.array_equal(sig.interpolate_fill_gpu(I[:1], cuda(mi), "cuda").cpu().numpy()[:, :, rows], z["ifg/rows"])
    d0 = (depth[0] / np.float32(255.0)).astype(np.float32)
    gxw = go.grid_x(go.pixel_offset(depth[:1], *args))[0].astype(np.float32)
    grid = np.stack([gxw, np.broadcast_to(go.linspace(1080)[:, None], gxw.shape)], -1)[None].astype(np.float32)
    dm = sig.detect_disocclusions_gpu(cuda(d0), cuda(grid), cuda(gxw), "cuda")
    assert np.array_equal(np.packbits(dm.cpu().numpy()), z["dis/mask"])


# widths: tiny, the workgroup-size cuts of the row kernels (256 / 1024 / 4096 columns), word edges, and the LDS limit
FUZZ_WIDTHS = [1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 8191, 16384]


def fuzz_inputs(rng, b, c, h, w):
    img = rng.random((b, c, h, w), dtype=np.float32)
    kind = rng.integers(0, 3)
    if kind == 0:
        d8 = np.stack([go.block_depth_u8(h, w, int(rng.integers(1 << 30)), block=int(rng.integers(2, 64))) for _ in range(b)])
    elif kind == 1:
        d8 = rng.integers(0, 256, (b, h, w))
    else:
        d8 = np.repeat(rng.integers(0, 256, (b, h, 1)), w, 2)   # (flat rows)
    depth = d8.astype(np.float32)
    scales = rng.random(b) < 0.5
    depth[scales] /= np.float32(255.0)
    return img, depth.astype(np.float32)


@pytest.mark.parametrize("w", FUZZ_WIDTHS)
def test_fuzz_against_the_restatement(w):
    rng = np.random.default_rng(1000 + w)
    for trial in range(3):
        b, c, h = int(rng.integers(1, 3)), int(rng.choice([1, 3, 4])), int(rng.integers(1, 6))
        img, depth = fuzz_inputs(rng, b, c, h, w)
        e = float(rng.choice([2.0, 1.0, 0.5]))
        dpx = float(rng.choice([-1, 1]) * rng.random() * max(w, 2) * 0.15)
        spx = float(rng.choice([0.0, rng.normal() * 3, rng.choice([-1, 1]) * 1.5 * w]))
        conv = float(rng.random())
        args = (dpx, spx, e, conv)
        I, D = cuda(img), cuda(depth)
        where = (w, trial, b, c, h, args)
        check(dict(warped=sig.apply_stereo_divergence_gpu(I, D, *args)), dict(warped=go.apply_stereo_divergence_gpu(img, depth, *args)), where)
        wr, m = sig.warp_and_fill_gpu(I, D, *args)
        ow, om = go.warp_and_fill_gpu(img, depth, *args)
        check(dict(warped=wr, mask=m), dict(warped=ow, mask=om), where)
        check(dict(mask=sig.compute_forward_mask_gpu(D, *args, "cuda")), dict(mask=go.compute_forward_mask_gpu(depth, *args)), where)
        pad = str(rng.choice(["border", "zeros", "reflection", "other"]))
        im1 = I[0].permute(1, 2, 0) if w in (1, 3, 4) else I[0]   # (a CHW image of width 1, 3 or 4 reads as HWC, as in the reference)
        wr, v = sig.apply_stereo_divergence_gpu_with_fill(im1, D[0], *args, fill_mode=pad)
        ow, ov = go.apply_stereo_divergence_gpu_with_fill(img[0], depth[0], *args, fill_mode=pad)
        check(dict(warped=wr, valid=v), dict(warped=ow, valid=ov), where + (pad,))
        mk = rng.random((b, h, w)) < rng.random()
        check(dict(filled=sig.interpolate_fill_gpu(I, cuda(mk), "cuda")), dict(filled=go.interpolate_fill_gpu(img, mk)), where,
              exact_colours=True)
        if w >= 2:
            grid = ((rng.random((1, h, w, 2)) - 0.5) * rng.choice([2.5, 40.0])).astype(np.float32)
            gxw = go.grid_x(go.pixel_offset(depth[:1], *args))[0].astype(np.float32)
            thr = float(rng.choice([0.02, 0.0, 0.3]))
            d0 = img[0, 0]
            got = sig.detect_disocclusions_gpu(cuda(d0), cuda(grid), cuda(gxw), "cuda", threshold=thr)
            check(dict(mask=got), dict(mask=go.detect_disocclusions_gpu(d0, grid, gxw, thr)), where)


def test_general_exponent_is_bounded():
    """exponent 1.3: the pixels where the correctly rounded powf and CPU torch's vectorised pow disagree by an ulp may move;
    at most 0.5 % of the mask pixels and 1 % of the colours (beyond 1e-6) may differ from the restatement."""
    rng = np.random.default_rng(77)
    for w in (97, 1920):
        img, depth = fuzz_inputs(rng, 2, 3, 5, w)
        args = (0.05 * w, 0.0, 1.3, 0.4)
        wr, m = sig.warp_and_fill_gpu(cuda(img), cuda(depth), *args)
        ow, om = go.warp_and_fill_gpu(img, depth, *args)
        assert (m.cpu().numpy() != om).mean() <= 0.005
        assert (np.abs(wr.cpu().numpy() - ow) > TOL).mean() <= 0.01
        mm = sig.compute_forward_mask_gpu(cuda(depth), *args, "cuda").cpu().numpy()
        assert (mm != go.compute_forward_mask_gpu(depth, *args)).mean() <= 0.005


def test_noncontiguous_and_host_inputs():
    rng = np.random.default_rng(5)
    img, depth = fuzz_inputs(rng, 2, 3, 6, 70)
    args = (6.0, 0.5, 2.0, 0.5)
    want_w, want_m = go.warp_and_fill_gpu(img, depth, *args)
    # host tensors, a channels-last view, a transposed depth view
    host = sig.warp_and_fill_gpu(torch.from_numpy(img), torch.from_numpy(depth), *args)
    cl = cuda(img.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2)
    dt = cuda(depth.transpose(0, 2, 1)).transpose(1, 2)
    assert not cl.is_contiguous() and not dt.is_contiguous()
    view = sig.warp_and_fill_gpu(cl, dt, *args)
    for wr, m in (host, view):
        check(dict(warped=wr, mask=m), dict(warped=want_w, mask=want_m), "views")
    # HWC and CHW into ..._with_fill, float64 and uint8 depth
    wr1, v1 = sig.apply_stereo_divergence_gpu_with_fill(torch.from_numpy(img[0].transpose(1, 2, 0).copy()),
                                                        torch.from_numpy(depth[0]).double()[None], *args, fill_mode="zeros")
    ow, ov = go.apply_stereo_divergence_gpu_with_fill(img[0], depth[0], *args, fill_mode="zeros")
    check(dict(warped=wr1, valid=v1), dict(warped=ow, valid=ov), "hwc")
    mk = rng.random((2, 6, 70)) < 0.3
    iv = cuda(img.transpose(0, 1, 3, 2).copy()).transpose(2, 3)
    assert not iv.is_contiguous()
    got = sig.interpolate_fill_gpu(iv, torch.from_numpy(mk), "cuda")
    assert np.array_equal(got.cpu().numpy(), go.interpolate_fill_gpu(img, mk))


def test_mismatched_inputs_raise_value_error():
    I, D = torch.zeros(2, 3, 4, 8).cuda(), torch.zeros(2, 4, 9).cuda()
    with pytest.raises(ValueError):
        sig.warp_and_fill_gpu(I, D, 1.0, 0.0, 2.0)
    with pytest.raises(ValueError):
        sig.apply_stereo_divergence_gpu(I[0], D[0], 1.0, 0.0, 2.0)
    with pytest.raises(ValueError):
        sig.interpolate_fill_gpu(I, torch.zeros(2, 4, 8, dtype=torch.uint8).cuda(), "cuda")
    with pytest.raises(ValueError):
        sig.detect_disocclusions_gpu(torch.zeros(4, 8).cuda(), torch.zeros(1, 4, 7, 2).cuda(), torch.zeros(4, 8).cuda(), "cuda")
    with pytest.raises(IndexError):
        sig.detect_disocclusions_gpu(torch.zeros(4, 1).cuda(), torch.zeros(1, 4, 1, 2).cuda(), torch.zeros(4, 1).cuda(), "cuda")


def test_too_wide_frame_is_refused_with_elimit():
    L = _native.lib()
    wmax = L.cs_grid_warp_max_width(_native.GRID_OP["stretch"])
    assert wmax >= 16384
    I, D = torch.rand(1, 1, 1, wmax + 1).cuda(), torch.rand(1, 1, wmax + 1).cuda()
    for fn in (lambda: sig.warp_and_fill_gpu(I, D, 10.0, 0.0, 2.0), lambda: sig.compute_forward_mask_gpu(D, 10.0, 0.0, 2.0, 0.5, "cuda")):
        with pytest.raises(_native.NativeError) as ei:
            fn()
        assert ei.value.code == _native.CS_ELIMIT
    # the widest accepted frame works, and the plain warp has no width limit
    I, D = torch.rand(1, 3, 2, wmax).cuda(), torch.rand(1, 2, wmax).cuda()
    wr, m = sig.warp_and_fill_gpu(I, D, 30.0, 0.0, 2.0)
    ow, om = go.warp_and_fill_gpu(I.cpu().numpy(), D.cpu().numpy(), 30.0, 0.0, 2.0)
    check(dict(warped=wr, mask=m), dict(warped=ow, mask=om), "wmax")
    wide = sig.apply_stereo_divergence_gpu(torch.rand(1, 1, 1, wmax + 7).cuda(), torch.rand(1, 1, wmax + 7).cuda(), 5.0, 0.0, 1.0)
    assert wide.shape == (1, 1, 1, wmax + 7)
