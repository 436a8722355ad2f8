"""StereoDiffusion Fast mode's warp, inpaint mask and gap pre-fill on the MI355X (cs_inpaintprep.hip through
stereodiffusion_nodes.prepare_inpaint and engine.inpaint_prepare): every case of tests/golden/inpaint_prep.npz against the
reference's own outputs, a seeded fuzz against the restatement (tools/inpaint_oracle.py) over widths 1 .. 16 384, batches
against their frames, non-contiguous and host inputs, and the refusal of a frame wider than the LDS bit row.

Contract: masks bit-exact; uint8 codes identical to the reference's; float `warped` / `filled` bit for bit the restatement's."""
import numpy as np
import pytest
import torch

import inpaint_oracle as io
from comfystereo_amd import _native, engine
from comfystereo_amd import stereodiffusion_nodes as sdn
from test_gpu_grid_warp import FUZZ_WIDTHS, fuzz_inputs
from test_inpaint_surface import case_inputs, check_case, load

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_floats(got, want, where):
    """(warped, filled, mask) tensors against the restatement's arrays."""
    for k, g, w in zip(("warped", "filled"), got[:2], want[:2]):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == np.float32, (where, k)
        differing = int((g.view(np.int32) != w.view(np.int32)).sum())
        print(where, k, "differing bit patterns", differing)
        assert differing == 0, (where, k, differing, float(np.abs(g - w).max()))
    m = got[2].cpu().numpy()
    assert m.dtype == bool and np.array_equal(m, want[2]), (where, "mask", int((m != want[2]).sum()))


def test_every_fixture_case_through_both_entries():
    z, meta = load()
    for c in meta["cases"]:
        img, depth = case_inputs(z, meta, c)
        want = io.prepare(img[None], depth[None], c["scale_factor"])
        # the device entry, with codes
        wr, fl, m, wu8, fu8 = engine.inpaint_prepare(cuda(img[None]), cuda(depth[None]), c["scale_factor"], codes=True)
        check_floats((wr, fl, m), want, c["id"])
        check_case(z, meta, c, m[0].cpu().numpy(), wu8[0].cpu().numpy(), fu8[0].cpu().numpy())
        assert np.array_equal(wu8.cpu().numpy(), io.codes(want[0])) and np.array_equal(fu8.cpu().numpy(), io.codes(want[1]))
        # the module function on one host frame: results on the host, codes by the reference's expression
        got = sdn.prepare_inpaint(torch.from_numpy(img), torch.from_numpy(depth), c["scale_factor"])
        assert all(not t.is_cuda for t in got) and got[0].shape == (3,) + depth.shape and got[2].shape == depth.shape
        check_floats(tuple(t[None] for t in got), want, c["id"] + "/host")
        check_case(z, meta, c, got[2].numpy(), io.codes(got[0].numpy()), io.codes(got[1].numpy()))


@pytest.mark.parametrize("w", FUZZ_WIDTHS)
def test_fuzz_against_the_restatement(w):
    assert FUZZ_WIDTHS[-1] <= _native.lib().cs_inpaint_prepare_max_width()
    rng = np.random.default_rng(2000 + w)
    for trial, h in enumerate([1, 2, 3, 5, int(rng.integers(6, 40))]):
        b = int(rng.integers(1, 4))
        img, depth = fuzz_inputs(rng, b, 3, h, w)   # block / noise / flat-row depths, 0..1 and 0..255 frames in one batch
        sf = float(rng.choice([-1, 1]) * rng.choice([0.3, 2.0, 5.0, 12.0]) * rng.random())
        thr = float(rng.choice([0.05, 0.05, 0.0, 0.2]))
        want = io.prepare(img, depth, sf, thr)
        got = engine.inpaint_prepare(cuda(img), cuda(depth), sf, thr, codes=True)
        where = (w, trial, b, h, sf, thr)
        check_floats(got[:3], want, where)
        # codes: of the kernel's own floats by the reference's expression, and of the restatement's
        assert np.array_equal(got[3].cpu().numpy(), io.codes(got[0].cpu().numpy())), where
        assert np.array_equal(got[4].cpu().numpy(), io.codes(got[1].cpu().numpy())), where
        assert np.array_equal(got[3].cpu().numpy(), io.codes(want[0])) and np.array_equal(got[4].cpu().numpy(), io.codes(want[1])), where


def small_batch():
    """Four 48 x 160 frames: a disc (masked on both of its sides), a flat depth, fully masked rows, frame edges on the 0..1 scale."""
    z, meta = load()
    by = {c["id"]: c for c in meta["cases"]}
    h, w = 48, 160
    imgs = np.stack([case_inputs(z, meta, by[k])[0][:, :h, :w] for k in ("disc_p5", "flat_0", "band_p5", "edges_p8")])
    deps = np.stack([io.depth_u8(kind, h, w, seed).astype(np.float32) for kind, seed in (("disc", 5), ("flat", 0), ("band", 6), ("edges", 0))])
    deps[3] /= np.float32(255.0)
    return imgs, deps


def test_a_batch_equals_its_frames_bit_for_bit():
    imgs, deps = small_batch()
    I, D = cuda(imgs), cuda(deps)
    for sf in (6.0, -6.0):
        batch = engine.inpaint_prepare(I, D, sf, codes=True)
        want = io.prepare(imgs, deps, sf)
        check_floats(batch[:3], want, ("batch", sf))
        assert want[2][0].any() and want[2][3].any()
        for k in range(imgs.shape[0]):
            one = engine.inpaint_prepare(I[k:k + 1], D[k:k + 1], sf, codes=True)
            for a, b in zip(batch, one):
                assert torch.equal(a[k], b[0]), ("frame", k, sf)


def ramp_batch():
    """small_batch() with frame 1 replaced by a depth that falls smoothly from near on the left to far on the right: at a
    positive scale factor the frame is squeezed, no source x leaves [-1, 1] and no step is deep enough to disocclude."""
    imgs, deps = small_batch()
    w = deps.shape[-1]
    deps[1] = np.broadcast_to(255 - (np.arange(w) * 255) // (w - 1), deps[1].shape).astype(np.float32)
    return imgs, deps


def test_an_empty_mask_inside_a_batch_and_fully_masked_rows():
    imgs, deps = ramp_batch()
    want = io.prepare(imgs, deps, 6.0)
    assert not want[2][1].any() and all(want[2][k].any() for k in (0, 2, 3))   # an empty mask between non-empty ones
    wr, fl, m = engine.inpaint_prepare(cuda(imgs), cuda(deps), 6.0)
    check_floats((wr, fl, m), want, "ramp")
    wr, fl, m = wr.cpu().numpy(), fl.cpu().numpy(), m.cpu().numpy()
    assert not m[1].any() and np.array_equal(fl[1], wr[1])   # the reference's early return: filled == warped
    # fully masked rows (frame 2's band) come out black in filled; warped keeps its colours there
    full = m[2].all(1)
    assert full.any() and not fl[2][:, full].any() and wr[2][:, full].any()
    # a scale factor of 0 moves nothing: every mask empty
    wr0, fl0, m0 = engine.inpaint_prepare(cuda(imgs), cuda(deps), 0.0)
    assert not m0.any() and torch.equal(fl0, wr0)
    check_floats((wr0, fl0, m0), io.prepare(imgs, deps, 0.0), "zero")


def test_noncontiguous_and_host_inputs():
    rng = np.random.default_rng(8)
    img, depth = fuzz_inputs(rng, 2, 3, 9, 70)
    want = io.prepare(img, depth, 7.0)
    host = sdn.prepare_inpaint(torch.from_numpy(img), torch.from_numpy(depth), 7.0)
    assert all(not t.is_cuda for t in host)
    cl = cuda(img.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2)
    dt = cuda(depth.transpose(0, 2, 1)).transpose(1, 2)
    assert not cl.is_contiguous() and not dt.is_contiguous()
    view = sdn.prepare_inpaint(cl, dt, 7.0)
    assert all(t.is_cuda for t in view)
    mixed = sdn.prepare_inpaint(cuda(img), torch.from_numpy(depth).double(), 7.0)   # device image, host float64 depth
    assert all(t.is_cuda for t in mixed)
    for got, name in ((host, "host"), (view, "views"), (mixed, "mixed")):
        check_floats(got, want, name)
    one = sdn.prepare_inpaint(cuda(img[1]), cuda(depth[1]), 7.0)
    assert one[0].shape == (3, 9, 70) and one[2].shape == (9, 70)
    check_floats(tuple(t[None] for t in one), tuple(a[1:2] for a in want), "single")
    with pytest.raises(ValueError):
        engine.inpaint_prepare(cuda(img), cuda(depth[:, :, :69]), 7.0)
    with pytest.raises(ValueError):
        engine.inpaint_prepare(cuda(img[:, :2]), cuda(depth), 7.0)


def test_compose_stereo_against_numpy():
    rng = np.random.default_rng(9)
    img, depth = fuzz_inputs(rng, 2, 3, 12, 64)
    img = (np.floor(img * 256).clip(0, 255) / np.float32(255.0)).astype(np.float32)   # k / 255
    wr, fl, m, wu8, fu8 = engine.inpaint_prepare(cuda(img), cuda(depth), 9.0, codes=True)
    left = cuda(np.rint(img.transpose(0, 2, 3, 1) * 255).astype(np.uint8))
    inpainted = cuda(rng.integers(0, 256, (2, 12, 64, 3)).astype(np.uint8))
    stereo, l, r = sdn.compose_stereo(left, wu8, inpainted, m)
    assert stereo.is_cuda and stereo.dtype == torch.uint8
    mn = m.cpu().numpy()
    assert mn.any() and not mn.all()
    right = np.stack([io.blend(mn[k], inpainted[k].cpu().numpy(), wu8[k].cpu().numpy()) for k in range(2)])
    assert np.array_equal(r.cpu().numpy(), right) and torch.equal(l, left)
    assert np.array_equal(stereo.cpu().numpy(), np.concatenate([left.cpu().numpy(), right], axis=2))


def test_one_column_above_the_width_limit_is_refused():
    L = _native.lib()
    wmax = L.cs_inpaint_prepare_max_width()
    assert wmax >= 8192
    I, D = torch.rand(1, 3, 1, wmax + 1).cuda(), torch.rand(1, 1, wmax + 1).cuda()
    with pytest.raises(_native.NativeError) as ei:
        engine.inpaint_prepare(I, D, 5.0)
    assert ei.value.code == _native.CS_ELIMIT
    # the widest accepted frame works
    rng = np.random.default_rng(10)
    img, depth = fuzz_inputs(rng, 1, 3, 4, wmax)
    check_floats(engine.inpaint_prepare(cuda(img), cuda(depth), 3.0), io.prepare(img, depth, 3.0), "wmax")
