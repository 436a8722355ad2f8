"""Quantised smooth depth with object silhouettes (tools/synth.scene8: an 8-bit gradient + flat ellipses, the kind of depth map the
reference's own fixture maker draws, /root/reference/create_test_images.py:3-77, and real estimators deliver) through the HIP path:
the reference node's outputs (tests/golden/scene8.npz, tools/make_goldens.py --only-scene8), the 1080p digests, and 4K-wide bands of
every technique against the oracle.  VERDICT r5 item 5.  -m gpu."""
import hashlib

import numpy as np
import pytest
import torch

import synth
from conftest import assert_warp_colours, scene8_case_expected, scene8_case_inputs
from oracle import node_oracle

pytestmark = pytest.mark.gpu
NAMES = ("stereoscope", "depth_left", "depth_right", "mask")
UI = {v: k for k, v in node_oracle.FILL_KEYS.items()}


@pytest.fixture(scope="module")
def engine():
    from comfystereo_amd import engine as e
    assert torch.cuda.is_available()
    return e


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_scene8_fixtures_of_the_reference_node(engine, golden_scene8):
    g = golden_scene8
    for case in g.meta["cases"]:
        img, depth = scene8_case_inputs(g, case)
        got = [t.cpu().numpy() for t in engine.generate(cuda(img), cuda(depth), case["divergence"], case["separation"], case["mode"],
                                                        case["balance"], case["convergence"], case["exponent"], case["fill"],
                                                        case["edge_threshold"], case["strength"], case["blur"], **case["kw"])]
        want = scene8_case_expected(g, case)
        cid = case["id"]
        if case["fill"] == "gpu_warp":   # (the fixture keeps every 8th row of the float32 colours)
            assert np.array_equal(got[3], want[3]), cid
            w, rs = img.shape[2], case["row_step"]
            for half, sl in (("L", slice(0, w)), ("R", slice(w, 2 * w))):
                assert_warp_colours(got[0][:, ::rs, sl], want[0][:, :, sl], want[3][:, ::rs] > 0, f"{cid}/{half}", channel_axis=3)
        else:
            assert np.array_equal(got[0], want[0]), cid
            assert np.array_equal(got[3], want[3]), cid
        assert np.array_equal(got[1][..., 0], want[1]) and np.array_equal(got[2][..., 0], want[2]), cid


def test_scene8_1080p_digests_of_the_reference(engine, golden_scene8):
    c = golden_scene8.meta["digest_1080p"]
    img = synth.image_u8(c["h"], c["w"], seed=c["image_seed"], hazards=False)[None].astype(np.float32) / np.float32(255.0)
    depth = synth.depth_batch(c["kind"], 1, c["h"], c["w"], channels=3)
    got = [t.cpu().numpy() for t in engine.generate(cuda(img), cuda(depth), c["divergence"], 0.0, c["mode"], 0.0, 0.5, 2.0, "polylines_soft",
                                                    20.0, 20.0, c["blur"], depth_blur_falloff=2.0, depth_blur_vert_smooth=6, batch_size=12)]
    k = [np.round(a * 255.0).astype(np.uint8) for a in (got[0], got[1][..., 0], got[2][..., 0])]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    assert sha(k[0]) == c["stereo_u8"] and sha(k[1]) == c["dl_u8"] and sha(k[2]) == c["dr_u8"]
    assert sha(np.packbits(got[3].astype(bool))) == c["mask"] and int(got[3].sum()) == c["mask_sum"]


@pytest.mark.parametrize("fill", ["none", "naive", "naive_interpolating", "inverse", "polylines_soft", "polylines_sharp", "hybrid_edge", "gpu_warp"])
@pytest.mark.parametrize("blur", [False, True])
def test_scene8_4k_wide_bands_vs_oracle(engine, fill, blur):
    """Every technique on 3840-wide bands of scene8 depth (cut where the three ellipses and their rims lie), divergence 8 as in the
    metric, blur off and on (the band is high enough for the vertical smoothing), SBS: the oracle's bits (gpu_warp: mask exact, colours
    within 2e-6 of the oracle, depth maps exact)."""
    n, h, w = 2, 72, 3840
    img = synth.image_f32(n, h, w, seed=61)
    full = [synth.scene8(2160, w, seed=s, soften=bool(s & 1)) for s in range(n)]
    depth = np.stack([f[y0:y0 + h] for f, y0 in zip(full, (760, 1480))])[..., None].repeat(3, -1)
    args = (8.0, 0.0, "left-right", 0.0, 0.5, 2.0)
    kw = dict(depth_blur_falloff=2.0, depth_blur_vert_smooth=6, batch_size=12)
    want = node_oracle.generate(img, depth, *args, UI[fill], 20.0, 20.0, blur, **kw)
    got = [t.cpu().numpy() for t in engine.generate(cuda(img), cuda(depth), *args, fill, 20.0, 20.0, blur, **kw)]
    if fill == "gpu_warp":
        assert np.array_equal(got[3], want[3])
        for half, sl in (("L", slice(0, w)), ("R", slice(w, 2 * w))):
            assert np.abs(got[0][:, :, sl] - want[0][:, :, sl]).max() <= 2e-6, half
    else:
        for g_, w_, name in zip(got, want, NAMES):
            assert np.array_equal(g_, w_), (fill, blur, name)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("fill", ["polylines_sharp", "polylines_soft"])
def test_second_tier_of_the_point_kernel_on_soft_silhouettes(engine, dev_switch, fill):
    """Round 6: the rows k_polypoint flags go through k_polypoint_listed -- the same tile function with PP_DCAP2 = 192 instead of 160
    slots for pixels under reversed segments and longer per-pixel lists (8 points / 12 segments sharp, 6 / 9 soft) -- before the row
    kernel (polylines_sharp by default; cs_debug_set pt_variant soft_point_tier2 forces it for soft, no_point_tier2 switches it off).
    Softened silhouettes at divergence 8 overflow the first tier's lists in many rows: with the second tier fewer rows reach the
    row kernel, and all three settings give the oracle's bits."""
    n, h, w = 2, 64, 3840
    img = synth.image_f32(n, h, w, seed=71)
    depth = np.stack([synth.scene8(2160, w, seed=s, soften=True)[y0:y0 + h] for s, y0 in ((2, 700), (5, 1500))])[..., None].repeat(3, -1)
    want = node_oracle.generate(img, depth, 8.0, 0.0, "left-right", 0.0, 0.5, 2.0, UI[fill], 20.0, 20.0, False, batch_size=12)
    p = engine.make_params(n, h, w, h, w, 3, fill, "left-right", 8.0, 0.0, 0.0, 0.5, 2.0, False, 20.0, 20.0, 1.0, 0, 12)
    redone = {}
    for variant in ("no_point_tier2", "soft_point_tier2", "default"):
        dev_switch("pt_variant", variant)
        plan = engine.Plan(p, torch.device("cuda"))
        got = [t.cpu().numpy() for t in plan.run(cuda(img), cuda(depth))]
        st = plan.stats()
        assert int(st[:, 9].sum()) == 0   # kernel error flags
        redone[variant] = int(st[:, 11].sum())
        for g_, w_, name in zip(got, want, NAMES):
            assert np.array_equal(g_, w_), (fill, variant, name)
    assert redone["no_point_tier2"] > 0, "no row was flagged: the test does not reach the second tier"
    assert redone["soft_point_tier2"] < redone["no_point_tier2"]
    assert redone["default"] == (redone["soft_point_tier2"] if fill == "polylines_sharp" else redone["no_point_tier2"])
