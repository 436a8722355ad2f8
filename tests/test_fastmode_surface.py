"""StereoDiffusion's Fast mode at any frame size (cs_pil_resize, stereodiffusion_nodes.pil_resize and generate_stereo_fast): the
public surface, the host-side argument validation, and the numpy restatement the GPU tests check the kernels against
(tools/pil_resize_oracle.py) held to Pillow itself and to the reference's own outputs in tests/golden/fast_mode.npz, on the CPU
(not gpu).  Every comparison is byte for byte."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import inpaint_oracle as io
import make_fastmode_goldens as mg
import pil_resize_oracle as po
from comfystereo_amd import _native, engine
from comfystereo_amd import stereodiffusion_nodes as sdn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["cs_pil_resize_workspace_bytes", "cs_pil_resize_max_taps", "cs_pil_resize"]
# (H, W) the issue lists for the fixture
SIZES = [(270, 480), (600, 800), (301, 777), (768, 432), (17, 23), (512, 512), (1080, 1920), (2160, 3840)]


def load():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fast_mode.npz"))
    return z, json.loads(str(z["meta"]))


def invert(filled_u8, mask=None, k=None):
    """The stand-in for the model the fixture was recorded with: 255 - image."""
    return 255 - filled_u8


def check_case(z, c, left, right, stereo=None, mask=None, filled_u8=None, depth512=None):
    """The reference's observables of case c against uint8 code arrays (left, right [H,W,3]; stereo [H,2W,3])."""
    cid = c["id"]
    for name, a in (("left", left), ("right", right)):
        assert a.shape == (c["h"], c["w"], 3) and a.dtype == np.uint8, (cid, name)
        bad = int((a[c["rows"]] != z[f"{cid}/{name}_rows"]).sum())
        print(cid, name, "mismatching bytes in the stored rows", bad)
        assert bad == 0, (cid, name, bad)
        assert io.digest(a) == c[f"sha_{name}"], (cid, name, "digest")
    if stereo is not None:
        assert io.digest(stereo) == c["sha_stereo"], (cid, "stereo digest")
    if depth512 is not None:
        assert np.array_equal(depth512, z[f"{cid}/depth512"]), (cid, "depth512")
    if mask is not None:
        want = (np.unpackbits(z[f"{cid}/mask"], count=512 * 512).reshape(512, 512).astype(bool) if c["called"]
                else np.zeros((512, 512), dtype=bool))
        assert np.array_equal(mask, want), (cid, "mask")
    if filled_u8 is not None and c["called"]:
        assert np.array_equal(filled_u8[c["rows512"]], z[f"{cid}/filled_rows"]), (cid, "filled rows")
        assert io.digest(filled_u8) == c["sha_filled"], (cid, "filled digest")


def test_new_exports_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    declared = set(re.findall(r"CS_API\s+[\w\s\*]+?\b(cs_\w+)\s*\(", hdr))
    L = _native.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _native.EXPORTS, name
        assert hasattr(L, name), name
    assert L.cs_version() == 4 == _native.ABI_VERSION
    for flag, value in re.findall(r"CS_PIL_(\w+) = (\d+)", hdr):
        assert _native.PIL_FLAG[flag.lower()] == int(value), flag
    assert len(_native.PIL_FLAG) == 3
    assert L.cs_pil_resize_max_taps() == 257


def test_python_signatures_and_docs():
    assert str(inspect.signature(engine.pil_resize)) == "(x, size, gray=False, f32=None, codes=True, f32_out=None)"
    assert str(inspect.signature(sdn.pil_resize)) == "(image_u8, size)"
    assert str(inspect.signature(sdn.generate_stereo_fast)) == "(image, depth_map, scale_factor, inpaint, threshold=0.05)"
    doc = sdn.__doc__
    assert "generate_stereo_fast" in doc and "pil_resize" in doc
    out_of_scope = doc[doc.index("Out of scope"):]
    assert "resize" not in out_of_scope and "model" in out_of_scope   # the resizes are no longer left to the caller


def test_host_side_refusals():
    L = _native.lib()
    call = L.cs_pil_resize
    big = 1 << 40
    # distinct non-null host addresses, far enough apart not to overlap: every refusal below comes before device work
    src, u8, f32, ws = 1 << 20, 1 << 24, 1 << 28, 1 << 32
    ok_args = (1, 40, 50, 3, 20, 30)
    assert call(None, *ok_args, 0, u8, f32, 0, ws, big, None) == _native.CS_EINVAL
    assert call(src, *ok_args, 0, u8, f32, 0, None, big, None) == _native.CS_EINVAL
    for dims in ((0, 40, 50, 3, 20, 30), (1, 0, 50, 3, 20, 30), (1, 40, 0, 3, 20, 30), (1, 40, 50, 3, 0, 30), (1, 40, 50, 3, 20, 0),
                 (-1, 40, 50, 3, 20, 30), (1, 40, 50, 3, -20, 30)):
        assert call(src, *dims, 0, u8, f32, 0, ws, big, None) == _native.CS_EINVAL, dims
        assert L.cs_pil_resize_workspace_bytes(*dims) == 0
    for c in (0, 2, 4):
        assert call(src, 1, 40, 50, c, 20, 30, 0, u8, f32, 0, ws, big, None) == _native.CS_EINVAL, c
    assert call(src, 1, 40, 50, 1, 20, 30, _native.PIL_FLAG["gray"], u8, f32, 0, ws, big, None) == _native.CS_EINVAL
    assert call(src, *ok_args, 8, u8, f32, 0, ws, big, None) == _native.CS_EINVAL              # unknown flag
    assert call(src, *ok_args, 0, u8, f32, 30 * 3 - 1, ws, big, None) == _native.CS_EINVAL     # pitch below a row
    assert call(src, *ok_args, 0, u8, f32 + 2, 0, ws, big, None) == _native.CS_EINVAL          # misaligned floats
    assert call(src + 2, *ok_args, _native.PIL_FLAG["in_f32"], u8, f32, 0, ws, big, None) == _native.CS_EINVAL
    # aliasing
    assert call(src, *ok_args, 0, src, f32, 0, ws, big, None) == _native.CS_EINVAL
    assert b"overlap" in L.cs_last_error()
    assert call(src, *ok_args, 0, src + 40 * 50 * 3 - 1, f32, 0, ws, big, None) == _native.CS_EINVAL
    assert call(src, *ok_args, 0, u8, src, 0, ws, big, None) == _native.CS_EINVAL
    assert call(src, *ok_args, 0, u8, u8, 0, ws, big, None) == _native.CS_EINVAL
    assert call(src, *ok_args, 0, u8, f32, 0, src, big, None) == _native.CS_EINVAL
    assert call(src, *ok_args, 0, ws, f32, 0, ws, big, None) == _native.CS_EINVAL
    # limits
    assert call(src, 65536, 4, 5, 3, 2, 3, 0, u8, f32, 0, ws, big, None) == _native.CS_ELIMIT
    assert call(src, 1, 65536, 5, 1, 65536, 3, 0, u8, None, 0, ws, big, None) == _native.CS_ELIMIT
    assert call(src, 1, 4, 5, 1, 4, 65536, 0, u8, None, 0, ws, big, None) == _native.CS_ELIMIT
    assert call(src, 1, 4, 6500, 1, 4, 100, 0, u8, None, 0, ws, big, None) == _native.CS_ELIMIT     # a factor of 65
    assert b"cs_pil_resize_max_taps" in L.cs_last_error()
    assert call(src, 1, 6500, 4, 1, 100, 4, 0, u8, None, 0, ws, big, None) == _native.CS_ELIMIT
    # workspace
    need = L.cs_pil_resize_workspace_bytes(*ok_args)
    assert need >= 40 * 30 * 3 and L.cs_pil_resize_workspace_bytes(1, 4, 6500, 1, 4, 100) == 0
    assert call(src, *ok_args, 0, u8, f32, 0, ws, need - 1, None) == _native.CS_EWORKSPACE
    # nothing asked for: nothing done
    assert call(src, *ok_args, 0, None, None, 0, ws, big, None) == _native.CS_OK


def test_python_entry_points_raise_without_a_device():
    u8 = torch.zeros(2, 4, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        engine.pil_resize(u8, (5, 5))                        # host tensor: the engine takes device tensors only
    for bad in (u8.float(), u8.numpy(), torch.zeros(8, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            sdn.pil_resize(bad, (5, 5))
    for size in ((0, 5), (5, -1), (5,)):
        with pytest.raises(ValueError):
            sdn.pil_resize(u8, size)
    with pytest.raises(ValueError):
        engine.pil_resize(u8, (5, 5), f32="nchw")
    with pytest.raises(ValueError):
        engine.pil_resize(u8[..., :1], (5, 5), gray=True)
    with pytest.raises(ValueError):
        engine.pil_resize(u8, (5, 5), codes=False)
    img, dep = torch.zeros(2, 4, 8, 3), torch.zeros(2, 4, 8)
    for args in ((img.numpy(), dep, 5.0, invert), (img, dep, 5.0, None), (img[0], dep[0], 5.0, invert), (img, dep[:1], 5.0, invert),
                 (img.to(torch.uint8), dep, 5.0, invert), (img, torch.zeros(2, 4, 8, 2), 5.0, invert)):
        with pytest.raises(ValueError):
            sdn.generate_stereo_fast(*args)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sdn.pil_resize(u8, (5, 5))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sdn.generate_stereo_fast(img, dep, 5.0, invert)


def test_restatement_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    total = 0
    for h, w in SIZES + [(64, 512), (1, 1), (2, 3)]:
        for c in (3, 1):
            for kind in ("random", "saturated"):
                if h * w > 1 << 20 and (c == 1 or kind == "saturated") and (h, w) != (1080, 1920):
                    continue   # (4K: RGB noise only, to keep the run short)
                a = rng.integers(0, 256, (h, w, c)).astype(np.uint8) if kind == "random" else \
                    (rng.integers(0, 2, (h, w, c)) * 255).astype(np.uint8)
                down = po.resize_hw(a, 512, 512)
                pil = lambda x, size: np.array(Image.fromarray(x if c == 3 else x[..., 0]).resize(size)).reshape(size[1], size[0], c)
                assert np.array_equal(down, pil(a, (512, 512))), (h, w, c, kind, "to 512")
                assert np.array_equal(po.resize(down, (w, h)), pil(down, (w, h))), (h, w, c, kind, "back")
                total += 2 * (down.size + h * w * c)
    assert np.array_equal(po.resize_hw(a, 2, 3), a)   # equal sizes: a copy
    print("bytes compared with Pillow:", total)


def test_gray_rule_on_equal_channels_and_tap_sums():
    k = np.arange(256, dtype=np.uint8)
    assert np.array_equal(po.gray_codes(np.stack([k, k, k], -1)), np.maximum(k.astype(int) - 1, 0))
    for n_in, n_out in ((3840, 512), (512, 3840), (777, 512), (23, 512), (512, 17), (1, 4), (4, 1)):
        xmin, count, taps = po.axis_taps(n_in, n_out)
        assert (count >= 1).all() and (xmin >= 0).all() and (xmin + count <= n_in).all()
        assert np.abs(taps.sum(1) - (1 << 22)).max() <= taps.shape[1]   # normalised, up to the rounding of each tap
        assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + count) >= 0).all()   # windows only move right


def test_restatement_reproduces_every_fixture_case():
    z, meta = load()
    cases = meta["cases"]
    assert sorted({(c["h"], c["w"]) for c in cases}) == sorted(SIZES)
    assert any(c["scale_factor"] > 0 and c["called"] for c in cases) and any(c["scale_factor"] < 0 and c["called"] for c in cases)
    assert sum(not c["called"] for c in cases) == 1 and any(c["coloured"] for c in cases)
    assert set(meta["versions"]) == {"pillow", "numpy", "torch"}
    for c in cases:
        img, dep = mg.inputs(c)
        r = po.fast_mode_frame(img, dep, c["scale_factor"], invert)
        assert r["called"] == c["called"], c["id"]
        check_case(z, c, r["left"], r["right"], np.hstack([r["left"], r["right"]]), r["mask"], r["filled_u8"], r["depth512"])


def test_identity_case_equals_the_old_fixture():
    z, meta = load()
    c = {c["id"]: c for c in meta["cases"]}["512x512_disc_p5"]
    old = np.load(os.path.join(ROOT, "tests", "golden", "inpaint_prep.npz"))
    old_c = {c["id"]: c for c in json.loads(str(old["meta"]))["cases"]}["disc_p5"]
    assert c["sha_filled"] == old_c["sha_filled"]
    assert np.array_equal(z["512x512_disc_p5/mask"], old["disc_p5/mask"])
    assert np.array_equal(z["512x512_disc_p5/depth512"], old["disc_p5/depth"])
