#!/usr/bin/env python3
"""Fixture of the whole of StereoDiffusion's Fast mode around its model, at frame sizes other than 512 x 512:
tests/golden/fast_mode.npz.

Build-machine only, like tools/make_inpaint_goldens.py: loads the reference's stereodiffusion_nodes through tools/refload.py and
runs StereoDiffusionNode._generate_stereo_fast_single itself (CPU torch, Pillow) on seeded inputs.  The inpainting model is
replaced by a recorder that keeps the `image` and `mask_image` it is handed and returns 255 - image, so the blended right eye
depends on the pre-fill and the resize back works on non-constant data; nothing of the reference's arithmetic is replaced.

  python tools/make_fastmode_goldens.py
Layout: `meta` = JSON {work, versions, cases: [{id, h, w, depth, depth_seed, image_seed, scale_factor, coloured, called, rows,
rows512, mask_share, sha_left, sha_right, sha_stereo, sha_filled, sha_mask, sha_depth512}]}; arrays 'cid/depth512' (the gray
uint8 depth after the resize, by Pillow: what the reference warps with), 'cid/mask' (np.packbits), 'cid/filled_rows' (the
recorder's input, uint8 [rows512, 512, 3]), 'cid/left_rows', 'cid/right_rows' (uint8 codes [rows, W, 3] of the returned eyes,
whose floats are code / 255).  Inputs are regenerated from their seeds (inputs() below is imported by the tests).
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import inpaint_oracle as io  # noqa: E402
import pil_resize_oracle as po  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fast_mode.npz")
S = 512
ROWS512 = [0, 1, 96, 255, 256, 357, 511]

# (id, H, W, depth kind, depth seed, image seed, scale factor, coloured depth)
CASES = [
    ("270x480_disc_p5", 270, 480, "disc", 31, 41, 5.0, False),
    ("600x800_edges_m8", 600, 800, "edges", 0, 42, -8.0, False),
    ("301x777_band_p5", 301, 777, "band", 33, 43, 5.0, False),
    ("768x432_disc_m5", 768, 432, "disc", 34, 44, -5.0, False),
    ("17x23_disc_p5", 17, 23, "disc", 35, 45, 5.0, False),
    ("17x23_rgb_m3", 17, 23, "disc", 36, 46, -3.0, True),
    ("512x512_disc_p5", 512, 512, "disc", 11, 21, 5.0, False),    # inpaint_prep.npz's disc_p5: both resizes are copies
    ("270x480_flat_0", 270, 480, "flat", 0, 47, 0.0, False),      # an empty mask: the early return
    ("1080x1920_disc_p5", 1080, 1920, "disc", 38, 48, 5.0, False),
    ("2160x3840_edges_m5", 2160, 3840, "edges", 0, 49, -5.0, False),
]


def rows_of(h):
    return sorted({0, 1, h // 3, h // 2, h - 2, h - 1} & set(range(h)))


def image_u8(h, w, seed):
    """Seeded colours with structure at every scale (noise alone resizes to flat gray): blocks of 1, 8 and 64 pixels mixed.
    At the working size itself: inpaint_oracle.image_u8, the images of inpaint_prep.npz (the cross-check with that fixture)."""
    if (h, w) == (S, S):
        return io.image_u8(h, w, seed)
    rng = np.random.default_rng(seed)
    out = np.zeros((h, w, 3), dtype=np.int64)
    for step, weight in ((64, 2), (8, 1), (1, 1)):
        g = rng.integers(0, 256, ((h + step - 1) // step, (w + step - 1) // step, 3))
        out += weight * np.repeat(np.repeat(g, step, 0), step, 1)[:h, :w]
    return (out // 4).astype(np.uint8)


def depth_input(kind, h, w, seed, coloured):
    """uint8 [h,w,3]: three equal channels, or three different ones."""
    base = io.depth_u8(kind, h, w, seed)
    if not coloured:
        return np.repeat(base[..., None], 3, -1)
    b = base.astype(np.int64)
    return np.stack([b, np.clip(b + 20, 0, 255), 255 - b // 2], -1).astype(np.uint8)


def node_floats(u8):
    """uint8 -> the float32 array tensor_to_numpy maps back onto exactly these codes ((k + 0.5) / 255: safe under truncation)."""
    return (u8.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)


def inputs(case):
    """(image float32 [H,W,3], depth float32 [H,W,3]) of a case dict or CASES tuple, as the node is handed them."""
    if isinstance(case, dict):
        h, w, kind, dseed, iseed, col = (case[k] for k in ("h", "w", "depth", "depth_seed", "image_seed", "coloured"))
    else:
        _, h, w, kind, dseed, iseed, _, col = case
    return node_floats(image_u8(h, w, iseed)), node_floats(depth_input(kind, h, w, dseed, col))


def codes(t):
    """The uint8 codes of a returned float tensor [1,H,W,3] (code / 255); asserted to be exactly that."""
    a = t[0].numpy()
    u8 = np.rint(a * 255).astype(np.uint8)
    assert a.dtype == np.float32 and np.array_equal(u8.astype(np.float32) / np.float32(255.0), a)
    return u8


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, prompt, image, mask_image, **kw):
        from PIL import Image
        self.calls.append((np.array(image), np.array(mask_image)))
        return types.SimpleNamespace(images=[Image.fromarray(255 - np.array(image))])


def main():
    import PIL
    import torch
    from PIL import Image
    import refload
    refload.quiet()
    mod = refload.load_sd_nodes()
    fn = mod.StereoDiffusionNode._generate_stereo_fast_single
    old = np.load(os.path.join(ROOT, "tests", "golden", "inpaint_prep.npz"))
    old_meta = {c["id"]: c for c in json.loads(str(old["meta"]))["cases"]}
    arrays, cases = {}, []
    for case in CASES:
        cid, h, w, kind, dseed, iseed, sf, col = case
        img, dep = inputs(case)
        rec = Recorder()
        stereo, left, right = fn(None, torch.from_numpy(img), torch.from_numpy(dep), sf, 0.5, 4, 1.0, rec, "", None, "cpu")
        stereo, left, right = codes(stereo), codes(left), codes(right)
        assert left.shape == (h, w, 3) and np.array_equal(stereo, np.hstack([left, right]))
        dep_u8 = depth_input(kind, h, w, dseed, col)
        assert np.array_equal(po.float_codes(dep), dep_u8) and np.array_equal(po.float_codes(img), image_u8(h, w, iseed))
        ref_gray = np.dot(dep_u8[..., :3], [0.2989, 0.5870, 0.1140]).astype(np.uint8)   # the reference's expression (:419)
        # the gray rule of this project must agree with the reference's BLAS product on every pixel of a committed case
        assert np.array_equal(ref_gray, po.gray_codes(dep_u8)), (cid, "gray: pick another seed")
        depth512 = np.array(Image.fromarray(ref_gray).resize((S, S)))
        rows = rows_of(h)
        arrays[f"{cid}/depth512"] = depth512
        arrays[f"{cid}/left_rows"] = left[rows]
        arrays[f"{cid}/right_rows"] = right[rows]
        c = dict(id=cid, h=h, w=w, depth=kind, depth_seed=dseed, image_seed=iseed, scale_factor=sf, coloured=col,
                 called=bool(rec.calls), rows=rows, rows512=ROWS512, sha_left=io.digest(left), sha_right=io.digest(right),
                 sha_stereo=io.digest(stereo), sha_depth512=io.digest(depth512))
        if rec.calls:
            (filled, mask255), = rec.calls
            assert set(np.unique(mask255)) <= {0, 255} and filled.shape == (S, S, 3)
            mask = mask255 > 0
            arrays[f"{cid}/mask"] = np.packbits(mask)
            arrays[f"{cid}/filled_rows"] = filled[ROWS512]
            c.update(sha_filled=io.digest(filled), sha_mask=io.digest(mask), mask_share=float(mask.mean()))
        else:
            c.update(mask_share=0.0)
        cases.append(c)
        print(cid, {k: v for k, v in c.items() if not k.startswith("sha_") and not k.startswith("rows")})
    by = {c["id"]: c for c in cases}
    assert not by["270x480_flat_0"]["called"] and all(c["called"] for c in cases if c["id"] != "270x480_flat_0")
    assert any(c["coloured"] for c in cases)
    # the identity case is the old fixture's disc_p5, seen through the recorder of this one
    assert by["512x512_disc_p5"]["sha_filled"] == old_meta["disc_p5"]["sha_filled"]
    versions = dict(pillow=PIL.__version__, numpy=np.__version__, torch=torch.__version__)
    np.savez_compressed(OUT, meta=json.dumps(dict(work=S, versions=versions, cases=cases)), **arrays)
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
