#!/usr/bin/env python3
"""Fixture of the front half of StereoDiffusion's Fast mode: tests/golden/inpaint_prep.npz.

Build-machine only, like tools/make_grid_goldens.py: loads the reference's stereodiffusion_nodes through tools/refload.py and
runs StereoDiffusionNode._generate_stereo_fast_single itself (CPU torch) on seeded 512 x 512 inputs, for which both of its PIL
resizes are identity copies.  The inpainting model is replaced by a recorder that keeps the `image` and `mask_image` it is
handed and returns one constant colour; nothing of the reference's arithmetic is replaced.  Observable per case: the pre-filled
image (`filled` codes), the mask, and -- through the returned right eye -- the `warped` codes outside the mask.

  python tools/make_inpaint_goldens.py
Layout: `meta` = JSON {rows, constant, cases: [{id, scale_factor, depth, image_seed, called, mask_share, sha_filled,
sha_right}]}; arrays 'cid/depth' (the gray uint8 depth the reference warps with), 'cid/mask' (np.packbits), 'cid/filled_rows',
'cid/right_rows' (uint8 [rows, W, 3]).  Images are regenerated from their seeds (inpaint_oracle.image_u8).  A case the reference
returns early from (empty mask: the model is never called) has only the right eye.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import inpaint_oracle as io  # noqa: E402
import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "inpaint_prep.npz")
S = 512
ROWS = [0, 1, 64, 66, 96, 200, 255, 256, 357, 510, 511]
CONSTANT = (7, 130, 251)   # the recorder's "inpainted" colour

# (id, depth kind, depth seed, image seed, scale factor)
CASES = [
    ("disc_p5", "disc", 11, 21, 5.0),
    ("disc_m5", "disc", 12, 22, -5.0),
    ("disc_p03", "disc", 13, 23, 0.3),
    # a flat depth shifts the whole frame by half the divergence: the columns that leave the frame are masked ...
    ("flat", "flat", 0, 24, 5.0),
    # ... and only a shift too small to move a grid value leaves the mask empty (the reference's early return)
    ("flat_0", "flat", 0, 29, 0.0),
    ("disc_tiny", "disc", 16, 30, 1e-6),
    ("edges_p8", "edges", 0, 25, 8.0),
    ("edges_m8", "edges", 0, 26, -8.0),
    ("band_p5", "band", 14, 27, 5.0),
    ("rgb_m3", "rgb", 15, 28, -3.0),
]


def depth_input(kind, seed):
    """The depth frame the node is handed, uint8 [S,S,3] (the reference's PIL step takes no other layout): three equal channels,
    or three different ones for kind 'rgb'.  Either way the reference warps with its own gray conversion of it."""
    if kind != "rgb":
        return np.repeat(io.depth_u8(kind, S, S, seed)[..., None], 3, -1)
    base = io.depth_u8("disc", S, S, seed).astype(np.int64)
    return np.stack([base, np.clip(base + 20, 0, 255), 255 - base // 2], -1).astype(np.uint8)


def as_node_tensor(u8):
    """uint8 -> the float tensor tensor_to_numpy maps back onto exactly these codes ((k + 0.5) / 255: safe under truncation)."""
    return torch.from_numpy((u8.astype(np.float32) + np.float32(0.5)) / np.float32(255.0))


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, prompt, image, mask_image, **kw):
        self.calls.append((np.array(image), np.array(mask_image)))
        from PIL import Image
        return types.SimpleNamespace(images=[Image.fromarray(np.broadcast_to(np.array(CONSTANT, np.uint8), (S, S, 3)).copy())])


def main():
    refload.quiet()
    mod = refload.load_sd_nodes()
    fn = mod.StereoDiffusionNode._generate_stereo_fast_single
    arrays, cases = {}, []
    for cid, kind, dseed, iseed, sf in CASES:
        dep_in = depth_input(kind, dseed)
        img = io.image_u8(S, S, iseed)
        rec = Recorder()
        _, left, right = fn(None, as_node_tensor(img), as_node_tensor(dep_in), sf, 0.5, 4, 1.0, rec, "", None, "cpu")
        assert np.array_equal(np.rint(left[0].numpy() * 255).astype(np.uint8), img), "the resizes are not identity copies"
        right = np.rint(right[0].numpy() * 255).astype(np.uint8)
        # the gray depth the reference warps with (its own conversion of an RGB depth frame, :419)
        gray = np.dot(dep_in[..., :3], [0.2989, 0.5870, 0.1140]).astype(np.uint8)
        arrays[f"{cid}/depth"] = gray
        arrays[f"{cid}/right_rows"] = right[ROWS]
        c = dict(id=cid, scale_factor=sf, depth=kind, image_seed=iseed, called=bool(rec.calls), sha_right=io.digest(right))
        if rec.calls:
            (filled, mask255), = rec.calls
            assert set(np.unique(mask255)) <= {0, 255}
            mask = mask255 > 0
            arrays[f"{cid}/mask"] = np.packbits(mask)
            arrays[f"{cid}/filled_rows"] = filled[ROWS]
            c.update(sha_filled=io.digest(filled), mask_share=float(mask.mean()), full_rows=int(mask.all(1).sum()),
                     edge_columns=[bool(mask[:, 0].any()), bool(mask[:, -1].any())])
        else:
            c.update(mask_share=0.0, full_rows=0, edge_columns=[False, False])
        cases.append(c)
        print(cid, {k: v for k, v in c.items() if k not in ("sha_right", "sha_filled")})
    by = {c["id"]: c for c in cases}
    assert not by["flat_0"]["called"] and not by["disc_tiny"]["called"] and by["band_p5"]["full_rows"] > 0
    assert all(by["edges_p8"]["edge_columns"]) and all(by["edges_m8"]["edge_columns"])
    np.savez_compressed(OUT, meta=json.dumps(dict(rows=ROWS, constant=list(CONSTANT), size=S, cases=cases)), **arrays)
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
