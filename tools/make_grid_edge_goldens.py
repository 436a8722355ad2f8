#!/usr/bin/env python3
"""tests/golden/grid_edges_nonfinite.npz: what the reference's grid-sample warps return on the CPU for the non-finite depth batches
of tools/grid_edge_inputs.py (NaN and infinite depth values).  Build-machine only, like tools/make_grid_goldens.py: loads the
reference through tools/refload.py.  Data only: the outputs as float32 / packed bool arrays, keyed '<batch>/<output>'.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import grid_edge_inputs as ge  # noqa: E402
import refload  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "grid_edges_nonfinite.npz")
T = torch.from_numpy


def main():
    refload.quiet()
    warnings.simplefilter("ignore")
    sig = refload.load_sig()
    arrays, meta = {}, []
    for k, kinds in enumerate(ge.NONFINITE_BATCHES):
        c = ge.nonfinite_depth_case(kinds)
        img, depth, args = c.inputs["image"], c.inputs["depth"], c.params["args"]
        arrays[f"b{k}/warp"] = sig.apply_stereo_divergence_gpu(T(img), T(depth), *args).numpy()
        wr, mr = sig.warp_and_fill_gpu(T(img), T(depth), *args)
        arrays[f"b{k}/stretch"], arrays[f"b{k}/stretch_mask"] = wr.numpy(), np.packbits(mr.numpy())
        arrays[f"b{k}/mask"] = np.packbits(sig.compute_forward_mask_gpu(T(depth), *args, "cpu").numpy())
        fr = [sig.apply_stereo_divergence_gpu_with_fill(T(img[f]), T(depth[f]), *args, fill_mode="border") for f in range(img.shape[0])]
        arrays[f"b{k}/fill:border"] = np.stack([f[0].numpy() for f in fr])
        arrays[f"b{k}/valid:border"] = np.packbits(np.stack([f[1].numpy().reshape(depth.shape[1:]) for f in fr]))
        meta.append(dict(id=f"b{k}", kinds=list(kinds), shape=list(img.shape)))
    np.savez_compressed(OUT, meta=json.dumps(dict(batches=meta, torch=torch.__version__)), **arrays)
    print(OUT, "written:", len(arrays), "arrays")


if __name__ == "__main__":
    main()
