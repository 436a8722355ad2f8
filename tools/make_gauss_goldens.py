#!/usr/bin/env python3
"""Fixtures of the reference's Gaussian depth blurs: tests/golden/gauss_blur.npz and gauss_signatures.json.

Build-machine only, like tools/make_grid_goldens.py: loads the reference through tools/refload.py, runs blur_depth_map,
edge_selective_blur_depth_map, left_direction_aware_blur_depth_map and right_direction_aware_blur_depth_map on seeded float32
maps (tools/gauss_oracle.depth_map) and writes inputs, parameters and outputs as data.

  python tools/make_gauss_goldens.py
Layout: `meta` = JSON {cases: [{id, fn, input, sigma, edge_threshold}], inputs: {name: {kind, h, w, seed}}}; arrays 'in/<name>'
and '<case id>/out'.  A case whose reference output differs from the restatement (tools/gauss_oracle.py) stops the script:
the input is then replaced and the case noted in DESIGN.md, never the comparison loosened.
"""
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import gauss_oracle as go  # noqa: E402
import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FUNCS = ["blur_depth_map", "edge_selective_blur_depth_map", "left_direction_aware_blur_depth_map",
         "right_direction_aware_blur_depth_map"]
SIGMAS = [0.2, 0.4, 1, 2.5, 7, 20, 70]
THRESHOLDS = [0.5, 6, 40]

# name: (kind, h, w, seed)
INPUTS = {
    "codes": ("codes", 48, 72, 11),
    "unit": ("unit", 40, 56, 12),
    "noise": ("noise", 40, 56, 13),
    "ellipse": ("ellipse", 96, 160, 14),
    "flat": ("flat", 24, 40, 15),
    "one_row": ("codes", 1, 90, 16),
    "one_col": ("noise", 70, 1, 17),
    "tiny": ("codes", 5, 3, 18),      # radius above W and above H from sigma 2.5 on
}


def plan():
    """(case id, function, input, sigma, threshold): every function on every input; every sigma and every threshold on the
    8-bit codes; the other inputs walk through the sigmas and thresholds."""
    cases = []
    k = 0
    for name in INPUTS:
        sig = SIGMAS if name in ("codes", "tiny") else [SIGMAS[(k + i) % len(SIGMAS)] for i in (0, 3)]
        for s in sig:
            cases.append((f"blur_{name}_{s}", FUNCS[0], name, s, None))
        for i, fn in enumerate(FUNCS[1:]):
            ths = THRESHOLDS if name == "codes" else [THRESHOLDS[(k + i) % 3]]
            for t in ths:
                s = SIGMAS[(k + i + 2) % len(SIGMAS)]
                cases.append((f"{fn.split('_')[0]}_{name}_{s}_{t}", fn, name, s, t))
        k += 1
    # blurred maps as inputs of the blending functions (0..255 floats with long fractions) run through 'ellipse' above;
    # sigma <= 0 through the blending functions: depth blended with itself
    cases.append(("edge_codes_zero_sigma", FUNCS[1], "codes", 0, 6))
    cases.append(("left_unit_negative_sigma", FUNCS[2], "unit", -1.5, 0.5))
    return cases


def main():
    refload.quiet()
    sig = refload.load_sig()
    sigs = {f: str(inspect.signature(getattr(sig, f))) for f in FUNCS}
    with open(os.path.join(OUT, "gauss_signatures.json"), "w") as fh:
        json.dump(sigs, fh, indent=1)
        fh.write("\n")
    arrays, cases = {}, []
    inputs = {name: go.depth_map(*spec) for name, spec in INPUTS.items()}
    for name, d in inputs.items():
        arrays[f"in/{name}"] = d
    for cid, fn, name, s, t in plan():
        d = inputs[name]
        args = (d.copy(), s) if t is None else (d.copy(), s, t)
        want = getattr(sig, fn)(*args)
        assert want.dtype == np.float32 and want.shape == d.shape, (cid, want.dtype, want.shape)
        got = getattr(go, fn)(*args)
        same = np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert same, f"{cid}: the restatement differs from the reference at {int((got.view(np.uint32) != want.view(np.uint32)).sum())} values"
        arrays[f"{cid}/out"] = want
        cases.append(dict(id=cid, fn=fn, input=name, sigma=s, edge_threshold=t))
    meta = dict(cases=cases, inputs={n: dict(kind=k, h=h, w=w, seed=sd) for n, (k, h, w, sd) in INPUTS.items()},
                numpy=np.__version__)
    path = os.path.join(OUT, "gauss_blur.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    print("gauss_blur.npz:", len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
