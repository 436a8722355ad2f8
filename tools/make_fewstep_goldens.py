"""Writes tests/golden/fewstep.npz: the outputs of tools/fewstep_oracle.py on the CPU for one step of the Euler and the LCM
sampler, over {float32, float16, bfloat16} x guidance on / off x 9 / 4 channels x the first, a middle and the last step of a 4-step
plan, on the seeded inputs of tools/fewstep_cases.py with their special values (+-0, +-inf, NaN, the largest finite value, the
smallest subnormal), and the coefficients and timesteps of that plan.

These are CPU torch results of this repository's own statement of the two published algorithms, NOT a capture of the reference
(which never wires its Euler scheduler and has no LCM sampler): the fixture pins the specification, so that a change of the
oracle's bits -- or of torch's CPU arithmetic under it -- shows as a diff.  tests/test_fewstep_surface.py regenerates it bit for
bit.

    python tools/make_fewstep_goldens.py [out.npz]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fewstep_cases as cases   # noqa: E402
import fewstep_oracle as oracle   # noqa: E402

N, HL, WL = 2, 5, 7


def raw(t):
    """The tensor's bits as a numpy integer array (bfloat16 has no numpy dtype)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]).numpy()


def build():
    arrays, meta = {}, {"note": "CPU torch results of tools/fewstep_oracle.py; not a reference capture", "shape": [N, HL, WL], "cases": [],
                        "timesteps": {}, "coeffs": {}}
    acp = oracle.alphas_cumprod()
    for sampler in oracle.SAMPLERS:
        ts = oracle.timesteps(sampler, cases.PLAN_STEPS)
        meta["timesteps"][sampler] = ts
        meta["coeffs"][sampler] = [list(oracle.coeffs(sampler, acp, ts, i)) for i in range(len(ts))]   # float32 values, exact in json
        seed = 0
        for dtype_name in cases.DTYPES:
            for cfg in (True, False):
                for channels in (9, 4):
                    for pos in cases.POSITIONS:
                        cid = f"{sampler}-{dtype_name}-{'cfg' if cfg else 'nocfg'}-c{channels}-{pos}"
                        c = cases.make(sampler, dtype_name, cfg, channels, pos, N, HL, WL, seed=seed, special=True)
                        out = cases.want(c)
                        for name in ("x", "state", "decode_in"):
                            if out[name] is not None:
                                arrays[f"{cid}/{name}"] = raw(out[name])
                        meta["cases"].append(dict(id=cid, sampler=sampler, dtype=dtype_name, cfg=cfg, channels=channels, pos=pos, seed=seed))
                        seed += 1
    arrays["meta"] = np.array(json.dumps(meta))
    return arrays


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fewstep.npz")
    np.savez_compressed(out, **build())
    print("wrote", out, os.path.getsize(out), "bytes")
