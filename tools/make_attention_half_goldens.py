#!/usr/bin/env python3
"""Fixture of the reference's stereo attention in float16 and bfloat16: tests/golden/bn_attention_half.npz.

Build-machine only, like tools/make_attention_goldens.py (whose loader, flavours and run_reference it uses): runs the
reference's BNAttention on CPU torch on the seeded inputs of tools/attention_half_oracle.case_inputs -- the float32 streams of
attention_oracle rounded to the dtype -- and writes the results as data.

  python tools/make_attention_half_goldens.py
Layout: `meta` = JSON {cases, sample, numpy, torch}; a case is one (shape, flavour, dtype).  The inputs are seeds.
  * value, sharp and plain cases: a seeded sample of at most SAMPLE output elements, `idx` (flat indices into
    [(c s b), n, (h d)]), `ref` (the reference in the case's dtype, stored as float32) and `ref64` (the same class on float64
    copies of the half-rounded inputs) at those indices, and e_ref = max |ref - ref64| over the WHOLE output: the reference's own
    half-precision error, the unit of the tests' bound.
  * routing cases: nothing but the seed and the gain.  The gain starts at attention_oracle's 1024 and is halved until the
    reference in that dtype returns finite values that are the targets' half-rounded v rows bit for bit (float16 scores
    overflow at 1024 * d); a case where the reference is not exact at any gain stops the script.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import attention_half_oracle as aho  # noqa: E402
import make_attention_goldens as mg  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SAMPLE = 1024
SHAPES = [(2, 1, 70, 40), (3, 1, 9, 160), (2, 1, 64, 64), (5, 2, 100, 80)]   # heads, samples, n, d
SHORT = {"float16": "f16", "bfloat16": "bf16"}


def plan():
    cases, seed = [], 500
    for fl, (mode, chunks, _cfg) in mg.FLAVOURS.items():
        for h, b, n, d in SHAPES:
            cases.append(dict(id=f"value_{fl}_{h}x{b}x{n}x{d}", kind="value", flavour=fl, mode=mode, chunks=chunks, heads=h,
                              samples=b, n=n, n_k=n, d=d, seed=seed))
            seed += 1
    for fl in ("cfg_uni", "cfg_bi"):   # hundreds of workgroups in flight
        mode, chunks, _ = mg.FLAVOURS[fl]
        cases.append(dict(id=f"value_{fl}_8x16x70x40", kind="value", flavour=fl, mode=mode, chunks=chunks, heads=8, samples=16,
                          n=70, n_k=70, d=40, seed=seed))
        seed += 1
    cases.append(dict(id="sharp_cfg_bi", kind="sharp", flavour="cfg_bi", mode="bi", chunks=2, heads=2, samples=1, n=70, n_k=70,
                      d=40, seed=seed, gain=3.0))
    seed += 1
    for name, h, n, n_k, d, cross in (("plain_cross77", 2, 70, 77, 40, True), ("plain_n9", 3, 9, 9, 160, False)):
        cases.append(dict(id=name, kind="plain", flavour="plain", mode="self", chunks=1, heads=h, samples=4, n=n, n_k=n_k, d=d,
                          seed=seed, cross=cross))
        seed += 1
    for mode in ("uni", "bi"):
        for h, b, n in ((2, 2, 70), (3, 1, 9)):
            for d in (40, 64, 80, 160):
                cases.append(dict(id=f"routing_{mode}_{h}x{b}x{n}x{d}", kind="routing", flavour="cfg_" + mode, mode=mode, chunks=2,
                                  heads=h, samples=b, n=n, n_k=n, d=d, seed=seed))
                seed += 1
    return [dict(c, id=c["id"] + "_" + SHORT[dt], dtype=dt) for c in cases for dt in aho.DTYPES]


def reference(ref, case, q, k, v, dtype):
    with torch.no_grad():
        return mg.run_reference(ref, case, *(torch.from_numpy(t).to(dtype) for t in (q, k, v)))


def main():
    ref = mg.load_ref()
    arrays, cases = {}, []
    for case in plan():
        tdt = getattr(torch, case["dtype"])
        if case["kind"] == "routing":
            gain = 1024.0
            while True:
                case["gain"] = gain
                q, k, v = aho.case_inputs(case)
                out = reference(ref, case, q, k, v, tdt)
                want = aho.to_torch(aho.routing_expected(case, v), case["dtype"])
                if bool(torch.isfinite(out.float()).all()) and torch.equal(out.view(torch.int16), want.view(torch.int16)):
                    break
                gain /= 2.0
                assert gain >= 16.0, f"{case['id']}: the reference does not route exactly at any gain"
            assert out.dtype == tdt
            cases.append(case)
            continue
        q, k, v = aho.case_inputs(case)
        for t in (q, k, v):   # the numpy rounding is torch's
            assert torch.equal(torch.from_numpy(t), torch.from_numpy(t).to(tdt).float())
        assert torch.equal(aho.to_torch(mg.ao.case_inputs(case)[0], case["dtype"]).float(), torch.from_numpy(q))
        out = reference(ref, case, q, k, v, tdt)
        out64 = reference(ref, case, q, k, v, torch.float64).numpy()
        assert out.dtype == tdt and out64.dtype == np.float64
        out = out.float().numpy()
        mine = aho.reference64(case, q, k, v)
        assert mine.shape == out64.shape and np.abs(mine - out64).max() <= 1e-12, (case["id"], np.abs(mine - out64).max())
        rs = np.random.RandomState(case["seed"] + 1)
        idx = np.sort(rs.choice(out.size, min(out.size, SAMPLE), replace=False)).astype(np.int32)
        arrays[case["id"] + "/idx"] = idx
        arrays[case["id"] + "/ref"] = out.reshape(-1)[idx]
        arrays[case["id"] + "/ref64"] = out64.reshape(-1)[idx]
        case["e_ref"] = float(np.abs(out.astype(np.float64) - out64).max())
        case["shape"] = list(out.shape)
        cases.append(case)
    meta = dict(cases=cases, sample=SAMPLE, numpy=np.__version__, torch=torch.__version__)
    path = os.path.join(OUT, "bn_attention_half.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    print("bn_attention_half.npz:", len(cases), "cases,", os.path.getsize(path), "bytes")
    for c in cases:
        print(f"  {c['id']:40s} " + (f"e_ref {c['e_ref']:.3e}" if "e_ref" in c else f"gain {c['gain']:g}"))


if __name__ == "__main__":
    main()
