#!/usr/bin/env python3
"""Fixture of the attention sweep: tests/golden/attention_sweep.npz -- every head-dim block (ND = 1 .. 5, full and partial, with
d % 8 == 4 in float32 and d % 16 == 8 in half), token counts one off every tile edge, and scores that ramp along the keys, for the
seven fused attention kernels in float32, float16 and bfloat16.

Build-machine only, like tools/make_attention_goldens.py and tools/make_attention_grad_goldens.py, whose loaders and reference calls
it uses: the reference's BNAttention (stereo_utils.py) for every `out`, torch autograd through the reference's einsum / softmax /
einsum strings (diffusion_utils.py:192-204) for the gradients.

  python tools/make_attention_sweep_goldens.py
Layout: `meta` = JSON {cases, factor, sample, over}; `idx` [rows, SAMPLE] int32 and `ref64` [rows, SAMPLE] float64.  Inputs are seeds
(attention_sweep_oracle.case_inputs / case_d_out).  Per case and tensor t (out; dq, dk, dv in SELF mode):
  e_ref[t]       max |reference in the case's dtype on the CPU - the same in float64| over the WHOLE tensor;
  tile_ratio[t]  gradients only: max |restatement in the kernels' arithmetic - float64| / e_ref[t] (grads_tiled / grads_kernel);
  rows[t]        the row of `idx` (flat indices, seeded) and `ref64` (the reference's float64 values there) that holds its sample.

The grid (attention_sweep_oracle's constants): SELF pairs (n, n_k) by rotation over the head dims, every pair with at least three of
them and all nine at the ND = 4 dims; UNI and BI with n = n_k one off the 32-, 64- and 128-token edges, two per dim and mode by
rotation, all nine in BI at the ND = 4 dims; the ramp cases.  heads 2 x samples 1 (2 CFG chunks in UNI / BI), every fifth case
heads 1 x samples 2.

Asserted here: the numpy float64 restatement equals the reference's float64 within 1e-12 x max(1, max |ref|); e_ref > 0 for every
tensor of a ramp case; at most 5 % of (case, gradient) pairs need more than FACTOR in the kernels' arithmetic (a seed that lands
above it is stepped first) and none at ND = 4; the file stays smaller than attention_grad.npz.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import attention_sweep_oracle as so  # noqa: E402
import make_attention_goldens as mg  # noqa: E402
import make_attention_grad_goldens as mgg  # noqa: E402
import make_attention_half_grad_goldens as mhg  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SAMPLE = 32
FACTOR = so.FACTOR
CAP = 0.05
SEED_STEP, SEED_TRIES = 1000, 6
RAMP = dict(span=60.0, noise=0.05)
FLAVOUR = {"uni": "cfg_uni", "bi": "cfg_bi"}


def plan():
    cases = []

    def add(dtype, kind, mode, n, n_k, d, **extra):
        h, b = (1, 2) if len(cases) % 5 == 4 else (2, 1)
        stem = "ramp" if kind == "ramp" else "sweep"
        cid = f"{stem}_{so.SHORT[dtype]}_{mode}_{h}x{b}x{n}x{n_k}x{d}"
        if any((c["dtype"], c["kind"], c["mode"], c["n"], c["n_k"], c["d"]) == (dtype, kind, mode, n, n_k, d) for c in cases):
            return
        cases.append(dict(id=cid, kind=kind, dtype=dtype, mode=mode, chunks=1 if mode == "self" else 2, heads=h, samples=b, n=n,
                          n_k=n_k, d=d, seed=2000 + len(cases), **extra))

    for dtype in so.DTYPES:
        dims = so.dims(dtype)
        full = [d for d in dims if so.nd(d) == 4]
        rest = [d for d in dims if so.nd(d) != 4]
        for d in full:
            for n, n_k in so.SELF_PAIRS:
                add(dtype, "value", "self", n, n_k, d)
        for t, d in enumerate(rest):
            for j in range(3):
                n, n_k = so.SELF_PAIRS[(3 * t + j) % len(so.SELF_PAIRS)]
                add(dtype, "value", "self", n, n_k, d)
        for n, n_k, d in so.GUARD:
            add(dtype, "value", "self", n, n_k, d if dtype == "float32" else so.half_dim(d))
        for t, d in enumerate(dims):
            for mode, shift in (("uni", 0), ("bi", 4)):
                for j in range(2):
                    n = so.VIEW_NS[(2 * t + j + shift) % len(so.VIEW_NS)]
                    add(dtype, "value", mode, n, n, d, flavour=FLAVOUR[mode])
        for d in full:
            for n in so.VIEW_NS:
                add(dtype, "value", "bi", n, n, d, flavour=FLAVOUR["bi"])
        for n, n_k in so.RAMP_PAIRS:
            for d in so.RAMP_DIMS:
                add(dtype, "ramp", "self", n, n_k, d, **RAMP)
    return cases


def reference(ref, case, q, k, v, d_out, dtype):
    """The reference in torch `dtype` on the CPU -> {tensor: float64 array}."""
    tq, tk, tv = (torch.from_numpy(t).to(dtype) for t in (q, k, v))
    # SELF is the class's plain path (is_cross: einsum(attn, v) and the heads folded back, stereo_utils.py:137-140)
    rc = dict(case, kind="plain", cross=True) if case["mode"] == "self" else case
    with torch.no_grad():
        out = mg.run_reference(ref, rc, tq, tk, tv)
    assert out.dtype == dtype
    res = {"out": out.double().numpy()}
    if case["mode"] == "self":
        if dtype in (torch.float32, torch.float64):
            g = mgg.torch_grads(case, q, k, v, d_out, dtype)
        else:
            g = mhg.torch_grads_t(case, q, k, v, d_out, dtype)
            assert all(t.dtype == dtype for t in g)
            g = tuple(t.double().numpy() for t in g)
        for t, a in zip(("dq", "dk", "dv"), g):
            res[t] = np.asarray(a, np.float64)
    return res


def measure(ref, case):
    """e_ref, tile_ratio, shapes and the float64 reference of one case at its current seed."""
    tdt = getattr(torch, case["dtype"])
    q, k, v = so.case_inputs(case)
    d_out = so.case_d_out(case)
    for t in (q, k, v, d_out):   # values of the dtype: the cast below rounds nothing
        assert t.dtype == np.float32 and torch.equal(torch.from_numpy(t), torch.from_numpy(t).to(tdt).float())
    own = reference(ref, case, q, k, v, d_out, tdt)
    r64 = reference(ref, case, q, k, v, d_out, torch.float64)
    mine = {"out": so.forward64(case, q, k, v)}
    if case["mode"] == "self":
        mine.update(zip(("dq", "dk", "dv"), so.grads64(case, q, k, v, d_out)))
        kern = dict(zip(("dq", "dk", "dv", "out", "lse"), so.restated(case, q, k, v, d_out)))
        ok, err = so.lse_ok(kern["lse"], so.lse64(case, q, k))
        assert ok, (case["id"], "lse", err)
    e_ref, ratio, shape = {}, {}, {}
    for t in so.tensors(case):
        w = r64[t]
        assert mine[t].shape == w.shape and np.abs(mine[t] - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), (case["id"], t)
        e_ref[t] = float(np.abs(own[t] - w).max())
        shape[t] = list(w.shape)
        if case["kind"] == "ramp":
            assert e_ref[t] > 0, (case["id"], t)
        if t == "out":
            continue
        got = kern[t].astype(np.float64)
        if e_ref[t] > 0:
            ratio[t] = float(np.abs(got - w).max() / e_ref[t])
        else:   # a single key: dq and dk are zero in the reference's arithmetic
            assert case["n_k"] == 1 and t in ("dq", "dk") and np.abs(w).max() == 0, (case["id"], t)
            if so.is_half(case):
                assert (np.abs(got) <= so.single_key_bounds(case, q, k, v, d_out)[("dq", "dk").index(t)]).all(), (case["id"], t)
            else:
                assert np.abs(got).max() == 0, (case["id"], t)
            ratio[t] = 0.0
    out_ratio = None
    if case["mode"] == "self":
        out_ratio = float(np.abs(so.go.unfold(r64["out"], case["heads"]) - so.go.unfold(kern["out"].astype(np.float64), case["heads"])).max()
                          / (e_ref["out"] or 1.0))
    return e_ref, ratio, shape, r64, out_ratio


def main():
    ref = mg.load_ref()
    mgg.load_ref()   # (the gradients' strings are diffusion_utils.py's: it must at least import)
    cases, idx, ref64, over, stepped = [], [], [], [], []
    for case in plan():
        for attempt in range(SEED_TRIES):
            e_ref, ratio, shape, r64, out_ratio = measure(ref, case)
            if all(r <= FACTOR for r in ratio.values()) or attempt == SEED_TRIES - 1:
                break
            stepped.append((case["id"], case["seed"], {t: round(r, 2) for t, r in ratio.items()}))
            case["seed"] += SEED_STEP
        case["e_ref"], case["shape"], case["rows"] = e_ref, shape, {}
        if ratio:
            case["tile_ratio"] = ratio
            over += [(case["id"], t, r) for t, r in ratio.items() if r > FACTOR]
        for j, t in enumerate(so.tensors(case)):
            rs = np.random.RandomState(case["seed"] + 1 + j)
            flat = r64[t].reshape(-1)
            ix = np.sort(rs.choice(flat.size, SAMPLE, replace=flat.size < SAMPLE)).astype(np.int32)
            case["rows"][t] = len(idx)
            idx.append(ix)
            ref64.append(flat[ix])
        cases.append(case)
        print(f"  {case['id']:36s} seed {case['seed']}  " + "  ".join(
            f"{t} {e_ref[t]:.2e}" + (f" x{ratio[t]:.2f}" if t in ratio else "") for t in so.tensors(case))
            + (f"  (out x{out_ratio:.2f})" if out_ratio is not None else ""))

    pairs = sum(len(c.get("tile_ratio", {})) for c in cases)
    print(f"{len(cases)} cases, {pairs} (case, gradient) pairs, {len(over)} above FACTOR {FACTOR}: {over or 'none'}")
    print("seeds stepped:", stepped or "none")
    assert len(over) <= CAP * pairs, (len(over), pairs)
    by_id = {c["id"]: c for c in cases}
    assert not [o for o in over if so.nd(by_id[o[0]]["d"]) == 4], "an ND = 4 case needs the widened bound"

    meta = dict(cases=cases, factor=FACTOR, sample=SAMPLE, over=len(over), pairs=pairs, numpy=np.__version__, torch=torch.__version__)
    path = os.path.join(OUT, "attention_sweep.npz")
    np.savez_compressed(path, meta=json.dumps(meta), idx=np.stack(idx), ref64=np.stack(ref64))
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(OUT, "attention_grad.npz"))
    print("attention_sweep.npz:", len(cases), "cases,", len(idx), "rows,", size, "bytes (attention_grad.npz:", limit, ")")
    assert size < limit


if __name__ == "__main__":
    main()
