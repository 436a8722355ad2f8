#!/usr/bin/env python3
"""Fixture of the latent shift's plan outside the workload's shapes, signs and exponents: tests/golden/stream_edges.npz.

Build-machine only, like tools/make_standard_goldens.py: loads the reference's stereo_utils.py and runs
stereo_shift_torch(x, disp, scale_factor, False, exponent) itself (CPU torch) on a one-channel payload whose value at column x
is x + 1.  The right half of what it returns is then the source column of every destination plus one, 0 in a hole: the plan,
from the reference's own sweep.

  python tools/make_stream_edge_goldens.py

Cases (`cases()`), the full product of
  the shapes (1,1,2), (2,5,7), (1,33,130), (1,64,64);
  the depth kinds flat, ramp, 8-pixel steps, 8-bit noise;
  the scale factors +-0.5, +-8, +-99.9, +-100, +-150 and +-(100 k / w) at k = 1, 2, w - 2, w - 1, searched among the
  neighbouring doubles until (scale_factor / 100) * w is the integer k exactly;
  the exponents 1, 2, 0.5, 0.75, 3, 0 and -1;
and three more disparities at (2,5,7): one NaN, one +inf, all NaN.  The depth of a case is not stored: `case_depth` makes it
again from the case's kind, shape and seed.

The margin.  torch.pow takes the exponents 1, 2, 0.5 and 0 exactly as the restatement does.  For 0.75 (torch's general pow) and 3
(torch multiplies twice) its power may differ from glibc's powf in the last place, so for these the seed of the case's depth is
searched (`SEEDS` of them) until every shift product that could be affected lies at least MARGIN from the nearest integer it
can cross.  Not counted, in the margin only: products that are 0, powers float32 holds exactly (pow(0, e), pow(1, e),
0.5 ** 3 ...), and the integer 0, which a product of a non-negative power cannot cross.  A case for which no seed holds the
margin is left out and listed in meta.left_out with the best margin found: a ramp or a noise map of thousands of pixels has
hundreds to thousands of distinct products, each with a chance of 2e-3 to lie that close to an integer once scale_px is large.
The exponent -1 (torch: one division; powf differs from it in the last place on some values) has no margin to hold -- with an
integer scale_px, 1 / 0.5 * scale_px is an integer by construction -- and none is asked of it: its tables are pinned by the
assertion below.

One name of the reference's module is replaced while it runs: `int`, by `_int`, which is Python's int except that of an
infinite or NaN value -- where Python raises, and the reference's call with it -- it returns a shift that leaves the row.  That
is what the kernels do with such a product (they cannot raise); meta.cases[*].raises says where the reference itself would have
raised (every exponent below 0: 0 ** e is inf at the map's minimum).

Layout: `meta` = JSON {margin, seeds, versions, left_out: [{id, margin}], cases: [{id, shape, kind, seed, scale_factor,
exponent, margin, raises, group, index}]}; one array per group, 'tables/<group>' int16 [cases of the group, B, H, W]: src_col,
-1 in a hole (`table(z, case)`); the groups are the four shapes and 'special'.

Asserted while making it: tools/standard_oracle.py's plan equals every table; every margin asked for holds; the file stays below
the 1 MiB a committed file may have.  No table entry is left out of any comparison.
"""
import importlib.util
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import standard_oracle as so  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "stream_edges.npz")
MARGIN = 1e-3
SHAPES = ((1, 1, 2), (2, 5, 7), (1, 33, 130), (1, 64, 64))
KINDS = ("flat", "ramp", "steps", "noise")
EXPONENTS = (1.0, 2.0, 0.5, 0.75, 3.0, 0.0, -1.0)
INEXACT = (0.75, 3.0)                # exponents at which torch.pow and powf may round differently (3: torch multiplies twice)
SEEDS = 64                           # depths tried for a case before it is left out
SPECIAL = ("one_nan", "one_inf", "all_nan")
SPECIAL_SHAPE = (2, 5, 7)


def depth(kind, b, h, w, seed=0):
    """The depth kinds of tests/test_gpu_standard_mode.py; the ramp's rows are offset by 0.01 there, the seed's own step here."""
    rng = np.random.default_rng(seed)
    if kind == "flat":
        return np.full((b, h, w), 0.25, dtype=np.float32)
    if kind == "ramp":
        step = np.float32(0.01 + 1e-4 * seed)
        return np.broadcast_to(np.linspace(0, 1, w, dtype=np.float32) + step * np.arange(h, dtype=np.float32)[:, None], (b, h, w)).copy()
    if kind == "steps":
        return (rng.integers(0, 5, (b, h, (w + 7) // 8)).repeat(8, -1)[:, :, :w] / np.float32(4)).astype(np.float32)
    return rng.integers(0, 256, (b, h, w)).astype(np.float32) / np.float32(255.0)   # 8-bit noise: many collisions


def case_depth(case):
    """The disparity of a fixture case (an entry of meta.cases) -> float32 [B,H,W]."""
    if case["kind"] in SPECIAL:
        return special_depth(case["kind"])
    return depth(case["kind"], *case["shape"], seed=case["seed"])


def special_depth(name):
    d = depth("noise", *SPECIAL_SHAPE, seed=77)
    if name == "one_nan":
        d[1, 2, 3] = np.nan
    elif name == "one_inf":
        d[1, 2, 3] = np.inf
    else:
        d[:] = np.nan
    return d


def integer_scale(k, w):
    """A scale factor near 100 k / w for which (scale_factor / 100.0) * w, as the reference computes it, is exactly k."""
    sf = 100.0 * k / w
    for cand in [sf] + [f(sf, n) for n in range(1, 9) for f in (lambda x, n: _step(x, n), lambda x, n: _step(x, -n))]:
        if (cand / 100.0) * w == float(k):
            return cand
    raise SystemExit(f"no double near {sf} makes scale_px the integer {k} at w = {w}")


def _step(x, n):
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def scale_factors(w):
    mags = [0.5, 8.0, 99.9, 100.0, 150.0]
    for k in (1, 2, w - 2, w - 1):
        if k >= 1:
            sf = integer_scale(k, w)
            if sf not in mags:
                mags.append(sf)
    return [s * m for m in mags for s in (1.0, -1.0)]


def shape_name(shape):
    return "x".join(str(s) for s in shape)


def cases():
    """[(id, shape, kind, scale_factor, exponent, group)] in the fixture's order, before any is left out."""
    out = []
    for shape in SHAPES:
        for kind in KINDS:
            for sf in scale_factors(shape[2]):
                for e in EXPONENTS:
                    out.append((f"{shape_name(shape)}/{kind}/sf{sf!r}/e{e!r}", shape, kind, sf, e, shape_name(shape)))
    for name in SPECIAL:
        for sf, e in ((8.0, 1.0), (-150.0, 1.0), (150.0, 0.5), (-8.0, 0.75), (100.0, 0.0)):
            out.append((f"special/{name}/sf{sf!r}/e{e!r}", SPECIAL_SHAPE, name, sf, e, "special"))
    return out


def table(z, case):
    """The table of a fixture case (an entry of meta.cases) -> int32 [B,H,W]."""
    return z[f"tables/{case['group']}"][case["index"]].astype(np.int32)


def pow_margin(disp, sf, e):
    """so.margin over the products whose power two correct libms may round differently: 0 < norm < 1 with a power that float32
    does not hold exactly."""
    if e not in INEXACT:
        return None
    nd = so.norm_depth(disp)
    prod, _ = so.shift_products(disp, sf, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        p64 = nd.astype(np.float64) ** e
    exact = p64.astype(np.float32).astype(np.float64) == p64
    p = prod.astype(np.float64)[np.isfinite(prod) & (prod != 0) & ~exact]
    near = np.rint(p)
    near[near == 0] = np.sign(p[near == 0])   # a power is never negative: a product does not cross 0, its nearest integer to cross is +-1
    return float(np.abs(p - near).min()) if p.size else float("inf")


def load_stereo_utils():
    import refload
    spec = importlib.util.spec_from_file_location("ref_stereo_utils", refload.REF + "/stereo_utils.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import torch
    su = load_stereo_utils()
    raised = []

    def _int(v):
        f = float(v)
        if math.isfinite(f):
            return int(v)
        raised.append(f)
        return 1 << 40

    su.int = _int
    tables, meta_cases, left_out, worst = {}, [], [], float("inf")
    for cid, shape, kind, sf, e, group in cases():
        # the first seed of the depth whose margin holds (flat has no seed; the non-finite maps have no margin to hold)
        best = -1.0
        for seed in range(SEEDS):
            d = special_depth(kind) if kind in SPECIAL else depth(kind, *shape, seed=seed)
            m = pow_margin(d, sf, e)
            if m is None or m >= MARGIN or kind in SPECIAL:
                break
            best = max(best, m)
        else:
            left_out.append(dict(id=cid, margin=best))
            continue
        b, h, w = shape
        payload = np.broadcast_to(np.arange(1, w + 1, dtype=np.float32), (b, 1, h, w)).copy()
        del raised[:]
        out = su.stereo_shift_torch(torch.from_numpy(payload), torch.from_numpy(d), sf, False, e).numpy()
        assert np.array_equal(out[:b], payload)
        t = out[b:, 0].astype(np.int64) - 1
        assert np.array_equal(t + 1, out[b:, 0]) and t.min() >= -1 and t.max() < w
        assert np.array_equal(so.plan(d, sf, e), t), (cid, "the restatement differs from the reference")
        if m is not None and kind not in SPECIAL:
            worst = min(worst, m)
        mine = tables.setdefault(group, [])
        meta_cases.append(dict(id=cid, shape=list(shape), kind=kind, seed=seed, scale_factor=sf, exponent=e,
                               margin=None if kind in SPECIAL else m, raises=bool(raised), group=group, index=len(mine)))
        mine.append(t.astype(np.int16))
    assert worst >= MARGIN
    versions = dict(numpy=np.__version__, torch=torch.__version__)
    meta = dict(margin=worst, seeds=SEEDS, versions=versions, left_out=left_out, cases=meta_cases)
    np.savez_compressed(OUT, meta=json.dumps(meta), **{f"tables/{g}": np.stack(v) for g, v in tables.items()})
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes", len(meta_cases), "cases, margin", worst)
    print(len(left_out), "left out:")
    for c in left_out:
        print("  ", c["id"], c["margin"])
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
