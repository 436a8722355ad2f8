"""The attention sweep's fixture without a GPU: tests/golden/attention_sweep.npz covers the grid it claims (every ND = 1 .. 5 per
kernel family, partial and full, with the half-pad last k-step; every SELF pair at three head dims or more; every UNI / BI token
count; the ramps in all three dtypes), the float64 restatement reproduces the stored samples, the restatements in the kernels'
arithmetic stay within the bound the GPU test applies, plain float32 numpy meets the LSE bound, and the widened bound stays rare."""
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import attention_sweep_oracle as so  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PATH = os.path.join(GOLDEN, "attention_sweep.npz")
FIX = np.load(PATH)
META = json.loads(str(FIX["meta"]))
CASES = {c["id"]: c for c in META["cases"]}
IDX, REF64 = FIX["idx"], FIX["ref64"]
FACTOR = 4.0
SELF = sorted(c for c in CASES if CASES[c]["mode"] == "self")


def of(dtype, mode=None, kind="value"):
    return [c for c in CASES.values() if c["dtype"] == dtype and c["kind"] == kind and (mode is None or c["mode"] == mode)]


@functools.lru_cache(maxsize=None)
def inputs(cid):
    case = CASES[cid]
    return so.case_inputs(case) + (so.case_d_out(case),)


def test_fixture_fits_and_is_well_formed():
    assert os.path.getsize(PATH) < os.path.getsize(os.path.join(GOLDEN, "attention_grad.npz")) < 1 << 20
    assert META["factor"] == FACTOR == so.FACTOR and len(CASES) == len(META["cases"])
    assert IDX.shape == REF64.shape == (sum(len(so.tensors(c)) for c in CASES.values()), META["sample"])
    rows = sorted(r for c in CASES.values() for r in c["rows"].values())
    assert rows == list(range(len(IDX)))
    for c in CASES.values():
        assert set(c["rows"]) == set(c["e_ref"]) == set(c["shape"]) == set(so.tensors(c))
        assert c["heads"] * c["samples"] * (1 if c["mode"] == "self" else 4) <= 8   # (c s b h) stays small
        assert (c["chunks"] == 2) == (c["mode"] != "self") and (c["n_k"] == c["n"] or c["mode"] == "self")
        assert c["d"] % (8 if so.is_half(c) else 4) == 0 and c["d"] <= 160
        for t in so.tensors(c):
            assert int(IDX[c["rows"][t]].max()) < int(np.prod(c["shape"][t]))
    assert sum((c["heads"], c["samples"]) == (1, 2) for c in CASES.values()) >= 12      # bh / H and bh % H are not always trivial
    assert {(c["heads"], c["samples"]) for c in CASES.values()} == {(2, 1), (1, 2)}


@pytest.mark.parametrize("dtype", so.DTYPES)
def test_every_head_dim_block_is_covered(dtype):
    dims, step = so.dims(dtype), 16 if dtype != "float32" else 8
    for mode in ("self", "uni", "bi"):
        mine = of(dtype, mode)
        assert {c["d"] for c in mine} == set(dims), mode
        by_nd = {b: {c["d"] for c in mine if so.nd(c["d"]) == b} for b in range(1, 6)}
        for b, ds in by_nd.items():
            assert any(d % 32 == 0 for d in ds), (mode, b, "a full block")
            assert any(d % 32 != 0 for d in ds), (mode, b, "a partial last block")
            assert any(d % step == step // 2 for d in ds), (mode, b, "a half-pad last k-step")


@pytest.mark.parametrize("dtype", so.DTYPES)
def test_every_token_edge_is_covered(dtype):
    mine = of(dtype, "self")
    nd4 = [d for d in so.dims(dtype) if so.nd(d) == 4]
    assert len(nd4) == 2
    for pair in so.SELF_PAIRS:
        ds = {c["d"] for c in mine if (c["n"], c["n_k"]) == pair}
        assert len(ds) >= 3 and set(nd4) <= ds, pair
    for d in so.dims(dtype):
        assert len([c for c in mine if c["d"] == d]) >= 3, d
    for mode in ("uni", "bi"):
        view = of(dtype, mode)
        assert {c["n"] for c in view} == set(so.VIEW_NS), mode
        for d in so.dims(dtype):
            assert len([c for c in view if c["d"] == d]) >= 2, (mode, d)
    for d in nd4:
        assert {c["n"] for c in of(dtype, "bi") if c["d"] == d} == set(so.VIEW_NS), d
    ramps = of(dtype, kind="ramp")
    assert {(c["n"], c["n_k"], c["d"]) for c in ramps} == {p + (d,) for p in so.RAMP_PAIRS for d in so.RAMP_DIMS}
    assert all(c["mode"] == "self" and c["span"] == 60.0 and all(e > 0 for e in c["e_ref"].values()) for c in ramps)
    # the guard-row cases of the GPU test
    want = so.GUARD if dtype == "float32" else tuple((n, n_k, so.half_dim(d)) for n, n_k, d in so.GUARD)
    assert set(want) <= {(c["n"], c["n_k"], c["d"]) for c in mine}
    assert [so.half_dim(d) for _, _, d in so.GUARD] == [128, 104, 96]


def test_the_widened_bound_stays_rare():
    pairs = [(c, t, r) for c in CASES.values() for t, r in c.get("tile_ratio", {}).items()]
    over = [(c["id"], t, r) for c, t, r in pairs if r > FACTOR]
    print(f"{len(over)} of {len(pairs)} (case, gradient) pairs above FACTOR: {over}")
    assert len(pairs) == 3 * len(SELF) == META["pairs"] and len(over) == META["over"]
    assert len(over) <= 0.05 * len(pairs)
    assert not [o for o in over if so.nd(CASES[o[0]]["d"]) == 4]
    assert all("tile_ratio" not in c for c in CASES.values() if c["mode"] != "self")


def test_ramp_scores_rise_and_fall_through_every_key_tile():
    """What the ramp is for, checked on its float64 scores: for an even query the maximum of every 32-key tile exceeds the one
    before (the online softmax rescales each time) and the first tile lies 30 nats or more below the last; for an odd query the
    mirror image; and no query is one-hot."""
    for c in (c for c in CASES.values() if c["kind"] == "ramp"):
        q, k, _, _ = inputs(c["id"])
        s = np.einsum("bid,bjd->bij", q.astype(np.float64), k.astype(np.float64)) * c["d"] ** -0.5
        tiles = np.stack([s[:, :, j:j + 32].max(-1) for j in range(0, c["n_k"], 32)], -1)   # [(b h), n, tiles]
        step = np.diff(tiles, axis=-1)
        assert (step[:, 0::2] > 0).all() and (step[:, 1::2] < 0).all(), c["id"]
        assert (np.abs(tiles[..., -1] - tiles[..., 0]) > 30).all(), c["id"]
        assert (s[:, 0::2].argmax(-1) >= c["n_k"] - 4).all() and (s[:, 1::2].argmax(-1) <= 3).all(), c["id"]
        if c["n_k"] % 32 == 1:   # the final maximum on the lone key of the tail tile, next to 31 masked lanes
            assert (s[:, 0::2].argmax(-1) == c["n_k"] - 1).any(), c["id"]
        p = np.exp(s - s.max(-1, keepdims=True))
        assert ((p / p.sum(-1, keepdims=True)).max(-1) < 0.9).all(), c["id"]


@pytest.mark.parametrize("cid", sorted(CASES))
def test_restatements_reproduce_the_fixture_and_meet_the_bounds(cid):
    case = CASES[cid]
    q, k, v, d_out = inputs(cid)
    if so.is_half(case):
        for t in (q, k, v, d_out):
            assert np.array_equal(t, so.hgo.aho.round_to(t, case["dtype"]))   # values of the dtype
    want = {"out": so.forward64(case, q, k, v)}
    if case["mode"] == "self":
        want.update(zip(("dq", "dk", "dv"), so.grads64(case, q, k, v, d_out)))
    for t in so.tensors(case):
        assert list(want[t].shape) == case["shape"][t], t
        ref = REF64[case["rows"][t]]
        assert np.abs(want[t].reshape(-1)[IDX[case["rows"][t]]] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), t
        assert case["e_ref"][t] >= 0
    if case["mode"] != "self":
        return
    # plain float32 numpy meets the LSE bound at this shape
    lse = so.lse64(case, q, k)
    ok, err = so.lse_ok(so.lse_plain32(case, q, k), lse)
    assert ok, err
    # the restatement in the kernels' arithmetic meets the bounds of tests/test_gpu_attention_sweep.py
    kern = dict(zip(("dq", "dk", "dv", "out", "lse"), so.restated(case, q, k, v, d_out)))
    ok, err = so.lse_ok(kern["lse"], lse)
    assert ok, err
    assert np.abs(kern["out"].astype(np.float64) - want["out"]).max() <= FACTOR * case["e_ref"]["out"]
    for j, t in enumerate(("dq", "dk", "dv")):
        got = kern[t].astype(np.float64)
        e_ref = case["e_ref"][t]
        if e_ref == 0:
            # (a single key: zero in the reference's float64; the numpy restatement sums dP and delta in two orders)
            assert case["n_k"] == 1 and t != "dv" and np.abs(want[t]).max() <= 1e-12
            if so.is_half(case):
                assert (np.abs(got) <= so.single_key_bounds(case, q, k, v, d_out)[j]).all(), t
            else:
                assert np.abs(got).max() == 0, t
            continue
        err = np.abs(got - want[t]).max()
        if so.is_half(case):   # (float64 sums rounded once: reproducible; the float32 restatement's matmul order is the BLAS's)
            assert err <= case["tile_ratio"][t] * e_ref * (1 + 1e-9), (t, err)
        assert err <= so.factor_for(case, t) * e_ref, (t, err, e_ref)
