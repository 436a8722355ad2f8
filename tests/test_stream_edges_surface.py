"""The latent shift's plan outside the workload's shapes, signs and exponents, on the CPU (not gpu): the numpy restatement the GPU
tests check the kernel against (tools/standard_oracle.py) held to the reference's own tables in tests/golden/stream_edges.npz
(tools/make_stream_edge_goldens.py), and to the other restatement of the same sweep (oracle/stereo_shift_oracle.py), which was
written independently.  Every comparison is bit for bit."""
import json
import os

import numpy as np

import make_stream_edge_goldens as mk
import standard_oracle as so
from oracle import stereo_shift_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "stream_edges.npz")


def load():
    with np.load(PATH) as f:
        z = {name: f[name] for name in f.files}      # every stacked array decompressed once
    return z, json.loads(str(z["meta"]))


def test_restatement_equals_every_table_of_the_fixture():
    z, meta = load()
    for c in meta["cases"]:
        d = mk.case_depth(c)
        got = so.plan(d, c["scale_factor"], c["exponent"])
        want = mk.table(z, c)
        assert got.shape == tuple(c["shape"]) and np.array_equal(got, want), (c["id"], int((got != want).sum()))


def test_the_two_restatements_agree_on_a_payload():
    z, meta = load()
    for c in meta["cases"]:
        if c["kind"] in mk.SPECIAL or c["raises"]:
            continue   # (a product that is no number: stereo_shift_oracle casts it, the plan lets the pixel leave the row)
        d = mk.case_depth(c)
        b, h, w = c["shape"]
        rng = np.random.default_rng(b * h * w)
        payload = rng.standard_normal((b, 3, h, w)).astype(np.float32)
        want = stereo_shift_oracle.stereo_shift(payload, d, c["scale_factor"], False, c["exponent"])
        assert np.array_equal(want[:b], payload)
        got = so.gather(payload, so.plan(d, c["scale_factor"], c["exponent"]))
        assert np.array_equal(got.view(np.int32), want[b:].view(np.int32)), c["id"]


def test_fixture_coverage_margin_and_size():
    z, meta = load()
    cases = meta["cases"]
    left_out = [c["id"] for c in meta["left_out"]]
    # the full product, in order, but for the cases whose margin no seed holds
    assert [c["id"] for c in cases] == [c[0] for c in mk.cases() if c[0] not in left_out] and set(left_out) <= {c[0] for c in mk.cases()}
    assert meta["margin"] >= mk.MARGIN == 1e-3 and meta["seeds"] == mk.SEEDS
    assert os.path.getsize(PATH) < 1 << 20
    for c in meta["left_out"]:
        shape, kind, _, e = c["id"].split("/")
        assert float(e[1:]) in mk.INEXACT and kind in ("ramp", "noise") and 0 <= c["margin"] < mk.MARGIN, c
    for shape in mk.SHAPES:
        mine = [c for c in cases if tuple(c["shape"]) == shape and c["kind"] not in mk.SPECIAL]
        w = shape[2]
        sfs = {c["scale_factor"] for c in mine}
        assert sfs == set(mk.scale_factors(w)) and {-s for s in sfs} == sfs and {0.5, 8.0, 99.9, 100.0, 150.0} <= sfs
        for k in {1, 2, w - 2, w - 1} - {0}:
            assert any((s / 100.0) * w == float(k) for s in sfs), (shape, k)   # scale_px an integer
        # every kind with every exponent and every scale factor: all of it for the exponents that ask no margin, and for the two
        # that do every scale factor (so both signs) on some kind that moves pixels, and every kind
        have = {(c["kind"], c["scale_factor"], c["exponent"]) for c in mine}
        for e in mk.EXPONENTS:
            if e not in mk.INEXACT:
                assert {(k, s) for k, s, e2 in have if e2 == e} == {(k, s) for k in mk.KINDS for s in sfs}, (shape, e)
            else:
                assert {k for k, s, e2 in have if e2 == e} == set(mk.KINDS), (shape, e)
                assert {s for k, s, e2 in have if e2 == e and k != "flat"} == sfs, (shape, e)
        for c in mine:
            if c["exponent"] in mk.INEXACT:
                d = mk.case_depth(c)
                assert c["margin"] >= mk.MARGIN and mk.pow_margin(d, c["scale_factor"], c["exponent"]) == c["margin"], c["id"]
            assert c["raises"] == (c["exponent"] < 0), c["id"]   # 0 ** e at the map's minimum
    special = [c for c in cases if c["kind"] in mk.SPECIAL]
    assert {c["kind"] for c in special} == set(mk.SPECIAL)
    ident = np.broadcast_to(np.arange(7, dtype=np.int16), mk.SPECIAL_SHAPE)
    for c in special:
        t = mk.table(z, c)
        if c["exponent"] == 0.0:
            assert not c["raises"] and int((t >= 0).sum()) == 0     # x ** 0 = 1, of a NaN too: every pixel shifts by scale_px = -w
        elif c["kind"] == "one_inf":
            # the reference raises (int() of a NaN product at the infinite pixel); with that pixel leaving the row, nothing else moves
            assert c["raises"] and t[1, 2, 3] == -1 and int((t != ident).sum()) == 1
        else:
            assert not c["raises"] and np.array_equal(t, ident), c["id"]   # a NaN makes the map flat: nothing moves


def test_exponents_one_and_a_half_are_as_they_were():
    """shift_products' values for the exponents the restatement always had, from their definitions."""
    d = mk.depth("noise", 2, 5, 7, seed=1)
    nd = so.norm_depth(d)
    for sf in (8.0, -150.0):
        scale = np.float32(((-1 * sf) / 100.0) * 7)
        for e, dv in ((1.0, nd), (0.5, np.sqrt(nd)), (2.0, nd * nd)):
            got, scale_px = so.shift_products(d, sf, e)
            assert got.dtype == np.float32 and scale_px == ((-1 * sf) / 100.0) * 7
            assert np.array_equal(got.view(np.int32), (dv * scale).view(np.int32)), (sf, e)
