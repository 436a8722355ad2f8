"""The temporal depth filter without a GPU: its exports, every refusal of the C entry point before any device work, the
workspace size, the properties of the specification (tools/temporal_oracle.py) and the conditions its fixture has to meet
(not gpu)."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

from comfystereo_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_temporal_goldens as goldens   # noqa: E402
import temporal_oracle as oracle   # noqa: E402

INF, NAN = float("inf"), float("nan")
FIXTURE = os.path.join(ROOT, "tests", "golden", "temporal_depth.npz")


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def test_the_exports_are_in_the_header_and_in_the_bindings():
    with open(os.path.join(ROOT, "include", "comfystereo_amd.h")) as f:
        header = f.read()
    for name in ("cs_temporal_depth_workspace_bytes", "cs_temporal_depth"):
        assert re.search(r"CS_API\s+\w+\s+" + name + r"\(", header), name
        assert name in _native.EXPORTS and name in _native.SIGNATURES
        assert hasattr(_native.lib(), name)
    assert _native.ABI_VERSION == 4 and _native.lib().cs_version() == 4
    assert len(_native.SIGNATURES["cs_temporal_depth"][1]) == 17 and len(_native.SIGNATURES["cs_temporal_depth_workspace_bytes"][1]) == 4


def test_the_kernel_file_shares_the_gray_expression():
    # the expression lives in the header the pre-passes share; no file of the family restates it or the access built on it
    csrc = os.path.join(ROOT, "comfystereo_amd", "csrc")
    text = {}
    for name in ("cs_gray4.h", "cs_temporal.hip", "cs_depthrange.hip", "cs_guideddepth.hip"):
        with open(os.path.join(csrc, name)) as f:
            text[name] = f.read()
        assert "0.2989" not in text[name], name
    assert "gray_of(" in text["cs_gray4.h"] and len(re.findall(r"struct\s+\w*Px4\b", text["cs_gray4.h"])) == 1
    for name in ("cs_temporal.hip", "cs_depthrange.hip"):
        assert '#include "cs_gray4.h"' in text[name], name
        assert not re.search(r"struct\s+\w*Px4\b|\bload_gray4\s*\(|range_load4|RPx4", text[name]), name   # (a call names its <CM, VEC>)


# ---- refusals: all of them before any launch, so addresses that are never read will do ----------------------------------------------
FAKE = 0x10000000   # a non-null, 16-byte aligned address nothing dereferences: every call below is refused first
FAR = 0x10000000    # the eight buffers lie this far apart: none overlaps another at any size used here


def _call(depth=FAKE, n=2, h=4, w=4, c=1, alpha=0.5, motion=0.1, cut=0.08, prev_raw=FAKE + 2 * FAR, prev=FAKE + 3 * FAR,
          valid=FAKE + 4 * FAR, out=FAKE + FAR, m=FAKE + 5 * FAR, cut_out=FAKE + 6 * FAR, ws=FAKE + 7 * FAR, ws_bytes=0):
    L = _native.lib()
    rc = L.cs_temporal_depth(depth, n, h, w, c, alpha, motion, cut, prev_raw, prev, valid, out, m, cut_out, ws, ws_bytes, None)
    return rc, L.cs_last_error().decode()


@pytest.mark.parametrize("name", ["depth", "prev_raw", "prev", "valid", "out", "m", "cut_out", "ws"])
def test_a_null_pointer_is_refused(name):
    assert _call(**{name: None}) == (_native.CS_EINVAL, "null pointer")


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(w=-3), dict(c=0)])
def test_a_non_positive_size_is_refused(kw):
    assert _call(**kw) == (_native.CS_EINVAL, "non-positive size")


@pytest.mark.parametrize("kw, word", [
    (dict(alpha=-0.01), "alpha"), (dict(alpha=1.01), "alpha"), (dict(alpha=NAN), "alpha"), (dict(alpha=INF), "alpha"),
    (dict(motion=-1e-9), "motion_threshold"), (dict(motion=NAN), "motion_threshold"), (dict(motion=-INF), "motion_threshold"),
    (dict(cut=-1e-9), "cut_threshold"), (dict(cut=NAN), "cut_threshold"), (dict(cut=-INF), "cut_threshold"),
])
def test_a_parameter_outside_its_range_is_refused(kw, word):
    rc, text = _call(**kw)
    assert rc == _native.CS_EINVAL and word in text


def test_the_limits_are_refused():
    rc, text = _call(n=65536)
    assert rc == _native.CS_ELIMIT and "65535 frames" in text
    rc, text = _call(n=1, h=65536, w=32768)
    assert rc == _native.CS_ELIMIT and "2^31 pixels" in text


def test_overlap_and_misalignment_are_refused():
    # depth is 128 bytes here, out 128, a state array 64: any two of the eight buffers
    for kw in (dict(out=FAKE + 16), dict(out=FAKE + 124), dict(prev=FAKE + FAR + 32), dict(prev_raw=FAKE + 64), dict(prev=FAKE + 2 * FAR + 60),
               dict(valid=FAKE + 3 * FAR), dict(m=FAKE + FAR + 124), dict(cut_out=FAKE + 5 * FAR + 4), dict(ws=FAKE + 2 * FAR + 8, ws_bytes=1024)):
        rc, text = _call(**kw)
        assert rc == _native.CS_EINVAL and "must not overlap" in text, kw
    assert _call(out=FAKE + 128)[0] == _native.CS_EWORKSPACE and _call(prev=FAKE + 2 * FAR + 64)[0] == _native.CS_EWORKSPACE   # (adjacent)
    rc, text = _call(depth=FAKE + 2)
    assert rc == _native.CS_EINVAL and "4-byte alignment" in text


def test_a_small_workspace_is_refused_and_the_edges_of_every_range_reach_that_check():
    L = _native.lib()
    need = L.cs_temporal_depth_workspace_bytes(2, 4, 4, 1)
    assert need > 0
    # in range: alpha 0 and 1, thresholds 0 and +inf, 65535 frames -- what refuses these calls is the workspace alone
    for kw in (dict(), dict(alpha=0.0), dict(alpha=1.0), dict(motion=0.0, cut=0.0), dict(motion=INF, cut=INF), dict(c=2), dict(c=3),
               dict(ws_bytes=need - 1)):
        assert _call(**kw) == (_native.CS_EWORKSPACE, "workspace too small"), kw
    assert _call(n=65535)[0] == _native.CS_EWORKSPACE


def test_the_workspace_size_is_monotonic_in_n_and_zero_for_no_work():
    L = _native.lib()
    for h, w in ((1, 1), (33, 131), (129, 128), (2160, 3840)):
        sizes = [L.cs_temporal_depth_workspace_bytes(n, h, w, 1) for n in range(1, 70)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], (h, w)
        assert L.cs_temporal_depth_workspace_bytes(64, h, w, 3) == L.cs_temporal_depth_workspace_bytes(64, h, w, 1)
    # one float32 per frame and range of 16 384 pixels
    assert L.cs_temporal_depth_workspace_bytes(64, 2160, 3840, 1) >= 64 * 507 * 4
    assert L.cs_temporal_depth_workspace_bytes(64, 129, 128, 1) >= 64 * 2 * 4
    for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, -1, 1), (4, 4, 4, 0)):
        assert L.cs_temporal_depth_workspace_bytes(*bad) == 0


# ---- the specification's own properties -------------------------------------------------------------------------------------------------
def _dyadic_clip(seed, n=6, h=5, w=7, c=1):
    """Values k / 256: every difference and sum of two of them is exact in float32."""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 257, (n, h, w, c)).astype(np.float32) / np.float32(256.0))


def test_alpha_one_with_infinite_thresholds_is_the_identity():
    # y = y' + 1 * (g - y') returns g exactly where g - y' is exact (Sterbenz: g within a factor 2 of y'; any two k / 256 here);
    # elsewhere the specification's two roundings can leave y one rounding of max(|g|, |y'|) away from g, which the second clip bounds
    d = _dyadic_clip(1)
    y, m, cut, state, still = oracle.temporal_depth(d, None, 1.0, INF, INF)
    assert np.array_equal(y, d[..., 0]) and cut.tolist() == [1, 0, 0, 0, 0, 0] and still[1:].all()
    case = next(c for c in goldens.cases() if c["id"] == "7x64_n9_c3")
    d = goldens.make_input(case)
    y, *_ = oracle.temporal_depth(d, None, 1.0, INF, INF)
    g = oracle.gray(d)
    scale = np.maximum(np.abs(g[1:]), np.abs(g[:-1]))
    # |fl(g - y') - (g - y')| <= u (|g| + |y'|), the sum's rounding <= u |g| (1 + ..), y' itself within 3 u of its g: under 4 u = 2^-22
    assert np.all(np.abs(y[1:].astype(np.float64) - g[1:]) <= scale * 2.0 ** -22)


def test_alpha_zero_repeats_the_frame_after_each_cut():
    d = _dyadic_clip(2, n=8)
    d[4:] += np.float32(2.0)   # a hard cut at frame 4
    y, m, cut, _, _ = oracle.temporal_depth(d, None, 0.0, INF, 0.9)
    assert cut.tolist() == [1, 0, 0, 0, 1, 0, 0, 0]
    for t in range(8):
        assert np.array_equal(y[t], d[0 if t < 4 else 4, ..., 0]), t


@pytest.mark.parametrize("c", [1, 3])
def test_splitting_a_batch_at_every_position_equals_the_whole(c):
    case = next(k for k in goldens.cases() if k["id"] == f"3x5_n9_c{c}")   # nine frames, a cut in the middle
    d = goldens.make_input(case)
    args = (case["alpha"], case["motion_threshold"], case["cut_threshold"])
    y, m, cut, state, _ = oracle.temporal_depth(d, None, *args)
    assert cut.sum() == 2
    for k in range(1, len(d)):
        y0, m0, c0, s0, _ = oracle.temporal_depth(d[:k], None, *args)
        y1, m1, c1, s1, _ = oracle.temporal_depth(d[k:], s0, *args)
        assert np.array_equal(np.concatenate([y0, y1]).view(np.int32), y.view(np.int32)), k
        assert np.array_equal(np.concatenate([m0, m1]), m) and np.array_equal(np.concatenate([c0, c1]), cut), k
        assert np.array_equal(s1.prev_raw, state.prev_raw) and np.array_equal(s1.prev, state.prev), k


def test_a_non_finite_pixel_passes_through_and_resets_itself():
    d = _dyadic_clip(3, n=5, h=2, w=3)
    for value in (np.nan, np.inf, -np.inf):
        e = d.copy()
        e[2, 1, 1, 0] = value
        y, m, cut, _, _ = oracle.temporal_depth(e, None, 0.5, INF, INF)
        assert np.array_equal(y[2, 1, 1], np.float32(value), equal_nan=True) and y[3, 1, 1] == e[3, 1, 1, 0] and np.isfinite(y[4]).all()
        assert cut.tolist() == [1, 0, 0, 0, 0]   # (an infinite or NaN mean is not above an infinite threshold)
    e = d.copy()
    e[2, 1, 1, 0] = np.nan
    y, m, cut, _, _ = oracle.temporal_depth(e, None, 0.5, 0.1, 2.0)   # (values in 0..1: no finite mean reaches 2)
    assert np.isnan(m[2]) and np.isnan(m[3]) and cut.tolist() == [1, 0, 0, 0, 0]   # a NaN mean is no cut


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_the_fixtures_meta_names_its_tool_and_says_what_it_is(fixture):
    meta = json.loads(str(fixture["meta"]))
    assert meta["tool"] == "tools/make_temporal_goldens.py" and "not a reference capture" in meta["note"]
    assert "CPU evaluation of the specification" in meta["note"]
    assert [c["id"] for c in meta["cases"]] == [c["id"] for c in goldens.cases()] and len(set(c["id"] for c in meta["cases"])) == len(meta["cases"])
    assert os.path.getsize(FIXTURE) < (1 << 20)


def test_every_case_keeps_m_one_percent_away_from_the_cut_threshold(fixture):
    meta = json.loads(str(fixture["meta"]))
    for case in meta["cases"]:
        thr = INF if case["cut_threshold"] == "inf" else case["cut_threshold"]
        m = fixture[case["id"] + "/m"]
        assert m.dtype == np.float64 and len(m) == case["n"]
        thr32 = float(np.float32(thr))
        finite = m[np.isfinite(m)]
        if np.isfinite(thr32) and thr32 > 0:
            assert np.all(np.abs(finite - thr32) >= 0.01 * thr32), case["id"]
        elif thr32 == 0:
            assert np.all((finite == 0) | (finite > 1e-30)), case["id"]
        assert goldens.margin_ok(m, thr), case["id"]


def test_the_fixture_is_what_its_tool_writes(fixture):
    got = goldens.build()
    assert sorted(got) == sorted(fixture)
    assert json.loads(str(got["meta"])) == json.loads(str(fixture["meta"]))
    for name in fixture:
        if name != "meta":
            assert got[name].dtype == fixture[name].dtype and np.array_equal(got[name], fixture[name], equal_nan=True), name


def test_the_cases_cover_what_the_kernels_can_get_wrong(fixture):
    cases = goldens.cases()
    assert {(c["h"], c["w"]) for c in cases} == {(1, 1), (3, 5), (7, 64), (5, 67), (33, 131), (129, 128), (2049, 2048), (4097, 4096)}
    # partial sums per frame: a second one; a second trip of the 256 threads that stage them; a second stage of 1024
    partials = {-(-c["h"] * c["w"] // goldens.CHUNK) for c in cases}
    assert partials == {1, 2, 257, 1025}
    assert {c["n"] for c in cases} == {1, 2, 9} and {c["c"] for c in cases} == {1, 2, 3}
    assert {c["special"] for c in cases} == {None, "nan", "pinf", "ninf", "nzero"}
    assert {c["alpha"] for c in cases} == {0.0, 0.37, 1.0}
    assert {c["motion_threshold"] for c in cases} >= {0.0, INF} and {c["cut_threshold"] for c in cases} >= {0.0, INF}
    assert any(c["offset"] for c in cases)
    # both branches of the motion test in one frame, and a hard cut inside the batch
    for case in cases:
        if case["n"] == 9 and case["w"] >= 32 and not case["special"] and not any(t in case["id"] for t in ("motion", "cut0", "identity")):
            y, m, cut, _, still = goldens.evaluate(case)
            t = 2
            assert cut[t] == 0 and still[t].any() and (~still[t]).any(), case["id"]
            if case["cut_at"] is not None and "cutinf" not in case["id"]:
                assert cut[case["cut_at"]] == 1 and cut.sum() == 2, case["id"]
