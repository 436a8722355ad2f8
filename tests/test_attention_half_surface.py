"""The half-precision stereo attention's surface without a GPU: the header's declaration and enum, the binding, the float64
restatement on half-rounded inputs against every case of tests/golden/bn_attention_half.npz, the fixture's metadata, and the
wrapper's argument checks, which raise before any pointer is passed."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import attention_half_oracle as aho  # noqa: E402

from comfystereo_amd import _native, engine, stereo_utils  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "bn_attention_half.npz")
FIX = np.load(PATH)
META = json.loads(str(FIX["meta"]))
CASES = {c["id"]: c for c in META["cases"]}


def test_header_declares_and_native_binds_the_entry():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    assert re.search(r"CS_API\s+int\s+cs_stereo_attention_half\s*\(\s*const void \*q, const void \*k, const void \*v, void \*out, "
                     r"int dtype,", hdr)
    assert re.search(r"enum\s+cs_attn_dtype\s*\{", hdr)
    for key, name in (("float16", "CS_ATTN_F16"), ("bfloat16", "CS_ATTN_BF16")):
        assert int(re.search(name + r"\s*=\s*(\d+)", hdr).group(1)) == _native.ATTN_DTYPE[key] == aho.ABI_DTYPE[key]
    assert "cs_stereo_attention_half" in _native.EXPORTS
    f = _native.lib().cs_stereo_attention_half
    assert f.restype is ctypes.c_int and len(f.argtypes) == 15 and f.argtypes[12] is ctypes.c_double


def test_abi_refuses_bad_arguments_without_device_work():
    f = _native.lib().cs_stereo_attention_half
    p = ctypes.c_void_p(256)
    args = lambda **kw: [kw.get(x, dflt) for x, dflt in (("dtype", 0), ("c", 2), ("s", 2), ("b", 1), ("h", 2), ("n", 8), ("n_k", 8), ("d", 40))]  # noqa: E731
    assert f(None, p, p, p, *args(), 0.1, 1, None) == _native.CS_EINVAL
    assert f(p, p, p, p, *args(dtype=2), 0.1, 1, None) == _native.CS_EINVAL
    assert f(p, p, p, p, *args(n=0), 0.1, 1, None) == _native.CS_EINVAL
    assert f(p, p, p, p, *args(), 0.1, 3, None) == _native.CS_EINVAL
    assert f(p, p, p, p, *args(s=1), 0.1, 1, None) == _native.CS_EINVAL
    assert f(p, p, p, p, *args(n_k=9), 0.1, 2, None) == _native.CS_EINVAL
    assert f(p, p, p, p, *args(), float("inf"), 0, None) == _native.CS_EINVAL
    assert f(p, p, p, p, *args(d=44), 0.1, 0, None) == _native.CS_ELIMIT
    assert f(p, p, p, p, *args(dtype=1, d=168), 0.1, 0, None) == _native.CS_ELIMIT
    assert b"head dimension" in _native.lib().cs_last_error()
    assert f(ctypes.c_void_p(264), p, p, p, *args(), 0.1, 1, None) == _native.CS_EINVAL
    assert f(p, p, p, p, *args(), 0.1, 1, None) == _native.CS_EINVAL   # out aliases q


def test_wrapper_checks_raise_before_any_pointer_is_passed():
    f = torch.zeros
    h, b = torch.float16, torch.bfloat16
    ok = dict(heads=2, scale=0.5, mode="uni", chunks=2)
    bad = [
        (f(8, 4, 8, dtype=h), f(8, 4, 8), f(8, 4, 8), ok),                                       # mixed: half q
        (f(8, 4, 8, dtype=h), f(8, 4, 8, dtype=h), f(8, 4, 8, dtype=b), ok),                     # mixed: float16 and bfloat16
        (f(8, 4, 8), f(8, 4, 8), f(8, 4, 8, dtype=b), ok),                                       # mixed: half v
        (f(8, 4, 8, dtype=torch.float64), f(8, 4, 8, dtype=torch.float64), f(8, 4, 8, dtype=torch.float64), ok),
        (f(8, 4, 8), f(8, 4, 8), f(8, 4, 8), dict(ok, out=f(4, 4, 16, dtype=h))),                # half out, float32 inputs
        (f(8, 4, 8, dtype=b), f(8, 4, 8, dtype=b), f(8, 4, 8, dtype=b), dict(ok, out=f(4, 4, 16))),   # float32 out, half inputs
        (f(8, 4, 8, dtype=b), f(8, 4, 8, dtype=b), f(8, 4, 8, dtype=b), dict(ok, out=f(4, 4, 16, dtype=h))),
        (f(8, 4, 44, dtype=h), f(8, 4, 44, dtype=h), f(8, 4, 44, dtype=h), ok),                  # d = 44 in half
        (f(8, 4, 168, dtype=b), f(8, 4, 168, dtype=b), f(8, 4, 168, dtype=b), ok),               # d above the limit
        (f(8, 4, 8, dtype=h), f(8, 4, 8, dtype=h), f(8, 4, 8, dtype=h), ok),                     # well-formed, but host memory
    ]
    for q, k, v, kw in bad:
        with pytest.raises(ValueError):
            engine.stereo_attention(q, k, v, **kw)
    with pytest.raises(ValueError, match="multiples of 4"):
        engine.stereo_attention(f(8, 4, 44, dtype=h), f(8, 4, 44, dtype=h), f(8, 4, 44, dtype=h), **ok)
    with pytest.raises(ValueError, match="share one dtype"):
        engine.stereo_attention(f(8, 4, 8, dtype=h), f(8, 4, 8), f(8, 4, 8), **ok)


def test_switch_defaults_to_the_upcast():
    assert stereo_utils.HALF_ATTENTION is False
    assert "HALF_ATTENTION" in stereo_utils.__doc__


def test_fixture_covers_the_cases_and_fits():
    assert os.path.getsize(PATH) < 1 << 20
    assert META["sample"] > 0
    for dt in aho.DTYPES:
        mine = [c for c in CASES.values() if c["dtype"] == dt]
        for fl in ("cfg_uni", "cfg_bi", "nocfg"):
            assert {(c["heads"], c["samples"], c["n"], c["d"]) for c in mine if c["kind"] == "value" and c["flavour"] == fl} >= \
                {(2, 1, 70, 40), (3, 1, 9, 160), (2, 1, 64, 64), (5, 2, 100, 80)}
        assert {c["mode"] for c in mine if c["kind"] == "value" and (c["heads"], c["samples"], c["n"], c["d"]) == (8, 16, 70, 40)} == \
            {"uni", "bi"}
        assert [c["gain"] for c in mine if c["kind"] == "sharp"] == [3.0]
        assert {(c["n"], c["n_k"]) for c in mine if c["kind"] == "plain"} == {(70, 77), (9, 9)}
        rout = {(c["mode"], c["n"], c["d"]) for c in mine if c["kind"] == "routing"}
        assert rout == {(m, n, d) for m in ("uni", "bi") for n in (9, 70) for d in (40, 64, 80, 160)}
        for c in mine:
            if c["kind"] == "routing":   # a power of two no larger than the float32 fixture's 1024
                assert 16 <= c["gain"] <= 1024 and np.log2(c["gain"]) % 1 == 0
    assert len(CASES) == len(META["cases"]) and {c["dtype"] for c in CASES.values()} == set(aho.DTYPES)


def test_rounding_is_the_dtypes():
    rs = np.random.RandomState(5)
    x = (rs.standard_normal(4096) * np.exp(rs.uniform(-6, 6, 4096))).astype(np.float32)
    for dt in aho.DTYPES:
        r = aho.round_to(x, dt)
        assert torch.equal(torch.from_numpy(r), torch.from_numpy(x).to(getattr(torch, dt)).float())
        assert torch.equal(aho.to_torch(r, dt).float(), torch.from_numpy(r))


@pytest.mark.parametrize("cid", sorted(c for c in CASES if CASES[c]["kind"] != "routing"))
def test_restatement_reproduces_the_reference_in_float64(cid):
    case = CASES[cid]
    q, k, v = aho.case_inputs(case)
    got = aho.reference64(case, q, k, v)
    assert list(got.shape) == case["shape"]
    assert np.abs(got.reshape(-1)[FIX[cid + "/idx"]] - FIX[cid + "/ref64"]).max() <= 1e-12
    # the recorded e_ref is the reference's own error in the dtype; the sampled reference values are values of the dtype
    assert 0 < case["e_ref"] < 1.0 and np.abs(FIX[cid + "/ref"] - FIX[cid + "/ref64"]).max() <= case["e_ref"]
    assert np.array_equal(aho.round_to(FIX[cid + "/ref"], case["dtype"]), FIX[cid + "/ref"])


@pytest.mark.parametrize("cid", sorted(c for c in CASES if CASES[c]["kind"] == "routing"))
def test_restatement_routes_exactly(cid):
    case = CASES[cid]
    q, k, v = aho.case_inputs(case)
    want = aho.routing_expected(case, v)
    assert np.array_equal(aho.round_to(want, case["dtype"]), want)
    got = aho.reference64(case, q, k, v)
    assert np.array_equal(got.astype(np.float32).view(np.uint32), want.view(np.uint32))
