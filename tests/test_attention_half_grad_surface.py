"""The half-precision differentiable attention's surface without a GPU: tests/golden/attention_half_grad.npz against the oracle
(float64 restatement, the restatement in the kernels' arithmetic), the three exported symbols and their prototypes, host-side
refusals, and the Python checks that raise before any pointer is passed."""
import ctypes
import functools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import attention_half_grad_oracle as hgo  # noqa: E402

from comfystereo_amd import _native, engine  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "attention_half_grad.npz")
FIX = np.load(PATH)
META = json.loads(str(FIX["meta"]))
CASES = {c["id"]: c for c in META["cases"]}
FACTOR = 4.0
NAMES = ("cs_attention_half_fwd_lse", "cs_attention_half_bwd_workspace_bytes", "cs_attention_half_bwd")


@functools.lru_cache(maxsize=None)
def inputs(cid):
    case = CASES[cid]
    return hgo.case_inputs(case) + (hgo.case_d_out(case),)


def test_fixture_covers_the_cases_in_both_dtypes_and_fits():
    assert os.path.getsize(PATH) < 1 << 20 and META["factor"] == FACTOR
    shapes = {(2, 4, 70, 70, 40), (2, 4, 70, 77, 40), (3, 4, 9, 9, 160), (5, 2, 100, 100, 80), (2, 1, 64, 64, 64), (1, 1, 33, 1, 8)}
    for dt in hgo.DTYPES:
        mine = [c for c in CASES.values() if c["dtype"] == dt]
        assert {(c["heads"], c["samples"], c["n"], c["n_k"], c["d"]) for c in mine if c["kind"] == "value"} == shapes
        sharp = [c for c in mine if c["kind"] == "sharp"]
        assert len(sharp) == 1 and sharp[0]["gain"] == 3.0 and (sharp[0]["n"], sharp[0]["n_k"], sharp[0]["d"]) == (70, 70, 40)
        small = [c for c in mine if c["kind"] == "small"]
        assert len(small) == 1 and small[0]["d_out_mul"] == 2.0 ** -12 and (small[0]["n"], small[0]["n_k"], small[0]["d"]) == (70, 77, 40)
        single = [c for c in mine if c["n_k"] == 1]
        assert len(single) == 1 and single[0]["e_ref"]["dq"] == 0 and single[0]["e_ref"]["dk"] == 0 and single[0]["e_ref"]["dv"] > 0
        assert set(META["toy"][dt]["e_ref"]) == {"out", "d_context", "d_x"}
    assert len(CASES) == 16


@pytest.mark.parametrize("cid", sorted(CASES))
def test_inputs_are_values_of_the_dtype(cid):
    case = CASES[cid]
    tdt = getattr(torch, case["dtype"])
    for t in inputs(cid):
        assert t.dtype == np.float32 and torch.equal(torch.from_numpy(t).to(tdt).float(), torch.from_numpy(t))
    if case["kind"] == "small":
        assert 0 < np.abs(inputs(cid)[3]).max() < 2e-3


@pytest.mark.parametrize("cid", sorted(CASES))
def test_float64_restatement_matches_the_stored_samples(cid):
    case = CASES[cid]
    g64 = hgo.grads64(case, *inputs(cid))
    for t, g in zip(("dq", "dk", "dv"), g64):
        assert list(g.shape) == case["shape"][t]
        ref = FIX[f"{cid}/{t}/ref64"]
        assert len(ref) <= 1024
        assert np.abs(g.reshape(-1)[FIX[f"{cid}/{t}/idx"]] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), t


@pytest.mark.parametrize("cid", sorted(CASES))
def test_kernel_order_restatement_is_within_the_recorded_ratio(cid):
    case = CASES[cid]
    q, k, v, d_out = inputs(cid)
    g64 = hgo.grads64(case, q, k, v, d_out)
    kern = hgo.grads_kernel(case, q, k, v, d_out)
    bounds = hgo.single_key_bounds(case, q, k, v, d_out) if case["n_k"] == 1 else None
    for j, t in enumerate(("dq", "dk", "dv")):
        got = kern[j].astype(np.float64)
        assert np.array_equal(kern[j], hgo.aho.round_to(kern[j], case["dtype"]))   # values of the dtype
        e_ref, ratio = case["e_ref"][t], case["tile_ratio"][t]
        if e_ref == 0:
            assert (np.abs(got) <= bounds[j]).all() and np.abs(g64[j]).max() == 0, t
        else:
            err = np.abs(got - g64[j]).max()
            assert err <= ratio * e_ref * (1 + 1e-9) + 1e-300, (t, err, ratio * e_ref)
    lse = hgo.lse64(case, q, k)
    assert np.abs(kern[4].astype(np.float64) - lse).max() <= 1e-5 * np.abs(lse).max()


def test_exports_and_prototypes():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    L = _native.lib()
    for name in NAMES:
        assert name in _native.EXPORTS and hasattr(L, name)
    assert ("CS_API int cs_attention_half_fwd_lse(const void *q, const void *k, const void *v, void *out, float *lse, int dtype, "
            "int b, int h, int n, int n_k, int d, double scale, void *stream);") in flat
    assert "CS_API size_t cs_attention_half_bwd_workspace_bytes(int b, int h, int n, int n_k, int d);" in flat
    assert ("CS_API int cs_attention_half_bwd(const void *q, const void *k, const void *v, const void *out, const float *lse, "
            "const void *d_out, void *dq, void *dk, void *dv, int dtype, int b, int h, int n, int n_k, int d, double scale, "
            "void *workspace, size_t workspace_bytes, void *stream);") in flat
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert L.cs_attention_half_fwd_lse.argtypes == [vp] * 5 + [ci] * 6 + [ctypes.c_double, vp]
    assert L.cs_attention_half_bwd.argtypes == [vp] * 9 + [ci] * 6 + [ctypes.c_double, vp, ctypes.c_size_t, vp]
    assert L.cs_attention_half_bwd_workspace_bytes.restype == ctypes.c_size_t
    assert "cs_attention_half_bwd" in hdr[hdr.index("CS_DEBUG_ATTN_WAVES = 12"):hdr.index("CS_DEBUG_KEYS = 13")]
    assert L.cs_version() == _native.ABI_VERSION


def _ptrs(count, bytes_each=1 << 24):
    """Distinct, 16-byte aligned, far-apart dummy addresses: refusals come before any of them is touched."""
    return [ctypes.c_void_p((1 << 32) + i * bytes_each) for i in range(count)]


def test_the_c_abi_refuses_on_the_host():
    L = _native.lib()
    p = _ptrs(10)
    b, h, n, n_k, d = 2, 2, 8, 9, 40
    need = L.cs_attention_half_bwd_workspace_bytes(b, h, n, n_k, d)
    assert need >= b * h * n * 4
    assert L.cs_attention_half_bwd_workspace_bytes(b, 0, n, n_k, d) == 0

    def fwd(ptrs=p, dtype=0, dims=(b, h, n, n_k, d), scale=0.1):
        return L.cs_attention_half_fwd_lse(*ptrs[:5], dtype, *dims, scale, None)

    def bwd(ptrs=p, dtype=1, dims=(b, h, n, n_k, d), ws_bytes=need):
        return L.cs_attention_half_bwd(*ptrs[:9], dtype, *dims, 0.1, ptrs[9], ws_bytes, None)

    for i in range(5):
        assert fwd(p[:i] + [None] + p[i + 1:]) == _native.CS_EINVAL, i
        assert fwd(p[:i] + [ctypes.c_void_p(p[i].value + 8)] + p[i + 1:]) == _native.CS_EINVAL, i
    for i in range(10):
        assert bwd(p[:i] + [None] + p[i + 1:]) == _native.CS_EINVAL, i
        assert bwd(p[:i] + [ctypes.c_void_p(p[i].value + 8)] + p[i + 1:]) == _native.CS_EINVAL, i
    for call in (fwd, bwd):
        assert call(dtype=2) == _native.CS_EINVAL and b"dtype" in L.cs_last_error()
        assert call(dtype=-1) == _native.CS_EINVAL
        assert call(dims=(b, h, n, n_k, 44)) == _native.CS_ELIMIT and b"multiple of 8" in L.cs_last_error()
        assert call(dims=(b, h, n, n_k, 164)) == _native.CS_ELIMIT
        assert call(dims=(b, h, 0, n_k, d)) == _native.CS_EINVAL
    assert fwd(scale=float("nan")) == _native.CS_EINVAL
    assert fwd(p[:3] + [p[0]] + p[4:]) == _native.CS_EINVAL                 # out aliases q
    assert fwd(p[:4] + [p[3]] + p[5:]) == _native.CS_EINVAL                 # lse aliases out
    assert bwd(ws_bytes=need - 1) == _native.CS_EWORKSPACE and b"workspace" in L.cs_last_error()
    assert bwd(p[:6] + [p[3]] + p[7:]) == _native.CS_EINVAL                 # dq aliases out
    assert bwd(p[:7] + [p[6]] + p[8:]) == _native.CS_EINVAL                 # dk aliases dq
    assert bwd(p[:9] + [p[5]]) == _native.CS_EINVAL                         # the workspace aliases d_out


class _NoPointer:
    """Stands in for the library: any entry point reached fails the test."""
    def __getattr__(self, name):
        if name == "cs_stereo_attention_max_head_dim":
            return lambda: 160
        raise AssertionError(f"{name} was reached: the check must come before any pointer is passed")


@pytest.fixture
def no_pointer(monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: _NoPointer())


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
def test_engine_checks_raise_before_any_pointer_is_passed(no_pointer, dtype):
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    z = lambda *s, dt=dtype: torch.zeros(*s, dtype=dt)  # noqa: E731
    q, k = z(4, 8, 40), z(4, 9, 40)
    bad = [
        (q, k, z(4, 9, 40, dt=other)),                 # two half dtypes
        (q, z(4, 9, 40, dt=torch.float32), k),         # half and float32
        (z(4, 8, 40, dt=torch.float32), k, k),
        (z(4, 8, 44), z(4, 9, 44), z(4, 9, 44)),       # d a multiple of 4, not of 8
        (z(4, 8, 164), z(4, 9, 164), z(4, 9, 164)),    # d above the limit
        (q, k, k),                                     # well-formed, but host memory
    ]
    for a, b, c in bad:
        with pytest.raises(ValueError):
            engine.attention_lse(a, b, c, 2, 0.1)
    out, lse, d_out = z(2, 8, 80), torch.zeros(4, 8), z(2, 8, 80)
    for o, l, g in ((out, z(4, 8), d_out),                           # lse in the half dtype
                    (out, lse.double(), d_out),
                    (out.float(), lse, d_out),                       # out float32, the rest half
                    (out, lse, d_out.float()),
                    (out, lse, z(2, 8, 80, dt=other)),
                    (out, lse, d_out)):                              # well-formed, but host memory
        with pytest.raises(ValueError):
            engine.attention_backward(q, k, k, o, l, g, 2, 0.1)
    with pytest.raises(ValueError):
        engine.attention_backward(z(4, 8, 44), z(4, 9, 44), z(4, 9, 44), z(2, 8, 88), lse, z(2, 8, 88), 2, 0.1)


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
def test_native_half_on_host_tensors_fails_like_the_default(dtype):
    q, k = torch.zeros(4, 8, 40, dtype=dtype, requires_grad=True), torch.zeros(4, 9, 40, dtype=dtype)
    errors = []
    for kwargs in ({}, {"native_half": True}):
        with pytest.raises(ValueError) as info:
            engine.differentiable_attention(q, k, k, 2, 0.1, **kwargs)
        errors.append(str(info.value))
    assert errors[0] == errors[1]
    with pytest.raises(ValueError):
        engine.differentiable_attention(q.detach().to(torch.float64), k, k, 2, 0.1, native_half=True)
