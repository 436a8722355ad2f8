"""The differentiable attention's surface without a GPU: exports, host-side refusals of cs_attention_fwd_lse / cs_attention_bwd,
the float64 gradient restatement against torch.autograd and against tests/golden/attention_grad.npz, and the
diffusion_utils drop-in's import and controller refusal."""
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
import attention_grad_oracle as go  # noqa: E402

from comfystereo_amd import _native  # noqa: E402

FIX = np.load(os.path.join(ROOT, "tests", "golden", "attention_grad.npz"))
META = json.loads(str(FIX["meta"]))
CASES = {c["id"]: c for c in META["cases"]}
NAMES = ("cs_attention_fwd_lse", "cs_attention_bwd_workspace_bytes", "cs_attention_bwd")


def test_exports_and_abi_version():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    L = _native.lib()
    for name in NAMES:
        assert re.search(r"CS_API\s+(int|size_t)\s+" + name + r"\s*\(", hdr), name
        assert name in _native.EXPORTS
        assert hasattr(L, name)
    assert L.cs_version() == _native.ABI_VERSION == 4
    assert "log2" in hdr[hdr.index("cs_attention_fwd_lse"):]   # the unit of lse is documented


def _ptrs(count, bytes_each=1 << 24):
    """Distinct, 16-byte aligned, far-apart dummy addresses: refusals come before any of them is touched."""
    return [ctypes.c_void_p((1 << 32) + i * bytes_each) for i in range(count)]


def test_fwd_lse_refuses_on_the_host():
    L = _native.lib()
    q, k, v, out, lse = _ptrs(5)
    ok = (2, 2, 8, 8, 40, 0.1, None)   # b, h, n, n_k, d, scale, stream
    assert L.cs_attention_fwd_lse(None, k, v, out, lse, *ok) == _native.CS_EINVAL
    assert L.cs_attention_fwd_lse(q, k, v, out, None, *ok) == _native.CS_EINVAL
    assert L.cs_attention_fwd_lse(ctypes.c_void_p(q.value + 4), k, v, out, lse, *ok) == _native.CS_EINVAL
    assert L.cs_attention_fwd_lse(q, k, v, out, ctypes.c_void_p(lse.value + 8), *ok) == _native.CS_EINVAL
    assert L.cs_attention_fwd_lse(q, k, v, out, lse, 2, 2, 0, 8, 40, 0.1, None) == _native.CS_EINVAL
    assert L.cs_attention_fwd_lse(q, k, v, out, lse, 2, 2, 8, 8, 42, 0.1, None) == _native.CS_ELIMIT
    assert L.cs_attention_fwd_lse(q, k, v, out, lse, 2, 2, 8, 8, 164, 0.1, None) == _native.CS_ELIMIT
    assert b"head dimension" in L.cs_last_error()
    assert L.cs_attention_fwd_lse(q, k, v, q, lse, *ok) == _native.CS_EINVAL          # out aliases q
    assert L.cs_attention_fwd_lse(q, k, v, out, out, *ok) == _native.CS_EINVAL        # lse aliases out
    assert L.cs_attention_fwd_lse(q, k, v, out, lse, 2, 2, 8, 8, 40, float("nan"), None) == _native.CS_EINVAL


def test_bwd_refuses_on_the_host():
    L = _native.lib()
    p = _ptrs(10)
    b, h, n, n_k, d = 2, 2, 8, 9, 40
    need = L.cs_attention_bwd_workspace_bytes(b, h, n, n_k, d)
    assert need >= b * h * n * 4

    def call(ptrs=p, dims=(b, h, n, n_k, d), ws_bytes=need):
        return L.cs_attention_bwd(*ptrs[:9], *dims, 0.1, ptrs[9], ws_bytes, None)

    for i in range(10):                                                    # every pointer: null, then misaligned
        assert call(p[:i] + [None] + p[i + 1:]) == _native.CS_EINVAL, i
        assert call(p[:i] + [ctypes.c_void_p(p[i].value + 4)] + p[i + 1:]) == _native.CS_EINVAL, i
    assert call(dims=(b, h, n, n_k, 42)) == _native.CS_ELIMIT
    assert call(dims=(b, h, n, n_k, 164)) == _native.CS_ELIMIT
    assert call(dims=(b, 0, n, n_k, d)) == _native.CS_EINVAL
    assert call(ws_bytes=need - 1) == _native.CS_EWORKSPACE
    assert b"workspace" in L.cs_last_error()
    assert call(p[:6] + [p[0]] + p[7:]) == _native.CS_EINVAL               # dq aliases q
    assert call(p[:7] + [p[6]] + p[8:]) == _native.CS_EINVAL               # dk aliases dq
    assert call(p[:9] + [p[5]]) == _native.CS_EINVAL                       # the workspace aliases d_out


def test_workspace_bytes_is_zero_for_non_positive_sizes():
    L = _native.lib()
    assert L.cs_attention_bwd_workspace_bytes(1, 8, 1024, 77, 40) >= 8 * 1024 * 4
    for dims in ((0, 8, 64, 64, 40), (1, 0, 64, 64, 40), (1, 8, 0, 64, 40), (1, 8, 64, -1, 40), (1, 8, 64, 64, 0)):
        assert L.cs_attention_bwd_workspace_bytes(*dims) == 0, dims


def _autograd64(case, q, k, v, d_out):
    tq, tk, tv = (torch.from_numpy(t).double().requires_grad_(True) for t in (q, k, v))
    h = case["heads"]
    attn = (torch.einsum("bid,bjd->bij", tq, tk) * case["d"] ** -0.5).softmax(-1)
    out = torch.einsum("bij,bjd->bid", attn, tv)
    bh, n, d = out.shape
    out = out.reshape(bh // h, h, n, d).permute(0, 2, 1, 3).reshape(bh // h, n, h * d)
    (out * torch.from_numpy(d_out).double()).sum().backward()
    return tq.grad.numpy(), tk.grad.numpy(), tv.grad.numpy()


@pytest.mark.parametrize("cid", sorted(CASES))
def test_restatement_equals_autograd_and_the_fixture(cid):
    case = CASES[cid]
    q, k, v = go.case_inputs(case)
    d_out = go.case_d_out(case)
    mine = go.grads(q, k, v, d_out, case["heads"], case["d"] ** -0.5)
    want = _autograd64(case, q, k, v, d_out)
    for t, g, w in zip(("dq", "dk", "dv"), mine, want):
        assert list(g.shape) == case["shape"][t]
        assert np.abs(g - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), t
        ref = FIX[f"{cid}/{t}/ref64"]
        assert np.abs(g.reshape(-1)[FIX[f"{cid}/{t}/idx"]] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), t
        assert 0 <= case["e_ref"][t] < 1e-4


def test_fixture_covers_the_cases_and_fits():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "attention_grad.npz")) < 1 << 20
    want = {(2, 4, 70, 70, 40), (2, 4, 70, 77, 40), (3, 4, 9, 9, 160), (5, 2, 100, 100, 80), (2, 1, 64, 64, 64), (1, 1, 33, 1, 4)}
    assert {(c["heads"], c["samples"], c["n"], c["n_k"], c["d"]) for c in CASES.values() if c["kind"] == "value"} == want
    sharp = [c for c in CASES.values() if c["kind"] == "sharp"]
    assert len(sharp) == 1 and (sharp[0]["heads"], sharp[0]["samples"], sharp[0]["n"], sharp[0]["n_k"], sharp[0]["d"]) == (2, 4, 70, 70, 40)
    bn = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "bn_attention.npz"))["meta"]))
    assert {c["gain"] for c in bn["cases"] if c["kind"] == "sharp"} == {sharp[0]["gain"]}
    single = CASES["grad_1x1x33x1x4"]   # one key: softmax = 1, dq and dk are zero in every arithmetic
    assert single["e_ref"]["dq"] == 0 and single["e_ref"]["dk"] == 0
    assert META["factor"] == 4.0 and all(r <= META["factor"] for c in CASES.values() for r in c["tile_ratio"].values())


def test_tile_order_restatement_stays_within_the_factor():
    """The float32 restatement in the kernels' order, on the smallest cases: the condition of the GPU test is attainable."""
    for cid in ("grad_3x4x9x9x160", "grad_1x1x33x1x4"):
        case = CASES[cid]
        q, k, v = go.case_inputs(case)
        d_out = go.case_d_out(case)
        scale = case["d"] ** -0.5
        ref = go.grads(q, k, v, d_out, case["heads"], scale)
        got = go.grads_tiled(q, k, v, d_out, case["heads"], scale)
        for t, g, w in zip(("dq", "dk", "dv"), got, ref):
            assert np.abs(g.astype(np.float64) - w).max() <= META["factor"] * case["e_ref"][t], (cid, t)
        lse = go.lse2(q, k, scale)
        assert np.abs(got[4] - lse).max() <= 1e-5 * np.abs(lse).max()


def test_diffusion_utils_imports_and_refuses_a_controller():
    from comfystereo_amd import diffusion_utils, stereo_utils

    class Poison:
        """Any attribute access (the UNet lookup probes attributes) fails the test."""
        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name}) before the controller was refused")

    with pytest.raises(TypeError):
        diffusion_utils.register_attention_control(Poison(), object())
    # controller=None installs on the modules named CrossAttention, by the reference's names, and restore_attention undoes it
    net = go.toy_model({k: FIX["toy/w/" + k] for k in META["toy"]["weights"]})
    mods = [net.down_blocks[0], net.down_blocks[1], net.mid_block, net.up_blocks[0]]
    assert diffusion_utils.register_attention_control(net, None) == 4
    assert all("forward" in m.__dict__ and hasattr(m, stereo_utils._SAVED_FORWARD) for m in mods)
    x, ctx, _ = (torch.from_numpy(t) for t in go.toy_inputs())
    with pytest.raises(ValueError):
        net.mid_block(x, ctx, torch.ones(2, 77, dtype=torch.bool))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            net.mid_block(x, ctx)
    stereo_utils.restore_attention(net)
    assert all("forward" not in m.__dict__ and not hasattr(m, stereo_utils._SAVED_FORWARD) for m in mods)


def test_engine_checks_raise_before_any_pointer_is_passed():
    from comfystereo_amd import engine
    f = torch.zeros
    q, k = f(4, 8, 40), f(4, 9, 40)
    bad = [
        (f(4, 8, 40, dtype=torch.float16), k, k),      # dtype
        (f(4, 8), k, k),                               # not 3-d
        (f(4, 40, 8).transpose(1, 2), k, k),           # not contiguous
        (q, k, f(4, 10, 40)),                          # k and v differ
        (f(4, 8, 42), f(4, 9, 42), f(4, 9, 42)),       # d not a multiple of 4
        (f(4, 8, 164), f(4, 9, 164), f(4, 9, 164)),    # d above the limit
        (f(3, 8, 40), f(3, 9, 40), f(3, 9, 40)),       # batch not b * heads
        (q, k, k),                                     # well-formed, but host memory
    ]
    for a, b, c in bad:
        with pytest.raises(ValueError):
            engine.attention_lse(a, b, c, 2, 0.1)
    with pytest.raises(ValueError):
        engine.attention_lse(q, k, k, 2, float("inf"))
    out, lse, d_out = f(2, 8, 80), f(4, 8), f(2, 8, 80)
    for o, l, g in ((f(2, 8, 40), lse, d_out), (out, f(4, 9), d_out), (out, lse, f(2, 8, 80).double()), (out, lse, d_out)):
        with pytest.raises(ValueError):
            engine.attention_backward(q, k, k, o, l, g, 2, 0.1)
