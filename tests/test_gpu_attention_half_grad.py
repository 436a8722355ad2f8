"""cs_attention_half_fwd_lse / cs_attention_half_bwd and the diffusion_utils drop-in with stereo_utils.HALF_ATTENTION on the GPU
against tests/golden/attention_half_grad.npz, in float16 and bfloat16: gradients within FACTOR x the reference's own error in that
dtype of float64, the forward bit for bit cs_stereo_attention_half's, bit-identical repeats in every workgroup shape, untouched
guard rows, the autograd function with and without native_half, the toy stack, the no-grad route, the memory bound and refusals
that write nothing."""
import ctypes
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import attention_grad_oracle as go  # noqa: E402
import attention_half_grad_oracle as hgo  # noqa: E402

from comfystereo_amd import _native, diffusion_utils, engine, stereo_utils  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(ROOT, "tests", "golden", "attention_half_grad.npz"))
META = json.loads(str(FIX["meta"]))
CASES = {c["id"]: c for c in META["cases"]}
GRAD_FIX = np.load(os.path.join(ROOT, "tests", "golden", "attention_grad.npz"))
FACTOR = 4.0   # the project's accuracy condition: at most FACTOR times further from float64 than the reference in the same dtype
assert META["factor"] == FACTOR
SHORTS = ("f16", "bf16")
DTYPE = {"f16": "float16", "bf16": "bfloat16"}


def factor_for(case, t):
    """FACTOR, or -- for a tensor whose restatement in the kernels' arithmetic itself misses it on the CPU -- twice that ratio."""
    r = case["tile_ratio"][t]
    return FACTOR if r <= FACTOR else max(FACTOR, 2.0 * r)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Inputs (values of the dtype, as float32) and the float64 gradients of a case, computed once and shared read-only."""
    case = CASES[cid]
    q, k, v = hgo.case_inputs(case)
    d_out = hgo.case_d_out(case)
    g64 = hgo.grads64(case, q, k, v, d_out)
    for a in (q, k, v, d_out) + tuple(g64):
        a.setflags(write=False)
    return q, k, v, d_out, g64


def device_inputs(cid):
    case = CASES[cid]
    return tuple(hgo.to_torch(np.array(t), case["dtype"], "cuda") for t in reference(cid)[:4])


def backward(cid):
    case = CASES[cid]
    q, k, v, d_out = device_inputs(cid)
    scale = case["d"] ** -0.5
    out, lse = engine.attention_lse(q, k, v, case["heads"], scale)
    return engine.attention_backward(q, k, v, out, lse, d_out, case["heads"], scale)


def check_grads(cid, grads, tag=""):
    case = CASES[cid]
    q, k, v, d_out, g64 = reference(cid)
    tdt = getattr(torch, case["dtype"])
    bounds = hgo.single_key_bounds(case, q, k, v, d_out) if case["n_k"] == 1 else None
    for j, (t, g, w) in enumerate(zip(("dq", "dk", "dv"), grads, g64)):
        assert g.dtype == tdt and list(g.shape) == case["shape"][t] and bool(torch.isfinite(g).all()), t
        got = g.float().cpu().numpy().astype(np.float64)
        err = np.abs(got - w).max()
        e_ref = case["e_ref"][t]
        print(f"{cid}{tag} {t}: max|grad - float64| = {err:.3e}, e_ref = {e_ref:.3e}, ratio {err / e_ref if e_ref else float(err != 0):.2f}")
        if e_ref == 0:
            # a single key: the exact gradient is zero; what float32 summation order alone allows (single_key_bounds)
            print(f"  max bound {bounds[j].max():.3e}")
            assert (np.abs(got) <= bounds[j]).all(), t
            continue
        assert err <= factor_for(case, t) * e_ref, (t, err, e_ref)
        # the fixture's own sample of the reference's float64 gradients
        assert np.abs(got.reshape(-1)[FIX[f"{cid}/{t}/idx"]] - FIX[f"{cid}/{t}/ref64"]).max() <= factor_for(case, t) * e_ref + 1e-12, t


def ids_of(*stems):
    return [f"{s}_{dt}" for s in stems for dt in SHORTS]


@pytest.mark.parametrize("cid", sorted(CASES))
def test_gradients_within_the_reference_error(cid):
    check_grads(cid, backward(cid))


@pytest.mark.parametrize("cid", sorted(CASES))
def test_forward_is_bit_identical_and_lse_is_right(cid):
    case = CASES[cid]
    q, k, v, _ = device_inputs(cid)
    scale = case["d"] ** -0.5
    out, lse = engine.attention_lse(q, k, v, case["heads"], scale)
    assert out.dtype == q.dtype and lse.dtype == torch.float32
    assert torch.equal(out, engine.stereo_attention(q, k, v, case["heads"], scale, "self"))
    want = hgo.lse64(case, *reference(cid)[:2])
    err = np.abs(lse.cpu().numpy().astype(np.float64) - want)
    assert lse.shape == want.shape and bool((err <= 1e-5 * np.abs(want)).all()), err.max()


@pytest.mark.parametrize("cid", ids_of("hgrad_2x4x70x77x40", "hgrad_3x4x9x9x160", "hgrad_5x2x100x100x80"))
def test_backward_is_deterministic_in_every_workgroup_shape(cid):
    first = backward(cid)
    again = backward(cid)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for waves in (1, 2):
        _native.debug_set("attn_waves", waves)
        try:
            one, two = backward(cid), backward(cid)
        finally:
            _native.debug_set("attn_waves", 0)
        assert all(torch.equal(a, b) for a, b in zip(one, two)), waves
        check_grads(cid, one, tag=f" waves={waves}")


@pytest.mark.parametrize("cid", ids_of("hgrad_2x4x70x77x40", "hgrad_3x4x9x9x160", "hgrad_1x1x33x1x8"))
def test_guard_rows_stay_untouched(cid):
    """Every output buffer of the C ABI is followed by a guard row of sentinels; partial tiles must not reach it."""
    case = CASES[cid]
    q, k, v, d_out = device_inputs(cid)
    b, h, n, n_k, d = case["samples"], case["heads"], case["n"], case["n_k"], case["d"]
    L = _native.lib()
    SENT = 12288.0   # exact in float16 and bfloat16
    code = hgo.ABI_DTYPE[case["dtype"]]

    def guarded(rows, width, dtype=q.dtype):
        return torch.full((rows + 1, width), SENT, device="cuda", dtype=dtype)

    out, lse = guarded(b * n, h * d), guarded(b * h, n, torch.float32)
    dq, dk, dv = guarded(b * h * n, d), guarded(b * h * n_k, d), guarded(b * h * n_k, d)
    nb = L.cs_attention_half_bwd_workspace_bytes(b, h, n, n_k, d)
    ws = torch.full((nb // 4 + 64,), SENT, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    scale = d ** -0.5
    _native.check(L.cs_attention_half_fwd_lse(p(q), p(k), p(v), p(out), p(lse), code, b, h, n, n_k, d, scale, st))
    _native.check(L.cs_attention_half_bwd(p(q), p(k), p(v), p(out), p(lse), p(d_out), p(dq), p(dk), p(dv), code, b, h, n, n_k, d, scale,
                                          p(ws), nb, st))
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool((t[-1] == SENT).all()), name
    assert bool((ws[nb // 4:] == SENT).all())
    want = backward(cid)
    assert torch.equal(dq[:-1].reshape(want[0].shape), want[0]) and torch.equal(dk[:-1].reshape(want[1].shape), want[1])
    assert torch.equal(dv[:-1].reshape(want[2].shape), want[2])


@pytest.mark.parametrize("dt", SHORTS)
def test_autograd_with_native_half(dt):
    cid = "hgrad_2x4x70x77x40_" + dt
    case = CASES[cid]
    q, k, v, d_out = device_inputs(cid)
    scale = case["d"] ** -0.5
    tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = engine.differentiable_attention(tq, tk, tv, case["heads"], scale, native_half=True)
    assert out.dtype == q.dtype
    assert torch.equal(out.detach(), engine.stereo_attention(q, k, v, case["heads"], scale, "self"))
    # what is saved for the backward: the half tensors and the float32 lse, no float32 copy
    saved = out.grad_fn.saved_tensors
    assert sorted(str(t.dtype) for t in saved) == sorted([str(q.dtype)] * 4 + ["torch.float32"])
    assert [t.shape for t in saved if t.dtype == torch.float32] == [torch.Size([q.shape[0], q.shape[1]])]
    out.backward(d_out.transpose(0, 1).contiguous().transpose(0, 1))   # a non-contiguous upstream gradient
    check_grads(cid, (tq.grad, tk.grad, tv.grad), tag=" autograd native_half")
    assert all(torch.equal(a, b) for a, b in zip((tq.grad, tk.grad, tv.grad), backward(cid)))


@pytest.mark.parametrize("dt", SHORTS)
def test_autograd_default_is_the_upcast_path(dt):
    cid = "hgrad_2x4x70x77x40_" + dt
    case = CASES[cid]
    q, k, v, d_out = device_inputs(cid)
    heads, scale = case["heads"], case["d"] ** -0.5
    tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = engine.differentiable_attention(tq, tk, tv, heads, scale)
    out.backward(d_out)
    # the parent's upcast, spelled out on the float32 entry points
    q32, k32, v32 = q.float(), k.float(), v.float()
    o32, lse = engine.attention_lse(q32, k32, v32, heads, scale)
    want_out = o32.to(q.dtype)
    g32 = engine.attention_backward(q32, k32, v32, o32, lse, d_out.float(), heads, scale)
    assert out.dtype == q.dtype and torch.equal(out.detach(), want_out)
    for got, want in zip((tq.grad, tk.grad, tv.grad), g32):
        assert got.dtype == q.dtype and torch.equal(got, want.to(q.dtype))
    # native_half with an input the half kernels do not take falls back to the same upcast
    tq2 = q.clone().requires_grad_(True)
    mixed = engine.differentiable_attention(tq2, k.float(), v.float(), heads, scale, native_half=True)
    assert mixed.dtype == q.dtype and torch.equal(mixed.detach(), want_out)


def toy_on_gpu(dtype):
    weights = json.loads(str(GRAD_FIX["meta"]))["toy"]["weights"]
    state = hgo.toy_state({k: GRAD_FIX["toy/w/" + k] for k in weights}, dtype)
    return go.toy_model(state, getattr(torch, dtype)).cuda()


@pytest.mark.parametrize("dt", SHORTS)
def test_toy_stack_gradients_and_restore(dt):
    dtype = DTYPE[dt]
    toy = META["toy"][dtype]
    net = toy_on_gpu(dtype)
    assert diffusion_utils.register_attention_control(net, None) == 4
    stereo_utils.HALF_ATTENTION = True
    try:
        res = hgo.toy_grads(net, dtype, getattr(torch, dtype), device="cuda")
    finally:
        stereo_utils.HALF_ATTENTION = False
    for t, g in zip(("out", "d_context", "d_x"), res):
        assert list(g.shape) == toy["shape"][t] and np.isfinite(g).all()
        err = np.abs(g.reshape(-1)[FIX[f"toy_{dt}/{t}/idx"]] - FIX[f"toy_{dt}/{t}/ref64"]).max()
        print(f"toy {dt} {t}: max|got - ref64| = {err:.3e}, e_ref = {toy['e_ref'][t]:.3e}, ratio {err / toy['e_ref'][t]:.2f}")
        assert err <= FACTOR * toy["e_ref"][t], t
    stereo_utils.restore_attention(net)
    fresh = toy_on_gpu(dtype)
    x, ctx, _ = (hgo.to_torch(t, dtype, "cuda") for t in hgo.toy_inputs(dtype))
    with torch.no_grad():
        assert torch.equal(net(x, ctx), fresh(x, ctx))
    assert all("forward" not in m.__dict__ for m in net.modules())


@pytest.mark.parametrize("dt", SHORTS)
def test_no_grad_route_is_the_half_inference_kernel(dt):
    dtype = DTYPE[dt]
    net = toy_on_gpu(dtype)
    layer = net.mid_block
    x, ctx, _ = (hgo.to_torch(t, dtype, "cuda") for t in hgo.toy_inputs(dtype))
    diffusion_utils.register_attention_control(net, None)
    with torch.no_grad():
        q, k, v = (layer.reshape_heads_to_batch_dim(t).contiguous() for t in (layer.to_q(x), layer.to_k(ctx), layer.to_v(ctx)))
        want = layer.to_out[0](engine.stereo_attention(q, k, v, layer.heads, layer.scale, "self"))
        upcast = layer.to_out[0](engine.stereo_attention(q.float(), k.float(), v.float(), layer.heads, layer.scale, "self").to(q.dtype))
        stereo_utils.HALF_ATTENTION = True
        try:
            got = layer(x, ctx)
        finally:
            stereo_utils.HALF_ATTENTION = False
        assert got.dtype == x.dtype and torch.equal(got, want) and not got.requires_grad
        assert torch.equal(layer(x, ctx), upcast)   # the switch off: the upcast, as before
    stereo_utils.restore_attention(net)


def test_memory_stays_below_one_half_score_matrix_and_the_default():
    heads, n, d = 8, 1024, 40
    gen = torch.Generator(device="cuda").manual_seed(5)
    q, k, v = (torch.randn(heads, n, d, device="cuda", generator=gen).half().requires_grad_(True) for _ in range(3))
    d_out = torch.randn(1, n, heads * d, device="cuda", generator=gen).half()

    def growth(**kwargs):
        q.grad = k.grad = v.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        out = engine.differentiable_attention(q, k, v, heads, d ** -0.5, **kwargs)
        out.backward(d_out)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    default = growth()
    native = growth(native_half=True)
    print(f"forward + backward growth: native_half {native} bytes, default {default} bytes, one half score matrix {heads * n * n * 2} bytes")
    assert native < heads * n * n * 2
    assert native < default
    assert q.grad is not None and q.grad.dtype == torch.float16 and bool(torch.isfinite(q.grad).all())


def test_refusals_write_nothing():
    L = _native.lib()
    count = 4 * 9 * 168
    outs = [torch.full((count,), 7.0, device="cuda", dtype=torch.float16) for _ in range(4)]
    o, dq, dk, dv = outs
    l = torch.full((count,), 7.0, device="cuda")
    ws = torch.full((4096,), 7.0, device="cuda")
    ins = [torch.zeros(count, device="cuda", dtype=torch.float16) for _ in range(3)]        # q, k, v
    out_in, d_out = torch.zeros(count, device="cuda", dtype=torch.float16), torch.zeros(count, device="cuda", dtype=torch.float16)
    lse_in = torch.zeros(count, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i = [p(t) for t in ins]
    fwd = lambda d, dtype=0, out=o: L.cs_attention_half_fwd_lse(*i, p(out), p(l), dtype, 2, 2, 8, 9, d, 0.1, st)  # noqa: E731
    need = L.cs_attention_half_bwd_workspace_bytes(2, 2, 8, 9, 40)
    bwd = lambda d, nb=need, dtype=0, dq_=dq: L.cs_attention_half_bwd(*i, p(out_in), p(lse_in), p(d_out), p(dq_), p(dk), p(dv), dtype,  # noqa: E731
                                                                      2, 2, 8, 9, d, 0.1, p(ws), nb, st)
    assert fwd(44) == _native.CS_ELIMIT and fwd(164) == _native.CS_ELIMIT
    assert fwd(40, dtype=2) == _native.CS_EINVAL
    assert fwd(40, out=ins[0]) == _native.CS_EINVAL
    assert bwd(44) == _native.CS_ELIMIT and bwd(164) == _native.CS_ELIMIT
    assert bwd(40, dtype=7) == _native.CS_EINVAL
    assert bwd(40, nb=need - 1) == _native.CS_EWORKSPACE
    assert bwd(40, dq_=out_in) == _native.CS_EINVAL       # dq aliases out
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [l, ws])
    assert all(bool((t == 0).all()) for t in ins + [out_in, d_out, lse_in])
    z = lambda n_: torch.zeros(4, n_, 44, device="cuda", dtype=torch.float16)  # noqa: E731
    with pytest.raises(ValueError):
        engine.attention_lse(z(8), z(9), z(9), 2, 0.1)
