"""cs_attention_fwd_lse / cs_attention_bwd and the diffusion_utils drop-in on the GPU against tests/golden/attention_grad.npz:
gradients within FACTOR x the reference's own float32 error of float64, the forward bit for bit cs_stereo_attention's, bit-identical
repeats, untouched guard rows, the toy stack through register_attention_control / restore_attention, the no-grad route, the
memory bound (less than one score matrix) and refusals that write nothing."""
import copy
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

from comfystereo_amd import _native, diffusion_utils, engine, stereo_utils  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(ROOT, "tests", "golden", "attention_grad.npz"))
META = json.loads(str(FIX["meta"]))
CASES = {c["id"]: c for c in META["cases"]}
FACTOR = 4.0   # the factor of tests/test_gpu_attention.py: the same float32 products, summed in another order
assert META["factor"] == FACTOR


def factor_for(case, t):
    """FACTOR, or -- for a tensor whose tile-order float32 restatement itself misses it on the CPU -- twice that restatement's ratio."""
    r = case["tile_ratio"][t]
    return FACTOR if r <= FACTOR else max(FACTOR, 2.0 * r)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Inputs and the float64 gradients of a case, computed once and shared (read-only) by the tests."""
    case = CASES[cid]
    q, k, v = go.case_inputs(case)
    d_out = go.case_d_out(case)
    g64 = go.grads(q, k, v, d_out, case["heads"], case["d"] ** -0.5)
    for a in (q, k, v, d_out) + tuple(g64):
        a.setflags(write=False)
    return q, k, v, d_out, g64


def device_inputs(cid):
    q, k, v, d_out, _ = reference(cid)
    return tuple(torch.from_numpy(np.array(t)).cuda() for t in (q, k, v, d_out))


def backward(cid):
    case = CASES[cid]
    q, k, v, d_out = device_inputs(cid)
    scale = case["d"] ** -0.5
    out, lse = engine.attention_lse(q, k, v, case["heads"], scale)
    return engine.attention_backward(q, k, v, out, lse, d_out, case["heads"], scale)


def check_grads(cid, grads, tag=""):
    case = CASES[cid]
    g64 = reference(cid)[4]
    for t, g, w in zip(("dq", "dk", "dv"), grads, g64):
        assert g.dtype == torch.float32 and list(g.shape) == case["shape"][t] and bool(torch.isfinite(g).all()), t
        got = g.cpu().numpy().astype(np.float64)
        err = np.abs(got - w).max()
        e_ref = case["e_ref"][t]
        print(f"{cid}{tag} {t}: max|grad - float64| = {err:.3e}, e_ref = {e_ref:.3e}, ratio {err / e_ref if e_ref else float(err != 0):.2f}")
        assert err <= factor_for(case, t) * e_ref, (t, err, e_ref)
        # the fixture's own sample of the reference's float64 gradients
        assert np.abs(got.reshape(-1)[FIX[f"{cid}/{t}/idx"]] - FIX[f"{cid}/{t}/ref64"]).max() <= factor_for(case, t) * e_ref + 1e-12, t


@pytest.mark.parametrize("cid", sorted(CASES))
def test_gradients_within_the_reference_error(cid):
    check_grads(cid, backward(cid))


def test_single_key_gives_exactly_zero_dq_and_dk():
    dq, dk, dv = backward("grad_1x1x33x1x4")
    assert bool((dq == 0).all()) and bool((dk == 0).all()) and bool((dv != 0).any())


@pytest.mark.parametrize("cid", sorted(CASES))
def test_forward_is_bit_identical_and_lse_is_right(cid):
    case = CASES[cid]
    q, k, v, _ = device_inputs(cid)
    scale = case["d"] ** -0.5
    out, lse = engine.attention_lse(q, k, v, case["heads"], scale)
    assert torch.equal(out, engine.stereo_attention(q, k, v, case["heads"], scale, "self"))
    want = go.lse2(*reference(cid)[:2], scale)
    err = np.abs(lse.cpu().numpy().astype(np.float64) - want)
    assert lse.shape == want.shape and bool((err <= 1e-5 * np.abs(want)).all()), err.max()


@pytest.mark.parametrize("cid", ("grad_2x4x70x77x40", "grad_3x4x9x9x160", "grad_5x2x100x100x80"))
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


@pytest.mark.parametrize("cid", ("grad_2x4x70x77x40", "grad_3x4x9x9x160", "grad_1x1x33x1x4"))
def test_guard_rows_stay_untouched(cid):
    """Every output buffer of the C ABI is followed by a guard row of sentinels; partial tiles must not reach it."""
    case = CASES[cid]
    q, k, v, d_out = device_inputs(cid)
    b, h, n, n_k, d = case["samples"], case["heads"], case["n"], case["n_k"], case["d"]
    L = _native.lib()
    SENT = 12345.0

    def guarded(rows, width):
        return torch.full((rows + 1, width), SENT, device="cuda")

    out, lse = guarded(b * n, h * d), guarded(b * h, n)
    dq, dk, dv = guarded(b * h * n, d), guarded(b * h * n_k, d), guarded(b * h * n_k, d)
    nb = L.cs_attention_bwd_workspace_bytes(b, h, n, n_k, d)
    ws = torch.full((nb // 4 + 64,), SENT, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    scale = d ** -0.5
    _native.check(L.cs_attention_fwd_lse(p(q), p(k), p(v), p(out), p(lse), b, h, n, n_k, d, scale, st))
    _native.check(L.cs_attention_bwd(p(q), p(k), p(v), p(out), p(lse), p(d_out), p(dq), p(dk), p(dv), b, h, n, n_k, d, scale, p(ws), nb, st))
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool((t[-1] == SENT).all()), name
    assert bool((ws[nb // 4:] == SENT).all())
    want = backward(cid)
    assert torch.equal(dq[:-1].reshape(want[0].shape), want[0]) and torch.equal(dk[:-1].reshape(want[1].shape), want[1])
    assert torch.equal(dv[:-1].reshape(want[2].shape), want[2])


def test_autograd_function_and_half_inputs():
    cid = "grad_2x4x70x77x40"
    case = CASES[cid]
    q, k, v, d_out = device_inputs(cid)
    scale = case["d"] ** -0.5
    tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = engine.differentiable_attention(tq, tk, tv, case["heads"], scale)
    assert torch.equal(out.detach(), engine.stereo_attention(q, k, v, case["heads"], scale, "self"))
    out.backward(d_out.transpose(0, 1).contiguous().transpose(0, 1))   # a non-contiguous upstream gradient
    check_grads(cid, (tq.grad, tk.grad, tv.grad), tag=" autograd")
    hq, hk, hv = (t.to(torch.bfloat16).requires_grad_(True) for t in (q, k, v))
    oh = engine.differentiable_attention(hq, hk, hv, case["heads"], scale)
    oh.float().sum().backward()
    assert oh.dtype == torch.bfloat16 and hq.grad.dtype == torch.bfloat16 and bool(torch.isfinite(hk.grad.float()).all())


def toy_on_gpu():
    return go.toy_model({k: FIX["toy/w/" + k] for k in META["toy"]["weights"]}).cuda()


def test_toy_stack_gradients_and_restore():
    toy = META["toy"]
    net = toy_on_gpu()
    assert diffusion_utils.register_attention_control(net, None) == 4
    res = go.toy_grads(net, device="cuda")
    for t, g in zip(("out", "d_context", "d_x"), res):
        assert list(g.shape) == toy["shape"][t] and np.isfinite(g).all()
        err = np.abs(g.astype(np.float64).reshape(-1)[FIX[f"toy/{t}/idx"]] - FIX[f"toy/{t}/ref64"]).max()
        print(f"toy {t}: max|got - ref64| = {err:.3e}, e_ref = {toy['e_ref'][t]:.3e}, ratio {err / toy['e_ref'][t]:.2f}")
        assert err <= FACTOR * toy["e_ref"][t], t
    stereo_utils.restore_attention(net)
    fresh = toy_on_gpu()
    x, ctx, _ = (torch.from_numpy(t).cuda() for t in go.toy_inputs())
    with torch.no_grad():
        assert torch.equal(net(x, ctx), fresh(x, ctx))
    assert all("forward" not in m.__dict__ for m in net.modules())


def test_an_editor_stacks_on_the_hook_and_restore_undoes_both():
    net = toy_on_gpu()
    diffusion_utils.register_attention_control(net, None)
    ed = stereo_utils.BNAttention(start_step=10 ** 6)
    stereo_utils.register_attention_editor_diffusers(net, ed)
    assert ed.num_att_layers == 4
    stereo_utils.restore_attention(net)
    assert all("forward" not in m.__dict__ for m in net.modules())


def test_no_grad_route_is_the_inference_kernel():
    net = toy_on_gpu()
    layer = net.mid_block
    x, ctx, _ = (torch.from_numpy(t).cuda() for t in go.toy_inputs())
    diffusion_utils.register_attention_control(net, None)
    with torch.no_grad():
        got = layer(x, ctx)
        q, k, v = (layer.reshape_heads_to_batch_dim(t).contiguous() for t in (layer.to_q(x), layer.to_k(ctx), layer.to_v(ctx)))
        want = layer.to_out[0](engine.stereo_attention(q, k, v, layer.heads, layer.scale, "self"))
    assert torch.equal(got, want) and not got.requires_grad and got.grad_fn is None
    # the ComfyUI call convention: value as the third positional argument, transformer_options, further keywords
    wrapper = type("Wrapper", (), {})()
    wrapper.comfy_model = type("M", (), {})()
    wrapper.comfy_model.model = type("M", (), {})()
    wrapper.comfy_model.model.diffusion_model = net
    diffusion_utils.register_attention_control(wrapper, None)
    with torch.no_grad():
        assert torch.equal(layer(x, ctx, None, None, transformer_options={}, extra=1), want)
        assert torch.equal(layer(x, context=ctx, value=ctx), want)


def test_memory_stays_below_one_score_matrix():
    heads, n, d = 8, 1024, 40
    gen = torch.Generator(device="cuda").manual_seed(5)
    q, k, v = (torch.randn(heads, n, d, device="cuda", generator=gen).requires_grad_(True) for _ in range(3))
    d_out = torch.randn(1, n, heads * d, device="cuda", generator=gen)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    out = engine.differentiable_attention(q, k, v, heads, d ** -0.5)
    out.backward(d_out)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    print(f"forward + backward growth {growth} bytes, one score matrix {heads * n * n * 4} bytes")
    assert growth < heads * n * n * 4
    assert q.grad is not None and bool(torch.isfinite(q.grad).all())


def test_refusals_write_nothing():
    L = _native.lib()
    buf = torch.zeros(4 * 8 * 9 * 164, device="cuda")
    outs = [torch.full((4 * 8 * 9 * 164,), 7.0, device="cuda") for _ in range(5)]
    ins = [torch.zeros(4 * 8 * 9 * 164, device="cuda") for _ in range(6)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o, l, dq, dk, dv = outs
    ws = torch.full((4096,), 7.0, device="cuda")
    i = [p(t) for t in ins]
    assert L.cs_attention_fwd_lse(i[0], i[1], i[2], p(o), p(l), 2, 2, 8, 9, 42, 0.1, st) == _native.CS_ELIMIT
    assert L.cs_attention_fwd_lse(i[0], i[1], i[2], p(o), p(l), 2, 2, 8, 9, 164, 0.1, st) == _native.CS_ELIMIT
    assert L.cs_attention_fwd_lse(i[0], i[1], i[2], i[0], p(l), 2, 2, 8, 9, 40, 0.1, st) == _native.CS_EINVAL
    bwd = lambda d, nb, dq_=dq: L.cs_attention_bwd(*i, p(dq_), p(dk), p(dv), 2, 2, 8, 9, d, 0.1, p(ws), nb, st)  # noqa: E731
    need = L.cs_attention_bwd_workspace_bytes(2, 2, 8, 9, 40)
    assert bwd(42, 16384) == _native.CS_ELIMIT
    assert bwd(164, 16384) == _native.CS_ELIMIT
    assert bwd(40, need - 1) == _native.CS_EWORKSPACE
    assert bwd(40, need, ins[3]) == _native.CS_EINVAL      # dq aliases out
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [ws]) and all(bool((t == 0).all()) for t in ins + [buf])
    for name in ("attention_lse", "differentiable_attention"):
        with pytest.raises(ValueError):
            getattr(engine, name)(torch.zeros(4, 8, 42, device="cuda"), torch.zeros(4, 9, 42, device="cuda"),
                                  torch.zeros(4, 9, 42, device="cuda"), 2, 0.1)
    # the forward-only entry points keep refusing tensors that require grad
    with pytest.raises(ValueError):
        qg = torch.zeros(4, 8, 40, device="cuda", requires_grad=True)
        engine.stereo_attention(qg, qg.detach(), qg.detach(), 2, 0.1, "self")
