"""The float16 / bfloat16 side of tools/attention_grad_oracle.py: the seeded inputs of tests/golden/attention_half_grad.npz rounded
to the dtype, the float64 gradients on those rounded inputs (the yardstick of the value tests), and a restatement in the arithmetic
of the half kernels (cs_attention_half.hip with LSE, cs_attention_half_bwd.hip).

A case is a case of attention_grad_oracle plus
  dtype      "float16" or "bfloat16": q, k, v and d_out are the float32 streams rounded to nearest-even in that dtype
             (attention_half_oracle.round_to);
  d_out_mul  optional power of two that multiplies d_out BEFORE the rounding (the small-gradient case: 2^-12, the size of an MSE
             loss's gradient over a latent, where float16 can lose dS).
Everything returns float32 arrays whose values are representable in the case's dtype, or float64.

grads_kernel(...) follows the kernels where they round:
  * scores and dP: the half-input MFMA multiplies half operands exactly and accumulates in float32; the float64 sum of the exact
    products, rounded once to float32, stands in for its internal order (which is not documented);
  * forward: online softmax over 32-key tiles in float32, P rounded to the dtype for P . V, the row sum taken from the unrounded
    float32 P, one division and one rounding of `out`; lse = m + log2(l) in float32;
  * delta: a float32 fmaf chain over the columns of dO * O;
  * P = exp2(sc2 * s - lse) and dS = P * (dP - delta) in float32, both rounded to the dtype (float16: gradual underflow, no
    power-of-two scaling) as operands of dV, dK, dQ;
  * dQ accumulated over 32-key tiles, dK and dV over 32-query tiles, in float32, one k-step of 16 rows at a time;
  * `* scale` in float32 and ONE rounding to the dtype on store.
"""
import numpy as np

import attention_grad_oracle as go
import attention_half_oracle as aho

DTYPES = aho.DTYPES
ABI_DTYPE = aho.ABI_DTYPE
SHORT = {"float16": "f16", "bfloat16": "bf16"}
LOG2E = go.LOG2E
TILE = 32
KSTEP = 16


def case_inputs(case):
    """q, k, v of a half-gradient case: float32 arrays holding values of case['dtype']."""
    return tuple(aho.round_to(t, case["dtype"]) for t in go.case_inputs(case))


def case_d_out(case):
    """The upstream gradient [(b), n, (h d)]: attention_grad_oracle's stream times d_out_mul, rounded to the dtype."""
    return aho.round_to(go.case_d_out(case) * np.float32(case.get("d_out_mul", 1.0)), case["dtype"])


def grads64(case, q, k, v, d_out):
    """float64 (dq, dk, dv) on the rounded inputs."""
    return go.grads(q, k, v, d_out, case["heads"], case["d"] ** -0.5)


def lse64(case, q, k):
    return go.lse2(q, k, case["d"] ** -0.5)


def _dot32(a, b):
    """a [., n, c], b [., m, c] holding half values -> a . b^T, exact products, one rounding to float32."""
    return np.einsum("bic,bjc->bij", a.astype(np.float64), b.astype(np.float64)).astype(np.float32)


def _acc_steps(acc, a, b):
    """acc [., m, c] float32 += a^T . b over the rows of a [., r, m] and b [., r, c] (half values), KSTEP rows per MFMA."""
    for r0 in range(0, a.shape[1], KSTEP):
        part = np.einsum("brm,brc->bmc", a[:, r0:r0 + KSTEP].astype(np.float64), b[:, r0:r0 + KSTEP].astype(np.float64))
        acc = (acc.astype(np.float64) + part).astype(np.float32)
    return acc


def grads_kernel(case, q, k, v, d_out):
    """The kernels' arithmetic -> (dq, dk, dv, out, lse): gradients and out as float32 arrays of dtype values, lse float32."""
    f = np.float32
    dt, heads = case["dtype"], case["heads"]
    q, k, v, d_out = (np.asarray(t, f) for t in (q, k, v, d_out))
    do = go.unfold(d_out, heads)
    bh, n, d = q.shape
    n_k = k.shape[1]
    scale = f(case["d"] ** -0.5)
    sc2 = f(scale * f(LOG2E))
    s2 = (_dot32(q, k) * sc2).astype(f)
    # forward
    m = np.full((bh, n), -np.inf, f)
    l = np.zeros((bh, n), f)
    acc = np.zeros((bh, n, d), f)
    for j0 in range(0, n_k, TILE):
        st = s2[:, :, j0:j0 + TILE]
        m_new = np.maximum(m, st.max(-1))
        alpha = np.exp2(m - m_new).astype(f)
        pt = np.exp2(st - m_new[..., None]).astype(f)
        l = (l * alpha + pt.sum(-1, dtype=f)).astype(f)
        acc = (acc * alpha[..., None]).astype(f)
        acc = _acc_steps(acc, aho.round_to(pt, dt).transpose(0, 2, 1), v[:, j0:j0 + TILE])
        m = m_new
    o = aho.round_to((acc / l[..., None]).astype(f), dt)
    lse = (m + np.log2(l).astype(f)).astype(f)
    # backward
    delta = np.zeros((bh, n), f)
    for c in range(d):
        delta = (delta.astype(np.float64) + do[..., c].astype(np.float64) * o[..., c].astype(np.float64)).astype(f)
    p = np.exp2(s2 - lse[..., None]).astype(f)
    ds = (p * (_dot32(do, v) - delta[..., None]).astype(f)).astype(f)
    ph, dsh = aho.round_to(p, dt), aho.round_to(ds, dt)
    dq = np.zeros((bh, n, d), f)
    for j0 in range(0, n_k, TILE):
        dq = _acc_steps(dq, dsh[:, :, j0:j0 + TILE].transpose(0, 2, 1), k[:, j0:j0 + TILE])
    dk = np.zeros((bh, n_k, d), f)
    dv = np.zeros((bh, n_k, d), f)
    for i0 in range(0, n, TILE):
        dk = _acc_steps(dk, dsh[:, i0:i0 + TILE], q[:, i0:i0 + TILE])
        dv = _acc_steps(dv, ph[:, i0:i0 + TILE], do[:, i0:i0 + TILE])
    rnd = lambda t: aho.round_to(np.asarray(t, f), dt)  # noqa: E731
    return rnd(dq * scale), rnd(dk * scale), rnd(dv), go.fold(o, heads), lse


def single_key_bounds(case, q, k, v, d_out):
    """One key: softmax = 1, the exact dq and dk are zero, and what is left is float32 summation order.  delta(i) and dP(i, 0)
    are two float32 sums of the same d exact products dO(i, c) V(0, c) (out = V(0) bit for bit), each within
    d 2^-24 A_i of the exact sum, A_i = sum_c |dO(i, c) V(0, c)|, so |dS(i)| <= P 2 d 2^-24 A_i with P = exp2(sc2 s - lse) = 1 up to
    the same kind of error in s.  dq(i, c) = scale dS(i) K(0, c); dk(0, c) = scale sum_i dS(i) Q(i, c).  The roundings of dS and of
    the stored value to the dtype, P's distance from 1 and the float32 accumulation of dk are covered by the slack 1 + 2^-4.
    -> (|dq| bound [(b h), n, d], |dk| bound [(b h), 1, d]) float64"""
    assert case["n_k"] == 1
    d = case["d"]
    do = go.unfold(np.asarray(d_out, np.float32), case["heads"]).astype(np.float64)
    a = np.abs(do * np.asarray(v, np.float64)).sum(-1)                      # [(b h), n]
    ds = 2.0 * d * 2.0 ** -24 * a * (1.0 + 2.0 ** -4)
    scale = case["d"] ** -0.5
    dq = scale * ds[..., None] * np.abs(np.asarray(k, np.float64))          # K(0, :) broadcasts over the queries
    dk = scale * np.einsum("bi,bic->bc", ds, np.abs(np.asarray(q, np.float64)))[:, None, :]
    return dq, dk


def to_torch(a, dtype, device=None):
    return aho.to_torch(a, dtype, device)


# ---- the toy stack (attention_grad_oracle.toy_model) in a half dtype ----------------------------------------------------------
def toy_state(state, dtype):
    """The fixture's float32 weights rounded to the dtype."""
    return {k_: aho.round_to(np.asarray(a), dtype) for k_, a in state.items()}


def toy_inputs(dtype):
    """attention_grad_oracle.toy_inputs rounded to the dtype."""
    return tuple(aho.round_to(t, dtype) for t in go.toy_inputs())


def toy_grads(net, dtype, compute, device=None):
    """MSE loss of the stack on the half-rounded inputs, computed in torch dtype `compute` -> (out, d loss / d context, d loss / d x)
    as float64 numpy arrays."""
    import torch
    x, ctx, target = (torch.from_numpy(t) for t in toy_inputs(dtype))
    if device is not None:
        x, ctx, target = x.to(device), ctx.to(device), target.to(device)
    x, ctx, target = x.to(compute).requires_grad_(True), ctx.to(compute).requires_grad_(True), target.to(compute)
    out = net(x, ctx)
    torch.nn.functional.mse_loss(out, target).backward()
    return tuple(t.detach().double().cpu().numpy() for t in (out, ctx.grad, x.grad))
