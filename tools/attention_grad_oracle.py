"""Restatement of the gradients of the plain attention the reference's diffusion_utils.register_attention_control installs
(diffusion_utils.py:180-205: sim = einsum(q, k) * scale, attn = softmax(sim), out = einsum(attn, v), heads folded back) in numpy,
and the seeded inputs of tests/golden/attention_grad.npz.

q [(b h), n, d], k and v [(b h), n_k, d]; out and d_out [(b), n, (h d)].  With dO = d_out unfolded to [(b h), n, d]:
  P = softmax(scale * q k^T),  O = P v,  delta_i = sum_c dO[i, c] O[i, c],  dP = dO v^T,  dS = P o (dP - delta)
  dv = P^T dO,   dk = scale * dS^T q,   dq = scale * dS k

grads(...)        float64: the yardstick of the value tests.
grads_tiled(...)  float32 in the order of the HIP kernels (cs_attention_bwd.hip): the forward's online softmax over 32-key tiles
                  leaves lse in log2 units, P is recomputed as exp2(sc2 * s - lse), dq is accumulated over 32-key tiles, dk and
                  dv over 32-query tiles.  The first products (scores, dP) and delta run the MFMA's own chain (chain_dot); inside a
                  tile of the second products numpy's matmul stands in for it: the order of at most 32 float32 additions
                  differs, which is what the tests' factor is for.
"""
import numpy as np

import attention_oracle as ao

LOG2E = 1.44269504088896340736
TILE = 32


def unfold(t, heads):
    """[(b), n, (h d)] -> [(b h), n, d]"""
    b, n, hd = t.shape
    return np.ascontiguousarray(t.reshape(b, n, heads, hd // heads).transpose(0, 2, 1, 3)).reshape(b * heads, n, hd // heads)


def fold(t, heads):
    """[(b h), n, d] -> [(b), n, (h d)]"""
    bh, n, d = t.shape
    return np.ascontiguousarray(t.reshape(bh // heads, heads, n, d).transpose(0, 2, 1, 3)).reshape(bh // heads, n, heads * d)


def lse2(q, k, scale):
    """float64 log2-sum-exp2 of the scaled scores, [(b h), n]: what cs_attention_fwd_lse stores."""
    s = np.einsum("bid,bjd->bij", np.asarray(q, np.float64), np.asarray(k, np.float64)) * (float(scale) * LOG2E)
    m = s.max(-1)
    return m + np.log2(np.exp2(s - m[..., None]).sum(-1))


def grads(q, k, v, d_out, heads, scale):
    """float64 -> (dq, dk, dv)"""
    q, k, v, d_out = (np.asarray(t, np.float64) for t in (q, k, v, d_out))
    do = unfold(d_out, heads)
    s = np.einsum("bid,bjd->bij", q, k) * float(scale)
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    o = np.einsum("bij,bjd->bid", p, v)
    delta = (do * o).sum(-1, keepdims=True)
    ds = p * (np.einsum("bid,bjd->bij", do, v) - delta)
    dv = np.einsum("bij,bid->bjd", p, do)
    dq = np.einsum("bij,bjd->bid", ds, k) * float(scale)
    dk = np.einsum("bij,bid->bjd", ds, q) * float(scale)
    return dq, dk, dv


def chain_dot(a, b):
    """a [(b h), n, d], b [(b h), m, d] float32 -> a . b^T [(b h), n, m] float32 as v_mfma_f32_32x32x2_f32 sums it in the kernels:
    one fmaf per column, k-step 4 g + t taking column 8 g + t and then column 8 g + 4 + t.  (The float32 product is exact in
    float64; the float64 sum rounded to float32 is fmaf up to a double rounding that needs a tie in the 29 dropped bits.)"""
    d = a.shape[-1]
    order = [c for g in range(0, d, 8) for t in range(4) for c in (g + t, g + 4 + t) if c < d]
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    acc = np.zeros(a.shape[:-1] + (b.shape[-2],), np.float32)
    for c in order:
        acc = (acc.astype(np.float64) + a64[..., :, None, c] * b64[..., None, :, c]).astype(np.float32)
    return acc


def chain_rowdot(a, b):
    """a, b [(b h), n, d] float32 -> sum_c a[., i, c] b[., i, c] [(b h), n] float32: chain_dot(a[:, i:i + 1], b[:, i:i + 1])[:, 0, 0]
    for every row i at once, the same fmaf chain in the same column order."""
    d = a.shape[-1]
    order = [c for g in range(0, d, 8) for t in range(4) for c in (g + t, g + 4 + t) if c < d]
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    acc = np.zeros(a.shape[:-1], np.float32)
    for c in order:
        acc = (acc.astype(np.float64) + a64[..., c] * b64[..., c]).astype(np.float32)
    return acc


def lse2_plain32(q, k, scale):
    """lse2 in plain float32 numpy (matmul, max, exp2, sum, log2; no tiling): what float32 arithmetic reaches without any care."""
    f = np.float32
    s = np.matmul(np.asarray(q, f), np.asarray(k, f).transpose(0, 2, 1)) * f(f(scale) * f(LOG2E))
    m = s.max(-1)
    return (m + np.log2(np.exp2(s - m[..., None]).sum(-1, dtype=f))).astype(f)


def grads_tiled(q, k, v, d_out, heads, scale):
    """float32, the kernels' tile order -> (dq, dk, dv, out, lse)"""
    f = np.float32
    q, k, v, d_out = (np.asarray(t, f) for t in (q, k, v, d_out))
    do = unfold(d_out, heads)
    bh, n, d = q.shape
    n_k = k.shape[1]
    scale = f(scale)
    sc2 = f(scale * f(LOG2E))
    s2 = chain_dot(q, k) * sc2          # scores in log2 units, as the kernels hold them
    # forward: online softmax over 32-key tiles
    m = np.full((bh, n), -np.inf, f)
    l = np.zeros((bh, n), f)
    acc = np.zeros((bh, n, d), f)
    for j0 in range(0, n_k, TILE):
        st = s2[:, :, j0:j0 + TILE]
        m_new = np.maximum(m, st.max(-1))
        alpha = np.exp2(m - m_new).astype(f)
        pt = np.exp2(st - m_new[..., None]).astype(f)
        l = (l * alpha + pt.sum(-1, dtype=f)).astype(f)
        acc = (acc * alpha[..., None] + np.matmul(pt, v[:, j0:j0 + TILE])).astype(f)
        m = m_new
    o = (acc / l[..., None]).astype(f)
    lse = (m + np.log2(l).astype(f)).astype(f)
    delta = chain_rowdot(do, o)   # (row by row: the same chain as dP)
    p = np.exp2(s2 - lse[..., None]).astype(f)
    dp = chain_dot(do, v)
    ds = (p * (dp - delta[..., None])).astype(f)
    dq = np.zeros((bh, n, d), f)
    for j0 in range(0, n_k, TILE):
        dq = (dq + np.matmul(ds[:, :, j0:j0 + TILE], k[:, j0:j0 + TILE])).astype(f)
    dk = np.zeros((bh, n_k, d), f)
    dv = np.zeros((bh, n_k, d), f)
    for i0 in range(0, n, TILE):
        dk = (dk + np.matmul(ds[:, i0:i0 + TILE].transpose(0, 2, 1), q[:, i0:i0 + TILE])).astype(f)
        dv = (dv + np.matmul(p[:, i0:i0 + TILE].transpose(0, 2, 1), do[:, i0:i0 + TILE])).astype(f)
    return (dq * scale).astype(f), (dk * scale).astype(f), dv, fold(o, heads), lse


def case_inputs(case):
    """q, k, v of a fixture case: attention_oracle.case_inputs (the case carries its keys)."""
    return ao.case_inputs(case)


def case_d_out(case):
    """The seeded upstream gradient of a fixture case, in out's layout [(b), n, (h d)], float32."""
    rs = np.random.RandomState(case["seed"] + 104729)
    return rs.standard_normal((case["samples"], case["n"], case["heads"] * case["d"])).astype(np.float32)


# ---- the toy stack of the fixture (diffusion_utils.register_attention_control) ------------------------------------------------
TOY = dict(dim=80, heads=2, tokens=70, ctx_tokens=77, ctx_dim=48, batch=2, seed=4321)


def toy_model(state=None, dtype=None):
    """A stand-in for a UNet whose attention modules are of a class named exactly `CrossAttention`, as the reference's walk wants
    (diffusion_utils.py:270): `down_blocks` (self-attention, then cross-attention on the context), `mid_block` (cross-attention)
    and `up_blocks` (self-attention), applied as a residual stack.  state: the fixture's weights {name: array}."""
    import torch
    import torch.nn as nn

    class CrossAttention(nn.Module):
        def __init__(self, ctx_dim=None):
            super().__init__()
            dim = TOY["dim"]
            self.heads = TOY["heads"]
            self.scale = (dim // self.heads) ** -0.5
            self.to_q = nn.Linear(dim, dim, bias=False)
            self.to_k = nn.Linear(ctx_dim or dim, dim, bias=False)
            self.to_v = nn.Linear(ctx_dim or dim, dim, bias=False)
            self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Dropout(0.0)])

        def reshape_heads_to_batch_dim(self, t):
            b, n, hd = t.shape
            h = self.heads
            return t.reshape(b, n, h, hd // h).permute(0, 2, 1, 3).reshape(b * h, n, hd // h)

        def reshape_batch_dim_to_heads(self, t):
            bh, n, d = t.shape
            h = self.heads
            return t.reshape(bh // h, h, n, d).permute(0, 2, 1, 3).reshape(bh // h, n, h * d)

        def forward(self, x, context=None, mask=None):
            ctx = x if context is None else context
            q, k, v = (self.reshape_heads_to_batch_dim(t) for t in (self.to_q(x), self.to_k(ctx), self.to_v(ctx)))
            attn = (torch.matmul(q, k.transpose(-1, -2)) * self.scale).softmax(-1)
            return self.to_out[0](self.reshape_batch_dim_to_heads(torch.matmul(attn, v)))

    class ToyUNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.down_blocks = nn.ModuleList([CrossAttention(), CrossAttention(TOY["ctx_dim"])])
            self.mid_block = CrossAttention(TOY["ctx_dim"])
            self.up_blocks = nn.ModuleList([CrossAttention()])

        def forward(self, x, context):
            x = x + self.down_blocks[0](x)
            x = x + self.down_blocks[1](x, context)
            x = x + self.mid_block(x, context)
            return x + self.up_blocks[0](x)

    torch.manual_seed(TOY["seed"])
    net = ToyUNet()
    if state is not None:
        net.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in state.items()})
    if dtype is not None:
        net = net.to(dtype)
    return net.eval()


def toy_inputs():
    """x [batch, tokens, dim], the context embedding [batch, ctx_tokens, ctx_dim] and the MSE target, float32."""
    rs = np.random.RandomState(TOY["seed"] + 1)
    x = rs.standard_normal((TOY["batch"], TOY["tokens"], TOY["dim"])).astype(np.float32)
    ctx = rs.standard_normal((TOY["batch"], TOY["ctx_tokens"], TOY["ctx_dim"])).astype(np.float32)
    target = rs.standard_normal((TOY["batch"], TOY["tokens"], TOY["dim"])).astype(np.float32)
    return x, ctx, target


def toy_grads(net, device=None, dtype=None):
    """MSE loss of the stack's output against the target, backward() -> (output, d loss / d context, d loss / d x) as numpy."""
    import torch
    x, ctx, target = (torch.from_numpy(t) for t in toy_inputs())
    if dtype is not None:
        x, ctx, target = x.to(dtype), ctx.to(dtype), target.to(dtype)
    if device is not None:
        x, ctx, target = x.to(device), ctx.to(device), target.to(device)
    x.requires_grad_(True)
    ctx.requires_grad_(True)
    out = net(x, ctx)
    torch.nn.functional.mse_loss(out, target).backward()
    return out.detach().cpu().numpy(), ctx.grad.cpu().numpy(), x.grad.cpu().numpy()
