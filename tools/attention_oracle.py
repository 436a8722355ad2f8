"""Restatement of the reference's stereo attention (stereo_utils.py BNAttention :91-188) in numpy, and the seeded inputs of
tests/golden/bn_attention.npz.

The reference's rearranges are index maps.  With q [(c s b h), n, d] and k, v [(c s b h), n_k, d] viewed as [c, s, b, h, ., d]:
  self  the query (c, s, b, h, i) sees the keys (c, s, b, h, :)                         forward :137-140 (is_cross or before
        start_step: einsum(attn, v), '(b h) n d -> b n (h d)')
  bi    ... sees (c, 0, b, h, :) followed by (c, 1, b, h, :)                            attn_batch :124-132 on each CFG chunk
        ('(s b h) n d -> (b h) (s n) d' puts the two views' tokens in one sequence), forward :156-162; :142-146 with c = 1
  uni   ... sees (c, 0, b, h, :)                                                        forward :163-171: ku[:_num_heads] is
        the left view's half of the chunk, so attn_batch's rearrange finds s = 1 for k and v
and the result is [(c s b), n, (h d)] (:132 '(b h) (s n) d -> (s b) n (h d)', :175 cat over the chunks; :139).
sim = einsum(q, k) * scale, attn = softmax(sim, -1), out = einsum(attn, v) (:128-131, :238-247).

attention(..., dtype=np.float64) is the yardstick of the value tests, dtype=np.float32 the same arithmetic in the reference's
precision (not its summation order: einsum's and the kernel's orders differ, which is what the tests' e_ref bound is for).
"""
import numpy as np

MODES = ("self", "uni", "bi")


def attention(q, k, v, heads, scale, mode, chunks=1, dtype=np.float64):
    """q [(c s b h), n, d], k / v [(c s b h), n_k, d] -> [(c s b), n, h * d] in `dtype`."""
    assert mode in MODES
    q, k, v = (np.asarray(t, dtype=dtype) for t in (q, k, v))
    bh, n, d = q.shape
    n_k = k.shape[1]
    s = 1 if mode == "self" else 2
    c = 1 if mode == "self" else chunks
    b = bh // (c * s * heads)
    assert c * s * b * heads == bh and k.shape == v.shape == (bh, n_k, d)
    q6 = q.reshape(c, s, b, heads, n, d)
    k6 = k.reshape(c, s, b, heads, n_k, d)
    v6 = v.reshape(c, s, b, heads, n_k, d)
    if mode == "uni":       # the left view's keys for both views
        kk, vv = k6[:, :1], v6[:, :1]
    elif mode == "bi":      # view 0's tokens followed by view 1's, for both views
        kk = np.concatenate([k6[:, 0], k6[:, 1]], axis=-2)[:, None]
        vv = np.concatenate([v6[:, 0], v6[:, 1]], axis=-2)[:, None]
    else:
        kk, vv = k6, v6
    sim = np.einsum("csbhid,csbhjd->csbhij", q6, np.broadcast_to(kk, (c, s) + kk.shape[2:])) * dtype(scale)
    sim = sim - sim.max(-1, keepdims=True)
    e = np.exp(sim)
    attn = e / e.sum(-1, keepdims=True)
    out = np.einsum("csbhij,csbhjd->csbhid", attn, np.broadcast_to(vv, (c, s) + vv.shape[2:]))
    # [c, s, b, h, n, d] -> [(c s b), n, (h d)]
    return np.ascontiguousarray(out.transpose(0, 1, 2, 4, 3, 5)).reshape(c * s * b, n, heads * d).astype(dtype)


def visible_keys(mode, n):
    """Number of keys a query sees (n keys per view)."""
    return 2 * n if mode == "bi" else n


def case_inputs(case):
    """The seeded float32 inputs of a fixture case (meta['cases'] entry) -> q, k, v.  np.random.RandomState streams are frozen
    by NumPy's compatibility policy, so the fixture records seeds, not megabytes of noise."""
    rs = np.random.RandomState(case["seed"])
    heads, b, n, n_k, d = case["heads"], case["samples"], case["n"], case["n_k"], case["d"]
    s = 1 if case["mode"] == "self" else 2
    bh = case["chunks"] * s * b * heads
    if case["kind"] == "routing":
        return routing_inputs(rs, case, bh)
    if case["kind"] == "ramp":
        return ramp_inputs(rs, case, bh)
    g = np.float32(case.get("gain", 1.0))
    q = rs.standard_normal((bh, n, d)).astype(np.float32) * g
    k = rs.standard_normal((bh, n_k, d)).astype(np.float32) * g
    v = rs.standard_normal((bh, n_k, d)).astype(np.float32)
    return q, k, v


def routing_inputs(rs, case, bh):
    """k: random +-1 vectors, pairwise distinct within every visible key set; q_i = 1024 k_target(i): the matching key's score
    leads every other by at least 2048 * scale, softmax is exactly one-hot in float32 and the output is the target's v row,
    bit for bit.  Returns q, k, v; routing_targets(case) are the targets."""
    heads, b, n, d, c = case["heads"], case["samples"], case["n"], case["d"], case["chunks"]
    while True:
        k = (rs.randint(0, 2, (bh, n, d)) * 2 - 1).astype(np.float32)
        k6 = k.reshape(c, 2, b * heads, n, d)
        both = np.concatenate([k6[:, 0], k6[:, 1]], axis=-2).reshape(-1, 2 * n, d)   # the largest visible set
        if all(len(np.unique(rows, axis=0)) == 2 * n for rows in both):
            break
    v = rs.standard_normal((bh, n, d)).astype(np.float32)
    tgt = routing_targets(case)
    q6 = np.empty((c, 2, b * heads, n, d), np.float32)
    t6 = tgt.reshape(c, 2, b * heads, n)
    for ci in range(c):
        for si in range(2):
            for j in range(b * heads):
                keys = np.concatenate([k6[ci, 0, j], k6[ci, 1, j]]) if case["mode"] == "bi" else k6[ci, 0, j]
                q6[ci, si, j] = np.float32(1024.0) * keys[t6[ci, si, j]]
    return q6.reshape(bh, n, d), k, v


def ramp_inputs(rs, case, bh):
    """Scores that climb (or fall) steadily along the keys instead of i.i.d. noise: with a fixed unit vector u,
    k_j = g_j u + noise, g_j rising linearly from 0 to A, and q_i = c_i u + noise, c_i in [0.9 A, 1.1 A] for even i and in
    [-1.1 A, -0.9 A] for odd i, A^2 = span * sqrt(d): a query's scaled scores span about case['span'] nats from the first key to the
    last.  For an even query the running maximum of the online softmax rises on every key tile and ends on the last key (every
    earlier tile's accumulator is rescaled by alpha < 1, the first tiles' probabilities vanish against the final maximum); for an
    odd query the maximum sits in tile 0 and the later tiles underflow.  Neighbouring keys differ by span / n_k nats, so the
    softmax is spread over several keys, not one-hot.  Returns q, k, v."""
    n, n_k, d = case["n"], case["n_k"], case["d"]
    u = rs.standard_normal(d)
    u /= np.sqrt((u * u).sum())
    amp = np.sqrt(case["span"] * np.sqrt(d))
    g = amp * np.arange(n_k) / max(n_k - 1, 1)
    c = amp * (0.9 + 0.2 * rs.random_sample((bh, n))) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    k = g[None, :, None] * u + case["noise"] * rs.standard_normal((bh, n_k, d))
    q = c[..., None] * u + case["noise"] * rs.standard_normal((bh, n, d))
    v = rs.standard_normal((bh, n_k, d))
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32)


def routing_targets(case):
    """[(c s b h), n] int: the index, in its visible key set, of the key each query matches."""
    rs = np.random.RandomState(case["seed"] + 7919)
    bh = case["chunks"] * 2 * case["samples"] * case["heads"]
    return rs.randint(0, visible_keys(case["mode"], case["n"]), (bh, case["n"]))


def routing_expected(case, v):
    """The v rows the targets select, in the output layout [(c s b), n, (h d)]."""
    heads, b, n, d, c = case["heads"], case["samples"], case["n"], case["d"], case["chunks"]
    v6 = v.reshape(c, 2, b, heads, n, d)
    t6 = routing_targets(case).reshape(c, 2, b, heads, n)
    out = np.empty((c, 2, b, n, heads, d), np.float32)
    for ci in range(c):
        for si in range(2):
            for bi in range(b):
                for hi in range(heads):
                    vis = np.concatenate([v6[ci, 0, bi, hi], v6[ci, 1, bi, hi]]) if case["mode"] == "bi" else v6[ci, 0, bi, hi]
                    out[ci, si, bi, :, hi] = vis[t6[ci, si, bi, hi]]
    return out.reshape(c * 2 * b, n, heads * d)


# ---- the toy attention model of the fixture (register_attention_editor_diffusers / restore_attention) -----------------------
TOY = dict(dim=80, heads=2, tokens=6, batch=4, steps=3, layers=2, start_step=1)


def toy_model(state=None, dtype=None):
    """A two-layer stand-in for a UNet: children `down_blocks` (a list holding one attention module) and `mid_block` (one),
    each with to_q / to_k / to_v / to_out like an SD attention block and a plain-attention forward of its own.  state: the
    fixture's weights {name: array}."""
    import torch
    import torch.nn as nn

    class ToyAttention(nn.Module):
        def __init__(self):
            super().__init__()
            dim = TOY["dim"]
            self.heads = TOY["heads"]
            self.scale = (dim // self.heads) ** -0.5
            self.to_q = nn.Linear(dim, dim, bias=False)
            self.to_k = nn.Linear(dim, dim, bias=False)
            self.to_v = nn.Linear(dim, dim, bias=False)
            self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Dropout(0.0)])

        def forward(self, x, encoder_hidden_states=None, attention_mask=None, **kwargs):
            ctx = x if encoder_hidden_states is None else encoder_hidden_states
            b, n, _ = x.shape
            h = self.heads

            def split(t):
                return t.reshape(t.shape[0], t.shape[1], h, -1).permute(0, 2, 1, 3)

            q, k, v = split(self.to_q(x)), split(self.to_k(ctx)), split(self.to_v(ctx))
            attn = (torch.matmul(q, k.transpose(-1, -2)) * self.scale).softmax(-1)
            out = torch.matmul(attn, v).permute(0, 2, 1, 3).reshape(b, n, -1)
            return self.to_out[0](out)

    class ToyUNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.down_blocks = nn.ModuleList([ToyAttention()])
            self.mid_block = ToyAttention()

    torch.manual_seed(1234)
    net = ToyUNet()
    if state is not None:
        net.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in state.items()})
    if dtype is not None:
        net = net.to(dtype)
    return net.eval()


def toy_input(call):
    rs = np.random.RandomState(9000 + call)
    return rs.standard_normal((TOY["batch"], TOY["tokens"], TOY["dim"])).astype(np.float32)


def toy_run(net, register, restore, editor, device=None, dtype=None):
    """steps x layers calls through the registered editor, then one call of each layer after restore ->
    (outputs, [(cur_att_layer, cur_step) after each call], editor.num_att_layers)."""
    import torch
    outs, book = [], []
    layers = [net.down_blocks[0], net.mid_block]

    def x_of(call):
        x = torch.from_numpy(toy_input(call))
        x = x.to(dtype) if dtype is not None else x
        return x.to(device) if device is not None else x

    with torch.no_grad():
        register(net, editor)
        call = 0
        for _step in range(TOY["steps"]):
            for layer in layers:
                outs.append(layer(x_of(call)).cpu().numpy())
                book.append((editor.cur_att_layer, editor.cur_step))
                call += 1
        restore(net)
        for layer in layers:
            outs.append(layer(x_of(call)).cpu().numpy())
            call += 1
    return outs, book, editor.num_att_layers
