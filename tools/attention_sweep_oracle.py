"""What the attention sweep (tests/golden/attention_sweep.npz) shares between its generator and its tests: one entry point per
question -- inputs, float64 yardsticks, the restatement in the kernels' arithmetic -- that sends a case to the float32 oracles
(attention_oracle, attention_grad_oracle) or to the half ones (attention_half_oracle, attention_half_grad_oracle) by its dtype.
Nothing is restated here.

A case is a case of those oracles (id, kind, mode, chunks, heads, samples, n, n_k, d, seed) plus
  dtype   "float32", "float16" or "bfloat16";
  kind    "value" (the seeded normal streams) or "ramp" (attention_oracle.ramp_inputs; span and noise ride in the case).
SELF cases run the forward, the forward with LSE and the backward (tensors out, dq, dk, dv); UNI / BI cases the forward (out).
"""
import numpy as np

import attention_grad_oracle as go
import attention_half_grad_oracle as hgo
import attention_oracle as ao

SHORT = {"float32": "f32", "float16": "f16", "bfloat16": "bf16"}
DTYPES = tuple(SHORT)
FACTOR = 4.0

F32_DIMS = (4, 12, 32, 36, 64, 68, 96, 100, 128, 132, 156, 160)
HALF_DIMS = (8, 24, 32, 40, 64, 72, 96, 104, 128, 136, 160)
SELF_PAIRS = ((33, 31), (128, 32), (129, 65), (1, 33), (31, 129), (65, 127), (32, 33), (127, 64), (161, 1))   # (n, n_k)
VIEW_NS = (31, 32, 33, 63, 64, 65, 127, 128, 129)                                                             # UNI / BI: n_k = n
RAMP_PAIRS = ((64, 129), (33, 127))
RAMP_DIMS = (40, 128)
GUARD = ((129, 65, 128), (1, 33, 100), (161, 1, 96))   # (n, n_k, d) of the guard-row cases in float32; float16 takes half_dim(d)


def is_half(case):
    return case["dtype"] != "float32"


def nd(d):
    """The kernels' template parameter: 32-column blocks of the head dimension."""
    return (d + 31) // 32


def dims(dtype):
    return F32_DIMS if dtype == "float32" else HALF_DIMS


def half_dim(d):
    """The half grid's head dimension nearest to a float32 one (the half kernels take multiples of 8); of two, the one with d's ND."""
    return min(HALF_DIMS, key=lambda h: (abs(h - d), nd(h) != nd(d)))


def tensors(case):
    return ("out", "dq", "dk", "dv") if case["mode"] == "self" else ("out",)


def case_inputs(case):
    """q, k, v as float32 arrays holding values of the case's dtype."""
    return hgo.case_inputs(case) if is_half(case) else go.case_inputs(case)


def case_d_out(case):
    return hgo.case_d_out(case) if is_half(case) else go.case_d_out(case)


def forward64(case, q, k, v):
    """[(c s b), n, (h d)] float64"""
    return ao.attention(q, k, v, case["heads"], case["d"] ** -0.5, case["mode"], case["chunks"])


def grads64(case, q, k, v, d_out):
    return go.grads(q, k, v, d_out, case["heads"], case["d"] ** -0.5)


def lse64(case, q, k):
    return go.lse2(q, k, case["d"] ** -0.5)


def lse_plain32(case, q, k):
    return go.lse2_plain32(q, k, case["d"] ** -0.5)


def lse_ok(got, want):
    """The sweep's LSE bound: 1e-5 relative to max(|want|, 1).  (With a single key an lse is one scaled score and can be
    arbitrarily close to 0: a purely relative bound is then no property of the arithmetic.)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    return bool((err <= 1e-5 * np.maximum(np.abs(want), 1.0)).all()), float(err.max())


def restated(case, q, k, v, d_out):
    """(dq, dk, dv, out, lse) in the kernels' arithmetic: grads_tiled (float32) or grads_kernel (half)."""
    if is_half(case):
        return hgo.grads_kernel(case, q, k, v, d_out)
    return go.grads_tiled(q, k, v, d_out, case["heads"], case["d"] ** -0.5)


def single_key_bounds(case, q, k, v, d_out):
    return hgo.single_key_bounds(case, q, k, v, d_out)


def factor_for(case, t):
    """FACTOR; for a gradient whose restatement in the kernels' arithmetic itself misses it on the CPU, twice that ratio."""
    r = case.get("tile_ratio", {}).get(t, 0.0)
    return FACTOR if r <= FACTOR else max(FACTOR, 2.0 * r)


def forced_waves(case):
    """The forced workgroup shapes a case runs in besides the default: the ones whose query-tile edge its n straddles, and both
    for the ramps."""
    if case["kind"] == "ramp":
        return (1, 2)
    return ((1,) if case["n"] in (31, 32, 33) else ()) + ((2,) if case["n"] in (63, 64, 65) else ())
