"""The float16 / bfloat16 side of tools/attention_oracle.py: the seeded inputs of tests/golden/bn_attention_half.npz, rounded to
the dtype, and the float64 restatement on those rounded inputs (the yardstick of the half kernel's value tests).

A case of the half fixture is a case of attention_oracle (same fields, same seeded float32 streams) plus
  dtype   "float16" or "bfloat16": q, k, v are the float32 streams rounded to nearest-even in that dtype;
  gain    routing cases only: q_i = gain * k_target(i) instead of attention_oracle's 1024 * k_target(i).  The reference computes
          the scores in the tensors' own dtype, and 1024 * d overflows float16; tools/make_attention_half_goldens.py records the
          largest power of two at which the reference itself returns the targets' v rows bit for bit.
Everything here returns float32 arrays whose values are exactly representable in the case's dtype; to_torch() converts without
rounding.  attention_oracle.py is not touched, so bn_attention.npz regenerates as before.
"""
import numpy as np

import attention_oracle as ao

DTYPES = ("float16", "bfloat16")
ABI_DTYPE = {"float16": 0, "bfloat16": 1}   # enum cs_attn_dtype


def round_to(x, dtype):
    """float32 array -> float32 array of the values rounded to nearest-even in `dtype` (finite inputs)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "float16":
        return x.astype(np.float16).astype(np.float32)
    assert dtype == "bfloat16"
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(x.shape)


def case_inputs(case):
    """q, k, v of a half-fixture case: float32 arrays holding values of case['dtype']."""
    q, k, v = ao.case_inputs(case)
    if case["kind"] == "routing":
        q = q * np.float32(case["gain"] / 1024.0)   # a power of two: exact
    return tuple(round_to(t, case["dtype"]) for t in (q, k, v))


def reference64(case, q, k, v):
    """The float64 restatement on the half-rounded inputs -> [(c s b), n, (h d)] float64."""
    return ao.attention(q, k, v, case["heads"], case["d"] ** -0.5, case["mode"], case["chunks"])


def routing_expected(case, v):
    """The (half-rounded) v rows the targets select, float32 holding values of the dtype."""
    return ao.routing_expected(case, v)


def to_torch(a, dtype, device=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if device is not None:
        t = t.to(device)
    return t.to(getattr(torch, dtype))
