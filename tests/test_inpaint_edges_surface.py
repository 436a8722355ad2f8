"""The reference side of tests/test_gpu_inpaint_edges.py, without a GPU: the conditions under which a bit-for-bit comparison with
tools/inpaint_edge_inputs.reference_step says something.  Seeding the PLMS restatement's state equals stepping it; the operand
table's outputs are mostly finite, reach float16's subnormals and both zeros; it tells the guidance scales and the history slots
apart; and CPU torch gives the same bits whatever the order of the elements."""
import functools

import pytest
import torch

import inpaint_edge_inputs as ei
import plms_oracle

HALF = ("float16", "bfloat16")
DTYPES = ("float32",) + HALF
NUM_STEPS = 6


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    """NaNs equal whatever their payload, as the GPU file compares."""
    return bool(((bits(a) == bits(b)) | (a.isnan() & b.isnan())).all())


@functools.lru_cache(maxsize=None)
def table(dtype_name):
    return ei.table(getattr(torch, dtype_name))


@functools.lru_cache(maxsize=None)
def reference(dtype_name, kind, guidance):
    return ei.reference_step(kind, table(dtype_name), guidance, NUM_STEPS, ei.KIND_COUNTER[kind])


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_seeding_the_oracle_equals_stepping_it(dtype_name):
    dtype = getattr(torch, dtype_name)
    g = torch.Generator().manual_seed(2)
    shape, guidance = (1, 4, 5, 7), 7.3
    sch = plms_oracle.PLMSOracle()
    sch.set_timesteps(NUM_STEPS)
    latents = torch.randn(shape, generator=g).to(dtype)
    kinds, first_sample = [], None
    assert len(sch.timesteps) == NUM_STEPS + 1
    for counter, t in enumerate(sch.timesteps):
        u, c = (torch.randn(shape, generator=g).to(dtype) for _ in range(2))
        kept = list(sch.ets)                         # before the step, the oldest first
        kind = ("first", "second", "order2", "order3", "order4")[min(counter, 4)]
        kinds.append(kind)
        first_sample = latents if counter == 0 else first_sample
        e = u + guidance * (c - u)
        want = sch.step(e, t, latents).prev_sample
        ops = {"sample": first_sample if kind == "second" else latents, "u": u, "t": c}
        for name, old in zip(("e1", "e2", "e3"), reversed(kept)):
            ops[name] = old
        prev, e_ref, dec = ei.reference_step(kind, ops, guidance, NUM_STEPS, counter)
        assert same_bits(prev, want) and same_bits(e_ref, e) and same_bits(dec, want / 0.18215), (dtype_name, counter, kind)
        latents = want
    assert kinds == ["first", "second", "order2", "order3", "order4", "order4", "order4"]


@pytest.mark.parametrize("kind", ei.KINDS)
@pytest.mark.parametrize("dtype_name", HALF)
def test_the_tables_outputs_are_mostly_finite(dtype_name, kind):
    """A condition on the inputs, not a tolerance: a table whose outputs were mostly NaN would compare equal vacuously.  The floor
    holds for the step's own outputs, prev and e; prev / 0.18215 leaves float16's range 5.5 times earlier and is printed only."""
    subnormal = 0
    for guidance in ei.GUIDANCES:
        for name, out in zip(("prev", "e", "decode_in"), reference(dtype_name, kind, guidance)):
            share = float(out.isfinite().float().mean())
            print(dtype_name, kind, guidance, name, "finite share", share)
            assert share >= 0.9 or name == "decode_in", (dtype_name, kind, guidance, name, share)
        prev = reference(dtype_name, kind, guidance)[0]
        subnormal += int(((prev != 0) & (prev.abs() < torch.finfo(prev.dtype).smallest_normal)).sum())
    if dtype_name == "float16" and kind != "order4":
        assert subnormal > 0, kind


@pytest.mark.parametrize("kind", ei.KINDS)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_signed_zero_table_gives_both_zeros(dtype_name, kind):
    dtype = getattr(torch, dtype_name)
    ops = ei.signed_zero_table(dtype)
    assert len({tuple(bits(ops[n])[k].item() for n in ei.OPERANDS) for k in range(64)}) == 64
    neg = bits(torch.tensor([-0.0], dtype=dtype))[0]
    seen = {"prev": set(), "e": set()}
    for guidance in ei.GUIDANCES:
        prev, e, _ = ei.reference_step(kind, ops, guidance, NUM_STEPS, ei.KIND_COUNTER[kind])
        for name, out in (("prev", prev), ("e", e)):
            assert bool((out == 0).all())
            seen[name] |= set(bits(out).tolist())
            print(dtype_name, kind, guidance, name, "negative zeros", int((bits(out) == neg).sum()), "of", out.numel())
    # over the scales: with a positive one e = u + g * (t - u) is -0 for no signs of u and t (t - u is -0 only when u is +0);
    # the negative scale gives it
    assert seen["prev"] == {0, int(neg)} and seen["e"] == {0, int(neg)}, (dtype_name, kind, seen)


@pytest.mark.parametrize("dtype_name", HALF)
def test_the_guidance_scales_differ_in_e(dtype_name):
    for every in ("sample", "t"):
        ops = ei.table(getattr(torch, dtype_name), every)
        a = ei.reference_step("first", ops, 7.3, NUM_STEPS, 0)[1]
        b = ei.reference_step("first", ops, 7.5, NUM_STEPS, 0)[1]
        assert not same_bits(a, b), (dtype_name, every)


@pytest.mark.parametrize("dtype_name", HALF)
def test_the_table_tells_the_history_slots_apart(dtype_name):
    ops = table(dtype_name)
    for kind, (a, b) in (("order3", ("e1", "e2")), ("order4", ("e2", "e3")), ("order4", ("e1", "e3"))):
        swapped = dict(ops)
        swapped[a], swapped[b] = ops[b], ops[a]
        got = ei.reference_step(kind, swapped, 7.5, NUM_STEPS, ei.KIND_COUNTER[kind])[0]
        assert not same_bits(got, reference(dtype_name, kind, 7.5)[0]), (dtype_name, kind, a, b)


@pytest.mark.parametrize("dtype_name", HALF)
def test_the_reference_does_not_depend_on_the_order_of_evaluation(dtype_name):
    """The same elements in another order -- other lanes of torch's vector loop, others in its scalar tail -- give the same bits."""
    ops = table(dtype_name)
    perm = torch.randperm(ops["sample"].numel() - 5, generator=torch.Generator().manual_seed(3))   # (a length with a scalar tail)
    shuffled = {name: v[perm].contiguous() for name, v in ops.items()}
    for kind in ei.KINDS:
        got = ei.reference_step(kind, shuffled, 7.3, NUM_STEPS, ei.KIND_COUNTER[kind])
        for out, want in zip(got, reference(dtype_name, kind, 7.3)):
            assert same_bits(out, want[perm]), (dtype_name, kind)
