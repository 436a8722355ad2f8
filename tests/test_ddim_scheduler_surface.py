"""comfystereo_amd.schedulers.DDIMScheduler against its independent statement tools/ddim_oracle.py, and the argument refusals of
engine.standard_step (no gpu)."""
import pytest
import torch

import ddim_oracle as do
from comfystereo_amd import engine, inpaint_runner, inversion, schedulers

DTYPES = [torch.float32, torch.float16, torch.bfloat16]


@pytest.mark.parametrize("n", [1, 5, 10, 50, 100, 1000])
def test_timesteps_are_leading_spaced(n):
    s = schedulers.DDIMScheduler()
    s.set_timesteps(n)
    assert s.num_inference_steps == n and s.timesteps.dtype == torch.int64
    assert s.timesteps.tolist() == do.ddim_timesteps(n) == [k * (1000 // n) for k in range(n - 1, -1, -1)]
    assert s.timesteps[-1] == 0 and s.config.num_train_timesteps == 1000


def test_alphas_are_the_inpainting_runners_bit_for_bit():
    s = schedulers.DDIMScheduler()
    assert torch.equal(s.alphas_cumprod.view(torch.int32), inpaint_runner.scaled_linear_alphas_cumprod().view(torch.int32))
    assert torch.equal(s.alphas_cumprod, do.DDIMOracle().alphas_cumprod)
    assert s.final_alpha_cumprod == s.alphas_cumprod[0]           # set_alpha_to_one=False
    assert schedulers.DDIMScheduler(set_alpha_to_one=True).final_alpha_cumprod == 1.0
    x = torch.ones(3)
    assert s.scale_model_input(x, 5) is x
    # the helpers moved here; inversion and inpaint_runner still find them
    assert inversion._sqrt is schedulers._sqrt and inpaint_runner._operand is schedulers._operand


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_coeffs_and_host_step_equal_the_oracle(dtype):
    s, o = schedulers.DDIMScheduler(), do.DDIMOracle()
    g = torch.Generator().manual_seed(2)
    sample = torch.randn((2, 4, 9, 7), generator=g).to(dtype)
    eps = torch.randn((2, 4, 9, 7), generator=g).to(dtype)
    for n in (1, 10, 50):
        s.set_timesteps(n)
        o.set_timesteps(n)
        for t in s.timesteps.tolist():
            a_t, a_prev = do.alphas_of_step(o.alphas_cumprod, o.final_alpha_cumprod, t, n)
            if t == 0:
                assert a_prev == o.alphas_cumprod[0] == a_t       # the last step goes to final_alpha_cumprod
            want = do.coefficients(a_t, a_prev, dtype)
            assert s.coeffs(t, dtype) == want, (n, t)
            assert all(float(torch.tensor(v, dtype=torch.float32)) == v for v in want)
            out = s.step(eps, t, sample)
            assert out["prev_sample"] is out.prev_sample and out.prev_sample.dtype == dtype
            assert torch.equal(out.prev_sample, o.step(eps, t, sample)["prev_sample"]), (n, t)
            assert torch.equal(out.prev_sample, do.step_rounded(eps, sample, want, dtype)), (n, t)
    # NullInversion's "prev" coefficients are these
    s.set_timesteps(10)
    inv = inversion.NullInversion.__new__(inversion.NullInversion)
    inv.model, inv._coeffs = type("M", (), {"scheduler": s})(), {}
    assert inv._step_coeffs("prev", 500, dtype) == s.coeffs(500, dtype)


def test_scheduler_refusals():
    with pytest.raises(ValueError):
        schedulers.DDIMScheduler(beta_schedule="linear")
    with pytest.raises(ValueError):
        schedulers.DDIMScheduler(clip_sample=True)
    s = schedulers.DDIMScheduler()
    with pytest.raises(ValueError):
        s.coeffs(0, torch.float32)
    for n in (0, 1001):
        with pytest.raises(ValueError):
            s.set_timesteps(n)


# ---- engine.standard_step refuses before the library is reached -----------------------------------------------------------------------
def good(dtype=torch.float32, b=1, c=4, h=3, w=5):
    return dict(noise_pred=torch.zeros((4 * b, c, h, w), dtype=dtype), x=torch.zeros((4 * b, c, h, w), dtype=dtype), guidance=3.0,
                coeffs=(0.5, 0.5, 0.5, 0.5), op="first", src_col=torch.zeros((b, h, w), dtype=torch.int32),
                mask=torch.zeros((b, h, w), dtype=torch.uint8), noise=torch.zeros((b, c, h, w), dtype=dtype))


BAD = {
    "dtype mix": dict(noise_pred=torch.zeros((4, 4, 3, 5), dtype=torch.float16)),
    "double": dict(x=torch.zeros((4, 4, 3, 5), dtype=torch.float64)),
    "noise dtype": dict(noise=torch.zeros((1, 4, 3, 5), dtype=torch.bfloat16)),
    "x rows": dict(x=torch.zeros((2, 4, 3, 5)), noise_pred=torch.zeros((2, 4, 3, 5))),
    "x dims": dict(x=torch.zeros((4, 4, 15))),
    "noise_pred shape": dict(noise_pred=torch.zeros((4, 4, 3, 6))),
    "noise shape": dict(noise=torch.zeros((2, 4, 3, 5))),
    "src_col shape": dict(src_col=torch.zeros((1, 3, 6), dtype=torch.int32)),
    "src_col dtype": dict(src_col=torch.zeros((1, 3, 5), dtype=torch.int64)),
    "mask dtype": dict(mask=torch.zeros((1, 3, 5), dtype=torch.bool)),
    "x not contiguous": dict(x=torch.zeros((4, 4, 5, 3)).transpose(2, 3)),
    "noise_pred not contiguous": dict(noise_pred=torch.zeros((4, 4, 5, 3)).transpose(2, 3)),
    "src_col not contiguous": dict(src_col=torch.zeros((1, 5, 3), dtype=torch.int32).transpose(1, 2)),
    "noise with reshift": dict(op="reshift"),
    "noise with none": dict(op="none"),
    "first without src_col": dict(src_col=None),
    "first without mask": dict(mask=None),
    "reshift without mask": dict(op="reshift", noise=None, mask=None),
    "unknown op": dict(op="shift"),
    "c2 zero": dict(coeffs=(0.5, 0.0, 0.5, 0.5)),
    "three coeffs": dict(coeffs=(0.5, 0.5, 0.5)),
    "nan guidance": dict(guidance=float("nan")),
    "inf coeff": dict(coeffs=(0.5, 0.5, float("inf"), 0.5)),
    "too wide": dict(x=torch.zeros((4, 1, 1, 8193)), noise_pred=torch.zeros((4, 1, 1, 8193)), op="none", noise=None),
    "x requires grad": dict(x=torch.zeros((4, 4, 3, 5), requires_grad=True)),
    "not a tensor": dict(x=[0.0]),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_standard_step_refuses(name, monkeypatch):
    def unreachable():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(engine._native, "lib", unreachable)
    with pytest.raises(ValueError):
        engine.standard_step(**{**good(), **BAD[name]})


def test_standard_step_without_a_gpu_gets_past_the_checks_only(monkeypatch):
    """Host tensors that pass every check are refused for being host tensors, last."""
    monkeypatch.setattr(engine._native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    for op, extra in (("first", {}), ("reshift", dict(noise=None)), ("none", dict(noise=None, src_col=None, mask=None))):
        with pytest.raises((ValueError, RuntimeError), match="device-resident|MI355X"):
            engine.standard_step(**{**good(), "op": op, **extra})


# ---- the fixture of the loop under a real DDIM step -------------------------------------------------------------------------------------
def test_fixture_is_what_the_oracle_driven_loop_gives_and_covers_the_cases():
    """tests/golden/standard_ddim.npz holds the reference's own loop over the fake model and the host DDIMOracle; its maker
    asserts that make_standard_ddim_goldens.restate_case -- the same loop without the reference -- equals it.  One small case is
    recomputed here; every case is present, with the coverage the maker's docstring states, within the size a file may have."""
    import json
    import os

    import numpy as np

    import make_standard_ddim_goldens as mk
    assert os.path.getsize(mk.OUT) < 1 << 20
    z = np.load(mk.OUT)
    meta = json.loads(str(z["meta"]))
    cases = {c["id"]: c for c in meta["cases"]}
    assert list(cases) == [c[0] for c in mk.CASES] and meta["guidance_scale"] == mk.GUIDANCE and meta["margin"] >= mk.MARGIN
    for key, values in (("dtype", {"float32", "float16", "bfloat16"}), ("steps", {5, 10}), ("direction", {"uni", "bi"}),
                        ("deblur", {True, False})):
        assert {c[key] for c in cases.values()} == values
    c = cases["f16_5_bi_uncond"]
    again = mk.restate_case(c["dtype"], c["steps"], c["direction"], c["deblur"], c["uncond"])
    for k, v in again.items():
        assert np.array_equal(v, z[f"{c['id']}/{k}"]), k
    assert 0 < z[f"{c['id']}/mask"].mean() < 1
