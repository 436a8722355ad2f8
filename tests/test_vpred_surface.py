"""v-prediction outside the GPU: the scheduler's prediction type and operand rule, the float64 consistency of the step and of the
loss gradient, model detection, the new exports, the refusals that come before the GPU, work_size, and the fixture (not gpu)."""
import enum
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import make_vpred_goldens as mk
import vpred_oracle as vo
from comfystereo_amd import _native, engine, inversion, model_wrappers, schedulers
from comfystereo_amd import stereodiffusion_nodes as sdn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
V = "v_prediction"
NEW = ["cs_ddim_step_pred", "cs_null_loss_grad_pred", "cs_null_loss_grad_frames_pred", "cs_standard_step_pred"]


# ---- the scheduler -----------------------------------------------------------------------------------------------------------------
def test_scheduler_prediction_type_and_operand_rule():
    assert schedulers.DDIMScheduler().config.prediction_type == "epsilon"
    v = schedulers.DDIMScheduler(prediction_type=V)
    e = schedulers.DDIMScheduler()
    assert v.config.prediction_type == V
    for bad in ("sample", "v", None, 1):
        with pytest.raises(ValueError, match="prediction_type"):
            schedulers.DDIMScheduler(prediction_type=bad)
    v.set_timesteps(10)
    e.set_timesteps(10)
    differs = 0
    for dtype in DTYPES:
        for t in (900, 500, 0):
            cv, ce = v.coeffs(t, dtype), e.coeffs(t, dtype)
            assert (cv[0], cv[2], cv[3]) == (ce[0], ce[2], ce[3])
            f32 = float(torch.tensor(float(v.alphas_cumprod[t]) ** 0.5, dtype=torch.float64).to(torch.float32))
            assert ce[1] == f32                                                                 # a divisor keeps its float32
            assert cv[1] == (f32 if dtype == torch.float32 else float(torch.tensor(f32).to(dtype)))   # a first operand is rounded
            differs += cv[1] != ce[1]
            assert cv == vo.coefficients(v.alphas_cumprod[t], v.alphas_cumprod[t - 100] if t >= 100 else v.final_alpha_cumprod, dtype)
    assert differs >= 4
    v.config.prediction_type = "sample"
    with pytest.raises(ValueError, match="prediction_type"):
        v.step(torch.zeros(4), 900, torch.zeros(4))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_host_step_against_the_restatements(dtype):
    s = schedulers.DDIMScheduler(prediction_type=V)
    s.set_timesteps(10)
    g = torch.Generator().manual_seed(3)
    x, v = torch.randn(257, generator=g).to(dtype), torch.randn(257, generator=g).to(dtype)
    for t in (900, 500, 0):
        got = s.step(v, t, x).prev_sample
        c = s.coeffs(t, dtype)
        assert got.dtype == dtype and torch.equal(got, vo.step_rounded(x, v, None, 1.0, c, dtype))   # every rounding, restated
        a_t, a_prev = s.alphas_cumprod[t], (s.alphas_cumprod[t - 100] if t >= 100 else s.final_alpha_cumprod)
        want = vo.step64(x.double().numpy(), v.double().numpy(), None, 1.0, vo.coeffs64(a_t, a_prev))
        ulp = {torch.float32: 2.0 ** -23, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}[dtype]
        # six roundings of values no larger than the operands' sum, plus the coefficients' own (one ulp each)
        assert np.max(np.abs(got.double().numpy() - want)) <= 12 * ulp * float(x.abs().max() + v.abs().max())


# ---- consistency in float64 --------------------------------------------------------------------------------------------------------------
def test_the_v_step_on_v_equals_the_epsilon_step_on_eps():
    rng = np.random.default_rng(7)
    for _ in range(20):
        a_t, a_o = rng.uniform(0.01, 0.99, 2)
        c = vo.coeffs64(a_t, a_o)
        x0, eps = rng.standard_normal(64), rng.standard_normal(64)
        x = c[1] * x0 + c[0] * eps
        v = c[1] * eps - c[0] * x0
        got, want = vo.step64(x, v, None, 1.0, c), vo.eps_step64(x, eps, c)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
        assert np.max(np.abs(got - (c[3] * x0 + c[2] * eps))) <= 1e-12 * np.max(np.abs(want))


def test_the_gradient_factor_equals_a_finite_difference():
    rng = np.random.default_rng(8)
    for guidance in (7.5, -2.0):
        a_t, a_o = rng.uniform(0.05, 0.95, 2)
        c = vo.coeffs64(a_t, a_o)
        u, cond, cur, prev = (rng.standard_normal(6) for _ in range(4))
        _, _, grad = vo.null_loss_grad64(u, cond, cur, prev, guidance, c)
        h = 1e-5
        for i in range(6):
            d = np.zeros(6)
            d[i] = h
            fd = (vo.loss64(u + d, cond, cur, prev, guidance, c) - vo.loss64(u - d, cond, cur, prev, guidance, c)) / (2 * h)
            assert abs(fd - grad[i]) <= 1e-6 * abs(grad[i]), (i, fd, grad[i])


# ---- model detection -----------------------------------------------------------------------------------------------------------------------
class ModelType(enum.Enum):
    EPS = 1
    V_PREDICTION = 2
    EDM = 5
    FLOW = 6


class SD20:
    pass


def comfy(model_type="absent", channels=4):
    unet = torch.nn.Conv2d(channels, 4, 1)
    inner = types.SimpleNamespace(diffusion_model=unet, model_config=SD20())
    if model_type != "absent":
        inner.model_type = model_type
    return types.SimpleNamespace(model=inner)


def wrapper(model_type):
    vae = types.SimpleNamespace(first_stage_model=torch.nn.Linear(1, 1))
    clip = types.SimpleNamespace(cond_stage_model=None)
    return model_wrappers.ComfyUIModelWrapper(comfy(model_type), clip, vae, device="cpu")


def test_model_detection():
    for kind, want in (("absent", "epsilon"), (ModelType.EPS, "epsilon"), ("EPS", "epsilon"), (ModelType.V_PREDICTION, V),
                       ("V_PREDICTION", V), ("v_prediction", V)):
        w = wrapper(kind)
        assert w.prediction_type == want and w.scheduler.config.prediction_type == want and w.is_supported() and w.model_type == "SD2"
    for kind in (ModelType.EDM, "FLOW"):
        w = wrapper(kind)
        assert w.prediction_type is None and not w.is_supported() and not w.is_supported("fast")
        assert (kind if isinstance(kind, str) else kind.name) in w.get_unsupported_message()


def test_fast_mode_refuses_a_v_prediction_model():
    with pytest.raises(ValueError, match="v-prediction"):
        model_wrappers.make_inpaint_runner(comfy(ModelType.V_PREDICTION, channels=9), None, None)
    with pytest.raises(ValueError, match="9 channels"):
        model_wrappers.make_inpaint_runner(comfy(ModelType.V_PREDICTION, channels=4), None, None)


# ---- exports, refusals, work size ------------------------------------------------------------------------------------------------------------
def test_new_exports():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    declared = set(re.findall(r"CS_API\s+[\w\s\*]+?\b(cs_\w+)\s*\(", hdr))
    L = _native.lib()
    for name in NEW:
        assert name in declared and name in _native.EXPORTS and hasattr(L, name), name
    assert int(re.search(r"CS_PRED_EPSILON\s*=\s*(\d+)", hdr).group(1)) == _native.PREDICTION["epsilon"]
    assert int(re.search(r"CS_PRED_V\s*=\s*(\d+)", hdr).group(1)) == _native.PREDICTION[V]
    # an unknown prediction: CS_EINVAL before any launch (no GPU here); c2 = 0 is refused under epsilon only
    import ctypes
    p, q = ctypes.c_void_p(256), ctypes.c_void_p(4096)
    assert L.cs_ddim_step_pred(p, q, None, p, 0, 4, 1.0, 0.5, 0.5, 0.5, 0.5, 7, None) == _native.CS_EINVAL and b"prediction" in L.cs_last_error()
    assert L.cs_ddim_step_pred(p, q, None, p, 0, 4, 1.0, 0.5, 0.0, 0.5, 0.5, 0, None) == _native.CS_EINVAL and b"c2" in L.cs_last_error()
    assert L.cs_standard_step_pred(p, q, 0, 1, 4, 2, 8, 1.0, 0.5, 0.5, 0.5, 0.5, -1, 0, None, None, None, None) == _native.CS_EINVAL
    assert b"prediction" in L.cs_last_error()


def test_engine_refuses_a_bad_prediction_before_the_gpu(monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    t = torch.zeros(8)
    x = torch.zeros(4, 4, 2, 2)
    flags = torch.ones(2, dtype=torch.uint8)
    c = (0.5, 0.5, 0.5, 0.5)
    for bad in ("v", "V_PREDICTION", None, 1):
        for fn in (lambda: engine.ddim_step_pred(t, t, None, 1.0, c, prediction=bad),
                   lambda: engine.null_loss_grad(t, t, t, t, 7.5, c, prediction=bad),
                   lambda: engine.NullTextLoss.apply(t, t, t, t, 7.5, c, bad),
                   lambda: engine.null_loss_grad_frames(t.view(2, 4), t.view(2, 4), t.view(2, 4), t.view(2, 4), 7.5, c, flags, 1e-3, prediction=bad),
                   lambda: engine.NullTextLossFrames.apply(t.view(2, 4), t.view(2, 4), t.view(2, 4), t.view(2, 4), 7.5, c, flags, 1e-3, None, bad),
                   lambda: engine.standard_step(x, x.clone(), 1.0, c, prediction=bad)):
            with pytest.raises(ValueError, match="prediction"):
                fn()
    # under v-prediction c2 = 0 passes the checks (the call then stops at the missing GPU, not at the coefficient)
    with pytest.raises((RuntimeError, ValueError), match="GPU|device"):
        engine.ddim_step_pred(t, t, None, 1.0, (1.0, 0.0, 0.5, 0.5), prediction=V)
    with pytest.raises(ValueError, match="alpha_t"):
        engine.ddim_step(t, t, None, 1.0, (1.0, 0.0, 0.5, 0.5))


def test_work_size_validation(monkeypatch):
    """The work size is the module switch (and NullInversion.work_size): the functions keep their signatures.  A bad value is refused
    by whichever of them runs; the default is 512."""
    assert sdn.STANDARD_WORK_SIZE == 512 and inversion.NullInversion.work_size == 512
    image, depth = torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8, 3)
    inv = inversion.NullInversion(types.SimpleNamespace(scheduler=schedulers.DDIMScheduler()), 5, 7.5)
    for bad in (0, -8, 4, 100, 512.0, "512", True, None):
        monkeypatch.setattr(sdn, "STANDARD_WORK_SIZE", bad)
        inv.work_size = bad
        for fn in (lambda: sdn.generate_stereo_standard(image, depth, 8.0, "uni", False, 5, 3.0, None, lambda u8: None),
                   lambda: sdn.generate_stereo_standard_frames(image, depth, 8.0, "uni", False, 5, 3.0, None, lambda u8: None),
                   lambda: sdn.text2stereoimage(None, ["", ""], None, None, torch.zeros(1, 8, 8), 8.0, "uni", False, 5, 3.0),
                   lambda: inv.invert(torch.zeros(8, 8, 3), ""),
                   lambda: inv.invert_frames(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), ""),
                   lambda: inversion.make_invert(None, 5, 7.5)(torch.zeros(8, 8, 3, dtype=torch.uint8)),
                   lambda: inversion.make_invert_frames(None, 5, 7.5)(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))):
            with pytest.raises(ValueError, match="work_size"):
                fn()
    # the validator that said [F,512,512,3] says the work size
    inv.work_size = 64
    with pytest.raises(ValueError, match=r"\[F,64,64,3\]"):
        inv.invert_frames(torch.zeros(1, 512, 512, 3, dtype=torch.uint8), "")
    del inv.work_size
    with pytest.raises(ValueError, match=r"\[F,512,512,3\]"):
        inv.invert_frames(torch.zeros(1, 64, 64, 3, dtype=torch.uint8), "")
    # the callables of make_invert read the switch when they run
    monkeypatch.setattr(sdn, "STANDARD_WORK_SIZE", 64)
    assert inversion._standard_work_size() == 64


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
def test_fixture_is_reproduced_and_the_oracle_agrees():
    z = np.load(mk.OUT)
    built = mk.build()
    assert sorted(z.files) == sorted(built)
    nan_free = 0
    for key in z.files:
        if key == "meta":
            assert str(z[key]) == str(built[key])
            continue
        a, b = z[key], built[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        if a.dtype == np.float64:
            assert a == b or (np.isnan(a) and np.isnan(b)), key
        else:
            assert np.array_equal(a, b), key
    for c in json.loads(str(z["meta"]))["cases"]:
        dtype = getattr(torch, c["dtype"])
        s, a, b, _ = mk.inputs(dtype)
        want = vo.step_rounded(s, a, b, c["guidance"], tuple(c["coeffs"]), dtype)
        got = torch.from_numpy(z[c["id"] + "/step"].view({2: np.int16, 4: np.int32}[s.element_size()])).view(dtype)
        assert torch.equal(got.isnan(), want.isnan()), c["id"]
        keep = ~want.isnan()
        assert torch.equal(got[keep].view(mk.BITS[dtype]), want[keep].view(mk.BITS[dtype])), c["id"]
        nan_free += int(keep.sum())
    assert nan_free > 0
