"""The few-step samplers of Fast mode without a GPU: the timestep lists against values written out by hand, the specification
(tools/fewstep_oracle.py) against a float64 restatement within a derived bound and against its fixtures, the runner's host plan
against the specification, and every refusal of the C entry points, the engine, the runner and the node (not gpu)."""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from comfystereo_amd import _native, engine, inpaint_runner as ir, model_wrappers, stereodiffusion_nodes as sdn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fewstep_cases as cases   # noqa: E402
import fewstep_fake_model as ffm   # noqa: E402
import fewstep_oracle as oracle   # noqa: E402
import make_fewstep_goldens   # noqa: E402

EULER = {1: [999], 2: [999, 499], 4: [999, 749, 499, 249], 8: [999, 874, 749, 624, 499, 374, 249, 124]}
LCM = {1: [999], 2: [999, 499], 4: [999, 759, 499, 259], 8: [999, 879, 759, 639, 499, 379, 259, 139]}


# ---- timesteps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler, table", [("euler", EULER), ("lcm", LCM)])
def test_timestep_lists_written_out_by_hand(sampler, table):
    for n, want in table.items():
        assert ir.fewstep_timesteps(sampler, n) == want, (sampler, n)
        assert oracle.timesteps(sampler, n) == want, (sampler, n)


def test_strength_slices_the_list_with_the_runners_rule():
    # int(4 * (1 - 0.5)) = 2 and int(4 * (1 - 0.6)) = int(1.6) = 1 entries are dropped from the front
    assert oracle.timesteps("euler", 4, 0.5) == [499, 249] and oracle.timesteps("euler", 4, 0.6) == [749, 499, 249]
    assert oracle.timesteps("lcm", 4, 0.5) == [499, 259] and oracle.timesteps("lcm", 4, 0.6) == [759, 499, 259]
    assert oracle.timesteps("lcm", 8, 0.5) == LCM[8][4:] and oracle.timesteps("euler", 1, 0.6) == [999]


def test_every_list_is_strictly_descending_and_51_lcm_steps_are_refused():
    for sampler in ("euler", "lcm"):
        for n in range(1, 51):
            ts = ir.fewstep_timesteps(sampler, n)
            assert ts == oracle.timesteps(sampler, n) and len(ts) == n and ts[0] == 999 and ts[-1] >= 0
            assert all(a > b for a, b in zip(ts, ts[1:])), (sampler, n)
    assert len(ir.fewstep_timesteps("euler", 51)) == 51
    for f in (ir.fewstep_timesteps, oracle.timesteps):
        with pytest.raises(ValueError, match="at most 50 steps, got 51"):
            f("lcm", 51)


# ---- coefficients ------------------------------------------------------------------------------------------------------------------
def test_the_runners_host_coefficients_are_the_specifications():
    acp = ir.scaled_linear_alphas_cumprod()
    assert torch.equal(acp, oracle.alphas_cumprod())
    for sampler in ("euler", "lcm"):
        for n in (1, 2, 4, 8):
            ts = oracle.timesteps(sampler, n)
            for i, t in enumerate(ts):
                t_next = ts[i + 1] if i + 1 < n else None
                k = ir.fewstep_coeffs(sampler, acp, t, t_next)
                assert k == oracle.coeffs(sampler, acp, ts, i) and len(k) == len(engine.FEWSTEP_COEFFS[sampler])
                assert all(float(np.float32(v)) == v for v in k)   # float32 values
    assert ir.euler_init_coeffs(acp, 999) == oracle.euler_init_coeffs(acp, 999)


def test_coefficients_at_the_ends():
    acp = oracle.alphas_cumprod()
    dsig, scale, sig_next = oracle.euler_coeffs(acp, 249, None)   # the last Euler step: sigma_next = 0, the input scale 1
    assert sig_next == 0.0 and scale == 1.0 and dsig == -float(oracle.sigma(acp, 249)) < 0
    k = oracle.lcm_coeffs(acp, 999, None)   # the last LCM step of a 1-step plan: a_next = 1, and c_skip -> 0 at large t
    assert k[4] == 1.0 and k[5] == 0.0 and 0 < k[3] < 3e-9 and abs(k[2] - 1) < 1e-7
    k0 = oracle.lcm_coeffs(acp, 0, None)   # t = 0: the boundary condition f(x, 0) = x
    assert k0[3] == 1.0 and k0[2] == 0.0


# ---- the specification against float64 ---------------------------------------------------------------------------------------------
def float64_restatement(c):
    """-> {name: (value, magnitude, roundings)} in float64 from the dtype's inputs and the float32 coefficients.  magnitude: the sum
    of the magnitudes of the expression's terms; roundings: how many roundings lie on the stored value's path, counted beside each
    expression.  Every rounding errs by at most eps(dtype) / 2 of its own result's magnitude (the float32 ones by far less), which
    later coefficients scale exactly as they scale the magnitude: |stored - value| <= roundings * eps * magnitude."""
    d = lambda t: None if t is None else t.double()   # noqa: E731
    k = [float(v) for v in c["k"]]
    s, pred = d(c["s"]), d(c["pred"])
    if c["cfg"]:
        u, t = pred.chunk(2)
        e, e_mag, r = u + c["guidance"] * (t - u), u.abs() + abs(c["guidance"]) * (t.abs() + u.abs()), 3   # difference, product, sum
    else:
        e, e_mag, r = pred, pred.abs(), 0
    if c["sampler"] == "euler":
        prev, mag, r = s + e * k[0], s.abs() + e_mag * abs(k[0]), r + 2                                      # product, sum
    else:
        x0, x0_mag = (s - k[0] * e) / k[1], (s.abs() + k[0] * e_mag) / k[1]                                  # product, difference, quotient
        prev, mag, r = k[2] * x0 + k[3] * s, abs(k[2]) * x0_mag + abs(k[3]) * s.abs(), r + 6                 # + product, product, sum
        if not c["last"]:
            prev, mag, r = k[4] * prev + k[5] * d(c["z"]), k[4] * mag + k[5] * d(c["z"]).abs(), r + 3        # + product, product, sum
    if c["channels"] == 4:
        il, nz, m = d(c["img_latent"]), d(c["noise0"]), c["mask_l"] != 0
        if c["last"]:
            keep, keep_mag, keep_r = il, il.abs(), 0
        elif c["sampler"] == "euler":
            keep, keep_mag, keep_r = il + k[2] * nz, il.abs() + k[2] * nz.abs(), 2                           # product, sum
        else:
            keep, keep_mag, keep_r = k[4] * il + k[5] * nz, k[4] * il.abs() + k[5] * nz.abs(), 3             # product, product, sum
        prev, mag = torch.where(m, prev, keep), torch.where(m, mag, keep_mag)
        r = torch.where(m, torch.tensor(r), torch.tensor(keep_r)).expand_as(prev)
    else:
        r = torch.full_like(prev, r)
    vae = float(np.float32(0.18215))
    out = {"decode_in": (prev / vae, mag / vae, r + 2)}                                                      # + quotient, the store
    if c["sampler"] == "euler":
        out["state"] = (prev, mag, r + 1)                                                                    # + the store
        out["x"] = (prev / k[1], mag / k[1], r + 2)                                                          # + quotient, the store
    else:
        out["x"] = (prev, mag, r + 1)                                                                        # + the store
    return out


@pytest.mark.parametrize("pos", list(cases.POSITIONS))
@pytest.mark.parametrize("channels", [9, 4])
@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("dtype_name", list(cases.DTYPES))
@pytest.mark.parametrize("sampler", ["euler", "lcm"])
def test_the_specification_is_within_the_derived_bound_of_float64(sampler, dtype_name, cfg, channels, pos):
    c = cases.make(sampler, dtype_name, cfg, channels, pos, 2, 5, 7, seed=77)
    got, eps = cases.want(c), torch.finfo(c["dtype"]).eps
    assert (got["state"] is None) == (sampler == "lcm")
    for name, (value, mag, roundings) in float64_restatement(c).items():
        err = (got[name].double() - value).abs()
        assert bool((err <= roundings * eps * mag).all()), (name, float((err / (eps * mag)).max()), float(roundings.max()))
        assert got[name].dtype == c["dtype"]


def test_the_first_latents_are_within_the_derived_bound_of_float64():
    acp = oracle.alphas_cumprod()
    for dtype_name, dtype in cases.DTYPES.items():
        g = torch.Generator().manual_seed(5)
        il, nz = torch.randn((2, 4, 5, 7), generator=g).to(dtype), torch.randn((2, 4, 5, 7), generator=g).to(dtype)
        x, state = oracle.first_latents("euler", il, nz, acp, 999)
        s0, scale = oracle.euler_init_coeffs(acp, 999)
        value, mag, eps = il.double() + s0 * nz.double(), il.double().abs() + s0 * nz.double().abs(), torch.finfo(dtype).eps
        assert bool(((state.double() - value).abs() <= 3 * eps * mag).all())                  # product, sum, the store
        assert bool(((x.double() - value / scale).abs() <= 4 * eps * mag / scale).all())      # product, sum, quotient, the store
        x, state = oracle.first_latents("lcm", il, nz, acp, 999)   # scheduler.add_noise, in the dtype: its roots (2 roundings each,
        a = float(acp[999])                                        # the alpha's and the root's), product, product, sum: 7
        value, mag = a ** 0.5 * il.double() + (1 - a) ** 0.5 * nz.double(), a ** 0.5 * il.double().abs() + (1 - a) ** 0.5 * nz.double().abs()
        assert state is None and bool(((x.double() - value).abs() <= 7 * eps * mag).all())


# ---- the specification against its fixtures ----------------------------------------------------------------------------------------
def test_the_fixtures_are_regenerated_bit_for_bit():
    with np.load(os.path.join(ROOT, "tests", "golden", "fewstep.npz")) as z:
        want = {name: z[name] for name in z.files}
    got = make_fewstep_goldens.build()
    assert sorted(got) == sorted(want) and len(json.loads(str(want["meta"]))["cases"]) == 2 * 3 * 2 * 2 * 3
    assert json.loads(str(got["meta"])) == json.loads(str(want["meta"]))
    for name in want:
        if name != "meta":
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name


# ---- refusals of the C entry points ------------------------------------------------------------------------------------------------
P = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]   # fake pointers, far apart and aligned: nothing dereferences them
K = (0.5, 1.5, 0.25, 0.125, 0.75, 0.5)


def step_args(**over):
    a = dict(noise_pred=P[0], x=P[1], dtype=1, n=1, hl=4, wl=4, channels=4, sampler=1, cfg=1, last=0, guidance=7.5, k0=K[0], k1=K[1],
             k2=K[2], k3=K[3], k4=K[4], k5=K[5], state=P[2], step_noise=P[3], img_latent=P[4], noise0=P[5], mask_l=P[6], decode_in=P[7])
    a.update(over)
    return list(a.values())


def init_args(**over):
    a = dict(img_latent=P[0], noise=P[1], x9=P[2], dtype=1, n=1, hl=4, wl=4, channels=4, cfg=1, sampler=0, k0=14.0, k1=14.1, x=P[3],
             state=P[4], mask_l=P[5])
    a.update(over)
    return list(a.values())


STEP_REFUSALS = [
    (dict(noise_pred=None), "null pointer"), (dict(x=None), "null pointer"),
    (dict(n=0), "non-positive size"), (dict(hl=0), "non-positive size"), (dict(wl=-1), "non-positive size"),
    (dict(dtype=3), "cs_inpaint_fewstep_step: unknown dtype"), (dict(dtype=-1), "cs_inpaint_fewstep_step: unknown dtype"),
    (dict(sampler=2), "cs_inpaint_fewstep_step: unknown sampler"), (dict(sampler=-1), "cs_inpaint_fewstep_step: unknown sampler"),
    (dict(channels=5), "channels must be 9"), (dict(channels=0), "channels must be 9"),
    (dict(sampler=0, state=None), "null state"),
    (dict(step_noise=None), "null step_noise"),
    (dict(img_latent=None), "4 channels take img_latent"), (dict(mask_l=None), "4 channels take img_latent"),
    (dict(noise0=None), "4 channels take img_latent"),
    (dict(guidance=float("nan")), "must be finite"), (dict(k3=float("inf")), "must be finite"), (dict(k0=float("-inf")), "must be finite"),
    (dict(k1=0.0), "k1 (Euler: the input scale, LCM: sqrt(a_t)) must not be 0"),
    (dict(decode_in=ctypes.c_void_p(4096 * 8 + 1)), "misaligned tensor"), (dict(x=ctypes.c_void_p(4096 * 2 + 1)), "misaligned tensor"),
    (dict(decode_in=P[1]), "must not overlap"), (dict(step_noise=ctypes.c_void_p(4096 * 2 + 64)), "must not overlap"),
]
INIT_REFUSALS = [
    (dict(img_latent=None), "null pointer"), (dict(x=None), "null pointer"),
    (dict(n=0), "non-positive size"), (dict(hl=-3), "non-positive size"), (dict(wl=0), "non-positive size"),
    (dict(dtype=3), "cs_inpaint_fewstep_init: unknown dtype"), (dict(sampler=2), "cs_inpaint_fewstep_init: unknown sampler"),
    (dict(channels=8), "channels must be 9"),
    (dict(x9=None), "4 channels take x9"), (dict(mask_l=None), "4 channels take x9"),
    (dict(state=None), "null state"),
    (dict(k0=float("nan")), "k0 and k1 must be finite"), (dict(k1=0.0), "k1 (the input scale) must not be 0"),
    (dict(state=ctypes.c_void_p(4096 * 5 + 1)), "misaligned tensor"),
    (dict(state=P[3]), "must not overlap"), (dict(mask_l=P[1]), "must not overlap"),
]


@pytest.mark.parametrize("entry, make, table", [("cs_inpaint_fewstep_step", step_args, STEP_REFUSALS),
                                                ("cs_inpaint_fewstep_init", init_args, INIT_REFUSALS)])
def test_the_c_entry_points_refuse_before_any_device_work(entry, make, table):
    """Fake pointers: a case that got as far as a launch would not come back with CS_EINVAL and this text."""
    fn = getattr(_native.lib(), entry)
    for over, text in table:
        rc = fn(*make(**over), None)
        msg = _native.lib().cs_last_error().decode()
        assert rc == _native.CS_EINVAL and text in msg, (entry, over, rc, msg)
    # a last LCM step needs neither step_noise nor noise0: with them missing the refusal is another one, further down the list
    rc = _native.lib().cs_inpaint_fewstep_step(*step_args(last=1, step_noise=None, noise0=None, k1=0.0), None)
    assert rc == _native.CS_EINVAL and "k1" in _native.lib().cs_last_error().decode()


# ---- refusals of the engine, the runner and the node -------------------------------------------------------------------------------
def test_the_engine_refuses_bad_arguments_by_name():
    x9, x4 = torch.zeros((2, 9, 4, 4), dtype=torch.float16), torch.zeros((2, 4, 4, 4), dtype=torch.float16)
    pred, lat = torch.zeros((2, 4, 4, 4), dtype=torch.float16), torch.zeros((1, 4, 4, 4), dtype=torch.float16)
    m = torch.zeros((1, 1, 4, 4), dtype=torch.float16)
    euler, lcm = (-1.0, 1.5, 0.5), K
    for kwargs, text in [
        (dict(sampler="ddim"), "unknown sampler 'ddim' (euler, lcm)"),
        (dict(noise_pred=pred[:, :3]), "noise_pred must be"),
        (dict(x=torch.zeros((2, 5, 4, 4), dtype=torch.float16)), "x must have 9 channels"),
        (dict(x=x9[:1]), "under guidance"), (dict(x=x9.float()), "share one dtype"),
        (dict(state=None), "state goes with sampler 'euler'"),
        (dict(sampler="lcm", coeffs=lcm, state=None), "step_noise goes with every step"),
        (dict(sampler="lcm", coeffs=lcm, state=None, step_noise=lat, last=True), "step_noise goes with every step"),
        (dict(x=x4), "a 4-channel x takes img_latent, mask_l"),
        (dict(x=x4, img_latent=lat, mask_l=m), "a 4-channel x takes img_latent, mask_l"),
        (dict(x=x4, img_latent=lat, mask_l=m[:, :, :2], noise0=lat), "mask_l must be [N,1,hl,wl]"),
        (dict(coeffs=(1.0, 2.0)), "coeffs must be 3 numbers"), (dict(coeffs=(1.0, float("nan"), 0.0)), "must be finite"),
        (dict(coeffs=(1.0, 0.0, 0.0)), "must not be 0"), (dict(state=lat.float()), "share one dtype"),
        (dict(decode_in=torch.zeros((1, 4, 4, 5), dtype=torch.float16)), "decode_in must be [N,4,hl,wl]"),
    ]:
        args = dict(noise_pred=pred, x=x9, sampler="euler", guidance=7.5, coeffs=euler, cfg=True, state=lat)
        args.update(kwargs)
        with pytest.raises(ValueError) as info:
            engine.fewstep_step(**args)
        assert text in str(info.value), (kwargs, str(info.value))
    for kwargs, text in [
        (dict(sampler="plms"), "unknown sampler 'plms'"), (dict(img_latent=lat[:, :3]), "img_latent must be [N,4,hl,wl]"),
        (dict(state=None), "sampler 'euler' takes state"), (dict(x=x4), "a 4-channel x takes prep"),
        (dict(coeffs=(1.0,)), "coeffs must be 2 numbers"), (dict(noise=lat.float()), "share one dtype"),
    ]:
        args = dict(img_latent=lat, noise=lat.clone(), coeffs=(14.0, 14.1), x=x9, sampler="euler", cfg=True, state=lat.clone())
        args.update(kwargs)
        with pytest.raises(ValueError) as info:
            engine.fewstep_latent_init(**args)
        assert text in str(info.value), (kwargs, str(info.value))


NINE_CHANNEL_MESSAGE = ("Connected model has 4 UNet input channels, but inpainting requires 9 channels. Please use an inpainting checkpoint "
                        "(e.g., sd-v1-5-inpainting).")


def test_the_runner_refuses_an_unknown_sampler_and_four_channels_with_plms():
    nine, four = ffm.FewStepModel("cpu", torch.float32), ffm.FewStepModel("cpu", torch.float32, in_channels=4)
    with pytest.raises(ValueError, match=r"unknown sampler 'dpm' \(plms, euler, lcm\)"):
        ir.InpaintRunner(*nine.parts(), sampler="dpm")
    for kwargs in (dict(), dict(sampler="plms")):
        with pytest.raises(ValueError) as info:
            ir.InpaintRunner(*four.parts(), **kwargs)
        assert str(info.value) == NINE_CHANNEL_MESSAGE
    for sampler in ("euler", "lcm"):
        assert ir.InpaintRunner(*four.parts(), sampler=sampler).sampler == sampler
        assert ir.InpaintRunner(*nine.parts(), sampler=sampler).in_channels == 9
    assert ir.InpaintRunner(*nine.parts()).sampler == "plms"
    three = ffm.FewStepModel("cpu", torch.float32, in_channels=3)
    with pytest.raises(ValueError, match="has 3 UNet input channels"):
        ir.InpaintRunner(*three.parts(), sampler="euler")
    runner = ir.InpaintRunner(*nine.parts(), sampler="euler")
    with pytest.raises(ValueError, match="built for sampler 'euler', not 'lcm'"):
        ir.make_inpaint(runner, "", sampler="lcm")
    with pytest.raises(ValueError, match="unknown sampler 'heun'"):
        ir.make_inpaint(runner, "", sampler="heun")
    assert callable(ir.make_inpaint(runner, "", sampler="euler")) and callable(ir.make_inpaint(runner, ""))


def comfy_model(in_channels, model_type=None):
    unet = types.SimpleNamespace(in_channels=in_channels)
    return types.SimpleNamespace(model=types.SimpleNamespace(diffusion_model=unet, model_type=model_type))


def test_make_inpaint_runner_and_the_node_switch():
    with pytest.raises(ValueError, match=r"unknown sampler 'ddim' \(plms, euler, lcm\)"):
        model_wrappers.make_inpaint_runner(comfy_model(9), None, None, sampler="ddim")
    with pytest.raises(ValueError) as info:
        model_wrappers.make_inpaint_runner(comfy_model(4), None, None)
    assert str(info.value) == NINE_CHANNEL_MESSAGE
    for sampler in ("plms", "euler", "lcm"):   # a v-prediction model is still refused in Fast mode, whatever the sampler
        for channels in (9,) if sampler == "plms" else (9, 4):
            with pytest.raises(ValueError, match="Fast mode's inpainting loop supports epsilon-prediction models only"):
                model_wrappers.make_inpaint_runner(comfy_model(channels, "V_PREDICTION"), None, None, sampler=sampler)
    assert sdn.FAST_SAMPLER == "plms"
    node = sdn.StereoDiffusionNode()
    image, depth = torch.zeros((1, 8, 8, 3)), torch.zeros((1, 8, 8, 3))
    old = sdn.FAST_SAMPLER
    try:
        sdn.FAST_SAMPLER = "ddim"
        with pytest.raises(ValueError, match=r"unknown sampler 'ddim' \(plms, euler, lcm\)"):
            node.generate_stereo(image, depth, 9.0, "uni", True, pipeline_mode=sdn.FAST_MODE, model=comfy_model(9), clip=object(), vae=object())
        sdn.FAST_SAMPLER = "lcm"
        with pytest.raises(ValueError, match="epsilon-prediction models only"):
            node.generate_stereo(image, depth, 9.0, "uni", True, pipeline_mode=sdn.FAST_MODE, model=comfy_model(4, "V_PREDICTION"),
                                 clip=object(), vae=object())
    finally:
        sdn.FAST_SAMPLER = old
