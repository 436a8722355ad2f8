"""Fast mode's inpainting loop without a GPU: the PLMS restatement the fixtures rest on, the fixtures' manifest, the stock-torch
composition the GPU tests use at other sizes, the refusals of the three entry points before any launch, the runner's surface."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import _native, engine, inpaint_runner as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import inpaint_fake_model as fm   # noqa: E402
import inpaintrun_stock as stock   # noqa: E402
import plms_oracle   # noqa: E402

NEW_EXPORTS = ["cs_inpaint_image_prep", "cs_inpaint_latent_init", "cs_inpaint_plms_step"]


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "inpaint_runner.npz"))
    return z, json.loads(str(z["meta"]))


def as_tensor(a, dtype_name):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.view(torch.bfloat16) if dtype_name == "bfloat16" else t


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ---- the scheduler, restated independently in float64 -----------------------------------------------------------------------------
def plms64(num_steps, timesteps, es, samples):
    """Every step's result in float64 from the published formulas: es[i], samples[i] are step i's guided prediction and sample."""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2
    acp = np.cumprod(1.0 - betas)
    ratio, kept, cur, out = 1000 // num_steps, [], None, []
    for counter, (t, e, s) in enumerate(zip(timesteps, es, samples)):
        prev_t = t - ratio
        if counter != 1:
            kept = kept[-3:] + [e]
        else:
            prev_t, t = t, t + ratio
        if len(kept) == 1 and counter == 0:
            m, cur = e, s
        elif len(kept) == 1 and counter == 1:
            m, s = (e + kept[-1]) / 2, cur
        elif len(kept) == 2:
            m = (3 * kept[-1] - kept[-2]) / 2
        elif len(kept) == 3:
            m = (23 * kept[-1] - 16 * kept[-2] + 5 * kept[-3]) / 12
        else:
            m = (55 * kept[-1] - 59 * kept[-2] + 37 * kept[-3] - 9 * kept[-4]) / 24
        a_t, a_p = acp[t], acp[prev_t] if prev_t >= 0 else acp[0]
        denom = a_t * np.sqrt(1 - a_p) + np.sqrt(a_t * (1 - a_t) * a_p)
        out.append(np.sqrt(a_p / a_t) * s - (a_p - a_t) * m / denom)
    return out


def oracle_against_float64(num_steps, timesteps, es, samples):
    sch = plms_oracle.PLMSOracle()
    sch.set_timesteps(num_steps)
    want = plms64(num_steps, timesteps, [e.double().numpy() for e in es], [s.double().numpy() for s in samples])
    worst = 0.0
    for t, e, s, w in zip(timesteps, es, samples, want):
        got = sch.step(e, torch.tensor(t), s).prev_sample
        assert got.dtype == torch.float32
        worst = max(worst, float(np.abs(got.double().numpy() - w).max() / max(1.0, np.abs(w).max())))
    return worst


def test_plms_oracle_against_a_float64_restatement(golden):
    """The margin: 4 x the error tools/make_inpaintrun_goldens.py measured for the oracle in float32 against itself in float64 on
    the fixtures' inputs (meta.oracle_err, 4.3e-7: a few float32 roundings of values around 1).  Here the float64 side is written
    again from the formulas, on the fixtures' inputs and on seeded ones for N = 20 and 50, sliced and not."""
    z, meta = golden
    margin = 4 * meta["oracle_err"]
    assert 1e-7 < margin < 1e-5
    worst = 0.0
    for c in meta["cases"]:
        if c["dtype"] != "float32" or not c["timesteps"]:
            continue
        outs, ins = torch.from_numpy(z[f"{c['id']}/unet_out"]), torch.from_numpy(z[f"{c['id']}/unet_in"])
        es = [o[:1] + c["guidance"] * (o[1:] - o[:1]) for o in outs]
        worst = max(worst, oracle_against_float64(c["steps"], c["timesteps"], es, [x[:1, :4] for x in ins]))
    g = torch.Generator().manual_seed(9)
    for n, start in ((20, 0), (50, 0), (20, 5)):
        ts = plms_oracle.plms_timesteps(n).tolist()[start:]
        es = [torch.randn(1, 4, 5, 7, generator=g) for _ in ts]
        samples = [torch.randn(1, 4, 5, 7, generator=g) for _ in ts]
        worst = max(worst, oracle_against_float64(n, ts, es, samples))
    print("oracle against float64:", worst, "margin", margin)
    assert worst <= margin


def test_timestep_lists():
    want = {1: [0], 2: [500, 0, 0], 3: [666, 333, 333, 0]}
    for n in (1, 2, 3, 20, 50):
        ts = plms_oracle.plms_timesteps(n).tolist()
        assert ts == ir.plms_timesteps(n)
        ratio = 1000 // n
        if n in want:
            assert ts == want[n]
        else:
            assert len(ts) == n + 1 and ts[0] == (n - 1) * ratio and ts[1] == ts[2] == (n - 2) * ratio and ts[-1] == 0
            assert ts[2:] == list(range((n - 2) * ratio, -1, -ratio))
    sch = plms_oracle.PLMSOracle()
    sch.set_timesteps(1)
    sch.step(torch.zeros(1), torch.tensor(0), torch.zeros(1))
    assert sch.counter == 1 and len(sch.ets) == 1
    sch.set_timesteps(20)   # resets the history and the counter
    assert sch.counter == 0 and sch.ets == [] and sch.timesteps.dtype == torch.int64


def test_kinds_and_coefficients_follow_counter_and_t_not_the_position():
    kinds, kept = [], 0
    for counter in range(7):
        kind, kept = ir.plms_kind(counter, kept)
        kinds.append(kind)
    assert kinds == ["first", "second", "order2", "order3", "order4", "order4", "order4"]
    sch = plms_oracle.PLMSOracle()
    acp, final = sch.alphas_cumprod, sch.final_alpha_cumprod
    # the second warm-up step at t goes from t + ratio to t, whatever came before it in the full list
    sc, da, denom = ir.plms_coeffs(acp, final, 1, 498, 166, torch.float32)
    assert (sc, da) == ir.plms_coeffs(acp, final, 0, 664, 166, torch.float32)[:2] and denom > 0
    # below zero: final_alpha_cumprod
    sc0, da0, _ = ir.plms_coeffs(acp, final, 0, 0, 1000, torch.float32)
    assert sc0 == 1.0 and da0 == 0.0
    # a half dtype rounds what multiplies, not what divides
    sch_, dah, denomh = ir.plms_coeffs(acp, final, 2, 332, 166, torch.float16)
    scf, daf, denomf = ir.plms_coeffs(acp, final, 2, 332, 166, torch.float32)
    assert sch_ == float(torch.tensor(scf).half()) and dah == float(torch.tensor(daf).half()) and denomh == denomf
    sa, sb = ir.add_noise_coeffs(acp, 664, torch.bfloat16)
    a = acp[664].to(torch.bfloat16)
    assert sa == float(plms_oracle.root(a)) and sb == float(plms_oracle.root(1 - a))


# ---- the fixtures -----------------------------------------------------------------------------------------------------------------
def test_manifest(golden):
    z, meta = golden
    cases = meta["cases"]
    assert "restated" in meta["scheduler"]
    for dtype in ("float32", "float16", "bfloat16"):
        mine = [c for c in cases if c["dtype"] == dtype]
        assert {c["steps"] for c in mine} == {1, 2, 3, 6}
        assert {c["strength"] for c in mine} == {1.0, 0.6, 0.0}
        assert {c["guidance"] for c in mine} == {0.0, 1.0, 7.5}
        assert {c["mask"] for c in mine} == {"zero", "one", "mixed"}
        assert {k for c in mine for k in c["kinds"]} == {"first", "second", "order2", "order3", "order4"}
        assert any(c["kinds"].count("order4") >= 3 for c in mine)   # the ring of four wraps
        assert any(not c["timesteps"] for c in mine)
    for c in cases:
        h, w = c["size"]
        assert z[f"{c['id']}/filled"].shape == (h, w, 3) and z[f"{c['id']}/mask"].shape == (h, w) and z[f"{c['id']}/codes"].shape == (h, w, 3)
        steps = len(c["timesteps"])
        assert z[f"{c['id']}/decode_in"].shape == (1, 4, h // 8, w // 8)
        if steps:
            assert z[f"{c['id']}/unet_in"].shape == (steps, 2, 9, h // 8, w // 8) and z[f"{c['id']}/unet_out"].shape == (steps, 2, 4, h // 8, w // 8)
            assert z[f"{c['id']}/latents"].shape == (1, 4, h // 8, w // 8)
        else:
            assert f"{c['id']}/unet_in" not in z.files
        if c["mask"] == "mixed" and steps:   # a negative pixel under the mask: -0.0 in the masked image's latents
            x0 = as_tensor(z[f"{c['id']}/unet_in"], c["dtype"])[0, 0, 5]
            assert ((x0 == 0) & (bits(x0) != 0)).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "inpaint_runner.npz")) < (1 << 20)


def test_stock_composition_gives_the_fixtures_bits(golden):
    """tools/inpaintrun_stock.py, the GPU tests' reference at other sizes, is the reference's loop: bit for bit on every fixture."""
    z, meta = golden
    for c in meta["cases"]:
        model = fm.FakeInpaintModel("cpu", getattr(torch, c["dtype"]))
        got = stock.run(model, c["prompt"], torch.from_numpy(z[f"{c['id']}/filled"]), torch.from_numpy(z[f"{c['id']}/mask"]), c["steps"],
                        c["guidance"], c["strength"], torch.Generator().manual_seed(c["seed"]))
        assert torch.equal(got["codes"], torch.from_numpy(z[f"{c['id']}/codes"])), c["id"]
        assert torch.equal(bits(got["decode_in"]), bits(as_tensor(z[f"{c['id']}/decode_in"], c["dtype"]))), c["id"]
        if c["timesteps"]:
            assert torch.equal(bits(torch.stack(got["unet_in"])), bits(as_tensor(z[f"{c['id']}/unet_in"], c["dtype"]))), c["id"]


# ---- the library and the wrappers, before any launch ------------------------------------------------------------------------------
def test_exports_and_signatures():
    import inspect
    L = _native.lib()
    for name in NEW_EXPORTS:
        assert name in _native.EXPORTS and hasattr(L, name)
    assert _native.ABI_VERSION == 4 and L.cs_version() == 4
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    for key, code in _native.PLMS_KIND.items():
        name = {"first": "FIRST", "second": "SECOND"}.get(key, key.upper())
        assert f"CS_PLMS_{name} = {code}" in hdr
    assert str(inspect.signature(engine.inpaint_image_prep)) == "(filled_u8, mask, x, latent_size)"
    assert str(inspect.signature(engine.inpaint_latent_init)) == "(mean_img, mean_masked, noise, coeffs, x, img_latent=None, decode_in=None)"
    assert str(inspect.signature(engine.plms_step)) == "(noise_pred, x, kind, guidance, coeffs, e_out=None, history=(), cur_sample=None, decode_in=None)"
    assert str(inspect.signature(ir.InpaintRunner.__call__)) == ("(self, prompt, filled_u8, mask, num_inference_steps=30, guidance_scale=7.5, "
                                                                 "strength=1.0, generator=None)")


def test_refusals_before_any_launch():
    """Host buffers stand in for device memory: every call here is refused by the argument checks, so nothing is launched."""
    L = _native.lib()
    EINVAL = _native.CS_EINVAL
    buf = (ctypes.c_uint8 * (1 << 16))()
    base = (ctypes.addressof(buf) + 255) & ~255

    def p(k):   # disjoint 4 KiB regions
        return ctypes.c_void_p(base + 4096 * k)

    n, h, w, hl, wl = 1, 8, 8, 2, 2
    prep, init, step = L.cs_inpaint_image_prep, L.cs_inpaint_latent_init, L.cs_inpaint_plms_step
    # image_prep(filled, mask, n, h, w, hl, wl, dtype, img, masked, x, stream)
    good = [p(0), p(1), n, h, w, hl, wl, 0, p(2), p(3), p(4), None]
    for i in (0, 1, 8, 9, 10):
        assert prep(*[None if j == i else a for j, a in enumerate(good)]) == EINVAL and b"null" in L.cs_last_error()
    for i in (2, 3, 4, 5, 6):
        assert prep(*[0 if j == i else a for j, a in enumerate(good)]) == EINVAL and b"non-positive" in L.cs_last_error()
    for bad in (-1, 3):
        assert prep(*[bad if j == 7 else a for j, a in enumerate(good)]) == EINVAL and b"dtype" in L.cs_last_error()
    assert prep(*[p(2) if j == 9 else a for j, a in enumerate(good)]) == EINVAL and b"overlap" in L.cs_last_error()    # masked on img
    assert prep(*[p(0) if j == 10 else a for j, a in enumerate(good)]) == EINVAL and b"overlap" in L.cs_last_error()   # x on filled
    assert prep(*[ctypes.c_void_p(base + 4096 * 2 + 2) if j == 8 else a for j, a in enumerate(good)]) == EINVAL and b"misaligned" in L.cs_last_error()
    # latent_init(mean_img, mean_masked, mean_dtype, noise, dtype, n, hl, wl, sa, sb, x, img_latent, decode_in, stream)
    good = [p(0), p(1), 0, p(2), 1, n, hl, wl, 0.5, 0.5, p(3), p(4), p(5), None]
    for i in (0, 1, 10, 11):
        assert init(*[None if j == i else a for j, a in enumerate(good)]) == EINVAL and b"null" in L.cs_last_error()
    for i in (5, 6, 7):
        assert init(*[-1 if j == i else a for j, a in enumerate(good)]) == EINVAL and b"non-positive" in L.cs_last_error()
    for i in (2, 4):
        assert init(*[3 if j == i else a for j, a in enumerate(good)]) == EINVAL and b"dtype" in L.cs_last_error()
    for i in (8, 9):
        for bad in (float("nan"), float("inf")):
            assert init(*[bad if j == i else a for j, a in enumerate(good)]) == EINVAL and b"finite" in L.cs_last_error()
    assert init(*[p(3) if j == 11 else a for j, a in enumerate(good)]) == EINVAL and b"overlap" in L.cs_last_error()   # img_latent on x
    assert init(*[p(2) if j == 12 else a for j, a in enumerate(good)]) == EINVAL and b"overlap" in L.cs_last_error()   # decode_in on noise
    # plms_step(noise_pred, x, dtype, n, hl, wl, kind, guidance, sc, da, denom, e_out, e1, e2, e3, cur_sample, decode_in, stream)
    good = [p(0), p(1), 2, n, hl, wl, 4, 7.5, 1.0, 0.1, 0.5, p(2), p(3), p(4), p(5), None, p(7), None]
    for i in (0, 1, 11, 12, 13, 14):
        assert step(*[None if j == i else a for j, a in enumerate(good)]) == EINVAL and b"null" in L.cs_last_error(), i
    for kind, needs in ((0, (11, 15)), (1, (12, 15)), (2, (11, 12)), (3, (11, 12, 13))):
        args = [kind if j == 6 else a for j, a in enumerate(good)]
        args[15] = p(6)
        for i in needs:
            assert step(*[None if j == i else a for j, a in enumerate(args)]) == EINVAL and b"null" in L.cs_last_error(), (kind, i)
    for i in (3, 4, 5):
        assert step(*[0 if j == i else a for j, a in enumerate(good)]) == EINVAL and b"non-positive" in L.cs_last_error()
    for bad in (-1, 3):
        assert step(*[bad if j == 2 else a for j, a in enumerate(good)]) == EINVAL and b"dtype" in L.cs_last_error()
    for bad in (-1, 5):
        assert step(*[bad if j == 6 else a for j, a in enumerate(good)]) == EINVAL and b"kind" in L.cs_last_error()
    for i in (7, 8, 9, 10):
        for bad in (float("nan"), float("-inf")):
            assert step(*[bad if j == i else a for j, a in enumerate(good)]) == EINVAL and b"finite" in L.cs_last_error()
    for zero in (0.0, 1e-60):   # (1e-60 is 0 as a float32)
        assert step(*[zero if j == 10 else a for j, a in enumerate(good)]) == EINVAL and b"denom" in L.cs_last_error()
    assert step(*[p(3) if j == 11 else a for j, a in enumerate(good)]) == EINVAL and b"overlap" in L.cs_last_error()   # e_out on e1
    assert step(*[p(1) if j == 16 else a for j, a in enumerate(good)]) == EINVAL and b"overlap" in L.cs_last_error()   # decode_in on x
    assert step(*[p(0) if j == 11 else a for j, a in enumerate(good)]) == EINVAL and b"overlap" in L.cs_last_error()   # e_out on noise_pred
    first = [0 if j == 6 else a for j, a in enumerate(good)]
    first[15] = p(2)
    assert step(*first) == EINVAL and b"overlap" in L.cs_last_error()   # cur_sample (written by FIRST) on e_out


def test_wrappers_refuse_bad_arguments_and_host_tensors(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = torch.zeros(2, 9, 2, 3)
    lat = torch.zeros(1, 4, 2, 3)
    filled, mask = torch.zeros(1, 16, 24, 3, dtype=torch.uint8), torch.zeros(1, 16, 24, dtype=torch.uint8)
    for call in (lambda: engine.inpaint_image_prep(filled, mask, x, (2, 3)),
                 lambda: engine.inpaint_latent_init(lat, lat.clone(), lat.clone(), (0.5, 0.5), x),
                 lambda: engine.plms_step(torch.zeros(2, 4, 2, 3), x, "first", 7.5, (1.0, 0.1, 0.5), e_out=lat.clone(), cur_sample=lat.clone())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    bad = [lambda: engine.inpaint_image_prep(filled.float(), mask, x, (2, 3)),
           lambda: engine.inpaint_image_prep(filled, mask[:, :8], x, (2, 3)),
           lambda: engine.inpaint_image_prep(filled, mask, x[:1], (2, 3)),
           lambda: engine.inpaint_image_prep(filled, mask, x, (0, 3)),
           lambda: engine.inpaint_latent_init(lat, lat.half(), None, None, x),
           lambda: engine.inpaint_latent_init(lat, lat.clone(), lat.half(), (0.5, 0.5), x),
           lambda: engine.inpaint_latent_init(lat, lat.clone(), lat.clone(), (0.5, float("nan")), x),
           lambda: engine.plms_step(torch.zeros(2, 4, 2, 3), x, "third", 7.5, (1.0, 0.1, 0.5)),
           lambda: engine.plms_step(torch.zeros(2, 4, 2, 3), x, "order2", 7.5, (1.0, 0.1, 0.5), e_out=lat.clone()),
           lambda: engine.plms_step(torch.zeros(2, 4, 2, 3), x, "second", 7.5, (1.0, 0.1, 0.5), e_out=lat.clone(), history=[lat], cur_sample=lat.clone()),
           lambda: engine.plms_step(torch.zeros(2, 4, 2, 3), x, "first", 7.5, (1.0, 0.1, 0.0), e_out=lat.clone(), cur_sample=lat.clone()),
           lambda: engine.plms_step(torch.zeros(2, 4, 2, 3).half(), x, "first", 7.5, (1.0, 0.1, 0.5), e_out=lat.clone(), cur_sample=lat.clone()),
           lambda: engine.plms_step(torch.zeros(3, 4, 2, 3), x, "first", 7.5, (1.0, 0.1, 0.5), e_out=lat.clone(), cur_sample=lat.clone())]
    for call in bad:
        with pytest.raises(ValueError):
            call()


def test_runner_surface():
    model = fm.FakeInpaintModel("cpu", torch.float32, in_channels=4)
    with pytest.raises(ValueError, match="has 4 UNet input channels, but inpainting requires 9 channels"):
        ir.InpaintRunner(*model.parts())
    model = fm.FakeInpaintModel("cpu", torch.float32)
    runner = ir.InpaintRunner(*model.parts())
    sch = plms_oracle.PLMSOracle()
    assert torch.equal(runner.alphas_cumprod, sch.alphas_cumprod) and runner.num_train_timesteps == 1000
    assert torch.equal(ir.InpaintRunner(*model.parts(), scheduler=sch).alphas_cumprod, sch.alphas_cumprod)
    # make_inpaint: the reference's prompt for an empty one, a fresh generator seeded seed + frame_index
    seen = []

    class Recorder:
        def __call__(self, prompt, filled_u8, mask, num_inference_steps, guidance_scale, strength, generator):
            seen.append((prompt, num_inference_steps, guidance_scale, strength, generator.initial_seed(), generator.device.type))
            return filled_u8

    inpaint = ir.make_inpaint(Recorder(), "", 12, 3.0, 0.8, seed=40)
    inpaint(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.bool), 2)
    ir.make_inpaint(Recorder(), "a cat", 5, 7.5, 1.0, seed=1)(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.bool), 0)
    assert seen == [("high quality, detailed", 12, 3.0, 0.8, 42, "cpu"), ("a cat", 5, 7.5, 1.0, 1, "cpu")]
