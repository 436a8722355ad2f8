"""Null-text inversion (comfystereo_amd.inversion; cs_ddim_step, cs_null_loss_grad, cs_adam_step): the public surface against the
reference's recorded signatures, the argument refusals, and the float64 restatement (tools/inversion_oracle.py) held to the
reference's own values in tests/golden/inversion_*.npz within the reference's recorded error (not gpu)."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import inversion_oracle as io_
import make_inversion_goldens as mk
from comfystereo_amd import _native, diffusion_utils, engine, inversion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["cs_ddim_step", "cs_null_loss_workspace_bytes", "cs_null_loss_grad", "cs_adam_step"]
DTYPES = ("float32", "float16", "bfloat16")


def load(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", f"inversion_{name}.npz"))
    return z, json.loads(str(z["meta"]))


def load_steps(dtype_name):
    """The kernel cases of a dtype, from its two files -> ({key: array}, cases, steps)."""
    arrays, cases = {}, []
    for suffix in ("", "_b"):
        z, meta = load(f"step_{dtype_name}{suffix}")
        arrays.update({k: z[k] for k in z.files if k != "meta"})
        cases += meta["cases"]
    return arrays, cases, meta["steps"]


def values(a, dtype_name):
    """A fixture array (bfloat16 as int16 patterns) as float64."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.view(torch.bfloat16) if dtype_name == "bfloat16" else t).double().numpy()


def test_signatures_equal_the_references():
    _, meta = load("surface")
    for key, params in meta["signatures"].items():
        cls, name = key.split(".")
        if name == "<properties>":
            for prop in params:
                assert isinstance(vars(getattr(inversion, cls))[prop], property), key
            continue
        fn = getattr(getattr(inversion, cls), name)
        got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in inspect.signature(fn).parameters.values()]
        assert got == params, key
    assert str(inspect.signature(inversion.make_invert)) == \
        "(model, num_ddim_steps, guidance_scale, null_text_optimization=True, num_inner_steps=10, early_stop_epsilon=1e-05)"
    assert str(inspect.signature(engine.ddim_step)) == "(sample, eps_a, eps_b, guidance, coeffs, out=None)"
    assert issubclass(engine.NullTextLoss, torch.autograd.Function)


def test_new_exports_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    declared = set(re.findall(r"CS_API\s+[\w\s\*]+?\b(cs_\w+)\s*\(", hdr))
    L = _native.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _native.EXPORTS and hasattr(L, name), name
    assert L.cs_version() == 4 == _native.ABI_VERSION
    assert L.cs_null_loss_workspace_bytes(16384) == 0 and L.cs_null_loss_workspace_bytes(32768) == 0
    assert L.cs_null_loss_workspace_bytes(32769) == 16 and L.cs_null_loss_workspace_bytes(-1) == 0


def test_einval_before_any_device_work():
    L = _native.lib()
    p = ctypes.c_void_p(256)
    E = _native.CS_EINVAL
    c = (0.5, 0.8, 0.3, 0.9)
    assert L.cs_ddim_step(None, p, None, p, 0, 4, 1.0, *c, None) == E and b"null" in L.cs_last_error()
    assert L.cs_ddim_step(p, None, None, p, 0, 4, 1.0, *c, None) == E
    assert L.cs_ddim_step(p, p, None, None, 0, 4, 1.0, *c, None) == E
    for count in (0, -1):
        assert L.cs_ddim_step(p, ctypes.c_void_p(4096), None, p, 0, count, 1.0, *c, None) == E
    for dtype in (-1, 3):
        assert L.cs_ddim_step(p, ctypes.c_void_p(4096), None, p, dtype, 4, 1.0, *c, None) == E and b"dtype" in L.cs_last_error()
    assert L.cs_ddim_step(p, ctypes.c_void_p(4096), None, p, 0, 4, 1.0, 0.5, 0.0, 0.3, 0.9, None) == E
    assert L.cs_ddim_step(p, ctypes.c_void_p(4096), None, p, 0, 4, float("nan"), *c, None) == E
    assert L.cs_ddim_step(p, ctypes.c_void_p(264), None, p, 0, 4, 1.0, *c, None) == E and b"overlap" in L.cs_last_error()   # out, eps_a
    assert L.cs_ddim_step(ctypes.c_void_p(260), ctypes.c_void_p(4096), None, p, 0, 4, 1.0, *c, None) == E and b"overlap" in L.cs_last_error()
    assert L.cs_ddim_step(p, ctypes.c_void_p(258), None, p, 0, 4, 1.0, *c, None) == E and b"misaligned" in L.cs_last_error()
    ptrs = [ctypes.c_void_p(4096 * (i + 1)) for i in range(7)]
    for hole in range(7):
        args = [None if i == hole else q for i, q in enumerate(ptrs)]
        assert L.cs_null_loss_grad(*args, 0, 4, 7.5, *c, None, 0, None) == E, hole
    assert L.cs_null_loss_grad(*ptrs, 0, 0, 7.5, *c, None, 0, None) == E
    assert L.cs_null_loss_grad(*ptrs, 0, -5, 7.5, *c, None, 0, None) == E
    assert L.cs_null_loss_grad(*ptrs, 7, 4, 7.5, *c, None, 0, None) == E
    assert L.cs_null_loss_grad(*ptrs, 0, 40000, 7.5, *c, None, 0, None) == _native.CS_EWORKSPACE
    for hole in range(4):
        args = [None if i == hole else q for i, q in enumerate(ptrs[:4])]
        assert L.cs_adam_step(*args, 0, 4, 1e-2, 0.9, 0.999, 1e-8, 1, None) == E, hole
    assert L.cs_adam_step(*ptrs[:4], 0, -1, 1e-2, 0.9, 0.999, 1e-8, 1, None) == E
    assert L.cs_adam_step(*ptrs[:4], 5, 4, 1e-2, 0.9, 0.999, 1e-8, 1, None) == E
    assert L.cs_adam_step(*ptrs[:4], 0, 4, 1e-2, 0.9, 0.999, 1e-8, 0, None) == E and b"step" in L.cs_last_error()
    assert L.cs_adam_step(*ptrs[:4], 0, 4, 1e-2, 1.0, 0.999, 1e-8, 1, None) == E


def test_engine_wrappers_refuse_bad_arguments():
    x = torch.zeros(1, 4, 5, 7)
    c = (0.5, 0.8, 0.3, 0.9)
    bad = [torch.zeros(1, 4, 5, 8), torch.zeros(1, 4, 5, 7, dtype=torch.float16), torch.zeros(1, 4, 7, 5).transpose(2, 3),
           torch.zeros(1, 4, 5, 7, dtype=torch.float64), np.zeros((1, 4, 5, 7), np.float32)]
    for b in bad:
        with pytest.raises(ValueError):
            engine.ddim_step(x, b, None, 1.0, c)
        with pytest.raises(ValueError):
            engine.ddim_step(x, x, b, 1.0, c)
        with pytest.raises(ValueError):
            engine.null_loss_grad(x, x, b, x, 7.5, c)
        with pytest.raises(ValueError):
            engine.adam_step(x, x, b, x, 1e-2, 1)
    with pytest.raises(ValueError):
        engine.ddim_step(x, x, None, 1.0, c[:3])
    with pytest.raises(ValueError):
        engine.ddim_step(x, x, None, 1.0, (0.5, 0.0, 0.3, 0.9))
    with pytest.raises(ValueError):
        engine.ddim_step(torch.zeros(0), torch.zeros(0), None, 1.0, c)
    with pytest.raises(ValueError):
        engine.adam_step(x, x, x, x, 1e-2, 0)
    with pytest.raises(ValueError):
        engine.adam_step(x, x, x, x, 1e-2, 1, beta1=1.0)
    if not torch.cuda.is_available():   # the package's RuntimeError where there is no GPU at all, after the argument checks
        with pytest.raises(RuntimeError):
            engine.ddim_step(x, x, None, 1.0, c)
        with pytest.raises(RuntimeError):
            engine.NullTextLoss.apply(x, x, x, x, 7.5, c)
        with pytest.raises(RuntimeError):
            engine.adam_step(x, x.clone(), x.clone(), x.clone(), 1e-2, 1)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_oracle_reproduces_the_reference_steps(dtype_name):
    """The float64 restatement against the reference's outputs: the step within a few roundings of the dtype, loss and gradient
    within the recorded reference error (which is that difference: the assertion pins the oracle and the fixture to each other)."""
    z, cases, _ = load_steps(dtype_name)
    seen = {"final": 0, "interior": 0, "with_b": 0, "single": 0, "loss": 0, "interior gradient": 0, "final gradient": 0}
    for case in cases:
        x = mk.case_inputs(case["seed"], case["count"], dtype_name, ("sample", "eps_a", "eps_b", "noise"))
        f = {k: v.double().numpy() for k, v in x.items()}
        want = values(z[f"{case['id']}/out"], dtype_name)
        got = io_.ddim_step(f["sample"], f["eps_a"], f["eps_b"] if case["with_b"] else None, case["guidance"], case["coeffs"])
        assert io_.err(got, want) <= 8 * io_.ulp(dtype_name, np.abs(want).max() * 8), case["id"]
        seen["final" if case["final_branch"] else "interior"] += 1
        seen["with_b" if case["with_b"] else "single"] += 1
        if case["loss"] is not None:
            prev = (torch.from_numpy(want) + 0.1 * x["noise"].double()).to(x["sample"].dtype).double().numpy()
            _, loss, grad = io_.null_loss_grad(f["eps_a"], f["eps_b"], f["sample"], prev, case["guidance"], case["coeffs"])
            assert abs(loss - case["loss"]) <= case["ref_err"]["loss"] * (1 + 1e-9) + 1e-300, case["id"]
            assert io_.err(grad, values(z[f"{case['id']}/grad"], dtype_name)) <= case["ref_err"]["grad"] * (1 + 1e-9) + 1e-300, case["id"]
            seen["loss"] += 1
            if case["guidance"] != 1.0:   # (1 - guidance) = 0 makes the gradient identically zero
                assert np.abs(grad).max() > 0
                seen["final gradient" if case["final_branch"] else "interior gradient"] += 1
    assert all(seen.values()), seen
    assert sorted({c["count"] for c in cases}) == [1, 63, 140, 16384, 16387, 32773]
    assert {c["guidance"] for c in cases if c["with_b"]} == {1.0, 7.5}


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_oracle_reproduces_the_reference_adam(dtype_name):
    z, meta = load(f"adam_{dtype_name}")
    assert [c["count"] for c in meta["cases"]] == [1, 77 * 8, 77 * 768 + 5]
    for case in meta["cases"]:
        p0 = mk.case_inputs(case["seed"], case["count"], dtype_name, ("param",))["param"]
        grads = mk.adam_grads(case["seed"] + 1, case["count"], dtype_name)
        assert case["count"] < 3 or bool((grads[1] == 0).any())
        want = io_.adam(p0.double().numpy(), [g.double().numpy() for g in grads], case["lr"])
        assert sorted(case["ref_err"]) == ["1", "10", "2"]
        for k, errs in case["ref_err"].items():
            for j, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
                if f"{case['id']}/{name}@{k}" not in z.files:   # the largest count stores the arrays of step 10 only
                    assert case["count"] == 77 * 768 + 5 and k != "10"
                    continue
                ref = values(z[f"{case['id']}/{name}@{k}"], dtype_name)
                assert io_.err(ref, want[int(k) - 1][j]) <= errs[name] * (1 + 1e-9) + 1e-300, (case["id"], k, name)


@pytest.mark.parametrize("form", ["exact", "attn"])
def test_margin_condition_holds(form):
    """Every loss the loop compares lies at least 20 % of its threshold away from it, one outer step breaks early and one runs
    all its inner steps: a last-bit difference cannot flip a break."""
    _, meta = load(f"e2e_{form}")
    assert io_.margins(meta["losses"], meta["epsilon"]) >= 0.2
    counts = [len(r) for r in meta["losses"]]
    assert counts == meta["inner_steps"] and len(counts) == meta["steps"]
    assert any(c < meta["inner"] for c in counts) and any(c == meta["inner"] for c in counts)
    for i, row in enumerate(meta["losses"]):   # the break is where the reference's own rule puts it
        thr = meta["epsilon"] + i * 2e-5
        assert all(x >= thr for x in row[:-1]) and (row[-1] < thr or len(row) == meta["inner"])


def test_make_invert_and_the_controller_refusal():
    import null_fake_model as nm
    model = nm.NullModel("attn")
    assert callable(inversion.make_invert(model, 5, 7.5))
    assert callable(inversion.make_invert(model, 5, 7.5, null_text_optimization=False, num_inner_steps=3, early_stop_epsilon=1e-4))
    with pytest.raises(TypeError):
        diffusion_utils.register_attention_control(model, inversion.EmptyControl())
    ctl = inversion.EmptyControl()
    assert ctl.step_callback(3) == 3 and ctl.between_steps() is None and ctl(5, True, "down") == 5
    inv = inversion.NullInversion(model, 5, 7.5)
    assert inv.scheduler is model.scheduler and list(model.scheduler.timesteps) == [801, 601, 401, 201, 1]
    # the coefficients are the reference's expressions on the scheduler's alphas (both final_alpha_cumprod branches and the interior)
    a = model.scheduler.alphas_cumprod
    for kind, t, a_t, a_o in (("prev", 401, a[401], a[201]), ("prev", 1, a[1], a[0]), ("next", 401, a[201], a[401]), ("next", 1, a[0], a[1])):
        want = tuple(float(np.float32(np.sqrt(np.float64(float(v))))) for v in (1 - a_t, a_t, 1 - a_o, a_o))   # correctly rounded
        assert inv._step_coeffs(kind, t, torch.float32) == want and inv._step_coeffs(kind, torch.tensor(t), torch.float32) == want
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            inv.invert(nm.seeded_image(11), "a photo")
