"""cs_stereo_attention_half (float16 / bfloat16 q, k, v and output on the half-input MFMA) on the GPU against
tests/golden/bn_attention_half.npz: exact routing in both dtypes and every workgroup shape, values within 4 x the reference's
own half-precision error of the float64 reference on the half-rounded inputs, the BNAttention drop-in behind
stereo_utils.HALF_ATTENTION, an `out` destination, and ABI refusals that write nothing."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import attention_half_oracle as aho  # noqa: E402

from comfystereo_amd import _native, engine, stereo_utils  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(ROOT, "tests", "golden", "bn_attention_half.npz"))
META = json.loads(str(FIX["meta"]))
CASES = {c["id"]: c for c in META["cases"]}
FACTOR = 4.0   # the factor of tests/test_gpu_attention.py: out may be this many times further from the float64 reference than
               # the reference in the same dtype is (e_ref, recorded by the fixture's maker from the reference alone)
ROUTING = sorted(c for c in CASES if CASES[c]["kind"] == "routing")
VALUES = sorted(c for c in CASES if CASES[c]["kind"] in ("value", "sharp", "plain"))


def editor_for(case):
    if case["kind"] == "plain":
        return stereo_utils.BNAttention(start_step=0 if case["cross"] else 4, direction="uni", use_cfg=True)
    return stereo_utils.BNAttention(start_step=0, direction=case["mode"], use_cfg=case["flavour"] != "nocfg")


def device_inputs(case):
    return tuple(aho.to_torch(t, case["dtype"], "cuda") for t in aho.case_inputs(case))


def run_engine(case):
    q, k, v = device_inputs(case)
    return engine.stereo_attention(q, k, v, case["heads"], case["d"] ** -0.5, case["mode"], case["chunks"])


def run_editor(case, half):
    q, k, v = device_inputs(case)
    ed = editor_for(case)
    stereo_utils.HALF_ATTENTION = half
    try:
        out = ed(q, k, v, None, None, bool(case.get("cross")), "mid", case["heads"], scale=case["d"] ** -0.5)
    finally:
        stereo_utils.HALF_ATTENTION = False
    assert ed.cur_att_layer == 1
    return out


def routing_want(case):
    v = aho.case_inputs(case)[2]
    return aho.to_torch(aho.routing_expected(case, v), case["dtype"], "cuda")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("cid", ROUTING)
def test_routing_is_bit_exact(cid):
    case = CASES[cid]
    out, want = run_engine(case), routing_want(case)
    assert out.dtype == getattr(torch, case["dtype"])
    assert same_bits(out, want), f"{int((out != want).sum())} of {want.numel()} values differ"


@pytest.mark.parametrize("waves", (1, 2, 4))
@pytest.mark.parametrize("cid", [c for c in ROUTING if CASES[c]["heads"] == 2])
def test_routing_is_bit_exact_in_every_workgroup_shape(cid, waves):
    """n = 70 puts a partial query tile and a wave with no query at all into one 4-wave workgroup; d = 40 .. 160 covers two to
    five output blocks and the half-empty last k-step."""
    case = CASES[cid]
    _native.debug_set("attn_waves", waves)
    try:
        out = run_engine(case)
    finally:
        _native.debug_set("attn_waves", 0)
    want = routing_want(case)
    assert same_bits(out, want), f"{int((out != want).sum())} of {want.numel()} values differ"


def check_values(cid, out):
    case = CASES[cid]
    assert out.dtype == getattr(torch, case["dtype"]) and list(out.shape) == case["shape"]
    assert bool(torch.isfinite(out.float()).all())
    got = out.float().cpu().numpy().astype(np.float64)
    err = np.abs(got.reshape(-1)[FIX[cid + "/idx"]] - FIX[cid + "/ref64"]).max()
    print(f"{cid}: max|out - ref64| = {err:.3e}, e_ref = {case['e_ref']:.3e}, ratio {err / case['e_ref']:.2f}")
    # the fixture holds a sample of ref64; the WHOLE output against the float64 restatement on the half-rounded inputs, which
    # tests/test_attention_half_surface.py holds to ref64 within 1e-12 -- e_ref was taken over the whole output
    full = aho.reference64(case, *aho.case_inputs(case))
    err_all = np.abs(got - full).max()
    print(f"{cid}: whole output max|out - float64| = {err_all:.3e}, ratio {err_all / case['e_ref']:.2f}")
    assert err <= FACTOR * case["e_ref"]
    assert err_all <= FACTOR * case["e_ref"] + 1e-12
    return got


@pytest.mark.parametrize("cid", VALUES)
def test_values_within_the_reference_error(cid):
    check_values(cid, run_engine(CASES[cid]))


@pytest.mark.parametrize("cid", ["value_cfg_uni_2x1x70x40_f16", "value_cfg_bi_2x1x70x40_bf16", "value_nocfg_5x2x100x80_f16",
                                 "plain_cross77_bf16"])
def test_bnattention_behind_the_switch(cid):
    case = CASES[cid]
    assert stereo_utils.HALF_ATTENTION is False
    native = run_editor(case, True)
    check_values(cid, native)
    # the default: upcast, float32 kernel, cast back -- bit for bit
    q, k, v = device_inputs(case)
    upcast = engine.stereo_attention(q.float(), k.float(), v.float(), case["heads"], case["d"] ** -0.5, case["mode"],
                                     case["chunks"]).to(q.dtype)
    assert same_bits(run_editor(case, False), upcast)
    # the switch is live: half probabilities round where the float32 kernel does not
    assert not torch.equal(native, upcast)
    assert stereo_utils.HALF_ATTENTION is False


def test_float32_inputs_ignore_the_switch():
    case = CASES["value_cfg_uni_2x1x70x40_f16"]
    q, k, v = (t.float() for t in device_inputs(case))
    outs = []
    for half in (False, True):
        stereo_utils.HALF_ATTENTION = half
        try:
            outs.append(editor_for(case)(q, k, v, None, None, False, "mid", case["heads"], scale=case["d"] ** -0.5))
        finally:
            stereo_utils.HALF_ATTENTION = False
    assert outs[0].dtype == torch.float32 and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("cid", ["plain_cross77_f16", "plain_n9_bf16"])
def test_out_destination_in_half(cid):
    case = CASES[cid]
    q, k, v = device_inputs(case)
    out = torch.full(case["shape"], float("nan"), device="cuda", dtype=q.dtype)
    res = engine.stereo_attention(q, k, v, case["heads"], case["d"] ** -0.5, "self", out=out)
    assert res is out
    check_values(cid, out)
    with pytest.raises(ValueError):
        engine.stereo_attention(q, k, v, case["heads"], case["d"] ** -0.5, "self", out=out.float())


def test_refusals_write_nothing():
    L = _native.lib()
    buf = torch.zeros(4 * 8 * 8 * 168, device="cuda", dtype=torch.float16)
    out = torch.full((4 * 8 * 8 * 168 + 8,), 7.0, device="cuda", dtype=torch.float16)
    p = ctypes.c_void_p(buf.data_ptr())
    o = ctypes.c_void_p(out.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = L.cs_stereo_attention_half
    assert f(p, p, p, o, 0, 2, 2, 1, 2, 8, 8, 44, 0.1, 0, st) == _native.CS_ELIMIT      # d = 44: a multiple of 4, not of 8
    assert b"head dimension" in L.cs_last_error()
    assert f(p, p, p, o, 1, 2, 2, 1, 2, 8, 8, 168, 0.1, 0, st) == _native.CS_ELIMIT     # d above the limit
    assert f(p, p, p, o, 2, 2, 2, 1, 2, 8, 8, 40, 0.1, 0, st) == _native.CS_EINVAL      # unknown dtype
    assert b"dtype" in L.cs_last_error()
    assert f(p, p, p, o, -1, 2, 2, 1, 2, 8, 8, 40, 0.1, 0, st) == _native.CS_EINVAL
    assert f(p, p, p, o, 0, 2, 1, 1, 2, 8, 8, 40, 0.1, 1, st) == _native.CS_EINVAL      # uni with one view
    assert f(p, p, p, ctypes.c_void_p(out.data_ptr() + 8), 0, 2, 2, 1, 2, 8, 8, 40, 0.1, 1, st) == _native.CS_EINVAL   # misaligned
    assert f(ctypes.c_void_p(buf.data_ptr() + 2), p, p, o, 1, 2, 2, 1, 2, 8, 8, 40, 0.1, 1, st) == _native.CS_EINVAL
    assert b"alignment" in L.cs_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
