"""cs_stereo_attention and the BNAttention drop-in on the GPU against tests/golden/bn_attention.npz: exact routing, values
within 4 x the reference's own float32 error of the float64 reference, the plain path, the registered toy module through the
plain-to-edited switch and after restore_attention, the half-precision upcast, and refusals that write nothing."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import attention_oracle as ao  # noqa: E402

from comfystereo_amd import _native, engine, stereo_utils  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(ROOT, "tests", "golden", "bn_attention.npz"))
META = json.loads(str(FIX["meta"]))
CASES = {c["id"]: c for c in META["cases"]}
FACTOR = 4.0   # out may be this many times further from the float64 reference than the float32 reference is


def editor_for(case):
    if case["kind"] == "plain":
        return stereo_utils.BNAttention(start_step=0 if case["cross"] else 4, direction="uni", use_cfg=True)
    return stereo_utils.BNAttention(start_step=0, direction=case["mode"], use_cfg=case["flavour"] != "nocfg")


def run_editor(case):
    q, k, v = (torch.from_numpy(t).cuda() for t in ao.case_inputs(case))
    ed = editor_for(case)
    out = ed(q, k, v, None, None, bool(case.get("cross")), "mid", case["heads"], scale=case["d"] ** -0.5)
    assert ed.cur_att_layer == 1
    return out, v


@pytest.mark.parametrize("cid", sorted(c for c in CASES if CASES[c]["kind"] == "routing"))
def test_routing_is_bit_exact(cid):
    case = CASES[cid]
    out, v = run_editor(case)
    want = torch.from_numpy(ao.routing_expected(case, v.cpu().numpy())).cuda()
    assert out.dtype == torch.float32 and out.shape == want.shape
    assert torch.equal(out, want), f"{int((out != want).sum())} of {want.numel()} values differ"


@pytest.mark.parametrize("waves", (1, 2))
@pytest.mark.parametrize("cid", sorted(c for c in CASES if CASES[c]["kind"] == "routing" and CASES[c]["heads"] == 2))
def test_routing_is_bit_exact_in_every_workgroup_shape(cid, waves):
    """The launcher runs 4-wave workgroups (n = 70 puts a partial query tile and a wave with no query at all into one
    workgroup); the 1- and 2-wave forms the sweeps select stay bit-exact too, for every number of output blocks."""
    case = CASES[cid]
    _native.debug_set("attn_waves", waves)
    try:
        out, v = run_editor(case)
    finally:
        _native.debug_set("attn_waves", 0)
    want = torch.from_numpy(ao.routing_expected(case, v.cpu().numpy())).cuda()
    assert torch.equal(out, want), f"{int((out != want).sum())} of {want.numel()} values differ"


@pytest.mark.parametrize("cid", sorted(c for c in CASES if CASES[c]["kind"] in ("value", "sharp", "plain")))
def test_values_within_the_reference_error(cid):
    case = CASES[cid]
    out, _ = run_editor(case)
    assert list(out.shape) == case["shape"] and bool(torch.isfinite(out).all())
    got = out.cpu().numpy().astype(np.float64).reshape(-1)[FIX[cid + "/idx"]]
    err = np.abs(got - FIX[cid + "/ref64"]).max()
    print(f"{cid}: max|out - ref64| = {err:.3e}, e_ref = {case['e_ref']:.3e}, ratio {err / case['e_ref']:.2f}")
    assert err <= FACTOR * case["e_ref"]
    # the fixture holds a sample of ref64 (file size); the WHOLE output against the float64 restatement, which
    # tests/test_attention_surface.py holds to ref64 within 1e-12 -- e_ref was taken over the whole output
    q, k, v = ao.case_inputs(case)
    full = ao.attention(q, k, v, case["heads"], case["d"] ** -0.5, case["mode"], case["chunks"])
    err_all = np.abs(out.cpu().numpy().astype(np.float64) - full).max()
    print(f"{cid}: whole output max|out - float64| = {err_all:.3e}, ratio {err_all / case['e_ref']:.2f}")
    assert err_all <= FACTOR * case["e_ref"] + 1e-12


def test_engine_modes_equal_the_restatement_with_out_and_chunks():
    """engine.stereo_attention directly: an `out` destination, and self mode at n_k = 77 and at n = 9 (one partial tile)."""
    for cid in ("plain_cross77", "plain_n9"):
        case = CASES[cid]
        q, k, v = (torch.from_numpy(t).cuda() for t in ao.case_inputs(case))
        out = torch.full(case["shape"], float("nan"), device="cuda")
        res = engine.stereo_attention(q, k, v, case["heads"], case["d"] ** -0.5, "self", out=out)
        assert res is out
        got = out.cpu().numpy().astype(np.float64).reshape(-1)[FIX[cid + "/idx"]]
        assert np.abs(got - FIX[cid + "/ref64"]).max() <= FACTOR * case["e_ref"]


def test_toy_module_through_the_switch_and_after_restore():
    toy = META["toy"]
    net = ao.toy_model({k: FIX["toy/w/" + k] for k in toy["weights"]}).cuda()
    ed = stereo_utils.BNAttention(start_step=toy["start_step"], total_steps=toy["steps"], direction="uni", use_cfg=True)
    outs, book, layers = ao.toy_run(net, stereo_utils.register_attention_editor_diffusers, stereo_utils.restore_attention, ed,
                                    device="cuda")
    assert layers == toy["num_att_layers"] and [list(b) for b in book] == toy["book"]
    assert len(outs) == toy["steps"] * toy["layers"] + toy["layers"]
    for i, o in enumerate(outs):
        err = np.abs(o.astype(np.float64) - FIX[f"toy/ref64/{i}"]).max()
        print(f"toy call {i}: max|out - ref64| = {err:.3e}, e_ref = {toy['e_ref'][i]:.3e}")
        assert err <= FACTOR * toy["e_ref"][i], i
    # the switch is in the record: the first step's outputs are plain attention, the later ones see the left view's keys
    assert np.abs(FIX["toy/ref64/0"][1] - FIX["toy/ref64/0"][0]).max() > 1e-3


def test_half_precision_is_the_float32_result_cast():
    case = CASES["value_cfg_uni_2x1x70x40"]
    q, k, v = (torch.from_numpy(t).cuda() for t in ao.case_inputs(case))
    for dt in (torch.float16, torch.bfloat16):
        qh, kh, vh = q.to(dt), k.to(dt), v.to(dt)
        got = editor_for(case)(qh, kh, vh, None, None, False, "mid", case["heads"], scale=case["d"] ** -0.5)
        want = editor_for(case)(qh.float(), kh.float(), vh.float(), None, None, False, "mid", case["heads"], scale=case["d"] ** -0.5)
        assert got.dtype == dt and torch.equal(got, want.to(dt))


def test_refusals_write_nothing():
    L = _native.lib()
    buf = torch.zeros(4 * 8 * 8 * 164, device="cuda")
    out = torch.full((4 * 8 * 8 * 164,), 7.0, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    o = ctypes.c_void_p(out.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.cs_stereo_attention(p, p, p, o, 2, 2, 1, 2, 8, 8, 42, 0.1, 0, st) == _native.CS_ELIMIT
    assert L.cs_stereo_attention(p, p, p, o, 2, 2, 1, 2, 8, 8, 164, 0.1, 0, st) == _native.CS_ELIMIT
    assert L.cs_stereo_attention(p, p, p, o, 2, 1, 1, 2, 8, 8, 40, 0.1, 1, st) == _native.CS_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(RuntimeError):
        qg = torch.zeros(8, 8, 40, device="cuda", requires_grad=True)
        stereo_utils.BNAttention(start_step=0)(qg, qg, qg, None, None, False, "mid", 2, scale=0.1)
