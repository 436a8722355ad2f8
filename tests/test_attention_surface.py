"""The stereo attention's surface without a GPU: exports, enum values, the numpy restatement against every fixture case
(tests/golden/bn_attention.npz), BNAttention's defaults and step bookkeeping against the recorded ones, and the wrapper's
argument checks, which raise before any pointer is passed."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import attention_oracle as ao  # noqa: E402

from comfystereo_amd import _native, engine, stereo_utils  # noqa: E402

FIX = np.load(os.path.join(ROOT, "tests", "golden", "bn_attention.npz"))
META = json.loads(str(FIX["meta"]))
CASES = {c["id"]: c for c in META["cases"]}


def test_exports_and_enum_values():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    for name in ("cs_stereo_attention", "cs_stereo_attention_max_head_dim"):
        assert re.search(r"CS_API\s+int\s+" + name + r"\s*\(", hdr), name
        assert name in _native.EXPORTS
        assert hasattr(_native.lib(), name)
    for key, name in (("self", "CS_ATTN_SELF"), ("uni", "CS_ATTN_UNI"), ("bi", "CS_ATTN_BI")):
        assert int(re.search(name + r"\s*=\s*(\d+)", hdr).group(1)) == _native.ATTN_MODE[key]
    assert _native.lib().cs_stereo_attention_max_head_dim() == 160
    assert _native.lib().cs_version() == _native.ABI_VERSION == 4


def test_fixture_covers_the_cases_and_fits():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "bn_attention.npz")) < 1 << 20
    shapes = {(2, 1, 70, 40), (5, 2, 100, 80), (3, 1, 9, 160), (2, 1, 64, 64), (8, 1, 256, 160)}
    for fl in ("cfg_uni", "cfg_bi", "nocfg"):
        assert {(c["heads"], c["samples"], c["n"], c["d"]) for c in CASES.values() if c["kind"] == "value" and c["flavour"] == fl} >= shapes
    assert {c["flavour"] for c in CASES.values() if c["kind"] == "sharp"} == {"cfg_uni", "cfg_bi"}
    assert {c["n_k"] for c in CASES.values() if c["kind"] == "plain"} == {70, 77, 9}
    rout = {(c["mode"], c["heads"], c["samples"], c["n"], c["d"]) for c in CASES.values() if c["kind"] == "routing"}
    assert rout >= {(m, h, b, n, d) for m in ("uni", "bi") for h, b, n in ((2, 2, 70), (3, 1, 9)) for d in (40, 64, 80, 160)}
    # ... and batches of 512 and 256 (c s b h) entries
    assert rout >= {(m, 8, b, 70, d) for m in ("uni", "bi") for b, d in ((16, 40), (16, 80), (8, 160), (8, 64))}


@pytest.mark.parametrize("cid", sorted(c for c in CASES if CASES[c]["kind"] != "routing"))
def test_restatement_reproduces_the_reference_in_float64(cid):
    case = CASES[cid]
    q, k, v = ao.case_inputs(case)
    got = ao.attention(q, k, v, case["heads"], case["d"] ** -0.5, case["mode"], case["chunks"])
    assert list(got.shape) == case["shape"]
    assert np.abs(got.reshape(-1)[FIX[cid + "/idx"]] - FIX[cid + "/ref64"]).max() <= 1e-12
    # the recorded e_ref is the reference's own float32 error: a few float32 ulps of O(1) values
    assert 0 < case["e_ref"] < 1e-4 and np.abs(FIX[cid + "/ref"] - FIX[cid + "/ref64"]).max() <= case["e_ref"]


@pytest.mark.parametrize("cid", sorted(c for c in CASES if CASES[c]["kind"] == "routing"))
def test_restatement_routes_exactly(cid):
    case = CASES[cid]
    q, k, v = ao.case_inputs(case)
    want = ao.routing_expected(case, v)
    for dtype in (np.float32, np.float64):
        got = ao.attention(q, k, v, case["heads"], case["d"] ** -0.5, case["mode"], case["chunks"], dtype)
        assert np.array_equal(got.astype(np.float32).view(np.uint32), want.view(np.uint32)), dtype


def test_bnattention_defaults_and_step_bookkeeping(monkeypatch):
    assert vars(stereo_utils.BNAttention()) == META["defaults"]
    ed = stereo_utils.BNAttention(start_step=2, total_steps=9, direction="bi", use_cfg=False)
    assert (ed.start_step, ed.total_steps, ed.direction, ed.use_cfg) == (2, 9, "bi", False)
    monkeypatch.setattr(stereo_utils.BNAttention, "forward", lambda self, *a, **kw: "out")
    legacy = stereo_utils.BNAttention(start_step=10 ** 6)
    seen = []
    for _ in range(len(META["legacy_steps"])):
        assert legacy(None, None, None, None, None, False, "mid", 2, scale=1.0) == "out"
        seen.append([legacy.cur_att_layer, legacy.cur_step])
    assert seen == META["legacy_steps"] and seen[31] == [32, 1]
    toy = META["toy"]
    ed = stereo_utils.BNAttention(start_step=toy["start_step"], total_steps=toy["steps"])
    ed.num_att_layers = toy["num_att_layers"]
    book = []
    for _ in range(toy["steps"] * toy["layers"]):
        ed(None, None, None, None, None, False, "mid", 2, scale=1.0)
        book.append([ed.cur_att_layer, ed.cur_step])
    assert book == toy["book"]


def test_register_counts_layers_and_restore_puts_the_forwards_back():
    net = ao.toy_model({k: FIX["toy/w/" + k] for k in META["toy"]["weights"]})
    ed = stereo_utils.BNAttention(start_step=1)
    own = [type(m).forward for m in (net.down_blocks[0], net.mid_block)]
    stereo_utils.register_attention_editor_diffusers(net, ed)
    assert ed.num_att_layers == META["toy"]["num_att_layers"] == 2
    assert all("forward" in m.__dict__ for m in (net.down_blocks[0], net.mid_block))
    x = torch.from_numpy(ao.toy_input(0))
    with pytest.raises(ValueError):
        net.mid_block(x, attention_mask=torch.ones(4, 6, dtype=torch.bool))
    stereo_utils.restore_attention(net)
    assert all("forward" not in m.__dict__ for m in (net.down_blocks[0], net.mid_block))
    assert [type(m).forward for m in (net.down_blocks[0], net.mid_block)] == own
    with torch.no_grad():   # the module's own forward again: the recorded plain attention, on the CPU
        i = META["toy"]["steps"] * META["toy"]["layers"]
        got = net.down_blocks[0](torch.from_numpy(ao.toy_input(i))).numpy()
    assert np.abs(got - FIX[f"toy/ref64/{i}"]).max() <= 1e-5


def test_unknown_direction_and_missing_gpu():
    q = torch.zeros(8, 4, 8)
    ed = stereo_utils.BNAttention(start_step=0, direction="sideways")
    if torch.cuda.is_available():
        q = q.cuda()
    with pytest.raises(ValueError, match="Unknown direction"):
        ed(q, q, q, None, None, False, "mid", 2, scale=1.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            stereo_utils.BNAttention(start_step=0)(q, q, q, None, None, False, "mid", 2, scale=1.0)


def test_wrapper_checks_raise_before_any_pointer_is_passed():
    f = torch.zeros
    ok = dict(heads=2, scale=0.5, mode="uni", chunks=2)
    bad = [
        (f(8, 4, 8), f(8, 4, 8), f(8, 4, 8), dict(ok, mode="left")),              # unknown mode
        (f(8, 4, 8).numpy(), f(8, 4, 8), f(8, 4, 8), ok),                          # not a tensor
        (f(8, 4), f(8, 4, 8), f(8, 4, 8), ok),                                     # not 3-d
        (f(8, 4, 8, dtype=torch.float16), f(8, 4, 8), f(8, 4, 8), ok),             # dtype
        (f(8, 8, 4).transpose(1, 2), f(8, 4, 8), f(8, 4, 8), ok),                  # not contiguous
        (f(8, 4, 8), f(8, 4, 8), f(8, 5, 8), ok),                                  # k and v differ
        (f(8, 4, 8), f(8, 5, 8), f(8, 5, 8), ok),                                  # uni with n_k != n
        (f(8, 4, 8), f(8, 4, 8), f(8, 4, 8), dict(ok, heads=3)),                   # batch not c * s * b * h
        (f(4, 4, 8), f(4, 4, 8), f(4, 4, 8), ok),                                  # one view only (s = 1) under uni with 2 chunks
        (f(8, 4, 42), f(8, 4, 42), f(8, 4, 42), ok),                               # d not a multiple of 4
        (f(8, 4, 164), f(8, 4, 164), f(8, 4, 164), ok),                            # d above the limit
        (f(8, 4, 8), f(8, 4, 8), f(8, 4, 8), dict(ok, scale=float("nan"))),        # scale
        (f(8, 4, 8, requires_grad=True), f(8, 4, 8), f(8, 4, 8), ok),              # forward only
        (f(8, 4, 8), f(8, 4, 8), f(8, 4, 8), dict(ok, out=f(2, 4, 16))),           # out of the wrong shape
        (f(0, 4, 8), f(0, 4, 8), f(0, 4, 8), ok),                                  # empty
        (f(8, 4, 8), f(8, 4, 8), f(8, 4, 8), ok),                                  # well-formed, but host memory
    ]
    for q, k, v, kw in bad:
        with pytest.raises(ValueError):
            engine.stereo_attention(q, k, v, **kw)


def test_abi_refuses_bad_arguments_without_device_work():
    import ctypes
    L = _native.lib()
    p = ctypes.c_void_p(256)
    args = lambda **kw: [kw.get(x, dflt) for x, dflt in (("c", 2), ("s", 2), ("b", 1), ("h", 2), ("n", 8), ("n_k", 8), ("d", 40))]  # noqa: E731
    assert L.cs_stereo_attention(None, p, p, p, *args(), 0.1, 1, None) == _native.CS_EINVAL
    assert L.cs_stereo_attention(p, p, p, p, *args(n=0), 0.1, 1, None) == _native.CS_EINVAL
    assert L.cs_stereo_attention(p, p, p, p, *args(), 0.1, 3, None) == _native.CS_EINVAL
    assert L.cs_stereo_attention(p, p, p, p, *args(s=1), 0.1, 1, None) == _native.CS_EINVAL
    assert L.cs_stereo_attention(p, p, p, p, *args(n_k=9), 0.1, 2, None) == _native.CS_EINVAL
    assert L.cs_stereo_attention(p, p, p, p, *args(d=42), 0.1, 0, None) == _native.CS_ELIMIT
    assert L.cs_stereo_attention(p, p, p, p, *args(d=164), 0.1, 0, None) == _native.CS_ELIMIT
    assert b"head dimension" in L.cs_last_error()
    assert L.cs_stereo_attention(ctypes.c_void_p(260), p, p, p, *args(), 0.1, 1, None) == _native.CS_EINVAL
    # the development switch of the tile-size sweeps: 0 (the launcher's choice), 1, 2 or 4 waves per workgroup
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    assert int(re.search(r"CS_DEBUG_ATTN_WAVES\s*=\s*(\d+)", hdr).group(1)) == _native.DEBUG["attn_waves"]
    for v, want in ((3, _native.CS_EINVAL), (8, _native.CS_EINVAL), (4, _native.CS_OK), (0, _native.CS_OK)):
        assert L.cs_debug_set(_native.DEBUG["attn_waves"], v) == want
