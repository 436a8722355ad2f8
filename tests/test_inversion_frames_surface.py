"""Null-text optimisation on F frames at once (cs_null_loss_grad_frames, cs_adam_step_frames, engine.null_loss_grad_frames,
engine.adam_step_frames, NullInversion.invert_frames, generate_stereo_standard_frames): the exports, the workspace layout, every
refusal before the device is reached, and the condition on the fixture's inputs (not gpu)."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import inversion_oracle as io_
import null_fake_model as nm
from comfystereo_amd import _native, engine, inversion
from comfystereo_amd import stereodiffusion_nodes as sdn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["cs_null_loss_frames_workspace_bytes", "cs_null_loss_grad_frames", "cs_adam_step_frames"]
C = (0.5, 0.8, 0.3, 0.9)


def test_new_exports_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    declared = set(re.findall(r"CS_API\s+[\w\s\*]+?\b(cs_\w+)\s*\(", hdr))
    L = _native.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _native.EXPORTS and hasattr(L, name), name
    assert L.cs_version() == _native.ABI_VERSION


def test_workspace_is_two_floats_per_block_and_frame_past_one_block():
    L = _native.lib()
    for frames, per, want in ((3, 1, 0), (3, 32768, 0), (1, 32769, 16), (3, 32769, 48), (5, 65537, 5 * 3 * 8), (0, 40000, 0), (3, 0, 0),
                              (-1, 40000, 0)):
        assert L.cs_null_loss_frames_workspace_bytes(frames, per) == want, (frames, per)
        if frames > 0 and per > 0:
            assert engine.null_loss_frames_workspace_bytes(frames, per) == want
            assert L.cs_null_loss_workspace_bytes(per) * frames == want   # the single-tensor layout, once per frame


def test_abi_refusals_before_any_launch():
    L = _native.lib()
    E, LIMIT = _native.CS_EINVAL, _native.CS_ELIMIT
    ptrs = [ctypes.c_void_p(1 << 20 + i) for i in range(9)]   # far apart: nothing overlaps

    def loss(ptrs=ptrs, dtype=0, frames=3, per=4, guidance=7.5, c=C, threshold=0.0, ws=None, ws_bytes=0):
        return L.cs_null_loss_grad_frames(*ptrs, dtype, frames, per, guidance, *c, threshold, ws, ws_bytes, None)

    for hole in range(9):
        assert loss([None if i == hole else q for i, q in enumerate(ptrs)]) == E and b"null" in L.cs_last_error(), hole
    for frames, per in ((0, 4), (3, 0), (-1, 4), (3, -1)):
        assert loss(frames=frames, per=per) == E and b"cs_null_loss_grad_frames" in L.cs_last_error()
    assert loss(frames=65536) == LIMIT and b"frames" in L.cs_last_error()
    assert loss(per=32768 * 0x7fffffff + 1) == LIMIT and b"per frame" in L.cs_last_error()
    for dtype in (-1, 3):
        assert loss(dtype=dtype) == E and b"dtype" in L.cs_last_error()
    assert loss(ptrs[:7] + [ptrs[7], ptrs[7]]) == E and b"active_out must not be active_in" in L.cs_last_error()
    assert loss(threshold=float("nan")) == E and b"threshold" in L.cs_last_error()
    assert loss(c=(0.5, 0.0, 0.3, 0.9)) == E and loss(guidance=float("inf")) == E
    assert loss(per=40000) == _native.CS_EWORKSPACE
    assert loss([ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[0]] + ptrs[5:]) == E and b"overlap" in L.cs_last_error()   # rec = eps_uncond
    assert loss(ptrs[:8] + [ctypes.c_void_p(ptrs[7].value + 2)]) == E and b"overlap" in L.cs_last_error()           # the two flag buffers

    def adam(ptrs=ptrs[:5], dtype=0, frames=3, per=4, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
        return L.cs_adam_step_frames(*ptrs, dtype, frames, per, lr, beta1, beta2, eps, step, None)

    for hole in range(5):
        assert adam([None if i == hole else q for i, q in enumerate(ptrs[:5])]) == E and b"null" in L.cs_last_error(), hole
    for frames, per in ((0, 4), (3, 0), (-2, 4)):
        assert adam(frames=frames, per=per) == E and b"cs_adam_step_frames" in L.cs_last_error()
    assert adam(frames=65536) == LIMIT
    assert adam(dtype=5) == E and b"cs_adam_step_frames: unknown dtype" in L.cs_last_error()
    assert adam(step=0) == E and b"step" in L.cs_last_error()
    assert adam(beta1=1.0) == E and adam(lr=float("nan")) == E
    # the single-tensor call's messages are what they were
    assert L.cs_adam_step(*ptrs[:4], 0, 4, 1e-2, 0.9, 0.999, 1e-8, 0, None) == E
    assert L.cs_last_error() == b"cs_adam_step: the step number counts from 1"


def test_engine_wrappers_refuse_before_the_library():
    x = torch.zeros(3, 4, 5, 7)
    on, off = torch.ones(3, dtype=torch.uint8), torch.zeros(3, dtype=torch.uint8)

    def loss(eu=x, ec=x, cur=x, prev=x, guidance=7.5, c=C, a_in=on, threshold=0.0, **kw):
        return engine.null_loss_grad_frames(eu, ec, cur, prev, guidance, c, a_in, threshold, **kw)

    bad = [torch.zeros(3, 4, 5, 8), torch.zeros(3, 4, 5, 7, dtype=torch.float16), torch.zeros(3, 4, 7, 5).transpose(2, 3),
           torch.zeros(3, 4, 5, 7, dtype=torch.float64), np.zeros((3, 4, 5, 7), np.float32), None]
    for b in bad:
        for name in ("ec", "cur", "prev"):
            with pytest.raises(ValueError):
                loss(**{name: b})
        if b is not None:
            with pytest.raises(ValueError):
                loss(rec=b)
            with pytest.raises(ValueError):
                engine.adam_step_frames(x, x.clone(), b, x.clone(), on, 1e-2, 1)
    refusals = [dict(eu=torch.zeros(0, 4), ec=torch.zeros(0, 4), cur=torch.zeros(0, 4), prev=torch.zeros(0, 4)),                    # F == 0
                dict(eu=torch.zeros(3, 0), ec=torch.zeros(3, 0), cur=torch.zeros(3, 0), prev=torch.zeros(3, 0)),                    # per == 0
                dict(eu=torch.zeros(12), ec=torch.zeros(12), cur=torch.zeros(12), prev=torch.zeros(12)),                            # no frame axis
                dict(a_in=on, active_out=on), dict(a_in=on, active_out=on[:]),                                                     # one buffer
                dict(a_in=torch.ones(2, dtype=torch.uint8)), dict(a_in=torch.ones(3, dtype=torch.bool)), dict(a_in=None),
                dict(active_out=torch.ones(4, dtype=torch.uint8)), dict(active_out=torch.ones(3)),
                dict(loss=torch.zeros(3, dtype=torch.float64)), dict(loss=torch.zeros(2)),
                dict(threshold=float("nan")), dict(c=C[:3]), dict(c=(0.5, 0.0, 0.3, 0.9)), dict(guidance=float("inf")),
                dict(workspace=torch.zeros(8))]
    for kw in refusals:
        with pytest.raises(ValueError):
            loss(**kw)
    many = torch.zeros(engine.MAX_FRAMES + 1, 1)
    with pytest.raises(ValueError, match="frames"):
        loss(eu=many, ec=many, cur=many, prev=many, a_in=torch.ones(engine.MAX_FRAMES + 1, dtype=torch.uint8))
    wide = torch.empty((1, engine.NULL_LOSS_MAX_COUNT + 1), device="meta")   # a shape without memory: the check is on the count
    with pytest.raises(ValueError, match="per frame"):
        loss(eu=wide, ec=wide, cur=wide, prev=wide, a_in=torch.ones(1, dtype=torch.uint8, device="meta"))
    big = torch.zeros(1, 32769)
    with pytest.raises(ValueError, match="workspace"):
        loss(eu=big, ec=big, cur=big, prev=big, a_in=on[:1], workspace=torch.zeros(8, dtype=torch.uint8))
    for kw in (dict(step=0), dict(step=True), dict(beta1=1.0), dict(lr=float("nan")), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            engine.adam_step_frames(x, x.clone(), x.clone(), x.clone(), on, **dict(dict(lr=1e-2, step=1), **kw))
    for flags in (on[:2], torch.ones(3), None):
        with pytest.raises(ValueError):
            engine.adam_step_frames(x, x.clone(), x.clone(), x.clone(), flags, 1e-2, 1)
    with pytest.raises(ValueError, match="frames"):
        engine.adam_step_frames(many, many.clone(), many.clone(), many.clone(), torch.ones(engine.MAX_FRAMES + 1, dtype=torch.uint8), 1e-2, 1)
    if not torch.cuda.is_available():   # the package's RuntimeError where there is no GPU at all, after the argument checks
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            loss(active_out=off)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            engine.NullTextLossFrames.apply(x, x, x, x, 7.5, C, on, 0.0)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            engine.adam_step_frames(x, x.clone(), x.clone(), x.clone(), on, 1e-2, 1)


def test_python_surface():
    sig = inspect.signature(inversion.NullInversion.invert_frames)
    assert list(sig.parameters) == ["self", "images", "prompt", "num_inner_steps", "early_stop_epsilon", "null_text_optimization"]
    assert [sig.parameters[n].default for n in ("num_inner_steps", "early_stop_epsilon", "null_text_optimization")] == [10, 1e-5, True]
    assert inspect.signature(inversion.make_invert_frames) == inspect.signature(inversion.make_invert)
    sig = inspect.signature(sdn.generate_stereo_standard_frames)
    assert list(sig.parameters) == ["image", "depth_map", "scale_factor", "direction", "deblur", "num_inference_steps", "guidance_scale",
                                    "model", "invert_frames", "frames_per_batch", "noise", "generator"]
    assert sig.parameters["frames_per_batch"].default == 4 and sdn.STANDARD_ALL_FRAMES is False
    model = nm.NullModel("exact")
    assert callable(inversion.make_invert_frames(model, 5, 7.5))
    inv = inversion.NullInversion(model, 5, 7.5)
    for images in (torch.zeros(512, 512, 3, dtype=torch.uint8), torch.zeros(2, 512, 512, 3), torch.zeros(0, 512, 512, 3, dtype=torch.uint8),
                   torch.zeros(2, 64, 64, 3, dtype=torch.uint8), None):
        with pytest.raises(ValueError, match="images"):
            inv.invert_frames(images, "")
    image, depth = torch.zeros(2, 8, 8, 3), torch.zeros(2, 8, 8, 3)
    ok = dict(image=image, depth_map=depth, scale_factor=8.0, direction="uni", deblur=False, num_inference_steps=5, guidance_scale=3.0,
              model=model, invert_frames=lambda u8: None)
    for kw in (dict(image=image[0]), dict(depth_map=depth[:1]), dict(direction="left"), dict(invert_frames=None), dict(frames_per_batch=0),
               dict(frames_per_batch=2.0), dict(num_inference_steps=0), dict(noise=torch.zeros(3, 4, 64, 64)), dict(image=torch.zeros(0, 8, 8, 3),
                                                                                                                depth_map=torch.zeros(0, 8, 8, 3))):
        with pytest.raises(ValueError):
            sdn.generate_stereo_standard_frames(**dict(ok, **kw))


def test_the_fixture_frames_stop_apart_on_the_float64_restatement():
    """The condition on the inputs of the GPU test, checked where the fixture was made: on the float64 restatement the three frames
    take the recorded numbers of inner steps -- in one outer step two different numbers, one of them the last -- and no loss lies
    closer to its threshold than the recorded margin, which is a thousand float32 roundings of a loss."""
    with open(os.path.join(ROOT, "tests", "golden", "inversion_frames.json")) as f:
        meta = json.load(f)
    model = nm.NullModel(meta["form"], "cpu", torch.float64)
    model.scheduler.set_timesteps(meta["steps"])
    tok = model.tokenizer
    ctx = torch.cat([model.text_encoder(tok([p]).input_ids)[0] for p in ("", meta["prompt"])])
    counts, margin = [], np.inf
    for seed in meta["seeds"]:
        image = torch.from_numpy(nm.seeded_image(seed)).double() / 127.5 - 1
        latent = model.vae.encode(image.permute(2, 0, 1)[None])["latent_dist"].mean * 0.18215
        ddim = io_.ddim_loop(model, latent, ctx[1:], meta["steps"])
        _, losses = io_.null_optimization(model, ddim, ctx, meta["steps"], meta["guidance"], meta["inner"], meta["epsilon"])
        counts.append([len(row) for row in losses])
        margin = min(margin, io_.margins(losses, meta["epsilon"]))
    per_step = [list(row) for row in zip(*counts)]
    assert per_step == meta["inner_steps"]
    assert any(len(set(row)) >= 2 and max(row) == meta["inner"] for row in per_step)
    assert margin >= meta["margin"] >= 1000 * 2.0 ** -24
