"""Every public function of comfystereo_amd/engine.py on arguments it must refuse: which exception, which message
(tests/golden/engine_refusals_cpu.json, tests/golden/engine_refusals_gpu.json, tests/test_engine_refusals.py).

    python tools/engine_refusals.py --device cpu  > tests/golden/engine_refusals_cpu.json
    python tools/engine_refusals.py --device cuda > tests/golden/engine_refusals_gpu.json      (on the MI355X)

From a fixed seed every function gets its single faults -- a wrong type, wrong dims, a wrong dtype, mixed dtypes, a non-contiguous
tensor, an empty one, mismatched shapes, requires_grad, unknown op / mode / padding strings, non-finite scalars, a `step` of the wrong
type, an `out` / `f32_out` of the wrong shape, dtype or stride, a host tensor among device tensors -- and random pairs of them.  With
--device cpu all tensors are host tensors, so the wrappers that look at the device first refuse there; with --device cuda the
tensors live on the GPU and the checks behind the device check are reached.

Nothing is ever launched: while the cases run, the library is replaced by a guard that answers the host-only queries (sizes,
limits, cs_output_shape) and raises `Accepted` from any other entry point.  A case that reaches one, or returns, was not refused:
the tool fails.  The refusals engine.py raised as `assert` until its argument checks were single-sourced are stored as the
ValueError they are now (FORMER_ASSERTS); a library from before that records AssertionError and --former-asserts rewrites the rows.

The functions of LATER -- the wrappers of the loops between model calls, which came after that -- were recorded from the engine as
it was before their own checks were single-sourced, and appended: the rows of the functions before them are the first recording's.
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from comfystereo_amd import _native, engine   # noqa: E402

PER_FUNCTION = 110     # single faults, then pairs until this many (fewer where a function has too few faults to pair)
MIN_PER_FUNCTION, MIN_TOTAL = 40, 3000
HOST_ONLY = ("cs_version", "cs_last_error", "cs_output_shape", "cs_workspace_bytes", "cs_stereo_attention_max_head_dim")
FORMER_ASSERTS = {
    "expand_u8": "codes must be uint8",
    "apply_stereo_divergence": "image_u8 must be uint8",
    "forward_warp": "image must have 3 channels ([B,3,H,W])",
    "forward_warp_mesh": "image must have 3 channels ([B,3,H,W])",
    "stereo_shift": "depthmaps must be [B,H,W] like input_images [B,C,H,W]",
}
LATER = ("inpaint_image_prep", "inpaint_latent_init", "plms_step", "standard_step")


class CorpusError(Exception):
    """A case was not refused, or the corpus is smaller than MIN_PER_FUNCTION / MIN_TOTAL."""


class Accepted(Exception):
    """An entry point that launches was reached: the arguments were not refused."""


class _Guard:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name in HOST_ONLY or name.endswith(("_workspace_bytes", "_workspace_bytes_for")):
            return getattr(self._real, name)

        def reached(*args):
            raise Accepted(name)
        return reached


# ---- faults: (id, function that spoils the keyword arguments of a good call) ----------------------------------------------------
JUNK = (("None", None), ("ndarray", np.zeros((2, 3), np.float32)), ("list", [1.0, 2.0]), ("int", 3), ("str", "tensor"),
        ("tuple", (1, 2)), ("float", 0.5), ("dict", {"a": 1}))
DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "i64": torch.int64,
          "i32": torch.int32, "i16": torch.int16, "i8": torch.int8, "u8": torch.uint8, "bool": torch.bool, "c64": torch.complex64}


def _set(arg, name, value):
    return (f"{arg}={name}", lambda kw: kw.__setitem__(arg, value))


def _map(arg, name, f):
    return (f"{arg}:{name}", lambda kw: kw.__setitem__(arg, f(kw[arg])))


def junk(arg, skip=()):
    return [_set(arg, n, v) for n, v in JUNK if n not in skip]


def values(arg, *vals):
    return [_set(arg, repr(v), v) for v in vals]


def cast(arg, *names):
    return [_map(arg, n, lambda t, n=n: t.to(DTYPES[n])) for n in names]


def fewer(arg):
    return [_map(arg, "fewer-dims", lambda t: t[0])]


def more(arg):
    return [_map(arg, "more-dims", lambda t: t[None])]


def strided(arg):
    return [_map(arg, "strided", lambda t: t.new_zeros(tuple(t.shape) + (2,))[..., 0])]


def resize(arg, axis, by=1):
    def f(t):
        shape = list(t.shape)
        shape[axis] = shape[axis] + by if by else 0
        return t.new_zeros(shape)
    return [_map(arg, f"axis{axis}{'+' + str(by) if by else '=0'}", f)]


def grad(arg):
    return [_map(arg, "requires-grad", lambda t: t.detach().clone().requires_grad_(True))]


def host(dev, *args):
    return [_map(a, "host", lambda t: t.cpu()) for a in args] if dev != "cpu" else []


BAD_FLOATS = ("abc", None, [1.0])


def scalars(*args, bad=BAD_FLOATS):
    return [a for arg in args for a in values(arg, *bad)]


# ---- the functions: a good call at the smallest shapes, and the faults each refuses -------------------------------------------
def _z(dev, *shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=dev)


PARAMS = dict(n=1, h=16, w=64, depth_h=16, depth_w=64, depth_c=3, fill="polylines_soft", mode="left-right", divergence=6.0,
              separation=0.3, stereo_balance=0.1, convergence_point=0.5, stereo_offset_exponent=2.0, depth_map_blur=True,
              depth_blur_strength=20.0, depth_blur_edge_threshold=20.0, depth_blur_falloff=2.0, depth_blur_vert_smooth=6, batch_size=12)
PARAM_FLOATS = ("divergence", "separation", "stereo_balance", "convergence_point", "stereo_offset_exponent", "depth_blur_strength",
                "depth_blur_edge_threshold", "depth_blur_falloff")
BAD_MODES = ("sideways", "", None, 3, "Left-Right", ["left-right"])
BAD_MODE_CODES = tuple(range(8, 30)) + tuple(range(-1, -11, -1))


def _params(**over):
    p = engine.make_params(**PARAMS)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _param_faults(key="p"):
    return [(f"{key}.mode={m}", lambda kw, m=m: kw.__setitem__(key, _params(mode=m))) for m in BAD_MODE_CODES]


def _attn(dev, dtype=torch.float32, grads=False):
    kw = dict(q=_z(dev, 4, 8, 40, dtype=dtype), k=_z(dev, 4, 9, 40, dtype=dtype), v=_z(dev, 4, 9, 40, dtype=dtype), heads=2, scale=0.1)
    if grads:
        kw.update(out=_z(dev, 2, 8, 80, dtype=dtype), lse=_z(dev, 4, 8), d_out=_z(dev, 2, 8, 80, dtype=dtype))
    return kw


def _qkv(dev, d, dtype=torch.float32):
    return dict(q=_z(dev, 4, 8, d, dtype=dtype), k=_z(dev, 4, 9, d, dtype=dtype), v=_z(dev, 4, 9, d, dtype=dtype))


def _attn_faults(dev, names=("q", "k", "v"), types=True):
    f = [a for n in names for a in (junk(n) if types else []) + cast(n, "f64", "i32", "f16", "bf16") + fewer(n) + more(n)
         + strided(n) + resize(n, 0) + resize(n, 2, 4) + resize(n, 1, 0)]
    f += values("heads", 0, -2, 3, "two", None) + values("scale", float("nan"), float("inf"), "abc", None)
    f += [("d=44:half", lambda kw: kw.update(_qkv(dev, 44, torch.float16))), ("d=42", lambda kw: kw.update(_qkv(dev, 42))),
          ("d=164", lambda kw: kw.update(_qkv(dev, 164)))]
    return f + host(dev, *names)


def _flat(dev, *names):
    return {n: _z(dev, 1, 4, 8, 8) for n in names}


def _flat_faults(dev, names, none_ok=()):
    f = []
    for n in names:
        f += junk(n, skip=("None",) if n in none_ok else ()) + cast(n, "f64", "i32", "f16", "bf16") + fewer(n) + strided(n) + resize(n, 3)
    f += resize(names[0], 0, 0)
    f += values("guidance", float("nan"), "abc", None)
    f += values("coeffs", (0.6, 0.8, 0.5), (0.6, 0.0, 0.5, 0.9), (0.6, float("inf"), 0.5, 0.9), 3.0, None, (0.6, 0.8, 0.5, 0.9, 1.0))
    return f + host(dev, *names)


COEFFS = (0.6, 0.8, 0.5, 0.86)


def _functions(dev):
    """name -> (call(**kw), good kw factory, faults)"""
    F = {}
    F["make_params"] = (engine.make_params, lambda: dict(PARAMS),
                        values("mode", *BAD_MODES) + values("fill", "fancy", None, 7)
                        + scalars("n", "h", "w", "depth_h", "depth_w", "depth_c", bad=("a", 1.5, None))
                        + scalars(*PARAM_FLOATS) + scalars("batch_size", "depth_blur_vert_smooth", bad=("x", None)))
    F["output_shape"] = (engine.output_shape, lambda: dict(p=_params()), junk("p") + _param_faults())
    F["Plan"] = (engine.Plan, lambda: dict(p=_params(), device=dev, stereo_u8=False, tie_pool_bytes=0),
                 junk("p") + _param_faults() + values("tie_pool_bytes", "x", None, [1])
                 + [("p.n=-1", lambda kw: kw.__setitem__("p", _params(n=-1))), ("p.h=-1", lambda kw: kw.__setitem__("p", _params(h=-1)))])
    F["Plan.run"] = (lambda **kw: engine.Plan(_params(), dev).run(**kw),
                     lambda: dict(image=_z(dev, 1, 16, 64, 3), depth=_z(dev, 1, 16, 64, 3)), junk("image") + junk("depth"))
    F["expand_u8"] = (engine.expand_u8, lambda: dict(codes=_z(dev, 1024, dtype=torch.uint8)),
                      junk("codes") + cast("codes", *(n for n in DTYPES if n != "u8")) + host(dev, "codes") + values("codes", b"bytes", 1 + 2j, True, {1, 2}, range(3), Ellipsis)
                      + [(f"codes:{n}{s}", lambda kw, n=n, s=s: kw.__setitem__("codes", _z(dev, *s, dtype=DTYPES[n])))
                         for n in ("f32", "i32", "bool", "f16", "i8", "f64", "i64") for s in ((4, 4), (2, 3, 5), (7,))])
    F["generate"] = (engine.generate,
                     lambda: dict(image=_z(dev, 1, 16, 64, 3), depth_map=_z(dev, 1, 16, 64, 3), divergence=6.0, separation=0.3,
                                  modes="left-right", stereo_balance=0.1, convergence_point=0.5, stereo_offset_exponent=2.0,
                                  fill="polylines_soft", depth_blur_edge_threshold=20.0, depth_blur_strength=20.0, depth_map_blur=True),
                     junk("image") + junk("depth_map") + fewer("image") + more("image") + resize("image", 3) + fewer("depth_map")
                     + values("modes", *BAD_MODES) + values("fill", "fancy", None, 7) + host(dev, "image", "depth_map")
                     + scalars("divergence", "separation", "stereo_balance", "convergence_point", "stereo_offset_exponent",
                               "depth_blur_edge_threshold", "depth_blur_strength"))
    F["apply_stereo_divergence"] = (
        engine.apply_stereo_divergence,
        lambda: dict(image_u8=_z(dev, 1, 16, 64, 3, dtype=torch.uint8), depth=_z(dev, 1, 16, 64), divergence=6.0, separation=0.3,
                     stereo_offset_exponent=2.0, fill="polylines_soft", convergence_point=0.5, dialect="D32"),
        junk("image_u8") + junk("depth") + cast("image_u8", "f32", "i32", "bool", "f16", "i8") + more("image_u8")
        + [_map("image_u8", "2-dims", lambda t: t[0, 0])] + values("fill", "fancy", None, 7) + values("dialect", "D16", None, 3)
        + scalars("divergence", "separation", "stereo_offset_exponent", "convergence_point") + host(dev, "image_u8", "depth"))
    blur = dict(depth=None, blur_strength=20.0, edge_threshold=20.0, falloff_exponent=2.0, vert_smooth_px=6)
    blur_faults = (junk("depth") + [_map("depth", "1-dim", lambda t: t[0, 0]), _map("depth", "0-dim", lambda t: t[0, 0, 0])]
                   + resize("depth", 2, 0) + scalars("blur_strength", "edge_threshold", "falloff_exponent")
                   + values("vert_smooth_px", "x", None, [1]) + host(dev, "depth"))
    F["directional_blur"] = (engine.directional_blur, lambda: dict(blur, depth=_z(dev, 2, 32, 64), blur_mask_width=None),
                             blur_faults + values("blur_mask_width", "abc", [1.0]))
    F["directional_blur_scipy"] = (engine.directional_blur_scipy, lambda: dict(blur, depth=_z(dev, 2, 32, 64), blur_mask_width=5),
                                   blur_faults + values("blur_mask_width", "abc", None, [1.0]))
    warp = dict(divergence_px=4.0, separation_px=0.5, stereo_offset_exponent=1.0, convergence_point=0.5, gradient_threshold=1.5)
    warp_faults = (junk("image") + junk("depth") + fewer("image") + more("image") + resize("image", 1) + resize("image", 1, -2)
                   + scalars(*warp) + host(dev, "image", "depth"))
    F["forward_warp"] = (engine.forward_warp, lambda: dict(warp, image=_z(dev, 1, 3, 16, 64), depth=_z(dev, 1, 16, 64), max_stretch=8),
                         warp_faults + values("max_stretch", "x", None, [1]))
    F["forward_warp_mesh"] = (engine.forward_warp_mesh, lambda: dict(warp, image=_z(dev, 1, 3, 16, 64), depth=_z(dev, 1, 16, 64)),
                              warp_faults)
    F["stereo_shift"] = (engine.stereo_shift,
                         lambda: dict(input_images=_z(dev, 1, 4, 16, 64), depthmaps=_z(dev, 1, 16, 64), scale_factor=8.0, shift_both=False,
                                      stereo_offset_exponent=1.0),
                         junk("input_images") + junk("depthmaps") + fewer("input_images") + more("input_images") + fewer("depthmaps")
                         + more("depthmaps") + resize("depthmaps", 0) + resize("depthmaps", 1) + resize("depthmaps", 2, -1)
                         + resize("input_images", 3) + scalars("scale_factor", "stereo_offset_exponent")
                         + host(dev, "input_images", "depthmaps"))
    shapes = ((5,), (2, 3), (2, 3, 4), (1, 1, 2, 2))
    lone = lambda arg: junk(arg) + ([(f"{arg}:host-{n}{s}", lambda kw, n=n, s=s: kw.__setitem__(arg, torch.zeros(*s, dtype=DTYPES[n])))  # noqa: E731
                                     for n in ("f32", "f64", "f16", "i32", "u8", "i64", "bf16", "bool") for s in shapes]
                                    + values(arg, b"bytes", 1 + 2j, True, {1, 2}, range(3), Ellipsis, np.float32(1.0), np.zeros(3)))
    F["test_powf"] = (engine.test_powf, lambda: dict(x=_z(dev, 8), y=2.0), lone("x") + scalars("y"))
    F["test_exp"] = (engine.test_exp, lambda: dict(x=_z(dev, 8)), lone("x"))
    grid = dict(divergence_px=4.0, separation_px=0.5, stereo_offset_exponent=1.0, convergence_point=0.5)
    F["grid_warp"] = (engine.grid_warp, lambda: dict(grid, image=_z(dev, 1, 3, 8, 16), depth=_z(dev, 1, 8, 16), op="warp", padding="border"),
                      values("op", "bend", None, 0) + values("padding", "mirror", None, 0) + junk("image") + junk("depth")
                      + cast("image", "bool", "c64") + cast("depth", "bool", "c64") + fewer("image") + more("image") + fewer("depth")
                      + more("depth") + resize("image", 0) + resize("image", 3) + resize("image", 1, 0) + resize("depth", 1, 0)
                      + [("empty", lambda kw: kw.update(image=_z(dev, 1, 3, 0, 16), depth=_z(dev, 1, 0, 16)))]
                      + scalars(*grid) + host(dev, "image", "depth"))
    F["interpolate_fill"] = (engine.interpolate_fill, lambda: dict(image=_z(dev, 1, 3, 8, 16), mask=_z(dev, 1, 8, 16, dtype=torch.bool)),
                             junk("image") + junk("mask") + cast("image", "bool", "c64") + cast("mask", "u8", "f32", "i32", "i64", "f16")
                             + fewer("image") + more("image") + fewer("mask") + more("mask") + resize("mask", 0) + resize("mask", 2)
                             + resize("image", 2) + host(dev, "image", "mask")
                             + [("empty", lambda kw: kw.update(image=_z(dev, 1, 3, 0, 16), mask=_z(dev, 1, 0, 16, dtype=torch.bool)))])
    dd = ("depth", "grid", "grid_x_warped")
    F["detect_disocclusions"] = (
        engine.detect_disocclusions,
        lambda: dict(depth=_z(dev, 8, 16), grid=_z(dev, 1, 8, 16, 2), grid_x_warped=_z(dev, 8, 16), threshold=0.02),
        [a for n in dd for a in junk(n) + cast(n, "bool", "c64") + fewer(n) + more(n) + resize(n, 1)] + scalars("threshold")
        + host(dev, *dd) + [("w=1", lambda kw: kw.update(depth=_z(dev, 8, 1), grid=_z(dev, 1, 8, 1, 2), grid_x_warped=_z(dev, 8, 1))),
                            ("h=0", lambda kw: kw.update(depth=_z(dev, 0, 16), grid=_z(dev, 1, 0, 16, 2), grid_x_warped=_z(dev, 0, 16)))])
    F["gaussian_taps"] = (engine.gaussian_taps, lambda: dict(sigma=1.0),
                          values("sigma", 0, 0.0, -0.0, -1, -1.5, -1e300, -1e-300, float("nan"), float("-inf"), float("inf"), "abc", "", "1.0x",
                                 None, [1.0], (1.0,), {"s": 1}, {1.0}, b"x", 1 + 2j, Ellipsis, -2, -3, -4, -5, -6, -7, -8, -0.25, -0.5, -0.75,
                                 -1e-9, -1e9, False, np.float32(-1.0), np.float64("nan"), np.int64(0), np.int32(-3), np.zeros(2), "nan", "-inf",
                                 "inf", "-3"))
    F["gaussian_blur"] = (engine.gaussian_blur, lambda: dict(depth=_z(dev, 16, 64), sigma=1.0, op="plain", edge_threshold=None),
                          values("op", "smooth", None, 0, "left", "right", "edge_selective") + junk("depth") + cast("depth", "f64", "f16", "u8", "i32")
                          + [_map("depth", "1-dim", lambda t: t[0]), _map("depth", "4-dims", lambda t: t[None, None])]
                          + resize("depth", 0, 0) + resize("depth", 1, 0) + values("sigma", "abc", None, [1.0], float("inf"))
                          + values("edge_threshold", "abc", [1.0]) + host(dev, "depth"))
    F["inpaint_prepare"] = (engine.inpaint_prepare,
                            lambda: dict(image=_z(dev, 1, 3, 8, 16), depth=_z(dev, 1, 8, 16), scale_factor=8.0, threshold=0.05, codes=False),
                            junk("image") + junk("depth") + cast("image", "bool", "c64") + cast("depth", "bool", "c64") + fewer("image")
                            + more("image") + fewer("depth") + more("depth") + resize("image", 1) + resize("image", 1, -1) + resize("image", 0)
                            + resize("depth", 2) + scalars("scale_factor", "threshold") + host(dev, "image", "depth")
                            + [("empty", lambda kw: kw.update(image=_z(dev, 1, 3, 0, 16), depth=_z(dev, 1, 0, 16)))])
    F["pil_resize"] = (engine.pil_resize,
                       lambda: dict(x=_z(dev, 1, 8, 16, 3, dtype=torch.uint8), size=(8, 4), gray=False, f32="nhwc", codes=True,
                                    f32_out=_z(dev, 1, 4, 8, 3)),
                       junk("x") + cast("x", "f64", "f16", "i32", "bool") + [_map("x", "2-dims", lambda t: t[0, 0]), _map("x", "5-dims", lambda t: t[None])]
                       + resize("x", 3) + resize("x", 3, -1) + values("f32", "nchw", 1, "planar", None)
                       + values("size", (0, 4), (8, -1), ("a", 4), (8,), (8, 4, 2), None, 8) + resize("x", 1, 0)
                       + junk("f32_out", skip=("None",)) + cast("f32_out", "f64", "f16", "u8") + fewer("f32_out") + resize("f32_out", 1)
                       + resize("f32_out", 3, -2) + strided("f32_out") + host(dev, "x", "f32_out")
                       + [_map("f32_out", "transposed", lambda t: t.new_zeros(1, 8, 4, 3).transpose(1, 2)),
                          ("gray:1-channel", lambda kw: kw.update(x=_z(dev, 1, 8, 16, 1, dtype=torch.uint8), gray=True, f32=None, f32_out=None)),
                          ("nothing-asked", lambda kw: kw.update(codes=False, f32=None, f32_out=None))])
    F["stereo_attention"] = (engine.stereo_attention, lambda: dict(_attn(dev), mode="self", chunks=1, out=None),
                             _attn_faults(dev) + [a for n in "qkv" for a in grad(n)] + values("mode", "both", None, 0)
                             + [("mode=uni:keys", lambda kw: kw.update(mode="uni")), ("mode=bi:chunks", lambda kw: kw.update(
                                 mode="bi", chunks=3, k=_z(dev, 4, 8, 40), v=_z(dev, 4, 8, 40)))]
                             + [(f"out:{n}", lambda kw, f=f: kw.__setitem__("out", f(_z(dev, 2, 8, 80))))
                                for n, f in (("f64", lambda t: t.double()), ("f16", lambda t: t.half()), ("shape", lambda t: t[:, :4]),
                                             ("strided", lambda t: t.new_zeros(2, 8, 80, 2)[..., 0]), ("ndarray", lambda t: np.zeros((2, 8, 80))),
                                             ("list", lambda t: [0.0]), ("dims", lambda t: t[0]))]
                             + ([("out:host", lambda kw: kw.__setitem__("out", torch.zeros(2, 8, 80)))] if dev != "cpu" else []))
    F["attention_lse"] = (engine.attention_lse, lambda: _attn(dev), _attn_faults(dev))
    grads = ("out", "lse", "d_out")
    F["attention_backward"] = (engine.attention_backward, lambda: _attn(dev, grads=True),
                               _attn_faults(dev) + [a for n in grads for a in junk(n) + cast(n, "f64", "f16") + fewer(n) + strided(n)
                                                    + resize(n, 1)] + host(dev, *grads))
    F["differentiable_attention"] = (engine.differentiable_attention, lambda: dict(_attn(dev), native_half=False),
                                     [a for a in _attn_faults(dev) if not a[0].endswith((":f16", ":bf16", ":strided", ":half"))]
                                     + [("native_half:d=164", lambda kw: kw.update(_qkv(dev, 164, torch.float16), native_half=True)),
                                        ("native_half:d=168", lambda kw: kw.update(_qkv(dev, 168, torch.bfloat16), native_half=True))])
    F["latent_shift_plan"] = (engine.latent_shift_plan, lambda: dict(disp=_z(dev, 1, 8, 8), scale_factor=8.0, stereo_offset_exponent=1.0),
                              junk("disp") + cast("disp", "f64", "f16", "i32", "bf16", "u8") + fewer("disp") + more("disp") + strided("disp")
                              + resize("disp", 0, 0) + resize("disp", 1, 0) + resize("disp", 2, 8185)
                              + values("scale_factor", float("nan"), float("inf"), "abc", None)
                              + values("stereo_offset_exponent", float("nan"), float("-inf"), "abc", None) + host(dev, "disp"))
    lat = ("left", "right", "noise")
    F["latent_shift_apply"] = (
        engine.latent_shift_apply,
        lambda: dict(left=_z(dev, 1, 4, 8, 8), right=_z(dev, 1, 4, 8, 8), src_col=_z(dev, 1, 8, 8, dtype=torch.int32),
                     mask=_z(dev, 1, 8, 8, dtype=torch.uint8), op="first", noise=_z(dev, 1, 4, 8, 8)),
        values("op", "again", None, 0, "reshift") + [a for n in lat for a in junk(n, skip=("None",) if n == "noise" else ()) + cast(n, "f64", "i32", "f16", "bf16")
                                                     + fewer(n) + strided(n) + resize(n, 1) + grad(n)]
        + resize("left", 2, 0) + [a for n in ("src_col", "mask") for a in junk(n) + cast(n, "i64", "f32", "bool") + fewer(n) + strided(n)
                                  + resize(n, 2)] + host(dev, *lat, "src_col", "mask"))
    F["decode_to_codes"] = (engine.decode_to_codes, lambda: dict(image=_z(dev, 1, 3, 8, 8)),
                            junk("image") + cast("image", *(n for n in DTYPES if n not in ("f32", "f16", "bf16")))
                            + fewer("image") + more("image") + strided("image") + [_map("image", "2-dims", lambda t: t[0, 0])]
                            + [a for ax in range(4) for a in resize("image", ax, 0)] + host(dev, "image")
                            + [(f"image:{n}-{what}", lambda kw, n=n, f=f: kw.__setitem__("image", f(_z(dev, 1, 3, 8, 8, dtype=DTYPES[n]))))
                               for n in ("f16", "bf16", "f64", "i32") for what, f in (("fewer-dims", lambda t: t[0]), ("more-dims", lambda t: t[None]),
                                                                                     ("strided", lambda t: t.new_zeros(1, 3, 8, 8, 2)[..., 0]),
                                                                                     ("empty", lambda t: t.new_zeros(1, 3, 0, 8)))])
    step = ("sample", "eps_a", "eps_b", "out")
    F["ddim_step"] = (engine.ddim_step, lambda: dict(_flat(dev, *step), guidance=3.0, coeffs=COEFFS),
                      _flat_faults(dev, step, none_ok=("eps_b", "out")) + [a for n in step for a in grad(n)])
    null = ("eps_uncond", "eps_cond", "latent_cur", "latent_prev")
    F["null_loss_grad"] = (engine.null_loss_grad, lambda: dict(_flat(dev, *null), guidance=3.0, coeffs=COEFFS), _flat_faults(dev, null))
    F["NullTextLoss"] = (lambda **kw: engine.NullTextLoss.apply(*(kw[n] for n in null + ("guidance", "coeffs"))),
                         lambda: dict(_flat(dev, *null), guidance=3.0, coeffs=COEFFS), _flat_faults(dev, null))
    adam = ("param", "grad", "exp_avg", "exp_avg_sq")
    F["adam_step"] = (engine.adam_step, lambda: dict(_flat(dev, *adam), lr=0.01, step=1, beta1=0.9, beta2=0.999, eps=1e-8),
                      [a for a in _flat_faults(dev, adam) if not a[0].startswith(("guidance", "coeffs"))]
                      + values("step", 0, -1, 1.0, True, "1", None) + values("lr", float("nan"), float("inf"), "abc", None)
                      + values("eps", -1e-8, float("nan"), "abc") + values("beta1", 1.0, -0.1, float("nan"), "abc")
                      + values("beta2", 1.0, 1.5, None) + [a for n in adam[1:] for a in grad(n)])
    F.update(_loop_functions(dev))
    return F


def _each(names, *kinds):
    return [a for n in names for kind in kinds for a in kind(n)]


def twice(arg, first, second):
    """One tensor spoilt in two ways: which fault is reported is the order of its checks."""
    (ia, fa), (ib, fb) = first(arg)[0], second(arg)[0]
    return [(f"{ia} & {ib.split(':', 1)[1]}", lambda kw: (fa(kw), fb(kw)))]


def _orders(names, dtype="f16"):
    """dtype before shape before stride, for every tensor of `names`"""
    to, grow = (lambda n: cast(n, dtype)), (lambda n: resize(n, -1))
    return [a for n in names for a in twice(n, to, grow) + twice(n, grow, strided) + twice(n, to, strided)]


def _loop_functions(dev):
    """The wrappers of the loops between model calls (LATER): Fast mode's three and Standard mode's fused step."""
    F = {}
    u8 = dict(dtype=torch.uint8)
    few = lambda n, skip=(): junk(n, skip=("list", "tuple", "float", "dict") + skip)   # noqa: E731  (room for pairs of faults)
    lat = lambda *lead: _z(dev, *lead, 2, 4)   # noqa: E731
    sizes = values("latent_size", (0, 4), (2, -1), (3, 4), ("a", 4), (2,), (2, 4, 1), None, 3)
    prep = ("filled_u8", "mask", "x")
    F["inpaint_image_prep"] = (
        engine.inpaint_image_prep,
        lambda: dict(filled_u8=_z(dev, 1, 8, 16, 3, **u8), mask=_z(dev, 1, 8, 16, **u8), x=lat(2, 9), latent_size=(2, 4)),
        _each(prep, few, fewer, more, strided) + cast("filled_u8", "f32", "i32", "bool", "f16") + cast("mask", "f32", "i32", "f16", "i64")
        + cast("x", "f64", "i32", "u8") + resize("filled_u8", 3) + resize("filled_u8", 1, 0) + resize("mask", 1) + resize("x", 0)
        + resize("x", 1) + resize("x", 3) + grad("x") + sizes + _orders(("x",), "f64") + host(dev, *prep))
    opt = ("noise", "img_latent", "decode_in")
    F["inpaint_latent_init"] = (
        engine.inpaint_latent_init,
        lambda: dict(mean_img=lat(1, 4), mean_masked=lat(1, 4), noise=lat(1, 4), coeffs=(0.8, 0.6), x=lat(2, 9), img_latent=lat(1, 4),
                     decode_in=lat(1, 4)),
        _each(("mean_img", "mean_masked", "x"), few, fewer, more, strided) + _each(opt, lambda n: few(n, ("None",)), fewer, more, strided, grad)
        + cast("mean_img", "f64", "i32") + cast("mean_masked", "f64", "i32", "f16", "bf16") + cast("x", "f64", "i32", "f16")
        + _each(opt, lambda n: cast(n, "f64", "f16", "bf16")) + resize("mean_img", 1) + resize("mean_img", 2, 0) + resize("mean_masked", 3)
        + resize("x", 0) + resize("x", 3) + resize("noise", 2) + resize("img_latent", 0) + resize("decode_in", 3) + grad("x")
        + _orders(opt) + _orders(("mean_masked",))
        + values("coeffs", (0.8,), (0.8, 0.6, 0.1), (float("nan"), 0.6), (0.8, float("inf")), ("a", 0.6), (None, 0.6), None, 3.0)
        + host(dev, "mean_img", "mean_masked", "x", *opt))
    first = lambda f: lambda hist: (f(hist[0]),)   # noqa: E731
    outs = ("e_out", "decode_in")
    F["plms_step"] = (
        engine.plms_step,
        lambda: dict(noise_pred=lat(2, 4), x=lat(2, 9), kind="order2", guidance=3.0, coeffs=(1.0, 0.5, 0.9), e_out=lat(1, 4),
                     history=(lat(1, 4),), cur_sample=None, decode_in=lat(1, 4)),
        values("kind", "third", None, 0, "first", "second", "order4")
        + _each(("noise_pred", "x") + outs, fewer, more, strided, grad) + _each(("noise_pred", "x", "e_out"), few)
        + few("cur_sample", ("None",)) + few("decode_in", ("None",)) + [_set("cur_sample", "f16-tensor", lat(1, 4).half())]
        + _each(("noise_pred", "x"), lambda n: cast(n, "f64", "i32", "f16", "bf16")) + _each(outs, lambda n: cast(n, "f64", "f16", "bf16"))
        + resize("noise_pred", 0) + resize("noise_pred", 1) + resize("noise_pred", 2, 0) + resize("x", 1) + resize("x", 3)
        + resize("e_out", 0) + resize("decode_in", 3) + _orders(outs)
        + [_set("history", "none", ()), _set("history", "two", (lat(1, 4), lat(1, 4))), _set("history", "None", None),
           _set("history", "int", 3), _set("history", "junk", ("a",)), _set("history", "[None]", (None,)),
           _map("history", "f16", first(lambda t: t.half())), _map("history", "shape", first(lambda t: t[:, :3])),
           _map("history", "strided", first(lambda t: t.new_zeros(1, 4, 2, 4, 2)[..., 0])),
           _map("history", "requires-grad", first(lambda t: t.clone().requires_grad_(True)))]
        + [("kind=first:history", lambda kw: kw.update(kind="first", history=())),
           ("kind=second:no-e_out", lambda kw: kw.update(kind="second", e_out=None)),
           ("kind=order4:history", lambda kw: kw.update(kind="order4", history=(lat(1, 4), lat(1, 4))))]
        + values("guidance", float("nan"), float("inf"), "abc", None)
        + values("coeffs", (1.0, 0.5), (1.0, 0.5, 0.9, 0.1), (1.0, 0.5, 0.0), (float("nan"), 0.5, 0.9), (1.0, 0.5, float("inf")),
                 ("a", 0.5, 0.9), None, 3.0)
        + host(dev, "noise_pred", "x", *outs) + ([_map("history", "host", first(lambda t: t.cpu()))] if dev != "cpu" else []))
    big = ("x", "noise_pred", "noise")
    wide = lambda *lead, **kw: _z(dev, *lead, 2, 8193, **kw)   # noqa: E731
    F["standard_step"] = (
        engine.standard_step,
        lambda: dict(noise_pred=_z(dev, 4, 4, 2, 8), x=_z(dev, 4, 4, 2, 8), guidance=3.0, coeffs=COEFFS, op="first",
                     src_col=_z(dev, 1, 2, 8, dtype=torch.int32), mask=_z(dev, 1, 2, 8, **u8), noise=_z(dev, 1, 4, 2, 8)),
        values("op", "again", None, 0, "reshift", "none") + _each(("x", "noise_pred", "src_col", "mask"), few)
        + few("noise", ("None",)) + _each(big + ("src_col", "mask"), fewer, more, strided) + _each(big, grad)
        + _each(("x", "noise_pred"), lambda n: cast(n, "f64", "i32", "f16", "bf16")) + cast("noise", "f64", "f16", "bf16")
        + cast("src_col", "i64", "f32", "i16", "bool") + cast("mask", "bool", "f32", "i32", "i64")
        + resize("x", 0) + resize("x", 1, 0) + resize("noise_pred", 3) + resize("noise", 1) + resize("src_col", 2) + resize("mask", 1)
        + _orders(("noise_pred", "noise")) + _orders(("src_col",), "i64") + _orders(("mask",), "bool")
        + [("w=8193", lambda kw: kw.update(noise_pred=wide(4, 4), x=wide(4, 4), noise=wide(1, 4), src_col=wide(1, dtype=torch.int32),
                                           mask=wide(1, **u8)))]
        + values("guidance", float("nan"), "abc", None)
        + values("coeffs", (0.6, 0.8, 0.5), (0.6, 0.0, 0.5, 0.9), (0.6, float("inf"), 0.5, 0.9), 3.0, None, (0.6, 0.8, 0.5, 0.9, 1.0))
        + host(dev, *big, "src_col", "mask"))
    return F


def _arg_of(fault_id):
    return fault_id.replace(":", "=").split("=")[0].split(".")[0]


def cases(dev):
    """[(function, case id, call, good kw factory, [faults])] in a fixed order: every single fault, then seeded pairs."""
    out = []
    for fn, (call, good, faults) in _functions(dev).items():
        ids = [f[0] for f in faults]
        assert len(set(ids)) == len(ids), (fn, sorted(i for i in ids if ids.count(i) > 1))
        picked = [(f,) for f in faults]
        rng = random.Random("engine_refusals/" + fn)
        pairs = [(a, b) for i, a in enumerate(faults) for b in faults[i + 1:] if _arg_of(a[0]) != _arg_of(b[0])]
        rng.shuffle(pairs)
        picked += pairs[: max(0, PER_FUNCTION - len(picked))]
        out += [(fn, " + ".join(f[0] for f in fs), call, good, fs) for fs in picked]
    return out


def run(dev):
    """[[function, case id, exception type, message]]; CorpusError if a case is not refused."""
    rows, accepted = [], []
    real = _native.lib
    guard = _Guard(real())
    _native.lib = lambda: guard
    try:
        for fn, cid, call, good, faults in cases(dev):
            kw = good()
            for _, spoil in faults:
                spoil(kw)
            try:
                call(**kw)
            except Accepted as e:
                accepted.append((fn, cid, f"reached {e}"))
            except Exception as e:   # noqa: BLE001  (the refusal, whatever its type: that is what is recorded)
                rows.append([fn, cid, type(e).__name__, str(e)])
            else:
                accepted.append((fn, cid, "returned"))
    finally:
        _native.lib = real
    if accepted:
        raise CorpusError("not refused:\n" + "\n".join(f"  {fn}: {cid} ({how})" for fn, cid, how in accepted))
    count = {}
    for row in rows:
        count[row[0]] = count.get(row[0], 0) + 1
    short = {fn: n for fn, n in count.items() if n < MIN_PER_FUNCTION}
    if short or len(rows) < MIN_TOTAL:
        raise CorpusError(f"corpus too small: {len(rows)} cases, short functions {short}")
    return rows


def store_former_asserts(rows):
    """The five refusals that were `assert`s: AssertionError rows become the ValueError the engine raises now."""
    for row in rows:
        if row[2] == "AssertionError":
            row[2], row[3] = "ValueError", FORMER_ASSERTS[row[0]]
    return rows


def dump(rows, device, out):
    """The corpus as JSON, compact: every distinct (exception type, message) once in "outcomes", and per function one line of
    [case id, index into outcomes]."""
    outcomes, by_function = [], {}
    for fn, cid, kind, msg in rows:
        if [kind, msg] not in outcomes:
            outcomes.append([kind, msg])
        by_function.setdefault(fn, []).append([cid, outcomes.index([kind, msg])])
    comment = "Recorded before the argument checks of engine.py were single-sourced."
    if any(kind == "ValueError" and msg == FORMER_ASSERTS.get(fn) for fn, _, kind, msg in rows):
        comment += ("  The rows of " + ", ".join(FORMER_ASSERTS) + " with the messages of tools/engine_refusals.py FORMER_ASSERTS"
                    " were AssertionError (no message) then: stored as ValueError.")
    if any(fn in LATER for fn, _, _, _ in rows):
        comment += ("  The rows of " + ", ".join(LATER) + " were appended later, recorded before the checks of the latent-loop"
                    " wrappers were single-sourced.")
    enc = lambda v: json.dumps(v, separators=(",", ":"), ensure_ascii=True)   # noqa: E731
    out.write('{"comment":%s,\n"device":%s,\n"outcomes":%s,\n"cases":{\n' % (enc(comment), enc(device), enc(outcomes)))
    out.write(",\n".join(f"{enc(fn)}:{enc(cases_)}" for fn, cases_ in by_function.items()) + "\n}}\n")


def load(path):
    """The rows [[function, case id, exception type, message]] of a file that dump() wrote -> (device, rows)"""
    with open(path) as f:
        golden = json.load(f)
    return golden["device"], [[fn, cid] + golden["outcomes"][i] for fn, cases_ in golden["cases"].items() for cid, i in cases_]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda"])
    ap.add_argument("--former-asserts", action="store_true", help="store AssertionError rows as today's ValueError (FORMER_ASSERTS)")
    args = ap.parse_args()
    try:
        rows = run(args.device)
    except CorpusError as e:
        sys.exit(str(e))
    if args.former_asserts:
        rows = store_former_asserts(rows)
    dump(rows, args.device, sys.stdout)


if __name__ == "__main__":
    main()
