"""ctypes binding of libcomfystereo_hip.so (the C ABI declared in include/comfystereo_amd.h).

There is no CPU fallback: if the HIP library is missing or does not load, importing this module's
`lib()` raises.  Build it with `python __graft_entry__.py` or `make -C comfystereo_amd/csrc`.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CS_LIB_PATH: development override (A/B timing of two builds of the same library in one GPU session)
LIB_PATH = os.environ.get("CS_LIB_PATH") or os.path.join(_HERE, "libcomfystereo_hip.so")

CS_OK, CS_EINVAL, CS_EWORKSPACE, CS_ELIMIT, CS_EHIP = 0, -1, -2, -3, -4

FILL = {
    "none": 0, "naive": 1, "naive_interpolating": 2, "polylines_soft": 3, "polylines_sharp": 4, "inverse": 5,
    "hybrid_edge": 6, "gpu_warp": 7,
    # branches of the reference dispatcher no UI string reaches (stereoimage_generation.py:1605-1610)
    "none_post": 8, "inverse_post": 9, "hybrid_edge_plus": 10,
}
MODE = {
    "left-right": 0, "right-left": 1, "top-bottom": 2, "bottom-top": 3, "red-cyan-anaglyph": 4, "left-only": 5,
    "only-right": 6, "cyan-red-reverseanaglyph": 7,
}

# enum cs_grid_op / cs_grid_padding (the reference's grid-sample warps, cs_grid_warp)
GRID_OP = {"warp": 0, "fill": 1, "mask": 2, "stretch": 3}
GRID_PADDING = {"border": 0, "zeros": 1, "reflection": 2}
# enum cs_gauss_op (the reference's Gaussian depth blurs, cs_gaussian_blur)
GAUSS_OP = {"plain": 0, "edge_selective": 1, "left": 2, "right": 3}
# enum cs_pil_flags (Pillow's bicubic resize with the Fast mode's code conversions, cs_pil_resize)
PIL_FLAG = {"in_f32": 1, "gray": 2, "out_planar": 4}
# enum cs_attn_mode (the reference's stereo attention, cs_stereo_attention)
ATTN_MODE = {"self": 0, "uni": 1, "bi": 2}
# enum cs_attn_dtype (the element type of cs_stereo_attention_half, cs_attention_half_fwd_lse and cs_attention_half_bwd)
ATTN_DTYPE = {"float16": 0, "bfloat16": 1}
# enum cs_latent_dtype / cs_latent_op (StereoDiffusion Standard mode's latent shift: cs_latent_shift_apply, cs_decode_to_codes)
LATENT_DTYPE = {"float32": 0, "float16": 1, "bfloat16": 2}
LATENT_OP = {"first": 0, "reshift": 1}
# enum cs_standard_op (the shift cs_standard_step applies after its DDIM step)
STANDARD_OP = {"none": 0, "first": 1, "reshift": 2}
# enum cs_prediction (what the model's answer is: cs_ddim_step_pred, cs_null_loss_grad_pred, cs_null_loss_grad_frames_pred,
# cs_standard_step_pred)
PREDICTION = {"epsilon": 0, "v_prediction": 1}
# enum cs_plms_kind (the linear multistep combination of cs_inpaint_plms_step)
PLMS_KIND = {"first": 0, "second": 1, "order2": 2, "order3": 3, "order4": 4}
# enum cs_dilate_shape / cs_dilate_near (the foreground depth edge dilation, cs_depth_dilate)
DILATE_SHAPE = {"square": 0, "disc": 1}
DILATE_NEAR = {"bright": 0, "dark": 1}
# enum cs_fewstep_sampler (the samplers of cs_inpaint_fewstep_init / cs_inpaint_fewstep_step)
FEWSTEP_SAMPLER = {"euler": 0, "lcm": 1}

# the ABI version the ctypes signatures below were written for (include/comfystereo_amd.h CS_ABI_VERSION)
ABI_VERSION = 4

# enum cs_debug_key (development switches; tests and profiling tools only)
DEBUG = {"dbg": 0, "no_tile": 1, "pt_variant": 2, "blur_two_pass": 3, "blur_edges_scalar": 4, "blur_full_copy": 5, "chunks": 6, "no_replay_kernel": 7,
         "blur_no_pre_edges": 8, "hybrid_unfused": 9, "gpuwarp_full_maps": 10,
         "hybrid_full_maps": 11, "attn_waves": 12}

# stats word ST_WARP_PATH (Plan.stats()[:, 12]): the gpu_warp kernel instantiation that warped a frame (cs_common.h GW_PATH_*, the
# list this mirrors; 0: no gpu_warp kernel ran).  Names: kernel<MINW, POW> (POW -1: exponent at run time); "node" -- the node's
# interleaved layout compiled in, "gen" -- forward_warp_gpu's keyword parameters away from their defaults
ST_WARP_PATH = 12
WARP_PATH = {
    "q<8,2>": 1, "q<8,-1>": 2, "q<6,2>": 3, "q<6,-1>": 4,
    "k<8,2,node>": 5, "k<8,-1,node>": 6, "k<6,2,node>": 7, "k<6,-1,node>": 8,
    "k<8,2>": 9, "k<8,-1>": 10, "k<6,2>": 11, "k<6,-1>": 12,
    "k<8,gen>": 13, "k<6,gen>": 14,
    "mesh<8>": 15, "mesh<6>": 16,
}
WARP_PATH_NAME = {v: k for k, v in WARP_PATH.items()}

# the values of the development switch DEBUG["pt_variant"] (cs_common.h PTV_*, the list this mirrors, names without the prefix;
# cs_debug_set refuses any other value)
PT_VARIANT = {
    "default": 0, "first_gen": 9,
    "gw_threads_512": 21, "gw_threads_256_narrow": 22, "gw_threads_1024": 23, "gw_six_waves": 24, "gw_generic_layout": 25,
    "gw_threads_256": 26, "gw_no_quad": 27,
    "lean_whole_rows": 44, "replay_wave_only": 45, "naive_no_tier2": 47, "tiny_replay_pool": 48, "no_point_tier2": 49,
    "soft_point_tier2": 50,
}


class Params(ctypes.Structure):
    """struct cs_params (include/comfystereo_amd.h)."""
    _fields_ = [
        ("n", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
        ("depth_h", ctypes.c_int32), ("depth_w", ctypes.c_int32), ("depth_c", ctypes.c_int32),
        ("fill", ctypes.c_int32), ("mode", ctypes.c_int32), ("batch_size", ctypes.c_int32),
        ("depth_map_blur", ctypes.c_int32), ("depth_blur_vert_smooth", ctypes.c_int32), ("flags", ctypes.c_int32),
        ("divergence", ctypes.c_double), ("separation", ctypes.c_double), ("stereo_balance", ctypes.c_double),
        ("convergence_point", ctypes.c_double), ("stereo_offset_exponent", ctypes.c_double),
        ("depth_blur_strength", ctypes.c_double), ("depth_blur_edge_threshold", ctypes.c_double),
        ("depth_blur_falloff", ctypes.c_double),
    ]


class NativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"comfystereo_amd native call failed ({code}): {msg}")
        self.code = code


_vp, _int, _dbl, _size, _ll, _flt = (ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.c_longlong,
                                      ctypes.c_float)
_pp, _ip, _dp = ctypes.POINTER(Params), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
_nhw = [_int, _int, _int]
_bhnnd = [_int, _int, _int, _int, _int]   # (b, h, n, n_k, d)

# name -> (restype, argtypes) of every entry point, in the order of include/comfystereo_amd.h: lib() applies it, EXPORTS lists it
SIGNATURES = {
    # version, limits, the fused node (cs_generate)
    "cs_version": (_int, []),
    "cs_last_error": (ctypes.c_char_p, []),
    "cs_max_width": (_int, [_int]),
    "cs_max_width_mode": (_int, [_int, _int]),
    "cs_max_width_params": (_int, [_pp]),
    "cs_output_shape": (_int, [_pp, _ip, _ip, _ip, _ip]),
    "cs_workspace_bytes": (_size, [_pp]),
    "cs_generate": (_int, [_pp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _size, _vp]),
    # apply_stereo_divergence
    "cs_asd_workspace_bytes": (_size, _nhw),
    "cs_asd_workspace_bytes_for": (_size, _nhw + [_int]),
    "cs_apply_stereo_divergence": (_int, [_vp, _vp] + _nhw + [_dbl, _dbl, _dbl, _int, _dbl, _vp, _vp, _size, _vp]),
    "cs_apply_stereo_divergence2": (_int, [_vp, _vp] + _nhw + [_dbl, _dbl, _dbl, _int, _dbl, _int, _vp, _vp, _size, _vp]),
    # the directional depth blurs
    "cs_blur_workspace_bytes": (_size, _nhw),
    "cs_directional_blur": (_int, [_vp] + _nhw + [_dbl, _dbl, _dbl, _dbl, _int, _vp, _vp, _vp, _size, _vp]),
    "cs_blur_scipy_workspace_bytes": (_size, _nhw),
    "cs_directional_blur_scipy": (_int, [_vp] + _nhw + [_dbl, _dbl, _dbl, _dbl, _int, _vp, _vp, _vp, _size, _vp]),
    # forward_warp_gpu
    "cs_warp_workspace_bytes": (_size, _nhw),
    "cs_forward_warp": (_int, [_vp, _vp] + _nhw + [_dbl, _dbl, _dbl, _dbl, _vp, _vp, _vp, _size, _vp]),
    "cs_forward_warp2": (_int, [_vp, _vp] + _nhw + [_dbl, _dbl, _dbl, _dbl, _dbl, _int, _vp, _vp, _vp, _size, _vp]),
    # the grid-sample warps
    "cs_grid_warp_workspace_bytes": (_size, _nhw),
    "cs_grid_warp_max_width": (_int, [_int]),
    "cs_grid_warp": (_int, [_vp, _vp, _int] + _nhw + [_dbl, _dbl, _dbl, _dbl, _int, _int, _vp, _vp, _vp, _size, _vp]),
    "cs_interpolate_fill": (_int, [_vp, _vp, _int] + _nhw + [_vp, _vp]),
    "cs_detect_disocclusions": (_int, [_vp, _vp, _vp, _int, _int, _dbl, _vp, _vp]),
    # Fast mode: inpaint preparation, Pillow's bicubic resize
    "cs_inpaint_prepare_workspace_bytes": (_size, _nhw),
    "cs_inpaint_prepare_max_width": (_int, []),
    "cs_inpaint_prepare": (_int, [_vp, _vp] + _nhw + [_dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _size, _vp]),
    "cs_pil_resize_workspace_bytes": (_size, [_int] * 6),
    "cs_pil_resize_max_taps": (_int, []),
    "cs_pil_resize": (_int, [_vp] + [_int] * 7 + [_vp, _vp, _size, _vp, _size, _vp]),
    # the Gaussian depth blurs, the mesh warp
    "cs_gaussian_blur_workspace_bytes": (_size, _nhw + [_int]),
    "cs_gaussian_blur_max_taps": (_int, []),
    "cs_gaussian_blur": (_int, [_int, _vp, _vp, _int, _dbl] + _nhw + [_vp, _vp, _size, _vp]),
    "cs_warp_mesh_workspace_bytes": (_size, _nhw),
    "cs_forward_warp_mesh": (_int, [_vp, _vp] + _nhw + [_dbl, _dbl, _dbl, _dbl, _dbl, _vp, _vp, _vp, _size, _vp]),
    # codes and host staging
    "cs_expand_u8": (_int, [_vp, _vp, _size, _vp]),
    "cs_pack_u8": (_int, [_vp, _vp, _size, _int, _int, _vp]),
    "cs_host_expand_u8": (_int, [_vp, _vp, _size, _int, _int, _int]),
    "cs_host_copy": (_int, [_vp, _vp, _size, _int]),
    "cs_take_f32": (_int, [_vp, _vp, _size, _int, _vp]),
    "cs_host_replicate_f32": (_int, [_vp, _vp, _size, _int, _int]),
    # StereoDiffusion: stereo_shift, Standard mode's latent shift, null-text inversion
    "cs_stereo_shift_workspace_bytes": (_size, []),
    "cs_stereo_shift": (_int, [_vp, _vp, _int] + _nhw + [_dbl, _int, _dbl, _vp, _vp, _size, _vp]),
    "cs_latent_shift_plan_workspace_bytes": (_size, []),
    "cs_latent_shift_plan": (_int, [_vp] + _nhw + [_dbl, _dbl, _vp, _vp, _size, _vp]),
    "cs_latent_shift_apply": (_int, [_vp, _vp, _vp, _vp, _vp] + [_int] * 6 + [_vp]),
    "cs_decode_to_codes": (_int, [_vp] + [_int] * 5 + [_vp, _vp]),
    "cs_ddim_step": (_int, [_vp, _vp, _vp, _vp, _int, _ll] + [_dbl] * 5 + [_vp]),
    "cs_null_loss_workspace_bytes": (_size, [_ll]),
    "cs_null_loss_grad": (_int, [_vp] * 7 + [_int, _ll] + [_dbl] * 5 + [_vp, _size, _vp]),
    "cs_adam_step": (_int, [_vp, _vp, _vp, _vp, _int, _ll, _dbl, _dbl, _dbl, _dbl, _int, _vp]),
    # null-text optimisation on F frames at once: per-frame losses, stop flags on the device, an Adam that skips stopped frames
    "cs_null_loss_frames_workspace_bytes": (_size, [_ll, _ll]),
    "cs_null_loss_grad_frames": (_int, [_vp] * 9 + [_int, _ll, _ll] + [_dbl] * 6 + [_vp, _size, _vp]),
    "cs_adam_step_frames": (_int, [_vp] * 5 + [_int, _ll, _ll, _dbl, _dbl, _dbl, _dbl, _int, _vp]),
    # StereoDiffusion Fast mode's inpainting loop outside its models
    "cs_inpaint_image_prep": (_int, [_vp, _vp] + [_int] * 6 + [_vp, _vp, _vp, _vp]),
    "cs_inpaint_latent_init": (_int, [_vp, _vp, _int, _vp, _int] + _nhw + [_dbl, _dbl, _vp, _vp, _vp, _vp]),
    "cs_inpaint_plms_step": (_int, [_vp, _vp] + [_int] * 5 + [_dbl] * 4 + [_vp] * 6 + [_vp]),
    # ... and its loop for few-step models (Euler, LCM)
    "cs_inpaint_fewstep_init": (_int, [_vp, _vp, _vp] + [_int] * 7 + [_dbl, _dbl, _vp, _vp, _vp, _vp]),
    "cs_inpaint_fewstep_step": (_int, [_vp, _vp] + [_int] * 8 + [_dbl] * 7 + [_vp] * 6 + [_vp]),
    # StereoDiffusion Standard mode between two UNet calls
    "cs_standard_step": (_int, [_vp, _vp] + [_int] * 5 + [_dbl] * 5 + [_int, _vp, _vp, _vp, _vp]),
    # the same four steps with the model's prediction type (epsilon, v)
    "cs_ddim_step_pred": (_int, [_vp, _vp, _vp, _vp, _int, _ll] + [_dbl] * 5 + [_int, _vp]),
    "cs_null_loss_grad_pred": (_int, [_vp] * 7 + [_int, _ll] + [_dbl] * 5 + [_int, _vp, _size, _vp]),
    "cs_null_loss_grad_frames_pred": (_int, [_vp] * 9 + [_int, _ll, _ll] + [_dbl] * 5 + [_int, _dbl, _vp, _size, _vp]),
    "cs_standard_step_pred": (_int, [_vp, _vp] + [_int] * 5 + [_dbl] * 5 + [_int, _int, _vp, _vp, _vp, _vp]),
    # the stereo attention, its differentiable form, their float16 / bfloat16 forms
    "cs_stereo_attention_max_head_dim": (_int, []),
    "cs_stereo_attention": (_int, [_vp] * 4 + [_int] * 7 + [_dbl, _int, _vp]),
    "cs_stereo_attention_half": (_int, [_vp] * 4 + [_int] * 8 + [_dbl, _int, _vp]),
    "cs_attention_fwd_lse": (_int, [_vp] * 5 + _bhnnd + [_dbl, _vp]),
    "cs_attention_bwd_workspace_bytes": (_size, _bhnnd),
    "cs_attention_bwd": (_int, [_vp] * 9 + _bhnnd + [_dbl, _vp, _size, _vp]),
    "cs_attention_half_fwd_lse": (_int, [_vp] * 5 + [_int] + _bhnnd + [_dbl, _vp]),
    "cs_attention_half_bwd_workspace_bytes": (_size, _bhnnd),
    "cs_attention_half_bwd": (_int, [_vp] * 9 + [_int] + _bhnnd + [_dbl, _vp, _size, _vp]),
    # temporal depth stabilisation of a video batch
    "cs_temporal_depth_workspace_bytes": (_size, [_int] * 4),
    "cs_temporal_depth": (_int, [_vp] + [_int] * 4 + [_dbl] * 3 + [_vp] * 7 + [_size, _vp]),
    # motion-compensated temporal depth stabilisation of a video batch
    "cs_motion_depth_workspace_bytes": (_size, [_int] * 5),
    "cs_motion_depth": (_int, [_vp] * 2 + [_int] * 4 + [_dbl] * 3 + [_int] * 3 + [_vp] * 11 + [_size, _vp]),
    # the same with a coarse-to-fine motion search on a luma pyramid
    "cs_motion_depth_pyramid_workspace_bytes": (_size, [_int] * 5),
    "cs_motion_depth_pyramid": (_int, [_vp] * 2 + [_int] * 4 + [_dbl] * 3 + [_int] * 3 + [_vp] * 11 + [_size, _vp]),
    # depth range clipping of a video batch
    "cs_depth_range_workspace_bytes": (_size, [_int] * 4),
    "cs_depth_range": (_int, [_vp] + [_int] * 6 + [_dbl, _int] + [_vp] * 10 + [_size, _vp]),
    # image-guided depth upsampling: the plan of a geometry, made once, and the pass over a batch
    "cs_guided_depth_plan_bytes": (_size, [_int] * 5),
    "cs_guided_depth_plan": (_int, [_int] * 5 + [_dbl, _dbl, _vp, _size, _vp]),
    "cs_guided_depth_apply": (_int, [_vp, _vp] + [_int] * 7 + [_vp, _size, _vp, _vp]),
    # foreground depth edge dilation
    "cs_depth_dilate": (_int, [_vp] + [_int] * 7 + [_flt, _vp, _vp]),
    # profiling, development switches, test hooks
    "cs_profile": (_int, [_int]),
    "cs_profile_read": (_int, [_dp, _ip]),
    "cs_profile_tiles": (_int, [_dp]),
    "cs_debug_set": (_int, [_int, _int]),
    "cs_test_powf": (_int, [_vp, _flt, _vp, _size, _vp]),
    "cs_test_exp": (_int, [_vp, _vp, _size, _vp]),
    "cs_test_edge_threshold": (_flt, [_flt]),
    "cs_test_blur_plan": (_int, [_dbl, _dbl, _int, _dbl] + _nhw + [_int]),
}
EXPORTS = list(SIGNATURES)

_lib = None


def _declare(L, name):
    f = getattr(L, name)
    f.restype, f.argtypes = SIGNATURES[name]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is not built (run `python __graft_entry__.py` or "
            "`make -C comfystereo_amd/csrc`).  comfystereo_amd has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    _declare(L, "cs_version")
    if L.cs_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {L.cs_version()}, these bindings were written for {ABI_VERSION}: "
                          "rebuild it (`make -C comfystereo_amd/csrc`)")
    for name in SIGNATURES:
        _declare(L, name)
    _lib = L
    return L


def debug_set(key, value):
    """cs_debug_set: development switch `key` (see DEBUG) := value (pt_variant: a PT_VARIANT name).  Process-wide; reset it to 0
    afterwards."""
    if key == "pt_variant" and isinstance(value, str):
        value = PT_VARIANT[value]
    check(lib().cs_debug_set(DEBUG[key], int(value)))


def check(rc):
    if rc != CS_OK:
        raise NativeError(rc, lib().cs_last_error().decode("utf-8", "replace"))
