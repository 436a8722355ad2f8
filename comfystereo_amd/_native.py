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

# the ABI version the ctypes signatures below were written for (include/comfystereo_amd.h CS_ABI_VERSION)
ABI_VERSION = 4

EXPORTS = [
    "cs_version", "cs_last_error", "cs_max_width", "cs_max_width_mode", "cs_max_width_params", "cs_output_shape", "cs_workspace_bytes", "cs_generate",
    "cs_asd_workspace_bytes", "cs_asd_workspace_bytes_for", "cs_apply_stereo_divergence", "cs_apply_stereo_divergence2", "cs_blur_workspace_bytes", "cs_directional_blur", "cs_blur_scipy_workspace_bytes", "cs_directional_blur_scipy",
    "cs_warp_workspace_bytes", "cs_forward_warp", "cs_forward_warp2", "cs_warp_mesh_workspace_bytes", "cs_forward_warp_mesh", "cs_expand_u8", "cs_pack_u8", "cs_host_expand_u8", "cs_host_copy", "cs_take_f32", "cs_host_replicate_f32", "cs_stereo_shift_workspace_bytes", "cs_stereo_shift", "cs_profile", "cs_profile_read", "cs_profile_tiles", "cs_debug_set",
    "cs_test_powf", "cs_test_exp", "cs_test_edge_threshold",
    "cs_grid_warp_workspace_bytes", "cs_grid_warp_max_width", "cs_grid_warp", "cs_interpolate_fill", "cs_detect_disocclusions",
    "cs_gaussian_blur_workspace_bytes", "cs_gaussian_blur_max_taps", "cs_gaussian_blur",
    "cs_inpaint_prepare_workspace_bytes", "cs_inpaint_prepare_max_width", "cs_inpaint_prepare",
    "cs_pil_resize_workspace_bytes", "cs_pil_resize_max_taps", "cs_pil_resize",
    "cs_stereo_attention_max_head_dim", "cs_stereo_attention", "cs_stereo_attention_half",
    "cs_attention_fwd_lse", "cs_attention_bwd_workspace_bytes", "cs_attention_bwd",
    "cs_attention_half_fwd_lse", "cs_attention_half_bwd_workspace_bytes", "cs_attention_half_bwd",
    "cs_latent_shift_plan_workspace_bytes", "cs_latent_shift_plan", "cs_latent_shift_apply", "cs_decode_to_codes",
    "cs_ddim_step", "cs_null_loss_workspace_bytes", "cs_null_loss_grad", "cs_adam_step",
]

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


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is not built (run `python __graft_entry__.py` or "
            "`make -C comfystereo_amd/csrc`).  comfystereo_amd has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    vp, c_int, c_double, c_size = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
    pp = ctypes.POINTER(Params)
    ip = ctypes.POINTER(ctypes.c_int)
    L.cs_version.restype = c_int
    L.cs_version.argtypes = []
    if L.cs_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {L.cs_version()}, these bindings were written for {ABI_VERSION}: "
                          "rebuild it (`make -C comfystereo_amd/csrc`)")
    L.cs_last_error.restype = ctypes.c_char_p
    L.cs_last_error.argtypes = []
    L.cs_max_width_mode.restype = c_int
    L.cs_max_width_mode.argtypes = [c_int, c_int]
    L.cs_max_width_params.restype = c_int
    L.cs_max_width_params.argtypes = [ctypes.POINTER(Params)]
    L.cs_max_width.restype = c_int
    L.cs_max_width.argtypes = [c_int]
    L.cs_output_shape.restype = c_int
    L.cs_output_shape.argtypes = [pp, ip, ip, ip, ip]
    L.cs_workspace_bytes.restype = c_size
    L.cs_workspace_bytes.argtypes = [pp]
    L.cs_generate.restype = c_int
    L.cs_generate.argtypes = [pp, vp, vp, vp, vp, vp, vp, vp, c_size, vp]
    L.cs_asd_workspace_bytes.restype = c_size
    L.cs_asd_workspace_bytes.argtypes = [c_int, c_int, c_int]
    L.cs_asd_workspace_bytes_for.restype = c_size
    L.cs_asd_workspace_bytes_for.argtypes = [c_int, c_int, c_int, c_int]
    L.cs_apply_stereo_divergence2.restype = c_int
    L.cs_apply_stereo_divergence2.argtypes = [vp, vp, c_int, c_int, c_int, c_double, c_double, c_double, c_int, c_double, c_int,
                                              vp, vp, c_size, vp]
    L.cs_apply_stereo_divergence.restype = c_int
    L.cs_apply_stereo_divergence.argtypes = [vp, vp, c_int, c_int, c_int, c_double, c_double, c_double, c_int, c_double,
                                             vp, vp, c_size, vp]
    L.cs_blur_workspace_bytes.restype = c_size
    L.cs_blur_workspace_bytes.argtypes = [c_int, c_int, c_int]
    L.cs_directional_blur.restype = c_int
    L.cs_directional_blur.argtypes = [vp, c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_int, vp, vp, vp,
                                      c_size, vp]
    L.cs_blur_scipy_workspace_bytes.restype = c_size
    L.cs_blur_scipy_workspace_bytes.argtypes = [c_int, c_int, c_int]
    L.cs_directional_blur_scipy.restype = c_int
    L.cs_directional_blur_scipy.argtypes = [vp, c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_int, vp, vp, vp, c_size, vp]
    L.cs_warp_workspace_bytes.restype = c_size
    L.cs_warp_workspace_bytes.argtypes = [c_int, c_int, c_int]
    L.cs_warp_mesh_workspace_bytes.restype = c_size
    L.cs_warp_mesh_workspace_bytes.argtypes = [c_int, c_int, c_int]
    L.cs_forward_warp_mesh.restype = c_int
    L.cs_forward_warp_mesh.argtypes = [vp, vp, c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_double, vp, vp, vp, c_size, vp]
    L.cs_forward_warp.restype = c_int
    L.cs_forward_warp.argtypes = [vp, vp, c_int, c_int, c_int, c_double, c_double, c_double, c_double, vp, vp, vp, c_size, vp]
    L.cs_forward_warp2.restype = c_int
    L.cs_forward_warp2.argtypes = [vp, vp, c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_double, c_int, vp, vp, vp, c_size, vp]
    L.cs_pack_u8.restype = c_int
    L.cs_pack_u8.argtypes = [vp, vp, c_size, c_int, c_int, vp]
    L.cs_host_expand_u8.restype = c_int
    L.cs_host_expand_u8.argtypes = [vp, vp, c_size, c_int, c_int, c_int]
    L.cs_host_copy.restype = c_int
    L.cs_host_copy.argtypes = [vp, vp, c_size, c_int]
    L.cs_take_f32.restype = c_int
    L.cs_take_f32.argtypes = [vp, vp, c_size, c_int, vp]
    L.cs_host_replicate_f32.restype = c_int
    L.cs_host_replicate_f32.argtypes = [vp, vp, c_size, c_int, c_int]
    L.cs_stereo_shift_workspace_bytes.restype = c_size
    L.cs_stereo_shift_workspace_bytes.argtypes = []
    L.cs_stereo_shift.restype = c_int
    L.cs_stereo_shift.argtypes = [vp, vp, c_int, c_int, c_int, c_int, c_double, c_int, c_double, vp, vp, c_size, vp]
    L.cs_expand_u8.restype = c_int
    L.cs_expand_u8.argtypes = [vp, vp, c_size, vp]
    L.cs_profile.restype = c_int
    L.cs_profile.argtypes = [c_int]
    L.cs_profile_read.restype = c_int
    L.cs_profile_read.argtypes = [ctypes.POINTER(c_double), ip]
    L.cs_profile_tiles.restype = c_int
    L.cs_profile_tiles.argtypes = [ctypes.POINTER(c_double)]
    L.cs_debug_set.restype = c_int
    L.cs_debug_set.argtypes = [c_int, c_int]
    L.cs_test_powf.restype = c_int
    L.cs_test_powf.argtypes = [vp, ctypes.c_float, vp, c_size, vp]
    L.cs_test_exp.restype = c_int
    L.cs_test_exp.argtypes = [vp, vp, c_size, vp]
    L.cs_test_edge_threshold.restype = ctypes.c_float
    L.cs_test_edge_threshold.argtypes = [ctypes.c_float]
    L.cs_grid_warp_workspace_bytes.restype = c_size
    L.cs_grid_warp_workspace_bytes.argtypes = [c_int, c_int, c_int]
    L.cs_grid_warp_max_width.restype = c_int
    L.cs_grid_warp_max_width.argtypes = [c_int]
    L.cs_grid_warp.restype = c_int
    L.cs_grid_warp.argtypes = [vp, vp, c_int, c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_int, c_int, vp, vp, vp,
                               c_size, vp]
    L.cs_interpolate_fill.restype = c_int
    L.cs_interpolate_fill.argtypes = [vp, vp, c_int, c_int, c_int, c_int, vp, vp]
    L.cs_detect_disocclusions.restype = c_int
    L.cs_detect_disocclusions.argtypes = [vp, vp, vp, c_int, c_int, c_double, vp, vp]
    L.cs_gaussian_blur_workspace_bytes.restype = c_size
    L.cs_gaussian_blur_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int]
    L.cs_gaussian_blur_max_taps.restype = c_int
    L.cs_gaussian_blur_max_taps.argtypes = []
    L.cs_gaussian_blur.restype = c_int
    L.cs_gaussian_blur.argtypes = [c_int, vp, vp, c_int, c_double, c_int, c_int, c_int, vp, vp, c_size, vp]
    L.cs_inpaint_prepare_workspace_bytes.restype = c_size
    L.cs_inpaint_prepare_workspace_bytes.argtypes = [c_int, c_int, c_int]
    L.cs_inpaint_prepare_max_width.restype = c_int
    L.cs_inpaint_prepare_max_width.argtypes = []
    L.cs_inpaint_prepare.restype = c_int
    L.cs_inpaint_prepare.argtypes = [vp, vp, c_int, c_int, c_int, c_double, c_double, vp, vp, vp, vp, vp, vp, c_size, vp]
    L.cs_pil_resize_workspace_bytes.restype = c_size
    L.cs_pil_resize_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int]
    L.cs_pil_resize_max_taps.restype = c_int
    L.cs_pil_resize_max_taps.argtypes = []
    L.cs_pil_resize.restype = c_int
    L.cs_pil_resize.argtypes = [vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, vp, vp, c_size, vp, c_size, vp]
    L.cs_stereo_attention_max_head_dim.restype = c_int
    L.cs_stereo_attention_max_head_dim.argtypes = []
    L.cs_stereo_attention.restype = c_int
    L.cs_stereo_attention.argtypes = [vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_int, vp]
    L.cs_stereo_attention_half.restype = c_int
    L.cs_stereo_attention_half.argtypes = [vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_int, vp]
    L.cs_attention_fwd_lse.restype = c_int
    L.cs_attention_fwd_lse.argtypes = [vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_double, vp]
    L.cs_attention_bwd_workspace_bytes.restype = c_size
    L.cs_attention_bwd_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, c_int]
    L.cs_attention_bwd.restype = c_int
    L.cs_attention_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_double, vp, c_size, vp]
    L.cs_attention_half_fwd_lse.restype = c_int
    L.cs_attention_half_fwd_lse.argtypes = [vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, c_double, vp]
    L.cs_attention_half_bwd_workspace_bytes.restype = c_size
    L.cs_attention_half_bwd_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, c_int]
    L.cs_attention_half_bwd.restype = c_int
    L.cs_attention_half_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, c_double, vp, c_size, vp]
    L.cs_latent_shift_plan_workspace_bytes.restype = c_size
    L.cs_latent_shift_plan_workspace_bytes.argtypes = []
    L.cs_latent_shift_plan.restype = c_int
    L.cs_latent_shift_plan.argtypes = [vp, c_int, c_int, c_int, c_double, c_double, vp, vp, c_size, vp]
    L.cs_latent_shift_apply.restype = c_int
    L.cs_latent_shift_apply.argtypes = [vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp]
    L.cs_decode_to_codes.restype = c_int
    L.cs_decode_to_codes.argtypes = [vp, c_int, c_int, c_int, c_int, c_int, vp, vp]
    c_ll = ctypes.c_longlong
    L.cs_ddim_step.restype = c_int
    L.cs_ddim_step.argtypes = [vp, vp, vp, vp, c_int, c_ll, c_double, c_double, c_double, c_double, c_double, vp]
    L.cs_null_loss_workspace_bytes.restype = c_size
    L.cs_null_loss_workspace_bytes.argtypes = [c_ll]
    L.cs_null_loss_grad.restype = c_int
    L.cs_null_loss_grad.argtypes = [vp, vp, vp, vp, vp, vp, vp, c_int, c_ll, c_double, c_double, c_double, c_double, c_double, vp,
                                    c_size, vp]
    L.cs_adam_step.restype = c_int
    L.cs_adam_step.argtypes = [vp, vp, vp, vp, c_int, c_ll, c_double, c_double, c_double, c_double, c_int, vp]
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
