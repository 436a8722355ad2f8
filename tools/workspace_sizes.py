"""Every size the C ABI reports for a grid of calls, and the code it returns for a sweep of refused calls -- host-side answers, no GPU
(tests/golden/workspace_bytes.json, tests/test_workspace_layout.py).

    python tools/workspace_sizes.py > tests/golden/workspace_bytes.json

records the answers of the library that comfystereo_amd._native loads (CS_LIB_PATH: another build of it).  RECORD ON A HOST WITHOUT A
GPU: a library from before the stats pre-pass helper launched k_stats_init on the fake statistics pointer before it refused
cs_stereo_shift's 2^31-element cases -- a failed launch without a device, a fault with one.  The current library refuses first.
The workspace carving is host code that several kernels share; a refactor of it must leave every one of these numbers as it was.
"""
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from comfystereo_amd import _native   # noqa: E402

FILLS = sorted(_native.FILL, key=_native.FILL.get)
MODES = ("left-right", "top-bottom", "red-cyan-anaglyph", "cyan-red-reverseanaglyph", "left-only")
NS, HS, WS = (1, 2, 5), (1, 130, 1080), (8, 640, 3840, 8192)
# pt_variant values that change a size: tiny_replay_pool shrinks the replay pool of the polylines techniques
VARIANTS = {"default": FILLS, "tiny_replay_pool": ("polylines_soft", "polylines_sharp")}
SHAPE_QUERIES = ("cs_asd_workspace_bytes", "cs_blur_workspace_bytes", "cs_blur_scipy_workspace_bytes", "cs_warp_workspace_bytes",
                 "cs_warp_mesh_workspace_bytes", "cs_grid_warp_workspace_bytes", "cs_inpaint_prepare_workspace_bytes")


def _params(n, h, w, fill, mode, blur, resize, flags, batch):
    p = _native.Params()
    p.n, p.h, p.w, p.depth_c = n, h, w, 3
    p.depth_h, p.depth_w = (max(1, h // 2), max(1, w // 2)) if resize else (h, w)
    p.fill, p.mode, p.batch_size = _native.FILL[fill], _native.MODE[mode], batch
    p.depth_map_blur, p.depth_blur_vert_smooth, p.flags = int(blur), 6, flags
    p.divergence, p.separation, p.stereo_balance, p.convergence_point, p.stereo_offset_exponent = 6.0, 0.3, 0.0, 0.1, 2.0
    p.depth_blur_strength, p.depth_blur_edge_threshold, p.depth_blur_falloff = 20.0, 20.0, 2.0
    return p


def generate_sizes(L, fill):
    """cs_workspace_bytes of one technique, in the fixed order of the loops below."""
    out = []
    for mode in MODES:
        for blur in (0, 1):
            for resize in (0, 1):
                for flags in (0, 24):   # (dialect bits 3 / 4: D32 and full D64)
                    for batch in ((1, 4) if fill == "gpu_warp" else (12,)):
                        for n in NS:
                            for h in HS:
                                for w in WS:
                                    p = _params(n, h, w, fill, mode, blur, resize, flags, batch)
                                    out.append(L.cs_workspace_bytes(ctypes.byref(p)))
    return out


def sizes(L):
    out = {"generate": {}, "asd_for": {}, "shape": {}, "fixed": {}}
    try:
        for variant, fills in VARIANTS.items():
            _native.check(L.cs_debug_set(_native.DEBUG["pt_variant"], _native.PT_VARIANT[variant]))
            for chunks in (0, 2):
                _native.check(L.cs_debug_set(_native.DEBUG["chunks"], chunks))
                for fill in fills:
                    out["generate"][f"{variant}/chunks{chunks}/{fill}"] = generate_sizes(L, fill)
            _native.check(L.cs_debug_set(_native.DEBUG["chunks"], 0))
            shapes = [(n, h, w) for n in NS for h in HS for w in WS]
            for fill in fills:
                if fill != "gpu_warp":
                    out["asd_for"][f"{variant}/{fill}"] = [L.cs_asd_workspace_bytes_for(n, h, w, _native.FILL[fill]) for n, h, w in shapes]
            for q in SHAPE_QUERIES:
                if variant == "default" or q == "cs_asd_workspace_bytes":
                    out["shape"][f"{variant}/{q}"] = [getattr(L, q)(n, h, w) for n, h, w in shapes]
    finally:
        L.cs_debug_set(_native.DEBUG["pt_variant"], 0)
        L.cs_debug_set(_native.DEBUG["chunks"], 0)
    out["fixed"] = {"cs_stereo_shift_workspace_bytes": L.cs_stereo_shift_workspace_bytes(),
                    "cs_latent_shift_plan_workspace_bytes": L.cs_latent_shift_plan_workspace_bytes()}
    return out


# ---- refused calls -------------------------------------------------------------------------------------------------------------
# Every case is refused before any device work: besides the defects drawn for it, its workspace is too small (the last check of
# every entry point), so its pointers (the address 16) are never followed.  The one exception: cs_stereo_shift looks at the size
# of the whole tensor after its workspace, so its 2^31-element cases come with a workspace that is large enough.
FAKE = 16
ENTRIES = ("cs_stereo_shift", "cs_latent_shift_plan", "cs_grid_warp", "cs_inpaint_prepare", "cs_forward_warp", "cs_forward_warp2",
           "cs_forward_warp_mesh", "cs_apply_stereo_divergence2")
DEFECTS = ("null", "size", "wide", "huge", "workspace")


def _case(rng, entry):
    """One refused call of `entry`: (arguments, the defects it carries)."""
    defects = {"workspace"} | {d for d in DEFECTS if rng.random() < 0.3}
    n, h, w, c = rng.choice((1, 2, 5)), rng.choice((1, 2, 130)), rng.choice((2, 8, 640)), rng.choice((1, 3, 4))
    if "size" in defects:
        which = rng.choice("nhw")
        bad = rng.choice((0, -1, -2 ** 31))
        n, h, w = (bad if which == "n" else n), (bad if which == "h" else h), (bad if which == "w" else w)
    if "wide" in defects and w > 0:
        w = rng.choice((8193, 16385, 20000, 65536, 1 << 20))
    if "huge" in defects and n > 0 and h > 0 and w > 0:   # 2^31 elements or more, by shape only
        n, h = rng.choice(((1, (2 ** 31 + w - 1) // w), (4, (2 ** 29 + w - 1) // w + 1), (65536, 40000)))
    ptr = lambda: None if ("null" in defects and rng.random() < 0.5) else FAKE   # noqa: E731
    ws_bytes = rng.choice((0, 16, 255))
    fill = rng.choice(sorted(_native.FILL.values()) + [-1, 11])
    if entry == "cs_stereo_shift":
        if "huge" in defects and rng.random() < 0.5:
            ws_bytes = 1 << 20
            defects.discard("workspace")
            if (n > 0 and h > 0 and w > 0 and n * h * w < 2 ** 31) or "null" in defects:
                ws_bytes = 0   # (not a 2^31 case after all, or one with pointers not all set: keep it refused at the workspace)
        return [ptr(), ptr(), n, c, h, w, 8.0, rng.choice((0, 1)), 1.0, ptr(), ptr(), ws_bytes, None]
    if entry == "cs_latent_shift_plan":
        return [ptr(), n, h, w, rng.choice((8.0, float("nan"))), 1.0, ptr(), ptr(), ws_bytes, None]
    if entry == "cs_grid_warp":
        return [ptr(), ptr(), n, c, h, w, 4.0, 0.5, 1.0, 0.5, rng.choice((0, 1, 2, 3, 4, -1)), rng.choice((0, 0, 1, 2, 3)), ptr(), ptr(),
                ptr(), ws_bytes, None]
    if entry == "cs_inpaint_prepare":
        return [ptr(), ptr(), n, h, w, 4.0, 0.05, ptr(), ptr(), ptr(), ptr(), ptr(), ptr(), ws_bytes, None]
    if entry == "cs_forward_warp":
        return [ptr(), ptr(), n, h, w, 4.0, 0.5, 1.0, 0.5, ptr(), ptr(), ptr(), ws_bytes, None]
    if entry == "cs_forward_warp2":
        return [ptr(), ptr(), n, h, w, 4.0, 0.5, 1.0, 0.5, rng.choice((1.5, 14.0)), rng.choice((8, 17)), ptr(), ptr(), ptr(), ws_bytes, None]
    if entry == "cs_forward_warp_mesh":
        return [ptr(), ptr(), n, h, w, 4.0, 0.5, 1.0, 0.5, rng.choice((1.5, -1.0)), ptr(), ptr(), ptr(), ws_bytes, None]
    assert entry == "cs_apply_stereo_divergence2"
    return [ptr(), ptr(), n, h, w, 4.0, 0.5, 1.0, fill, 0.5, rng.choice((0, 0, 1, 3, 4)), ptr(), ptr(), ws_bytes, None]


def refused_calls(entry, count=400):
    rng = random.Random("refused/" + entry)
    return [_case(rng, entry) for _ in range(count)]


def error_codes(L):
    return {entry: [getattr(L, entry)(*args) for args in refused_calls(entry)] for entry in ENTRIES}


def main():
    L = _native.lib()
    out = sizes(L)
    out["refused"] = error_codes(L)
    for entry, codes in out["refused"].items():
        assert all(c != _native.CS_OK for c in codes), entry
    json.dump(out, sys.stdout, separators=(",", ":"), sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
