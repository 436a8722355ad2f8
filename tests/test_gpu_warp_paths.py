"""Every kernel path of gpu_warp (the node's default technique) against the C oracle and against each other.  -m gpu.

gw_launch (cs_gpuwarp.hip) picks one of the k_gpuwarp_q / k_gpuwarp instantiations per call from the width, the exponent, the
layout, the eyes and the buffers' alignment, and records the pick in every frame's ST_WARP_PATH stats word (_native.WARP_PATH).
Each case below names the path it is built to reach under the default choice and under the development switch pt_variant
(_native.PT_VARIANT): gw_no_quad k_gpuwarp in the node layout, gw_generic_layout the generic layout, gw_threads_512 /
gw_threads_256_narrow / gw_threads_1024 / gw_threads_256 the workgroup sizes 512 / 256 (rows of at most 1024) / 1024 / 256,
gw_six_waves the 6-wave instantiation at 512 threads.  Every run is checked
  * path: the recorded code is the expected one (a shape that quietly leaves the k_gpuwarp_q predicate fails here);
  * against node_oracle.generate: all four outputs array_equal.  The oracle follows the kernels' float32 arithmetic operation for
    operation, and every path has been measured bit-equal to it; the 2e-6 the other node-level tests allow (and the 1e-4 of
    test_gpu_parity / test_gpu_dropin, which compare with torch-captured fixtures) would let an ulp-level slip of one path through;
  * across paths: all four outputs bit-identical as uint32 -- the header of k_gpuwarp_q promises k_gpuwarp's expressions, operation
    for operation, and x + 0 * p == x for the finite pixels in [0, 1] used here.
The one documented deviation (k_gpuwarp_q skips the image row whose vertical weight is exactly zero, so a non-finite pixel there
does not propagate) has a test of its own."""
import numpy as np
import pytest
import torch

import synth
from comfystereo_amd import _native
from oracle import node_oracle

pytestmark = pytest.mark.gpu
UI = "GPU Warp (Fast)"
TOL = 2e-6
F32 = np.float32
NAMES = ("stereoscope", "depth_left", "depth_right", "mask")
BLUR_KW = dict(depth_blur_falloff=2.0, depth_blur_vert_smooth=6)
MAX_ERR = {}   # largest colour difference from the oracle seen per path name (printed by the last test)


@pytest.fixture(scope="module")
def engine():
    from comfystereo_amd import engine as e
    assert torch.cuda.is_available()
    return e


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def C(w, h, e, depth, n=1, mode="left-right", bal=0.0, div=8.0, sep=0.0, conv=0.5, blur=False, bs=4, paths=None):
    return dict(w=w, h=h, e=e, depth=depth, n=n, mode=mode, bal=bal, div=div, sep=sep, conv=conv, blur=blur, bs=bs, paths=paths)


def case_id(c):
    return f"{c['w']}x{c['h']}-e{c['e']}-{c['depth']}-{c['mode']}-b{c['bal']}-d{c['div']}-c{c['conv']}" + ("-blur" if c["blur"] else "")


# The widths: a wave of k_gpuwarp_q stages 252 columns and its lane 63 re-stages the next wave's first group, so a pass covers 1008 /
# 2016 / 4032 columns at 256 / 512 / 1024 threads; 256 / 512 / 1024 threads at 1024 / 2048 columns; the lazy blur tiles' second word
# of bits at 2048 and their limit at 4096 (blur on); 7760 and 7763 (cs_max_width of gpu_warp).  Widths that are not multiples of 4
# take k_gpuwarp.  Four 512-thread workgroups per CU (the 8-wave instantiations) fit up to ~1940 columns for k_gpuwarp and ~2010 for
# k_gpuwarp_q; 1.3 is the exponent that adds the powf tables to the LDS, which moves that cut (1920, 1984).
WIDTHS = [
    C(8, 3, 2.0, "random8", div=8.0, paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_256_narrow": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(12, 2, 1.3, "stepped", div=8.0, paths={"default": "q<6,-1>", "gw_no_quad": "k<6,-1,node>", "gw_generic_layout": "k<6,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_256_narrow": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(248, 5, 2.0, "blobs", div=12.0, paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_256_narrow": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(252, 3, 0.5, "stepped", div=8.0, paths={"default": "q<6,-1>", "gw_no_quad": "k<6,-1,node>", "gw_generic_layout": "k<6,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_256_narrow": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(256, 2, 2.0, "noisy_ramp", div=8.0, paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_256_narrow": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(508, 5, 3.0, "clipped", div=8.0, paths={"default": "q<6,-1>", "gw_no_quad": "k<6,-1,node>", "gw_generic_layout": "k<6,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_256_narrow": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(1008, 3, 2.0, "stepped", div=8.0, paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_256_narrow": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(1012, 1, 0.0, "blobs", div=8.0, paths={"default": "q<6,-1>", "gw_no_quad": "k<6,-1,node>", "gw_generic_layout": "k<6,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_256_narrow": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(1020, 5, 2.0, "random8", div=8.0, paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_256_narrow": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(1024, 2, 1.0, "stepped", div=8.0, paths={"default": "q<6,-1>", "gw_no_quad": "k<6,-1,node>", "gw_generic_layout": "k<6,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_256_narrow": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(1028, 3, 2.0, "stepped", div=8.0, paths={"default": "q<8,2>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "q<8,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(1028, 3, 1.3, "blobs", div=8.0, paths={"default": "q<8,-1>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(1920, 3, 1.3, "radial", div=4.5, paths={"default": "q<8,-1>", "gw_no_quad": "k<6,-1,node>", "gw_generic_layout": "k<6,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(1940, 3, 2.0, "blobs", paths={"default": "q<8,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(1984, 2, 1.3, "blobs", paths={"default": "q<6,-1>", "gw_no_quad": "k<6,-1,node>", "gw_generic_layout": "k<6,-1>", "gw_threads_512": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(1984, 5, 2.0, "blobs", paths={"default": "q<8,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(2016, 2, 2.0, "stepped", div=8.0, paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(2020, 5, 1.3, "blobs", div=8.0, paths={"default": "q<6,-1>", "gw_no_quad": "k<6,-1,node>", "gw_generic_layout": "k<6,-1>", "gw_threads_512": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(2044, 1, 2.0, "clipped", div=8.0, paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(2048, 3, 2.0, "stepped", div=8.0, blur=True, paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(2052, 2, 1.0, "blobs", div=8.0, blur=True, paths={"default": "q<8,-1>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<8,-1>"}),
    C(4032, 3, 2.0, "stepped", div=8.0, paths={"default": "q<8,2>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<8,2>"}),
    C(4036, 1, 0.5, "random8", div=8.0, paths={"default": "q<8,-1>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<8,-1>"}),
    C(4092, 5, 2.0, "blobs", div=8.0, paths={"default": "q<8,2>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<8,2>"}),
    C(4096, 2, 2.0, "stepped", div=8.0, blur=True, paths={"default": "q<8,2>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<8,2>"}),
    C(4100, 3, 1.3, "blobs", div=8.0, blur=True, paths={"default": "q<8,-1>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<8,-1>"}),
    C(7760, 5, 2.0, "stepped", div=3.0, paths={"default": "q<8,2>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<8,2>"}),
    C(7760, 2, 1.3, "blobs", div=8.0, paths={"default": "q<8,-1>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<8,-1>"}),
    C(9, 3, 2.0, "random8", div=8.0, paths={"default": "k<6,2,node>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "k<8,2,node>", "gw_threads_256_narrow": "k<6,2,node>", "gw_threads_1024": "k<8,2,node>", "gw_threads_256": "k<6,2,node>", "gw_six_waves": "k<6,2,node>"}),
    C(1023, 2, 1.3, "stepped", div=8.0, paths={"default": "k<6,-1,node>", "gw_no_quad": "k<6,-1,node>", "gw_generic_layout": "k<6,-1>", "gw_threads_512": "k<8,-1,node>", "gw_threads_256_narrow": "k<6,-1,node>", "gw_threads_1024": "k<8,-1,node>", "gw_threads_256": "k<6,-1,node>", "gw_six_waves": "k<6,-1,node>"}),
    C(2049, 5, 2.0, "blobs", div=8.0, blur=True, paths={"default": "k<8,2,node>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "k<6,2,node>", "gw_threads_1024": "k<8,2,node>", "gw_threads_256": "k<6,2,node>", "gw_six_waves": "k<8,2,node>"}),
    C(7763, 3, 2.0, "stepped", div=3.0, paths={"default": "k<8,2,node>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "k<6,2,node>", "gw_threads_1024": "k<8,2,node>", "gw_threads_256": "k<6,2,node>", "gw_six_waves": "k<8,2,node>"}),
]
# the eight modes (anaglyphs and single-eye modes: the generic layout), stereo_balance (+-1: one eye is the source image), divergence
# of both signs (negative: both eyes are the source image) and up to gaps of 200 columns, convergence 0 / 0.5 / 1
MODES = [
    C(516, 3, 2.0, "blobs", mode="left-right", paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_256_narrow": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(516, 3, 2.0, "blobs", mode="right-left", paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_256_narrow": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(516, 3, 2.0, "blobs", mode="top-bottom", paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_256_narrow": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(516, 3, 2.0, "blobs", mode="bottom-top", paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_256_narrow": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(516, 3, 2.0, "blobs", mode="red-cyan-anaglyph", paths={"default": "k<6,2>", "gw_no_quad": "k<6,2>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "k<8,2>", "gw_threads_256_narrow": "k<6,2>", "gw_threads_1024": "k<8,2>", "gw_threads_256": "k<6,2>", "gw_six_waves": "k<6,2>"}),
    C(516, 3, 2.0, "blobs", mode="cyan-red-reverseanaglyph", paths={"default": "k<6,2>", "gw_no_quad": "k<6,2>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "k<8,2>", "gw_threads_256_narrow": "k<6,2>", "gw_threads_1024": "k<8,2>", "gw_threads_256": "k<6,2>", "gw_six_waves": "k<6,2>"}),
    C(516, 3, 2.0, "blobs", mode="left-only", paths={"default": "k<6,2>", "gw_no_quad": "k<6,2>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "k<8,2>", "gw_threads_256_narrow": "k<6,2>", "gw_threads_1024": "k<8,2>", "gw_threads_256": "k<6,2>", "gw_six_waves": "k<6,2>"}),
    C(516, 3, 2.0, "blobs", mode="only-right", paths={"default": "k<6,2>", "gw_no_quad": "k<6,2>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "k<8,2>", "gw_threads_256_narrow": "k<6,2>", "gw_threads_1024": "k<8,2>", "gw_threads_256": "k<6,2>", "gw_six_waves": "k<6,2>"}),
    C(516, 3, 1.3, "clipped", mode="red-cyan-anaglyph", paths={"default": "k<6,-1>", "gw_no_quad": "k<6,-1>", "gw_generic_layout": "k<6,-1>", "gw_threads_512": "k<8,-1>", "gw_threads_256_narrow": "k<6,-1>", "gw_threads_1024": "k<8,-1>", "gw_threads_256": "k<6,-1>", "gw_six_waves": "k<6,-1>"}),
    C(1028, 3, 2.0, "stepped", bal=0.5, paths={"default": "q<8,2>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "q<8,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(1028, 3, 2.0, "stepped", bal=-0.5, paths={"default": "q<8,2>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "q<8,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(1028, 3, 2.0, "stepped", bal=1.0, paths={"default": "k<8,2,node>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "k<8,2,node>", "gw_threads_1024": "k<8,2,node>", "gw_threads_256": "k<6,2,node>", "gw_six_waves": "k<6,2,node>"}),
    C(1028, 3, 2.0, "stepped", bal=-1.0, paths={"default": "k<8,2,node>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "k<8,2,node>", "gw_threads_1024": "k<8,2,node>", "gw_threads_256": "k<6,2,node>", "gw_six_waves": "k<6,2,node>"}),
    C(1028, 3, 2.0, "stepped", div=-6.0, conv=0.5, paths={"default": "k<8,2,node>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "k<8,2,node>", "gw_threads_1024": "k<8,2,node>", "gw_threads_256": "k<6,2,node>", "gw_six_waves": "k<6,2,node>"}),
    C(1028, 3, 2.0, "stepped", div=12.0, conv=0.0, paths={"default": "q<8,2>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "q<8,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(1028, 3, 1.3, "stepped", div=12.0, conv=1.0, paths={"default": "q<8,-1>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(1028, 3, 1.0, "stepped", div=20.0, conv=0.5, paths={"default": "q<8,-1>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(1028, 3, 1.0, "stepped", div=-20.0, conv=0.5, paths={"default": "k<8,-1,node>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "k<8,-1,node>", "gw_threads_1024": "k<8,-1,node>", "gw_threads_256": "k<6,-1,node>", "gw_six_waves": "k<6,-1,node>"}),
    C(1028, 3, 1.3, "stepped", div=-12.0, bal=-1.5, paths={"default": "k<8,-1,node>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "k<8,-1,node>", "gw_threads_1024": "k<8,-1,node>", "gw_threads_256": "k<6,-1,node>", "gw_six_waves": "k<6,-1,node>"}),
]
# depth that forces rare branches: a flat frame (no range), a range just above / just below 1e-6, a range beyond 2^40 (the IEEE
# division instead of the division core) with numerators beyond 2^60, 13 frames in sub-batches of 12 mixing maxima <= 1 and > 1
DEPTHS = [
    C(1028, 3, 2.0, "flat", paths={"default": "q<8,2>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "q<8,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(1028, 3, 2.0, "range_above", paths={"default": "q<8,2>", "gw_no_quad": "k<8,2,node>", "gw_generic_layout": "k<8,2>", "gw_threads_512": "q<8,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
    C(1028, 3, 1.3, "range_below", paths={"default": "q<8,-1>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(1028, 3, 1.0, "huge", paths={"default": "q<8,-1>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "q<8,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<6,-1>"}),
    C(2052, 2, 1.3, "huge", paths={"default": "q<8,-1>", "gw_no_quad": "k<8,-1,node>", "gw_generic_layout": "k<8,-1>", "gw_threads_512": "q<6,-1>", "gw_threads_1024": "q<8,-1>", "gw_threads_256": "q<6,-1>", "gw_six_waves": "q<8,-1>"}),
    C(516, 2, 2.0, "mixed13", paths={"default": "q<6,2>", "gw_no_quad": "k<6,2,node>", "gw_generic_layout": "k<6,2>", "gw_threads_512": "q<8,2>", "gw_threads_256_narrow": "q<6,2>", "gw_threads_1024": "q<8,2>", "gw_threads_256": "q<6,2>", "gw_six_waves": "q<6,2>"}),
]


def range_pair(above):
    """Two depth values > 1 (no x255 scaling; forward_warp_gpu divides them by 255) whose float32 range after that division is the
    first above / the last at or below 1e-6 -- the kernel's has_range test (range > (float)1e-6)."""
    base = F32(3.0)
    lo = base / F32(255.0)
    t = base
    while True:
        nxt = np.nextafter(t, F32(4.0), dtype=F32)
        if (nxt / F32(255.0) - lo) > F32(1e-6):
            return (base, nxt) if above else (base, t)
        t = nxt


def make_depth(c):
    n, h, w, kind = c["n"], c["h"], c["w"], c["depth"]
    if kind == "flat":
        return np.full((n, h, w, 3), 0.4, F32)
    pattern = synth.depth_batch("stepped", n, h, w, channels=1)[..., 0]
    if kind in ("range_above", "range_below"):
        a, b = range_pair(kind == "range_above")
        d = np.where(pattern > 0.4, b, a).astype(F32)
        assert ((d.max() / F32(255.0) - d.min() / F32(255.0)) > F32(1e-6)) == (kind == "range_above")
        return d[..., None]   # (one channel: the gray conversion of three would round the values)
    if kind == "huge":
        vals = np.array([0.0, 7.5, 1e13, 5e18, 1e21], F32)   # (/255: a range beyond 2^40, numerators beyond 2^60)
        idx = np.minimum((pattern * 6).astype(np.int64), 4)
        return vals[idx][..., None]
    if kind == "mixed13":
        d = synth.depth_batch("blobs", n, h, w, channels=3)
        d[[3, 7]] *= F32(255.0)   # frames 0-11 form one sub-batch whose maximum is > 1; frame 12 alone stays <= 1
        return d
    return synth.depth_batch(kind, n, h, w, channels=3)


def run(engine, dev_switch, img, depth, c, variant="default", views=None):
    """One node call through a Plan (-> outputs as numpy, the path names recorded per frame).  views: output tensors to use instead
    of the Plan's own (the alignment test)."""
    n, h, w = img.shape[:3]
    dev_switch("pt_variant", variant)
    try:
        p = engine.make_params(n, h, w, depth.shape[1], depth.shape[2], depth.shape[3], "gpu_warp", c["mode"], c["div"], c["sep"],
                               c["bal"], c["conv"], c["e"], c["blur"], 20.0, 20.0, 2.0, 6, c["bs"])
        plan = engine.Plan(p, img.device)
        if views is not None:
            plan.stereo, plan.depth_l, plan.depth_r, plan.mask = views
        out = [t.cpu().numpy().copy() for t in plan.run(img, depth)]
        codes = plan.stats()[:, _native.ST_WARP_PATH].numpy()
    finally:
        dev_switch("pt_variant", "default")
    return out, [_native.WARP_PATH_NAME.get(int(k), int(k)) for k in codes]


def oracle_of(img, depth, c):
    return node_oracle.generate(img, depth, c["div"], c["sep"], c["mode"], c["bal"], c["conv"], c["e"], UI, 20.0, 20.0, c["blur"],
                                batch_size=c["bs"], **BLUR_KW)


def check_vs_oracle(got, want, what):
    """-> the largest colour difference (reported by the last test); asserts all four outputs equal to the oracle's."""
    for k in (1, 2, 3):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, NAMES[k])
    assert got[0].shape == want[0].shape, what
    err = float(np.abs(got[0].astype(np.float64) - want[0].astype(np.float64)).max())
    assert err <= TOL and np.array_equal(got[0], want[0]), (what, err, int((got[0] != want[0]).sum()))
    return err


def check_all_paths(engine, dev_switch, c):
    img = synth.image_f32(c["n"], c["h"], c["w"], seed=c["w"] + c["h"])
    depth = make_depth(c)
    want = oracle_of(img, depth, c)
    it, dt = cuda(img), cuda(depth)
    first = None
    for variant, path in c["paths"].items():
        got, seen = run(engine, dev_switch, it, dt, c, variant)
        what = (case_id(c), variant, path)
        assert seen == [path] * c["n"], (what, seen)
        err = check_vs_oracle(got, want, what)
        MAX_ERR[path] = max(MAX_ERR.get(path, 0.0), err)
        if first is None:
            first = got
        else:
            for k in range(4):
                diff = int((got[k].view(np.uint32) != first[k].view(np.uint32)).sum())
                assert diff == 0, (what, NAMES[k], diff)


@pytest.mark.parametrize("c", WIDTHS, ids=case_id)
def test_widths_every_path(engine, dev_switch, c):
    check_all_paths(engine, dev_switch, c)


@pytest.mark.parametrize("c", MODES, ids=case_id)
def test_modes_balance_divergence_every_path(engine, dev_switch, c):
    check_all_paths(engine, dev_switch, c)


@pytest.mark.parametrize("c", DEPTHS, ids=case_id)
def test_rare_depth_branches_every_path(engine, dev_switch, c):
    if c["depth"] == "mixed13":
        c = dict(c, n=13, bs=12)
    check_all_paths(engine, dev_switch, c)


def kind_of(path):
    return "q" if path.startswith("q<") else ("k node" if path.endswith(",node>") else "k generic")


@pytest.mark.parametrize("seed", range(4))
def test_plateaus_spikes_and_ties_every_path(engine, dev_switch, seed):
    """The hostile depth of test_gpu_fuzz.make_case (plateaus, two-level patterns, ramps with jumps, spikes: exact ties in the scatter
    rounds), widened to a multiple of 4 and to one column less: the default path, k_gpuwarp in the node layout (gw_no_quad) and the generic
    layout (gw_generic_layout), each against the oracle and bit-identical to the others."""
    from test_gpu_fuzz import make_case
    rng = np.random.default_rng(4400 + seed)
    for _ in range(4):
        img8, d, div, sep, e, conv = make_case(rng)
        reps = int(rng.integers(2, 6))
        d = np.concatenate([np.roll(d, int(rng.integers(0, d.shape[1])), axis=1) for _ in range(reps)], axis=1)
        img8 = np.concatenate([np.roll(img8, int(rng.integers(0, img8.shape[1])), axis=1) for _ in range(reps)], axis=1)
        w4 = d.shape[1] & ~3
        for w in (w4, w4 - 1):
            h = d.shape[0]
            img = (img8[:, :w].astype(F32) / F32(255.0))[None]
            depth = np.ascontiguousarray(d[:, :w, None])[None]
            c = C(w, h, e, "make_case", div=float(abs(div)), sep=sep, conv=conv)
            q = w % 4 == 0 and w >= 8
            want = oracle_of(img, depth, c)
            it, dt = cuda(img), cuda(depth)
            first = None
            # (divergence > 0, balance 0, left-right: both eyes run, the node layout -- k_gpuwarp_q exactly when w % 4 == 0)
            for variant, kind in (("default", "q" if q else "k node"), ("gw_no_quad", "k node"), ("gw_generic_layout", "k generic")):
                got, seen = run(engine, dev_switch, it, dt, c, variant)
                assert kind_of(seen[0]) == kind, (case_id(c), variant, seen)
                err = check_vs_oracle(got, want, (case_id(c), variant))
                MAX_ERR[seen[0]] = max(MAX_ERR.get(seen[0], 0.0), err)
                if first is None:
                    first = got
                for k in range(4):
                    assert np.array_equal(got[k].view(np.uint32), first[k].view(np.uint32)), (case_id(c), variant, NAMES[k])


NODE_LAYOUT = {"q<8,2>", "q<8,-1>", "q<6,2>", "q<6,-1>", "k<8,2,node>", "k<8,-1,node>", "k<6,2,node>", "k<6,-1,node>"}
GENERIC = {"k<8,2>", "k<8,-1>", "k<6,2>", "k<6,-1>"}
COVERAGE = [   # (width, exponent, pt_variant) -> the instantiation it reaches
    (1024, 2.0, "default", "q<6,2>"), (1024, 1.3, "default", "q<6,-1>"), (1028, 2.0, "default", "q<8,2>"), (1028, 1.0, "default", "q<8,-1>"),
    (1024, 2.0, "gw_no_quad", "k<6,2,node>"), (1023, 0.5, "default", "k<6,-1,node>"), (1028, 2.0, "gw_no_quad", "k<8,2,node>"), (2049, 3.0, "default", "k<8,-1,node>"),
    (1024, 2.0, "gw_generic_layout", "k<6,2>"), (1024, 0.0, "gw_generic_layout", "k<6,-1>"), (4100, 2.0, "gw_generic_layout", "k<8,2>"), (2052, 1.3, "gw_generic_layout", "k<8,-1>"),
]


def test_designed_cases_reach_every_instantiation(engine, dev_switch):
    """A short walk over designed cases reaches every node-layout instantiation gw_launch can choose and, through pt_variant gw_generic_layout, every
    generic one; each agrees with the default path's bits of its case."""
    seen = set()
    for w, e, variant, path in COVERAGE:
        c = C(w, 2, e, "blobs", n=2)
        img = synth.image_f32(2, 2, w, seed=w)
        it, dt = cuda(img), cuda(make_depth(c))
        base, _ = run(engine, dev_switch, it, dt, c, "default")
        got, codes = run(engine, dev_switch, it, dt, c, variant)
        assert codes == [path, path], (w, e, variant, codes)
        seen.add(codes[0])
        for k in range(4):
            assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), (w, e, variant, NAMES[k])
    assert seen == NODE_LAYOUT | GENERIC, sorted(NODE_LAYOUT | GENERIC - seen)


def test_unaligned_outputs_through_the_c_abi(engine, dev_switch):
    """The header states no alignment requirement for the output buffers: outputs that are views at a 4-byte offset inside a larger
    allocation (a ctypes caller can pass such pointers) take k_gpuwarp instead of k_gpuwarp_q and give the same bits.  Every access
    stays inside the allocation: each view ends one float before it does."""
    c = C(1028, 3, 2.0, "stepped", n=2)
    img = synth.image_f32(2, 3, 1028, seed=9)
    it, dt = cuda(img), cuda(make_depth(c))
    base, codes = run(engine, dev_switch, it, dt, c)
    assert codes == ["q<8,2>"] * 2
    shapes = [b.shape for b in base]

    def off(shape):
        buf = torch.zeros(int(np.prod(shape)) + 2, dtype=torch.float32, device="cuda")
        return buf, buf[1:1 + int(np.prod(shape))].view(shape)

    for which in (None, 0, 1, 2, 3):   # all four outputs misaligned, then one at a time
        bufs = [off(s) if which in (None, k) else (None, torch.empty(s, dtype=torch.float32, device="cuda")) for k, s in enumerate(shapes)]
        views = [v for _, v in bufs]
        got, codes = run(engine, dev_switch, it, dt, c, views=views)
        assert codes == ["k<8,2,node>"] * 2, (which, codes)
        for k in range(4):
            assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), (which, NAMES[k])
        for buf, _ in bufs:   # the guard floats around each view are untouched
            if buf is not None:
                assert buf[0].item() == 0.0 and buf[-1].item() == 0.0, which


def row_taps(h):
    """The vertical taps of output row y in the kernels' float32 arithmetic (torch.linspace(-1, 1, h) as two-sided fused
    multiply-adds -- exact here through float64 -- and the grid_sample unnormalisation): (iy0, iy1, weight of iy1)."""
    step = F32(2.0) / F32(h - 1) if h > 1 else F32(0.0)
    taps = []
    for y in range(h):
        gy = F32(float(step) * y - 1.0) if y < h // 2 else F32(1.0 - float(step) * (h - y - 1))
        yy = min(max(F32(F32(gy + F32(1.0)) * F32(F32(h - 1) / F32(2.0))), F32(0.0)), F32(h - 1))
        iy0 = int(np.floor(yy))
        taps.append((iy0, min(iy0 + 1, h - 1), F32(yy - F32(iy0))))
    return taps


def test_non_finite_pixel_in_the_zero_weight_row(engine, dev_switch):
    """DESIGN.md section 2, deviation D1: a NaN and a +Inf in image row r, which for output row r - 1 is the second row of the vertical
    blend with weight exactly 0.  k_gpuwarp (and the oracle, and the reference) multiply it by 0: NaN there.  k_gpuwarp_q reads one
    row where the weight is 0: finite.  Everything else is identical, and at 1921 columns (k_gpuwarp) the answer is the oracle's."""
    h, r = 6, 3
    taps = row_taps(h)
    partners = [y for y, (i0, i1, wn) in enumerate(taps) if i1 == r and i0 != r and wn == 0.0]
    assert partners == [r - 1] and taps[r][0] == r
    for w in (1920, 1921):
        c = C(w, h, 2.0, "stepped", n=1, div=2.0)
        img = synth.image_f32(1, h, w, seed=12)
        img[0, r, 500, 1] = np.nan
        img[0, r, 1300, 0] = np.inf
        depth = make_depth(c)
        want = oracle_of(img, depth, c)
        it, dt = cuda(img), cuda(depth)
        k, kc = run(engine, dev_switch, it, dt, c, "gw_no_quad")
        assert kc == ["k<8,2,node>"]
        for a, b in ((k, want),):
            assert np.array_equal(np.isnan(a[0]), np.isnan(b[0])) and np.array_equal(np.isinf(a[0]), np.isinf(b[0]))
            fin = np.isfinite(b[0])
            assert np.array_equal(a[0][fin], b[0][fin])
            for j in (1, 2, 3):
                assert np.array_equal(a[j], b[j]), NAMES[j]
        assert np.isnan(want[0][0, r - 1]).any() and (~np.isfinite(want[0][0, r])).sum() >= 2
        d, dc = run(engine, dev_switch, it, dt, c, "default")
        if w % 4:
            assert dc == ["k<8,2,node>"]
            for j in range(4):
                assert np.array_equal(d[j].view(np.uint32), k[j].view(np.uint32)), NAMES[j]
            continue
        assert dc == ["q<8,2>"]
        diff = (d[0].view(np.uint32) != k[0].view(np.uint32)) & ~(np.isnan(d[0]) & np.isnan(k[0]))
        rows = np.nonzero(diff.any(axis=(2, 3))[0])[0].tolist()
        assert rows == partners, rows
        # in the partner row: exactly the pixels k_gpuwarp turns into NaN through the unweighted row, finite in k_gpuwarp_q
        assert np.array_equal(diff[0, r - 1], np.isnan(k[0][0, r - 1])), "the deviation is not confined to the zero-weight taps"
        assert np.isfinite(d[0][0, r - 1]).all()
        for j in (1, 2, 3):
            assert np.array_equal(d[j], k[j]), NAMES[j]


@pytest.mark.parametrize("seed", range(8))
def test_node_fuzz_hostile_depth(engine, dev_switch, seed):
    """Seeded node-level fuzz of gpu_warp on the hostile generators (saturated and 8-bit-noise depth, test_gpu_fuzz.make_case
    plateaus), random shapes, modes, balance, exponents and blur: the default path and k_gpuwarp (pt_variant gw_no_quad) against the oracle
    and against each other: bit-identical."""
    from test_gpu_fuzz import make_case
    rng = np.random.default_rng(7100 + seed)
    modes = ["left-right", "right-left", "top-bottom", "bottom-top", "red-cyan-anaglyph", "cyan-red-reverseanaglyph", "left-only",
             "only-right"]
    for _ in range(8):
        n, h = int(rng.integers(1, 4)), int(rng.integers(1, 7))
        w = int(rng.choice([8, 64, 200, 333, 516, 700, 1028, 1031, 1540, 2052, 3080, 4096]))
        kind = str(rng.choice(["clipped", "random8", "blobs", "stepped", "noisy_ramp", "make_case"]))
        if kind == "make_case":
            rows = [make_case(rng)[1][0] for _ in range(n)]   # one row of 0..255 levels per frame, tiled to the width
            d = np.stack([np.tile(r_, w // r_.size + 1)[:w] for r_ in rows])
            depth = np.ascontiguousarray(np.repeat(d[:, None, :], h, axis=1)[..., None]).astype(F32)
        else:
            depth = synth.depth_batch(kind, n, h, w, channels=3)
        c = C(w, h, float(rng.choice([2.0, 1.0, 0.5, 1.3, 0.0, 3.0])), kind, n=n, mode=str(rng.choice(modes)),
              bal=float(rng.choice([0.0, 0.3, -0.5, 1.0])), div=float(rng.choice([2.0, 5.0, 8.0, 12.0, -4.0])),
              sep=float(rng.choice([0.0, 0.5, -1.0])), conv=float(rng.choice([0.0, 0.5, 1.0])), blur=bool(rng.random() < 0.5),
              bs=int(rng.integers(1, 4)))
        img = synth.image_f32(n, h, w, seed=seed * 10 + w)
        want = oracle_of(img, depth, c)
        it, dt = cuda(img), cuda(depth)
        a, pa = run(engine, dev_switch, it, dt, c, "default")
        b, pb = run(engine, dev_switch, it, dt, c, "gw_no_quad")
        for got, path in ((a, pa[0]), (b, pb[0])):
            err = check_vs_oracle(got, want, (seed, case_id(c), path))
            MAX_ERR[path] = max(MAX_ERR.get(path, 0.0), err)
        assert kind_of(pb[0]) != "q", pb
        for k in range(4):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (seed, case_id(c), pa, pb, NAMES[k])


def test_report_largest_colour_difference_per_path():
    """(Runs last: prints what the tests above measured -- the largest colour difference from the oracle per path; -s shows it.)"""
    for path in sorted(MAX_ERR, key=str):
        print(f"gpu_warp path {path}: max |colour - oracle| = {MAX_ERR[path]:.3g}")
    assert all(v <= TOL for v in MAX_ERR.values())
