"""`StereoDepthStabilizerMotionPyramid` -- ComfyUI node in front of the Stereo Image Node's depth input: the motion-compensated
temporal depth filter of `StereoDepthStabilizerMotion` with a wide-range, coarse-to-fine motion search
(stereoimage_generation.stabilize_depth_motion_pyramid, cs_motion_depth_pyramid).

The other node's full search stops at 32 pixels per frame, 0.8 % of a 4K frame's width: a pan or a fast object moves further, its
blocks come back unmatched and pass unfiltered.  This node searches a three-level pyramid of the colour frames' luma: a full search
over search_range / 4 on the quarter-size plane, then a few candidates per block on the half- and the full-size plane, so that the
vectors reach search_range + 3 pixels.

Limits: the motion is integer-pel with one vector per 16 x 16 block; nothing regularises the vector field beyond `smoothness`; the
motion is found at the depth map's resolution; search_range is a multiple of 4 in 4..120; a coarse-to-fine search follows what the
coarse levels found and can miss a vector that the full search of the same range would find, small objects that vanish at quarter
size above all.  The defaults of search_range, smoothness and match_threshold are starting values that nobody has tuned on
footage.

The node instance keeps the filter's state between executions, like `StereoDepthStabilizerMotion`: `reset`, another frame size or
another device start a new clip.
"""
import torch

from . import stereoimage_generation
from .depth_nodes_common import ClipNode
from .depth_stabilizer import NEVER
from .depth_stabilizer_motion import UNTUNED, StereoDepthStabilizerMotion


class StereoDepthStabilizerMotionPyramid(ClipNode):
    @classmethod
    def INPUT_TYPES(cls):
        types = StereoDepthStabilizerMotion.INPUT_TYPES()   # (a new dictionary per call)
        types["optional"]["search_range"] = ("INT", {"default": 64, "min": 4, "max": 120, "step": 4,
                                                     "tooltip": "Largest motion per frame, in pixels of the depth map, on either axis (the vectors reach 3 more). A multiple of 4." + UNTUNED})
        return types

    RETURN_TYPES = ("IMAGE", "MASK", "MASK")
    RETURN_NAMES = ("stabilized_depth_map", "scene_cut_mask", "unmatched_mask")
    FUNCTION = "stabilize"
    CATEGORY = "image/stereo"

    def stabilize(self, depth_map, image, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=64, smoothness=32,
                  match_threshold=12, batch_size=16, reset=False):
        """-> (the filtered depth in depth_map's layout and on its device, a mask [N,H,W] that is 1 on every pixel of a frame the
        filter took for a scene cut, a mask [N,H,W] that is 1 on every pixel of a block that found no match)."""
        n, h, w = self._continue_clip(depth_map, reset)
        motion_threshold = float("inf") if motion_threshold >= NEVER else motion_threshold
        cut_threshold = float("inf") if cut_threshold >= NEVER else cut_threshold
        cuts, unmatched = [], []
        y, self._state = stereoimage_generation.stabilize_depth_motion_pyramid(depth_map, image, self._state, alpha, motion_threshold,
                                                                               cut_threshold, search_range, smoothness, match_threshold,
                                                                               batch_size, cuts=cuts, unmatched=unmatched)
        cut_mask = torch.cat(cuts).to(torch.float32)[:, None, None].expand(n, h, w).contiguous()
        blocks = torch.cat(unmatched).to(torch.float32)
        un_mask = blocks.repeat_interleave(16, dim=1).repeat_interleave(16, dim=2)[:, :h, :w].contiguous()
        return y, cut_mask, un_mask


NODE_CLASS_MAPPINGS = {
    "StereoDepthStabilizerMotionPyramid": StereoDepthStabilizerMotionPyramid,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "StereoDepthStabilizerMotionPyramid": "Stereo Depth Stabilizer (motion compensated, wide range)",
}
