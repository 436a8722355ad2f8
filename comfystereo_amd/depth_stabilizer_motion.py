"""`StereoDepthStabilizerMotion` -- ComfyUI node in front of the Stereo Image Node's depth input: the motion-compensated temporal
depth filter of stereoimage_generation.stabilize_depth_motion (cs_motion_depth) over the depth maps of a clip.

`StereoDepthStabilizer` reads the filter's state at the pixel itself, so whatever moved by more than a pixel or two -- the walking
person, the panned background, every silhouette of a moving object -- passes unfiltered.  This node reads it where the pixel's
16 x 16 block came from, found on the clip's colour frames by a full-search block matcher, and so filters moving content as well.
Where a block finds no match it passes unfiltered, which is the other node's behaviour.

Limits: the motion is integer-pel with one vector per 16 x 16 block; nothing regularises the vector field beyond `smoothness`; the
motion is found at the depth map's resolution.  The defaults of search_range, smoothness and match_threshold are starting values
that nobody has tuned on footage.

The node instance keeps the filter's state between executions, like `StereoDepthStabilizer`: `reset`, another frame size or
another device start a new clip.
"""
import torch

from . import stereoimage_generation
from .depth_nodes_common import ClipNode
from .depth_stabilizer import NEVER


UNTUNED = " The default is a starting value, not tuned on footage."


class StereoDepthStabilizerMotion(ClipNode):
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "depth_map": ("IMAGE",),
                "image": ("IMAGE", {"tooltip": "The frames the depth maps belong to: the motion is found on them. Another size than the depth maps' is resized to it."}),
            },
            "optional": {
                "alpha": ("FLOAT", {"default": 0.5, "min": 0.0, "max": 1.0, "step": 0.01,
                                    "tooltip": "Weight of the new frame where the filter applies: 1 keeps the input, 0 freezes it."}),
                "motion_threshold": ("FLOAT", {"default": 0.1, "min": 0.0, "max": NEVER, "step": 0.005,
                                               "tooltip": "A pixel that differs from the filtered value of the place it came from by this much or more passes unfiltered. 1000000 = never."}),
                "cut_threshold": ("FLOAT", {"default": 0.08, "min": 0.0, "max": NEVER, "step": 0.005,
                                            "tooltip": "Mean absolute frame difference above which a frame starts a new scene. 1000000 = never."}),
                "search_range": ("INT", {"default": 16, "min": 0, "max": 32, "step": 1,
                                         "tooltip": "Largest motion per frame, in pixels of the depth map, on either axis. 0 = no motion search." + UNTUNED}),
                "smoothness": ("INT", {"default": 32, "min": 0, "max": 4096, "step": 1,
                                       "tooltip": "Penalty per pixel of vector length, in units of summed 8-bit luma difference over a block: larger prefers short vectors." + UNTUNED}),
                "match_threshold": ("INT", {"default": 12, "min": 0, "max": 255, "step": 1,
                                            "tooltip": "Mean 8-bit luma difference per pixel above which a block counts as unmatched and passes unfiltered." + UNTUNED}),
                "batch_size": ("INT", {"default": 16, "min": 1, "max": 64, "step": 1,
                                       "tooltip": "Frames uploaded per sub-batch."}),
                "reset": ("BOOLEAN", {"default": False, "tooltip": "Forget the earlier frames: this batch starts a new clip."}),
            }
        }

    RETURN_TYPES = ("IMAGE", "MASK", "MASK")
    RETURN_NAMES = ("stabilized_depth_map", "scene_cut_mask", "unmatched_mask")
    FUNCTION = "stabilize"
    CATEGORY = "image/stereo"

    def stabilize(self, depth_map, image, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=16, smoothness=32,
                  match_threshold=12, batch_size=16, reset=False):
        """-> (the filtered depth in depth_map's layout and on its device, a mask [N,H,W] that is 1 on every pixel of a frame the
        filter took for a scene cut, a mask [N,H,W] that is 1 on every pixel of a block that found no match)."""
        n, h, w = self._continue_clip(depth_map, reset)
        motion_threshold = float("inf") if motion_threshold >= NEVER else motion_threshold
        cut_threshold = float("inf") if cut_threshold >= NEVER else cut_threshold
        cuts, unmatched = [], []
        y, self._state = stereoimage_generation.stabilize_depth_motion(depth_map, image, self._state, alpha, motion_threshold, cut_threshold,
                                                                       search_range, smoothness, match_threshold, batch_size, cuts=cuts,
                                                                       unmatched=unmatched)
        cut_mask = torch.cat(cuts).to(torch.float32)[:, None, None].expand(n, h, w).contiguous()
        blocks = torch.cat(unmatched).to(torch.float32)
        un_mask = blocks.repeat_interleave(16, dim=1).repeat_interleave(16, dim=2)[:, :h, :w].contiguous()
        return y, cut_mask, un_mask


NODE_CLASS_MAPPINGS = {
    "StereoDepthStabilizerMotion": StereoDepthStabilizerMotion,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "StereoDepthStabilizerMotion": "Stereo Depth Stabilizer (motion compensated)",
}
