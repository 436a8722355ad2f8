"""`StereoDepthStabilizer` -- ComfyUI node in front of the Stereo Image Node's depth input: the temporal depth filter of
stereoimage_generation.stabilize_depth (cs_temporal_depth) over the depth maps of a clip.

The reference has no counterpart: it normalises every frame alone, so the frame-to-frame flicker of a monocular depth estimator
becomes disparity jitter.  The node instance keeps the filter's state between executions, which is how a chunked video loader
feeds a long clip: every execution continues where the last one stopped, bit for bit as if the clip had come in one batch.
`reset`, another frame size or another device start a new clip.
"""
import torch

from . import stereoimage_generation
from .depth_nodes_common import ClipNode


NEVER = 1000000.0   # the widgets' largest threshold: it and anything above it is passed on as +inf


class StereoDepthStabilizer(ClipNode):
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "depth_map": ("IMAGE",),
            },
            "optional": {
                "alpha": ("FLOAT", {"default": 0.5, "min": 0.0, "max": 1.0, "step": 0.01,
                                    "tooltip": "Weight of the new frame where nothing moved: 1 keeps the input, 0 freezes it."}),
                # (both thresholds are in the units of the depth map, 0..1 from ComfyUI; NEVER and anything above it stands for
                # +inf, which a FLOAT widget cannot hold: no pixel ever counts as moved, no frame as a cut)
                "motion_threshold": ("FLOAT", {"default": 0.1, "min": 0.0, "max": NEVER, "step": 0.005,
                                               "tooltip": "A pixel that differs from its filtered value by this much or more moved: it passes unfiltered. 1000000 = never."}),
                "cut_threshold": ("FLOAT", {"default": 0.08, "min": 0.0, "max": NEVER, "step": 0.005,
                                            "tooltip": "Mean absolute frame difference above which a frame starts a new scene. 1000000 = never."}),
                "batch_size": ("INT", {"default": 16, "min": 1, "max": 64, "step": 1,
                                       "tooltip": "Frames uploaded per sub-batch."}),
                "reset": ("BOOLEAN", {"default": False, "tooltip": "Forget the earlier frames: this batch starts a new clip."}),
            }
        }

    RETURN_TYPES = ("IMAGE", "MASK")
    RETURN_NAMES = ("stabilized_depth_map", "scene_cut_mask")
    FUNCTION = "stabilize"
    CATEGORY = "image/stereo"

    def stabilize(self, depth_map, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, batch_size=16, reset=False):
        """-> (the filtered depth in depth_map's layout and on its device, a mask [N,H,W] that is 1 on every pixel of a frame the
        filter took for a scene cut -- the first frame of a clip among them -- and 0 elsewhere)."""
        n, h, w = self._continue_clip(depth_map, reset)
        motion_threshold = float("inf") if motion_threshold >= NEVER else motion_threshold
        cut_threshold = float("inf") if cut_threshold >= NEVER else cut_threshold
        cuts = []
        y, self._state = stereoimage_generation.stabilize_depth(depth_map, self._state, alpha, motion_threshold, cut_threshold,
                                                                batch_size, cuts=cuts)
        mask = torch.cat(cuts).to(torch.float32)[:, None, None].expand(n, h, w).contiguous()
        return y, mask


NODE_CLASS_MAPPINGS = {
    "StereoDepthStabilizer": StereoDepthStabilizer,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "StereoDepthStabilizer": "Stereo Depth Stabilizer",
}
