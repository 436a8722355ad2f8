"""`StereoDepthRange` -- ComfyUI node in front of the Stereo Image Node's depth input: percentile clipping of the near and far end
of the depth maps of a clip with bounds that are smoothed over time (stereoimage_generation.clip_depth_range, cs_depth_range;
DESIGN.md section 5).

The reference has no counterpart: it normalises every frame by its own extremes, so a handful of outlier pixels flatten the
scene and extremes that change from frame to frame make it pump.  The node sits behind `StereoDepthStabilizer`, whose scene-cut
mask it takes, or stands alone.  The instance keeps the two bounds between executions, which is how a chunked video loader
feeds a long clip: every execution continues where the last one stopped, bit for bit as if the clip had come in one batch.
`reset`, another frame size or another device start a new clip.
"""
import torch

from . import stereoimage_generation
from .depth_nodes_common import ClipNode


LIMIT = ("The stereo step's range equals these bounds only while a smoothed bound lies within the frame's own extremes (the "
         "ordinary case with a non-zero clip); otherwise the frame's own extreme rules, as without this node.")


class StereoDepthRange(ClipNode):
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "depth_map": ("IMAGE",),
            },
            "optional": {
                "scene_cut_mask": ("MASK", {"tooltip": "The Stereo Depth Stabilizer's second output: the bounds restart at every frame whose mask is non-zero at pixel (0, 0)."}),
                "clip_low": ("FLOAT", {"default": 0.005, "min": 0.0, "max": 0.49, "step": 0.001,
                                       "tooltip": "Fraction of the pixels below the lower bound: they are raised to it. 0 keeps the frame's minimum. " + LIMIT}),
                "clip_high": ("FLOAT", {"default": 0.005, "min": 0.0, "max": 0.49, "step": 0.001,
                                        "tooltip": "Fraction of the pixels above the upper bound: they are lowered to it. 0 keeps the frame's maximum. " + LIMIT}),
                "smoothing": ("FLOAT", {"default": 0.2, "min": 0.0, "max": 1.0, "step": 0.01,
                                        "tooltip": "Weight of a frame's own bounds against the preceding frame's: 1 takes every frame's own, 0 keeps the first frame's until a cut."}),
                "normalize": ("BOOLEAN", {"default": False, "tooltip": "Map the clamped range to 0..1."}),
                "batch_size": ("INT", {"default": 16, "min": 1, "max": 64, "step": 1,
                                       "tooltip": "Frames uploaded per sub-batch."}),
                "reset": ("BOOLEAN", {"default": False, "tooltip": "Forget the earlier frames: this batch starts a new clip."}),
            }
        }

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("clipped_depth_map",)
    FUNCTION = "clip"
    CATEGORY = "image/stereo"

    def clip(self, depth_map, scene_cut_mask=None, clip_low=0.005, clip_high=0.005, smoothing=0.2, normalize=False, batch_size=16,
             reset=False):
        """-> (the clamped depth in depth_map's layout and on its device,)."""
        n, _, _ = self._continue_clip(depth_map, reset)
        cuts = None if scene_cut_mask is None else [self._cuts_of(scene_cut_mask, n)]
        y, self._state = stereoimage_generation.clip_depth_range(depth_map, self._state, clip_low, clip_high, smoothing, normalize,
                                                                 batch_size, cuts=cuts)
        return (y,)

    @staticmethod
    def _cuts_of(mask, n):
        """MASK [N,H,W] (or [N,H,W,1]) -> int32 [N]: 1 where the frame's mask is non-zero at pixel (0, 0)."""
        if mask.dim() < 3 or mask.shape[0] != n:
            raise ValueError(f"scene_cut_mask must have one [H,W] mask per frame ({n}), got shape {tuple(mask.shape)}")
        return (mask.reshape(n, -1)[:, 0] != 0).to(torch.int32)


NODE_CLASS_MAPPINGS = {
    "StereoDepthRange": StereoDepthRange,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "StereoDepthRange": "Stereo Depth Range",
}
