"""`StereoDepthEdgeDilate` -- ComfyUI node in front of the Stereo Image Node's depth input: foreground depth edge dilation
(stereoimage_generation.dilate_depth_edges, cs_depth_dilate).

The reference has no counterpart.  A frame's silhouettes are anti-aliased: the outermost one to three pixels of an object are
mixtures of foreground and background colour.  A depth edge that sits exactly on the colour edge gives half of those mixed pixels
the background's depth; the warp leaves them behind, a thin outline of the object stays on the background beside every
disocclusion, and the hole fill stretches it.  The node grows the near surface outward by a few pixels, and only where the depth
jumps: smooth slopes pass bit for bit.

Its place in the chain is last: behind `StereoDepthStabilizer`, `StereoDepthRange` and `StereoDepthGuidedUpsample`, at the frame's
resolution and directly in front of the Stereo Image Node -- the upsampler puts depth edges on colour edges one pixel wide, this
node moves them to the outside of the anti-aliased rim.  It keeps no state: every frame is treated on its own, stills included.
"""
from . import stereoimage_generation


class StereoDepthEdgeDilate:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "depth_map": ("IMAGE", {"tooltip": "The depth maps at the frames' resolution: the last step of the chain, behind the guided upsampler and directly in front of the Stereo Image Node."}),
            },
            "optional": {
                "radius": ("INT", {"default": 2, "min": 1, "max": 8, "step": 1,
                                   "tooltip": "Pixels by which the near surface grows: the width of the frames' anti-aliased rim, 1 to 3 at most resolutions."}),
                "shape": (["disc", "square"], {"default": "disc", "tooltip": "The window: a disc grows silhouettes evenly in every direction, a square is a little cheaper and grows corners further."}),
                "near": (["bright", "dark"], {"default": "bright", "tooltip": "Which values are near the camera: bright for ComfyUI's depth maps, dark for inverted ones."}),
                "threshold": ("FLOAT", {"default": 0.04, "min": 0.0, "max": 1.0, "step": 0.005,
                                        "tooltip": "A pixel takes the nearest depth of its window only where that lies at least this far in front of it. Depth is 0..1, 0.04 is about ten 8-bit levels: smooth slopes stay untouched, silhouettes move. 0 dilates everything."}),
                "batch_size": ("INT", {"default": 16, "min": 1, "max": 64, "step": 1, "tooltip": "Frames uploaded per sub-batch."}),
            }
        }

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("dilated_depth_map",)
    FUNCTION = "dilate"
    CATEGORY = "image/stereo"

    def dilate(self, depth_map, radius=2, shape="disc", near="bright", threshold=0.04, batch_size=16):
        """-> (the dilated depth, in depth_map's channel layout and on its device,)."""
        stereoimage_generation._device_for(depth_map)   # (without a GPU the package's RuntimeError, before anything else)
        return (stereoimage_generation.dilate_depth_edges(depth_map, radius, shape, near, threshold, batch_size),)


NODE_CLASS_MAPPINGS = {
    "StereoDepthEdgeDilate": StereoDepthEdgeDilate,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "StereoDepthEdgeDilate": "Stereo Depth Edge Dilate",
}
