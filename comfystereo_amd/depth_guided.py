"""`StereoDepthGuidedUpsample` -- ComfyUI node in front of the Stereo Image Node's depth input: joint bilateral upsampling of the
depth maps to their frames' size, guided by the frames (stereoimage_generation.upsample_depth_guided, cs_guided_depth_plan /
cs_guided_depth_apply).

The reference has no counterpart: where the depth map is smaller than the frame -- an estimator's 384 to 518 pixels against 1080p
or 4K -- it stretches the map bilinearly, every silhouette becomes a ramp several pixels wide, and the warp smears the pixels
floating on that ramp into a halo around every object.  Here the frame, which knows where the silhouettes are, decides which
low-resolution samples a pixel takes its depth from, so depth edges land on colour edges and stay one pixel wide.

Its place in the chain is last: behind `StereoDepthStabilizer` and `StereoDepthRange`, which are cheaper at the estimator's
resolution, and directly in front of the Stereo Image Node, which then finds a depth map of the frame's size and resizes nothing.
It keeps no state: every frame is upsampled on its own, stills included.
"""
from . import stereoimage_generation


class StereoDepthGuidedUpsample:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "image": ("IMAGE", {"tooltip": "The frames the depth maps belong to: the guide, and the size of the result."}),
                "depth_map": ("IMAGE", {"tooltip": "The depth maps, no larger than the frames."}),
            },
            "optional": {
                "radius": ("INT", {"default": 2, "min": 1, "max": 3, "step": 1,
                                   "tooltip": "Low-resolution samples on either side of a pixel: 2 radius + 1 taps per axis."}),
                "sigma_spatial": ("FLOAT", {"default": 1.0, "min": 0.05, "max": 8.0, "step": 0.05,
                                            "tooltip": "Width of the spatial Gaussian, in pixels of the depth map."}),
                "sigma_range": ("FLOAT", {"default": 0.1, "min": 0.005, "max": 3.0, "step": 0.005,
                                          "tooltip": "Width of the colour Gaussian, in units of the summed difference of the three 8-bit channels over 255: smaller keeps depth edges tighter on colour edges, larger approaches a plain smooth resize."}),
                "batch_size": ("INT", {"default": 16, "min": 1, "max": 64, "step": 1, "tooltip": "Frames uploaded per sub-batch."}),
            }
        }

    RETURN_TYPES = ("IMAGE",)
    RETURN_NAMES = ("upsampled_depth_map",)
    FUNCTION = "upsample"
    CATEGORY = "image/stereo"

    def upsample(self, image, depth_map, radius=2, sigma_spatial=1.0, sigma_range=0.1, batch_size=16):
        """-> (the depth at the frames' size, in depth_map's channel layout and on its device,)."""
        stereoimage_generation._device_for(image)   # (without a GPU the package's RuntimeError, before anything else)
        return (stereoimage_generation.upsample_depth_guided(image, depth_map, radius, sigma_spatial, sigma_range, batch_size),)


NODE_CLASS_MAPPINGS = {
    "StereoDepthGuidedUpsample": StereoDepthGuidedUpsample,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "StereoDepthGuidedUpsample": "Stereo Depth Guided Upsample",
}
