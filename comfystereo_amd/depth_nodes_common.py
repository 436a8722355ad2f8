"""What `StereoDepthStabilizer` and `StereoDepthRange` share: an instance carries a clip's state from one execution to the next,
and `reset`, another frame size or another device start a new clip.
"""
from . import stereoimage_generation


class ClipNode:
    def __init__(self):
        self._state = None
        self._key = None

    def _start_clip_if(self, key, reset):
        """reset, another frame size or another device: the next frames start a new clip."""
        if reset or key != self._key:
            self._state, self._key = None, key

    def _continue_clip(self, depth_map, reset):
        """The clip of depth_map's frame size on the device the pass will run on goes on, or a new one starts; without a GPU the
        package's RuntimeError, before anything else.  -> n, h, w of depth_map"""
        device = stereoimage_generation._device_for(depth_map)
        n, h, w = depth_map.shape[:3]
        self._start_clip_if((h, w, device), reset)
        return n, h, w
