"""The gray depth of a frame is one map for every depth pre-pass (csrc/cs_gray4.h): the temporal filter and the range clipping,
each set so that it returns the gray depth itself, give the same bits on either access path and for every treatment of C, and those
are the bits of tools/temporal_oracle.py's gray on the host.  Nothing here has a tolerance.

  temporal_depth, alpha = 1, both thresholds +inf, no state: frame 0 has no predecessor and passes; frame 1 is y0 + 1 * (g1 - y0),
      which is g1 exactly where g1 - y0 is exact.  The input lies in [0.5, 1), so every gray value lies in [0.4999, 1) (the three
      weights sum to 0.9999), any two within a factor of two of each other: the difference is exact (Sterbenz).
  depth_range, clip_low = clip_high = 0, beta = 1, no cut, no normalize, no state: the bounds are the frame's own extremes and the
      clamp to them changes nothing."""
import os
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import temporal_oracle as oracle   # noqa: E402

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.mark.parametrize("h, w, c, offset", [
    (8, 64, 1, 0), (8, 64, 3, 0),      # h * w % 4 == 0 on the 16-byte grid: the 16-byte path
    (5, 67, 3, 0),                     # h * w % 4 != 0: the guarded path, with a tail lane
    (7, 64, 2, 0),                     # neither 1 nor 3 channels: channel 0
    (8, 64, 3, 1),                     # one float off the 16-byte grid: the guarded path on a size the 16-byte path takes
], ids=["8x64_c1", "8x64_c3", "5x67_c3", "7x64_c2", "8x64_c3_off16"])
def test_the_temporal_filter_and_the_range_clipping_read_the_same_gray_depth(h, w, c, offset):
    host = np.random.RandomState(h * w + c).uniform(0.5, 1.0, (2, h, w, c)).astype(np.float32)
    assert np.isfinite(host).all() and host.min() >= 0.5 and host.max() < 1.0 and len(np.unique(host)) > h * w
    flat = torch.empty(host.size + offset, dtype=torch.float32, device="cuda")
    depth = flat[offset:].view(host.shape)
    depth.copy_(torch.from_numpy(host))
    assert depth.is_contiguous() and depth.data_ptr() % 16 == 4 * offset
    y_temporal = engine.temporal_depth(depth, None, 1.0, INF, INF)[0].cpu().numpy()
    y_range = engine.depth_range(depth, None, 0.0, 0.0, 1.0, None, False)[0].cpu().numpy()
    gray = oracle.gray(host)
    assert y_temporal.shape == y_range.shape == gray.shape == (2, h, w)
    assert np.array_equal(y_temporal.view(np.uint32), y_range.view(np.uint32))
    assert np.array_equal(y_temporal.view(np.uint32), gray.view(np.uint32))
