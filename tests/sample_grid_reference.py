"""A NumPy restatement of the grid-supersampled clip (mmhip_render_clip_sampled, include/mmhip.h): the sampling offsets of
the grid, the order of a frame's K * sx * sy sub-samples, and their mean -- tests/shutter_reference.py's, over all of
them.  It shares no code with the library.  (tests/test_clip_sampled_api.py, tests/test_gpu_clip_sampled.py)"""
import numpy as np

from tests import shutter_reference as R

f32, f64 = np.float32, np.float64


def grid(aa):
    """(sx, sy) of render_clip's `aa`: an int n is (n, n)."""
    return (aa, aa) if isinstance(aa, int) else tuple(aa)


def offsets(n):
    """float32 [n]: o_a = (float)(((double)a + 0.5) / (double)n - 0.5)."""
    return np.array([f32((f64(a) + f64(0.5)) / f64(n) - f64(0.5)) for a in range(n)], f32)


def order(samples, sx, sy):
    """The (j, b, a) of sub-sample s = j * (sx * sy) + b * sx + a, for s = 0 .. K * sx * sy - 1: a runs fastest."""
    out = [(j, b, a) for j in range(samples) for b in range(sy) for a in range(sx)]
    for s, (j, b, a) in enumerate(out):
        assert s == j * sx * sy + b * sx + a
    return out


def combine(maps, bpp=4, floatmap=False):
    """One frame from its sub-sample maps float32 [K, sy, sx, ..., 4], summed in the order above."""
    maps = np.asarray(maps, f32)
    k, sy, sx = maps.shape[:3]
    flat = np.stack([maps[j, b, a] for j, b, a in order(k, sx, sy)])
    return R.combine(flat, bpp=bpp, floatmap=floatmap)
