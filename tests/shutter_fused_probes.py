"""Probe filters of the fused motion blur's tests (tests/test_clip_shutter_fused_api.py, tests/test_gpu_clip_shutter_fused.py):
one per code path of mm_pixels_shutter's sub-sample loop."""
import numpy as np

from tests import clip_probes
from tests import filters as F

# an arithmetic-only escape loop whose constants depend on t: the ordinary kernel runs in pair mode, so the fused kernel's
# generic form is compared with pair-mode floats
PAIR = """filter escape_t ()
  ct = t * 0.5 + 0.1;
  n = 0; w = x; v = y; ca = x * 1.5 + ct; cb = y * 1.5 - ct;
  while (w * w + v * v < 4) && (n < 9) do
    tt = w * v; u = w * w - v * v + ca; v = tt + tt + cb; w = u; n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
"""
# in(xy, frame) of a sequence, at coordinates that move with t (the hot fetch in the maps path)
SEQUENCE = """filter seq_t (image in)
  in(xy * 1.2 + xy:[t * 0.3, -0.07], frame)
end
"""
# the frame constants read neither t nor frame -- one slot serves every sub-sample --, the pixel code reads t
# (t is read under a condition of the pixel's: outside one the read itself would be a frame constant)
SHARED = """filter shared_slot (image in, float k: 0-2 (0.7))
  s = sin(k * 3);
  if x > 0 then
    in(xy * s + xy:[x * t, 0])
  else
    in(xy * 0.9 - xy:[0, y * t])
  end
end
"""
# RAND: a call counter per pixel, which starts again in every sub-sample
RANDOM = """filter noisy ()
  p = rand(0, 1);
  q = rand(0, 1) * t;
  rgba:[p, q, rand(-1, 1) * x + t, 1]
end
"""
# a recursive filter function whose coordinates move with t
RECURSIVE = """filter rtree (image in, int depth: 1-16 (3))
  if depth < 2 then
    in(xy * (1 + t * 0.2))
  else
    in(xy) * 0.5 + rtree(in, depth - 1, xy * 0.8 + xy:[t * 0.1, 0]) * 0.5
  end
end
"""
# channel values out of range, negative, infinite and NaN at some pixels: the store's clamp and the float map's bits
EXTREME = """filter extreme ()
  big = exp(900 * (x + t - 0.5));
  rgba:[big, 0 - exp(900 * (y - t)), big - big, (x + y) * 3 * t]
end
"""

W, H = 97, 61
SEQ = np.random.default_rng(7).integers(0, 256, (3, H, W, 4), dtype=np.uint8)

# name -> (text, or the name of a fixture of tests/filters.py; Filter options; the frames of `in`, None: a synthetic image)
PROBES = {
    "pair": (PAIR, {}, None),
    "wave": (clip_probes.WAVE, {}, None),
    "sequence": (SEQUENCE, {}, SEQ),
    "shared": (SHARED, {}, None),
    "rand": (RANDOM, {}, None),
    "recursive": (RECURSIVE, {}, None),
    "droste": ("droste", {}, None),
    "mandelbrot": ("mandelbrot", {"specialize": True}, None),
    "extreme": (EXTREME, {}, None),
}
# filters that are not fused: the call is the maps path
BLUR = """stretched filter blur_t (stretched image in)
  b = gaussian_blur(in, 0.04 + t * 0.05, 0.05);
  b(xy)
end
"""
FALLBACKS = {"blur": (BLUR, {}, None), "closure": ("closure_timed_arg", {}, None)}
# a cheap arithmetic filter that reads t, for frames beyond 4 GiB of float map
CHEAP = "filter cheap () rgba:[x * 0.5 + 0.5 + t, y * 0.5 + 0.5 - t, x * y + t * 3, 1] end"


def compiled(name):
    import mathmap_amd as mm
    src, opts, image = PROBES[name] if name in PROBES else FALLBACKS[name]
    return (F.load(src, **opts) if src in F.NAMES else mm.Filter(src, **opts)), image


def invoke(flt, image, w=W, h=H):
    inv = flt.invoke(w, h)
    if F.image_names(flt):
        if image is None:
            inv.set_image("in", F.synthetic_image(w, h, seed=5))
        else:
            inv.set_image("in", image[:, :h, :w] if image.shape[1] >= h and image.shape[2] >= w else image)
    return inv
