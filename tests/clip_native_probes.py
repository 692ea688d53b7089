"""Filters and helpers of the native clip batches' tests (tests/test_clip_native_api.py, tests/test_gpu_clip_natives.py):
gaussian_blur calls whose arguments follow t, read by the pixel in different ways."""

# (a) the blur's own bytes are the frame (direct output), both deviations follow t
DIRECT_T = """
stretched filter direct_t (stretched image in, float s: 0-1 (0.02))
  b = gaussian_blur(in, s * (1 + t), s * (1 + 2 * t));
  b(xy)
end
"""

# (c) the blur sampled at distorted coordinates, mixed with the input
DISTORTED = """
stretched filter distorted (stretched image in, float s: 0-1 (0.02))
  b = gaussian_blur(in, s * (1 + t), s * 1.5);
  b(xy * 0.9 + xy:[0.05 * sin(t * 6), 0.02]) * 0.6 + in(xy) * 0.4
end
"""

# (d) a blur of a blur, t in both
CHAIN = """
stretched filter chain (stretched image in, float s: 0-1 (0.02))
  p = gaussian_blur(in, s * (1 + t), s);
  q = gaussian_blur(p, s, s * (1 + 2 * t));
  q(xy)
end
"""

# a chain whose two results are both read by the pixel
CHAIN_BOTH = """
stretched filter chain_both (stretched image in, float s: 0-1 (0.02))
  p = gaussian_blur(in, s * (1 + t), s);
  q = gaussian_blur(p, s, s * (1 + 2 * t));
  p(xy) * 0.5 + q(xy * 0.8) * 0.5
end
"""

# (e) a call that only some frames make
CONDITIONAL = """
stretched filter conditional (stretched image in, float s: 0-1 (0.02))
  if t > 0.5 then
    b = gaussian_blur(in, s * (1 + t), s); b(xy)
  else
    in(xy)
  end
end
"""

# (f) a call under pixel-dependent control: hoisted, made by every frame
HOISTED = """
stretched filter hoisted (stretched image in, float s: 0-1 (0.02))
  if y > t - 0.5 then
    c = gaussian_blur(in, s * 3, s * (1 + t)); c(xy) * 0.5 + in(xy) * 0.5
  else
    in(xy)
  end
end
"""

# (j) a horizontal deviation that falls below half a pixel at small t (the FIR path)
FIR_AT_ZERO = """
stretched filter fir_at_zero (stretched image in, float s: 0-1 (0.02))
  b = gaussian_blur(in, s * t, s);
  b(xy)
end
"""

# not eligible: a blur inside a loop of the frame-constant code
IN_LOOP = """
filter in_loop (image in, float s: 0-1 (0.02), int n: 0-8 (2))
  img = in; i = 0;
  while i < n do img = gaussian_blur(img, s, s * (i + 1)); i = i + 1 end;
  img(xy)
end
"""

# a plain (not stretched) filter: the canvas's aspect ratio scales its coordinates
PLAIN = """
filter plain (image in, float s: 0-1 (0.03))
  b = gaussian_blur(in, s * (1 + t), s);
  b(xy) * 0.7 + in(xy) * 0.3
end
"""


def job_bytes(w, h):
    """(checkpoint bytes, map bytes) of one blur of a w x h frame: 4 doubles per line and channel every 16 steps, the
    larger of the two passes, rounded up to 256; a float4 map."""
    ck_v = -(-h // 16) * 4 * (w * 4) * 8
    ck_h = -(-w // 16) * 4 * (h * 4) * 8
    return -(-max(ck_v, ck_h) // 256) * 256, w * h * 16


def bytes_per_frame(w, h, sites):
    ck, m = job_bytes(w, h)
    return sites * (ck + 2 * m)
