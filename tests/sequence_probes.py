"""Probe filters for multi-frame input drawables (tests/test_image_sequence_api.py, tests/test_gpu_image_sequence.py).

Each text has `{F}` where a fetch's frame number goes, so that one filter can be compiled as written (the GPU's side),
with a literal in its place (the oracle's side: it binds one frame per image and only range-checks the number), or with
the expression moved into a channel (the index map of a pixel-dependent frame number).  The coordinates are affine in
xy -- no libm --, so the GPU's arithmetic is the oracle's and every comparison is byte for byte.
"""

# one fetch, reaching outside the image on every side (edge behaviour / edge colours take part)
SELECT = """
filter seq_select (image in, float n: 0-16 (0))
  in(xy * 1.3 + xy:[0.11, -0.07], {F})
end
"""
FRAME_OF_ANIMATION = "frame"          # in(xy, frame)
FRAME_OF_USERVAL = "n - 8"            # in(xy, n): the tests pass n + 8, so that -1 is reachable inside the declared range

# plain in(xy): lowers to ORIG_VAL(x, y, in, t)
PLAIN = """
filter seq_plain (image in)
  in(xy * 1.3 + xy:[0.11, -0.07])
end
"""

# slit-scan: the frame number differs from pixel to pixel.  off - 8 shifts it (fractional and negative values: -0.5 must
# read frame 0), k stretches it beyond K, big makes it huge away from the centre column, and the square root of a negative number is
# NaN: on the centre row of a frame of odd height, where y = 0 (the language's own division returns 0 for 0 / 0).
SLIT = """
filter seq_slit (image in, float off: 0-16 (8), float k: 0-16 (1.75), float big: 0-1 (0))
  in(xy * 1.3 + xy:[0.11, -0.07], {F})
end
"""
SLIT_FRAME = "off - 8 + k * (x + 1) + big * x * 10000000.0 * 10000000.0 + 0 * sqrt(abs(y) - 0.0001)"
# the same expression as a channel: rendered as a float map it is the index map
SLIT_INDEX = """
filter seq_slit_index (image in, float off: 0-16 (8), float k: 0-16 (1.75), float big: 0-1 (0))
  rgba:[%s, 0, 0, 1]
end
""" % SLIT_FRAME

# three fetches of one image at three frame-constant frames
BLEND = """
filter seq_blend (image in)
  (in(xy * 0.9, frame - 1) + in(xy * 0.9, frame) + in(xy * 0.9, frame + 1)) / 3
end
"""
# what the oracle can render of it: three images of one frame each, each fetch with a literal frame number -- 0, or a
# number out of range where the sequence has no such frame (an unbound image would not do: it is not what a drawable
# without that frame reads as)
BLEND_ORACLE = """
filter seq_blend3 (image a, image b, image c)
  (a(xy * 0.9, {A}) + b(xy * 0.9, {B}) + c(xy * 0.9, {C})) / 3
end
"""

# a fetch with a frame argument inside a recursive filter function (a run-time call of filter_seq_tree)
RECURSIVE = """
filter seq_tree (image in, int depth: 1-16 (3), float n: 0-16 (0))
  if depth < 2 then
    in(xy, {F})
  else
    in(xy, {F}) * 0.5 + seq_tree(in, depth - 1, n, xy * 0.8) * 0.5
  end
end
"""
# ... and inside a closure handed to gaussian_blur
CLOSURE = """
filter seq_inner (image in, float n: 0-16 (0))
  in(xy * 1.1, {F})
end

filter seq_blur_of_closure (image in, float n: 0-16 (0))
  b = gaussian_blur(seq_inner(in, n), 0.02, 0.02);
  b(xy)
end
"""
# native consumers of the drawable itself: frame 0, whatever t and frame are
BLUR = """
filter seq_blur (image in)
  b = gaussian_blur(in, 0.02, 0.03);
  b(xy * 0.9)
end
"""
RENDER = """
filter seq_render (image in)
  whole = render(in);
  whole(xy * 0.9)
end
"""


def _large_body(last):
    """A body past the generator's own limit for the unrolled loop (pixel_stats > 400 statements): it gets the large-body
    kernel, one pixel per work-item, whose fetches are the early-exit ones.  150 steps of a contraction, exact in float
    on both sides."""
    lines = ["filter seq_large (image in, float off: 0-16 (8), float k: 0-16 (1.75), float big: 0-1 (0))", "  a0 = x;"]
    lines += ["  a%d = a%d * 0.5 + %d * y * 0.0001;" % (i, i - 1, i % 7) for i in range(1, 150)]
    return "\n".join(lines + [last, "end"]) + "\n"


LARGE = _large_body("  in(xy * 1.3 + xy:[a149 * 0.01, -0.07], {F})")
LARGE_FRAME = "off - 8 + k * (x + 1) + a149 * 0.001 + 0 * sqrt(abs(y) - 0.0001)"
LARGE_INDEX = _large_body("  rgba:[%s, 0, 0, 1]" % LARGE_FRAME)


def text(template, frame):
    return template.replace("{F}", "(%s)" % frame)
