"""numpy restatements of the image fetch and the pixel output: apply_edge_behaviour, get_pixel, get_orig_val_pixel,
get_orig_val_intersample_pixel, get_floatmap_pixel and render_image's drawable branch (builtins/builtins.c:40-346), the
resize wrapper (compiler.c:1715-1773, opmacros.h:199-216) and calc_lines' store (new_template.c.in:279-293).  A helper:
no tests in here.

Written from the reference's sources, not from the oracle (oracle/mm_oracle_rt.c) or the device code (mm_device.h,
native_filters.hip), and pinned against the oracle by tests/test_fetch_reference.py.  Every operation is rounded as the
C source rounds it: float32 where both operands are float, float64 where a double constant takes part, then back.

The fetches take *coordinate arrays*: float32, the filter's p[0] and p[1] of `in(p)`, one element per pixel.  They return
(float32 [.., 4], covered): `covered` is False where a pixel coordinate is NaN or infinite or its magnitude reaches
2**31 px (2**30 px with a stride) -- there the reference's int conversions are x86's and the sums are no weights of
anything; those pixels are left to the comparison with the oracle (test_nan_and_huge_coordinates_follow_x86_conversion).
Images are uint8 [h, w, 4] or, as a sequence of frames, [n, h, w, 4]; colours are 0xRRGGBBAA like the reference's color_t.
"""
import numpy as np

EDGE_COLOR, EDGE_WRAP, EDGE_REFLECT, EDGE_ROTATE = range(4)
EDGE_PAIRS = [(ex, ey) for ex in range(4) for ey in range(4)]
EDGE_COLOURS = (0x20406080, 0xC0A01055)            # what the tests set: no channel equal to another, none 0 or 255
WHITE = 0xFFFFFFFF
INT_MIN = -2 ** 31

f32, f64 = np.float32, np.float64


def _quiet(fn):
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def _wrap32(v):
    """An int64 array as 32-bit two's complement: what `int` arithmetic leaves on x86."""
    return ((np.asarray(v, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def _c_mod(a, n):
    """C's `%` on ints: the quotient truncates, the result has the dividend's sign."""
    return np.fmod(np.asarray(a, np.int64), np.int64(n))


def _neg32(a):
    """-x on an int: INT_MIN stays INT_MIN."""
    return _wrap32(-np.asarray(a, np.int64))


@_quiet
def _cvtt(d):
    """(int) of a double as cvttsd2si converts it: truncation, and INT_MIN for NaN and whatever does not fit."""
    d = np.asarray(d, f64)
    ok = np.isfinite(d) & (d > -2147483649.0) & (d < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, d, 0.0)), float(INT_MIN)).astype(np.int64)


def resize_factors(pw, ph, flags):
    """resize_image_if_necessary (compiler.c:1715-1773): the factors ORIG_VAL multiplies the coordinates by
    (opmacros.h:203-207), or None where the image gets no wrapper.  `flags`: "default" (`image in`: unit and square,
    max(pw, ph) / pw and max(pw, ph) / ph), "stretched" (unit only: no wrapper) or "pixel" (2 / pw, 2 / ph).  DIV is
    (float)a / (float)b (opmacros.h:41): float quotients."""
    if flags == "stretched":
        return None
    if flags == "pixel":
        return f32(f32(2) / f32(pw)), f32(f32(2) / f32(ph))
    assert flags == "default", flags
    m = max(pw, ph)
    return f32(f32(m) / f32(pw)), f32(f32(m) / f32(ph))


@_quiet
def apply_factors(x, y, factors):
    """ORIG_VAL's `x *= x_factor; y *= y_factor` (opmacros.h:203-207): float products."""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    if factors is None:
        return x, y
    return x * f32(factors[0]), y * f32(factors[1])


@_quiet
def drawable_transform(x, y, w, h):
    """get_image_drawable (builtins.c:142-143) with calc_image_values' scales (userval.c:272-276): middle = 1.0,
    scale = (float)((n - 1) / 2.0); x = (x + middle_x) * scale_x, y = -((y - middle_y) * scale_y), all float."""
    sx, sy = f32((w - 1) / 2.0), f32((h - 1) / 2.0)
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    return (x + f32(1.0)) * sx, -((y - f32(1.0)) * sy)


def apply_edge_behaviour(x, y, width, height, edge):
    """builtins.c:40-119 on int arrays (int64 holding 32-bit values): C's `%`, negation and subtraction that wrap.  The
    x switch runs first and ROTATE mirrors the other axis, which the y switch then sees."""
    x, y = _wrap32(x), _wrap32(y)
    ex, ey = edge
    lo, hi = x < 0, x >= width
    if ex == EDGE_WRAP:
        x = np.where(lo, _c_mod(x, width) + width, np.where(hi, _c_mod(x, width), x))
    elif ex in (EDGE_REFLECT, EDGE_ROTATE):
        x = np.where(lo, _c_mod(_neg32(x), width), np.where(hi, (width - 1) - _c_mod(x, width), x))
        if ex == EDGE_ROTATE:
            y = np.where(lo | hi, _wrap32((height - 1) - y), y)
    lo, hi = y < 0, y >= height
    if ey == EDGE_WRAP:
        y = np.where(lo, _c_mod(y, height) + height, np.where(hi, _c_mod(y, height), y))
    elif ey in (EDGE_REFLECT, EDGE_ROTATE):
        y = np.where(lo, _c_mod(_neg32(y), height), np.where(hi, (height - 1) - _c_mod(y, height), y))
        if ey == EDGE_ROTATE:
            x = np.where(lo | hi, _wrap32((width - 1) - x), x)
    return x, y


def _colour_bytes(c):
    return np.array([(c >> 24) & 0xff, (c >> 16) & 0xff, (c >> 8) & 0xff, c & 0xff], np.uint8)


def get_pixel(frames, x, y, frame, edge, colours):
    """get_pixel (builtins.c:121-130) -> mathmap.c:1195-1209 -> cmdline_mathmap_get_pixel (mathmap_cmdline.c:131-184):
    the edge behaviour, then x outside -> edge colour x, y outside -> edge colour y, and only then a frame number
    outside [0, N) -> white.  Returns the colour's four bytes, uint8 [.., 4].  `frame`: an int or an int array."""
    frames = np.asarray(frames, np.uint8)
    if frames.ndim == 3:
        frames = frames[None]
    n, h, w, _ = frames.shape
    x, y = apply_edge_behaviour(x, y, w, h, edge)
    frame = np.broadcast_to(np.asarray(frame, np.int64), x.shape)
    out_x, out_y = (x < 0) | (x >= w), (y < 0) | (y >= h)
    bad_frame = (frame < 0) | (frame >= n)
    inside = ~(out_x | out_y | bad_frame)
    px = frames[np.where(inside, frame, 0), np.where(inside, y, 0), np.where(inside, x, 0)]
    px = np.where(bad_frame[..., None], _colour_bytes(WHITE), px)
    px = np.where(out_y[..., None], _colour_bytes(colours[1]), px)
    px = np.where(out_x[..., None], _colour_bytes(colours[0]), px)
    return px.astype(np.uint8)


@_quiet
def _tuple_from_bytes(b):
    """TUPLE_FROM_COLOR (opmacros.h:176-181): byte / 255.0 in double, stored as float."""
    return (np.asarray(b, f64) / 255.0).astype(f32)


@_quiet
def _covered(limit, *coords):
    ok = np.ones(np.shape(coords[0]), bool)
    for c in coords:
        ok &= np.isfinite(c) & (np.abs(np.asarray(c, f64)) < limit)
    return ok


@_quiet
def fetch_nearest(frames, x, y, edge, colours, factors=None, frame=0, supersampling=False):
    """get_orig_val_pixel (builtins.c:148-161) behind ORIG_VAL: `x += 0.5` adds in double and rounds back to float
    (left out under supersampling), floor in double, (int) like cvttsd2si."""
    frames = np.asarray(frames, np.uint8)
    h, w = frames.shape[-3], frames.shape[-2]
    x, y = drawable_transform(*apply_factors(x, y, factors), w, h)
    ok = _covered(2.0 ** 31, x, y)
    if not supersampling:
        x, y = (x.astype(f64) + 0.5).astype(f32), (y.astype(f64) + 0.5).astype(f32)
        ok &= _covered(2.0 ** 31, x, y)
    px = get_pixel(frames, _cvtt(np.floor(x.astype(f64))), _cvtt(np.floor(y.astype(f64))), frame, edge, colours)
    return _tuple_from_bytes(px), ok


@_quiet
def _taps(v, pixel_inc):
    """builtins.c:186-218 on one axis: (v1, v2, v2fact)."""
    if pixel_inc > 1:
        v = (v.astype(f64) - pixel_inc / 2.0).astype(f32)                   # x -= pixel_inc_x / 2.0
        v1 = _cvtt(np.floor((v / f32(pixel_inc)).astype(f64)) * float(pixel_inc))   # floor(x / inc) * inc: float quotient, double after
        v2 = _wrap32(v1 + pixel_inc)
        fact = (v - v1.astype(f32)) / f32(pixel_inc)
    else:
        v1 = _cvtt(np.floor(v.astype(f64)))
        v2 = _wrap32(v1 + 1)
        fact = v - v1.astype(f32)
    return v, v1, v2, fact


@_quiet
def fetch_bilinear(frames, x, y, edge, colours, factors=None, frame=0, pixel_inc=1):
    """get_orig_val_intersample_pixel (builtins.c:163-245) behind ORIG_VAL, operation for operation: `1.0 - x2fact` in
    double and rounded to float, the four weight products, the four channel products (unsigned * float) and the three
    sums in float in the source's order, rintf (ties to even), (color_t) & 0xff, TUPLE_FROM_COLOR."""
    frames = np.asarray(frames, np.uint8)
    h, w = frames.shape[-3], frames.shape[-2]
    x, y = drawable_transform(*apply_factors(x, y, factors), w, h)
    ok = _covered(2.0 ** 31 if pixel_inc <= 1 else 2.0 ** 30, x, y)
    x, x1, x2, x2fact = _taps(x, pixel_inc)
    y, y1, y2, y2fact = _taps(y, pixel_inc)
    ok &= _covered(2.0 ** 31 if pixel_inc <= 1 else 2.0 ** 30, x, y)
    x1fact, y1fact = (1.0 - x2fact.astype(f64)).astype(f32), (1.0 - y2fact.astype(f64)).astype(f32)
    facts = (x1fact * y1fact, x1fact * y2fact, x2fact * y1fact, x2fact * y2fact)
    taps = ((x1, y1), (x1, y2), (x2, y1), (x2, y2))
    total = None
    for (tx, ty), fact in zip(taps, facts):
        term = get_pixel(frames, tx, ty, frame, edge, colours).astype(f32) * fact[..., None]
        total = term if total is None else total + term
    rounded = np.rint(total)
    byte = np.where(ok[..., None], rounded, 0.0).astype(np.int64) & 0xff      # (-0.0 is byte 0)
    return _tuple_from_bytes(byte), ok


@_quiet
def floatmap_coefficients(w, h):
    """floatmap_alloc (floatmap.c:39-41): ax = bx = (float)(w - 1) / 2.0, by likewise, ay = by * -1.0 -- (ax, bx, ay, by)."""
    ax = f32(f64(f32(w - 1)) / 2.0)
    by = f32(f64(f32(h - 1)) / 2.0)
    return ax, ax, f32(f64(by) * -1.0), by


@_quiet
def float_map_of(image, W, H, edge, colours, factors=None, supersampling=False):
    """render_image's drawable branch (builtins.c:303-343): the W x H float map of an input drawable, each pixel
    ORIG_VAL(((float)x - bx) / ax, ((float)y - by) / ay, image, 0.0) with the *nearest* fetch whatever the invocation
    samples with (builtins.c:306).  A map one pixel wide or high divides by ax = 0: not covered."""
    ax, bx, ay, by = floatmap_coefficients(W, H)
    fx = (np.arange(W, dtype=f32) - bx) / ax
    fy = (np.arange(H, dtype=f32) - by) / ay
    fx, fy = np.broadcast_to(fx[None, :], (H, W)), np.broadcast_to(fy[:, None], (H, W))
    m, ok = fetch_nearest(image, fx, fy, edge, colours, factors=factors, supersampling=supersampling)
    return m, ok & np.isfinite(fx) & np.isfinite(fy)


@_quiet
def float_map_fetch(fmap, x, y, factors=None):
    """get_floatmap_pixel (builtins.c:247-265) behind ORIG_VAL: ix = (int)lrintf(ax * x + bx), a float product and sum,
    ties to even; black outside the map, no edge behaviour.  Not covered where ax * x + bx is not finite or reaches
    2**31 in magnitude (lrintf's long, cut to an int, is x86's there)."""
    fmap = np.asarray(fmap, f32)
    h, w = fmap.shape[:2]
    ax, bx, ay, by = floatmap_coefficients(w, h)
    x, y = apply_factors(x, y, factors)
    vx, vy = ax * x + bx, ay * y + by
    ok = _covered(2.0 ** 31, vx, vy)
    ix = np.rint(np.where(ok, vx, -1.0)).astype(np.int64)
    iy = np.rint(np.where(ok, vy, -1.0)).astype(np.int64)
    inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    out = np.where(inside[..., None], fmap[np.where(inside, iy, 0), np.where(inside, ix, 0)], f32(0.0))
    return out.astype(f32), ok


def clamp01(v):
    """CLAMP01 (opmacros.h:128, MAX(0, MIN(1, x))) as the store sees it: NaN ends up as byte 0, like 0 does."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), f32(0.0), np.minimum(np.maximum(v, f32(0.0)), f32(1.0))).astype(f32)


def grey_double(r, g, b):
    """new_template.c.in:282-284: (r * 0.299 + g * 0.587 + b * 0.114) * 255.0 in double, left to right."""
    r, g, b = (clamp01(c).astype(f64) for c in (r, g, b))
    return (r * 0.299 + g * 0.587 + b * 0.114) * 255.0


def grey_float32(r, g, b):
    """The same sum with every product and sum rounded to float32: what the store must *not* compute."""
    r, g, b = (clamp01(c) for c in (r, g, b))
    return (r * f32(0.299) + g * f32(0.587) + b * f32(0.114)) * f32(255.0)


def pack(fmap, bpp):
    """calc_lines' store (new_template.c.in:279-293) of a float map: uint8 [h, w, bpp].  Products in double, the
    conversion to unsigned char truncates; grey for bpp 1 and 2, alpha at bpp - 1 for bpp 2 and 4."""
    fmap = np.asarray(fmap, f32)
    out = np.empty(fmap.shape[:-1] + (bpp,), np.uint8)
    if bpp in (1, 2):
        out[..., 0] = np.trunc(grey_double(fmap[..., 0], fmap[..., 1], fmap[..., 2])).astype(np.uint8)
    else:
        for c in range(3):
            out[..., c] = np.trunc(clamp01(fmap[..., c]).astype(f64) * 255.0).astype(np.uint8)
    if bpp in (2, 4):
        out[..., bpp - 1] = np.trunc(clamp01(fmap[..., 3]).astype(f64) * 255.0).astype(np.uint8)
    return out


# ---- probes and the case table (shared by tests/test_fetch_reference.py and tests/test_gpu_fetch.py) ---------------------

_UV = ", ".join("float %s: -1000000000-1000000000 (%d)" % (n, d) for n, d in (("sx", 1), ("sy", 1), ("ox", 0), ("oy", 0)))
_P = "xy:[x * sx + ox, y * sy + oy]"

# The map is affine in the filter's x and y and comes in as user values, so one compiled kernel serves every image size
# and every map.  COORDS renders the same expressions (and x, y themselves) as a float map: the coordinate arrays.
COORDS = {False: "filter fetch_coords (%s)\n  rgba:[x * sx + ox, y * sy + oy, x, y]\nend\n" % _UV,
          True: "stretched filter fetch_coords_stretched (%s)\n  rgba:[x * sx + ox, y * sy + oy, x, y]\nend\n" % _UV}     # [stretched filter?]
FETCH = {"default": "filter fetch_default (image in, %s)\n  in(%s)\nend\n" % (_UV, _P),
         "stretched": "filter fetch_stretched (stretched image in, %s)\n  in(%s)\nend\n" % (_UV, _P)}
# a per-pixel frame number: -1 .. 3 over x in [-1, 1], on a sequence of three frames ({F}: see frame_index)
FRAME_EXPR = "floor(x * 2 + 1.5)"
FETCH_FRAME = "filter fetch_frame (image in, %s)\n  in(%s, {F})\nend\n" % (_UV, _P)

_BIG_UV = ", ".join("float big%d: 0-1000000000 (1)" % i for i in (1, 2, 3))

# Wild coordinates, left to the oracle: rows in four bands take x + inf, x - inf, x + NaN and x + big (or y, with
# vert = 1); q = exp(x * 1000 + 900) is +inf right of x = -0.81 and a finite number up to 1e38 left of it.
_WILD = """
filter fetch_wild (image in, %s, float vert: 0-1 (0))
  big = big1 * big2 * big3;
  q = exp(x * 1000 + 900);
  band = floor((y + 1) * 2);
  d = if band < 1 then q else if band < 2 then q * (0 - 1) else if band < 3 then q * 0 else big end end end;
  px = if vert < 0.5 then x + d else x end;
  py = if vert < 0.5 then y else y + d end;
  {OUT}
end
""" % _BIG_UV
WILD, WILD_COORDS = (_WILD.replace("{OUT}", out) for out in ("in(xy:[px, py])", "rgba:[px, py, x, y]"))
# big1 * big2 * big3: 2**31, 2**32 and 1e19 (beyond a long)
WILD_BIG = ((65536.0, 32768.0, 1.0), (65536.0, 65536.0, 1.0), (1e9, 1e9, 10.0))


def wild_uservals(big, vert=0):
    return {"big1": big[0], "big2": big[1], "big3": big[2], "vert": vert}

# gaussian_blur at deviation 0 skips both passes: the map is render_image's (builtins.c:303-343).  The last statement
# samples a map (get_floatmap_pixel): that one, or what another native call makes of it -- a second blur (a native
# filter's image argument is stripped of its resize wrapper: the same map) or render() (not stripped: behind the wrapper
# the map is sampled into a new one).  {KIND}: "" or "stretched ", for the filter and its image alike.
_WILD_D = ("  big = big1 * big2 * big3;\n  q = exp(x * 1000 + 900);\n  band = floor((y + 1) * 2);\n"
           "  d = if band < 1 then q else if band < 2 then q * (0 - 1) else if band < 3 then q * 0 else big end end end;\n")
_FM_FORMS = {"blur": ("", "b"), "blur_blur": ("  c = gaussian_blur(b, 0, 0);\n", "c"), "blur_render": ("  c = render(b);\n", "c"),
             "render": ("", "b")}      # b = render(in): the drawable keeps its wrapper, so render_image samples beyond its edges


def floatmap_probe(form, stretched, wild=False):
    """The float-map probe `form` (blur, blur_blur, blur_render, render).  `stretched`: a stretched filter on a stretched image
    (no resize wrapper anywhere), else the default of both.  `wild`: coordinates like WILD's instead of the affine map."""
    kind = "stretched " if stretched else ""
    more, last = _FM_FORMS[form]
    if wild:
        return ("%sfilter fm_%s_wild (%simage in, %s)\n%s  b = gaussian_blur(in, 0, 0);\n%s  %s(xy:[x + d, y])\nend\n"
                % (kind, form, kind, _BIG_UV, _WILD_D, more, last))
    first = "  b = render(in);\n" if form == "render" else "  b = gaussian_blur(in, 0, 0);\n"
    return "%sfilter fm_%s (%simage in, %s)\n%s%s  %s(%s)\nend\n" % (kind, form, kind, _UV, first, more, last, _P)


FRAME_SIZES = [(40, 24), (5, 3)]
IMAGE_SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (2, 3), (13, 7), (53, 37), (9, 30), (40, 24)]
FLOATMAP_FRAMES = [(40, 24), (33, 21), (5, 3), (1, 7), (9, 1)]


def image_sizes_for(frame):
    """Every image size on every frame, 40 x 24 on the frame of its own size only."""
    return [s for s in IMAGE_SIZES if s != (40, 24) or frame == (40, 24)]


def maps_for(iw, ih, factors=None, big=2.5e8):
    """(name, sx, sy, ox, oy).  A texel is 2 / (n - 1) of the image's own unit coordinates (over the wrapper's factor).
    `big`: 2.5e8 keeps the 13-wide image's pixel coordinate just under 2**31; the strided fetch's cap is 2**30."""
    fx, fy = (1.0, 1.0) if factors is None else (float(factors[0]), float(factors[1]))
    tx = 2.0 / (iw - 1) / fx if iw > 1 else 0.5
    ty = 2.0 / (ih - 1) / fy if ih > 1 else 0.5
    maps = [("identity", 1.0, 1.0, 0.0, 0.0),
            ("one texel", 1.0, 1.0, tx, -ty),
            ("half a texel", 1.0, 1.0, tx / 2, ty / 2),
            ("minus half a texel", 1.0, 1.0, -tx / 2, -ty / 2),
            ("affine", 2.7, 2.7, 0.31, -0.23),
            ("mirrored", -1.3, 0.7, 0.0, 0.0),
            ("one point", 0.0, 0.0, 0.2, 0.1),
            ("tiny at the centre", 1e-30, 1e-30, 0.0, 0.0),
            ("tiny at the corner", 1e-30, 1e-30, -1.0 / fx, 1.0 / fy),
            ("1e6", 1e6, 1e6, 0.31, -0.23)]
    if (iw, ih) == (13, 7):
        maps.append(("just under 2**31 px", big, big, 0.31, -0.23))
    return maps


def map_uservals(m):
    return dict(zip(("sx", "sy", "ox", "oy"), m[1:]))


def random_frames(n, w, h, seed):
    """n frames of random RGBA bytes, uint8 [n, h, w, 4]."""
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 4), np.uint8)


@_quiet
def frame_index(x):
    """FRAME_EXPR as ORIG_VAL's frame argument sees it: float product and sum, floor, (int)."""
    x = np.asarray(x, f32)
    return _cvtt(np.floor(x * f32(2) + f32(1.5)).astype(f64))


# ---- the output ramp ---------------------------------------------------------------------------------------------------

# 257 x 17, a stretched filter: x = (col - 128) / 128 and y = (8 - row) / 8 are exact, so k = (x + 1) * 128 is the column
# and row = (1 - y) * 8 the row without a floor -- only + - * / and comparisons, which pair mode covers too.  u = k / 255.
#   rows 0-2    red = green = blue = u (the grey pack's sensitive values, white among them; column 256 is above 1), alpha u (1 + eps)
#   rows 3-10   three different channels within a few ulps of byte boundaries
#   rows 11-12  values below 0 and above 1
#   rows 13-16  NaN, +inf, -inf and -0, each in every channel
RAMP_SIZE = (257, 17)
RAMP = """
stretched filter fetch_ramp ()
  k = (x + 1) * 128;
  row = (1 - y) * 8;
  u = k / 255;
  eps = (row - 8) * 0.00000003;
  inf = (u + 100000000) * 100000000 * 100000000 * 100000000 * 100000000;
  ninf = inf * (0 - 1);
  nan = inf * 0;
  nz = u * 0 * (0 - 1);
  if row < 2.5 then
    rgba:[u, u, u, u * (1 + eps)]
  else if row < 10.5 then
    rgba:[u * (1 + eps), (256 - k) / 255 * (1 - eps), (k * 0.5 + row * 8) / 255 * (1 + eps * 3), (255 - k) / 255 * (1 - eps * 2)]
  else if row < 12.5 then
    rgba:[u * 3 - 1, 1.5 - u * 2, u * (0 - 1), u + 0.5 + eps]
  else if row < 13.5 then rgba:[nan, ninf, inf, nz]
  else if row < 14.5 then rgba:[inf, nan, nz, ninf]
  else if row < 15.5 then rgba:[ninf, nz, nan, inf]
  else rgba:[nz, inf, ninf, nan]
  end end end end end end
end
"""


def grey_sensitive_ks():
    """The k in 0 .. 255 for which r = g = b = k / 255 packs to another grey byte when the sum is evaluated in
    float32 instead of double (computed, not listed: the store's double evaluation is what the template asks for)."""
    u = (np.arange(256, dtype=f64) / 255.0).astype(f32)
    with np.errstate(all="ignore"):
        exact = np.trunc(grey_double(u, u, u)).astype(np.int64)
        single = np.trunc(grey_float32(u, u, u).astype(f64)).astype(np.int64)
    return [int(k) for k in np.nonzero(exact != single)[0]]


# ---- what the probes compute, restated ------------------------------------------------------------------------------------

@_quiet
def own_coordinates(W, H):
    """render_image's coordinates of a W x H map's own pixels (builtins.c:326,330): ((float)x - bx) / ax, float [H, W] each."""
    ax, bx, ay, by = floatmap_coefficients(W, H)
    fx, fy = (np.arange(W, dtype=f32) - bx) / ax, (np.arange(H, dtype=f32) - by) / ay
    return np.broadcast_to(fx[None, :], (H, W)), np.broadcast_to(fy[:, None], (H, W))


def floatmap_probe_reference(form, stretched, image, W, H, x, y, edge, colours, supersampling=False):
    """floatmap_probe(form, stretched) on a W x H frame at the coordinate arrays x, y: (map, covered).
    b is render_image of the drawable without its wrapper (a native filter's image argument is stripped), a W x H map
    behind the wrapper of the filter's flags (compiler.c:2218-2219).  blur_blur's c is a copy of b behind the same
    wrapper; blur_render's c samples b at c's own coordinates times the wrapper's factors, and render()'s result gets
    no wrapper."""
    flags = "stretched" if stretched else "default"
    if form == "render":      # render(in): in behind its own wrapper; the result is a plain map
        b, ok = float_map_of(image, W, H, edge, colours, factors=resize_factors(image.shape[1], image.shape[0], flags), supersampling=supersampling)
        out, ok2 = float_map_fetch(b, x, y)
        return out, ok2 & bool(ok.all())
    b, ok = float_map_of(image, W, H, edge, colours, supersampling=supersampling)
    wrapper = resize_factors(W, H, flags)
    covered = bool(ok.all())
    if form == "blur_render":
        b, ok = float_map_fetch(b, *own_coordinates(W, H), factors=wrapper)
        covered, wrapper = covered and bool(ok.all()), None
    out, ok = float_map_fetch(b, x, y, factors=wrapper)
    return out, ok & covered


def frame_probe_oracle(render, index, num_frames):
    """The oracle binds one frame per image and only range-checks a frame number, so FETCH_FRAME's frame is put together
    from one render per frame number: `render(literal, k)` renders FETCH_FRAME with {F} = literal on frame k of the
    sequence -- literal 0 on frame k for the numbers the sequence has, the number itself (out of range: white, after the
    edge tests) on frame 0 for the others; each pixel is taken from the render of its own number, index[pixel]."""
    out = None
    for k in sorted(int(v) for v in np.unique(index)):
        m = render("0", k) if 0 <= k < num_frames else render("(0 - %d)" % -k if k < 0 else str(k), 0)
        out = np.zeros_like(m) if out is None else out
        out[index == k] = m[index == k]
    return out
