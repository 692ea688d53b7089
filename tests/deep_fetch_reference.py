"""numpy restatement of the float32 drawable fetch (include/mmhip.h, mmhip_set_image_sequence_float_*): the drawable
fetch of tests/fetch_reference.py with the byte step taken out.  A helper: no tests in here.

Written from the semantics stated in include/mmhip.h, not from the device code (mm_device.h mm_orig_val_deep).  The
coordinates, the taps, the weights, the edge behaviour and the order of a tap's tests are fetch_reference's own functions,
imported; what differs is what a tap returns -- the texel's four floats as stored, an edge colour as TUPLE_FROM_COLOR
makes it, or ones -- and that the bilinear result is the weighted sum itself, every product and sum rounded to float32,
with no rintf and no division by 255.

Images are float32 [h, w, 4] or, as a sequence, [n, h, w, 4].  The fetches return (float32 [.., 4], covered) like
fetch_reference's: `covered` is False where a pixel coordinate is NaN, infinite or reaches 2**31 px."""
import numpy as np

from tests.fetch_reference import (_colour_bytes, _covered, _cvtt, _quiet, _taps, _tuple_from_bytes, apply_edge_behaviour, apply_factors,
                                   drawable_transform)

f32, f64 = np.float32, np.float64

# |fetch_bilinear_deep(bytes / 255) - fetch_bilinear(bytes)| on covered pixels.  With E the exact sum of byte * weight
# over the four taps (weights in [0, 1], their sum within 2**-22 of 1):
#   the 8-bit fetch returns RN(rint(S) / 255), S the float32 evaluation of E: four products and three sums of values
#     below 256, each within 2**-24 relative, so |S - E| <= 7 * 2**-16; rint moves S by at most 0.5; the quotient is at
#     most 1 and its rounding at most 2**-25;
#   the deep fetch evaluates the sum of RN(byte / 255) * weight: every tap value is within 2**-25 of byte / 255, which
#     the weights pass on as at most 2**-25 * (1 + 2**-22); the four products are at most 1 (2**-25 each), the three
#     partial sums may exceed 1 by the weights' 2**-22 (2**-24 each).
# 0.5 / 255 + 7 * 2**-16 / 255 + (1 + 1 + 4 + 6) * 2**-25, and one more 2**-25 for the (1 + 2**-22) factors.
BILINEAR_BYTE_BOUND = 0.5 / 255 + 7 * 2.0 ** -16 / 255 + 13 * 2.0 ** -25


def _colour_tuple(c):
    return _tuple_from_bytes(_colour_bytes(c))


def get_pixel_deep(frames, x, y, frame, edge, colours):
    """One tap: the edge behaviour, then x outside -> edge colour x, y outside -> edge colour y, then a frame number
    outside [0, N) -> ones, otherwise the texel as stored.  float32 [.., 4]; `frame`: an int or an int array."""
    frames = np.asarray(frames, f32)
    if frames.ndim == 3:
        frames = frames[None]
    n, h, w, _ = frames.shape
    x, y = apply_edge_behaviour(x, y, w, h, edge)
    frame = np.broadcast_to(np.asarray(frame, np.int64), x.shape)
    out_x, out_y = (x < 0) | (x >= w), (y < 0) | (y >= h)
    bad_frame = (frame < 0) | (frame >= n)
    inside = ~(out_x | out_y | bad_frame)
    px = frames[np.where(inside, frame, 0), np.where(inside, y, 0), np.where(inside, x, 0)]
    px = np.where(bad_frame[..., None], f32(1.0), px)
    px = np.where(out_y[..., None], _colour_tuple(colours[1]), px)
    px = np.where(out_x[..., None], _colour_tuple(colours[0]), px)
    return px.astype(f32)


@_quiet
def fetch_nearest_deep(frames, x, y, edge, colours, factors=None, frame=0, supersampling=False):
    """The nearest fetch: fetch_reference.fetch_nearest's coordinates, the tap itself."""
    frames = np.asarray(frames, f32)
    h, w = frames.shape[-3], frames.shape[-2]
    x, y = drawable_transform(*apply_factors(x, y, factors), w, h)
    ok = _covered(2.0 ** 31, x, y)
    if not supersampling:
        x, y = (x.astype(f64) + 0.5).astype(f32), (y.astype(f64) + 0.5).astype(f32)
        ok &= _covered(2.0 ** 31, x, y)
    return get_pixel_deep(frames, _cvtt(np.floor(x.astype(f64))), _cvtt(np.floor(y.astype(f64))), frame, edge, colours), ok


@_quiet
def fetch_bilinear_deep(frames, x, y, edge, colours, factors=None, frame=0):
    """The bilinear fetch: fetch_reference.fetch_bilinear's taps and weights, then per channel
    ((p1 * f1 + p2 * f2) + p3 * f3) + p4 * f4 in float32."""
    frames = np.asarray(frames, f32)
    h, w = frames.shape[-3], frames.shape[-2]
    x, y = drawable_transform(*apply_factors(x, y, factors), w, h)
    ok = _covered(2.0 ** 31, x, y)
    x, x1, x2, x2fact = _taps(x, 1)
    y, y1, y2, y2fact = _taps(y, 1)
    x1fact, y1fact = (1.0 - x2fact.astype(f64)).astype(f32), (1.0 - y2fact.astype(f64)).astype(f32)
    facts = (x1fact * y1fact, x1fact * y2fact, x2fact * y1fact, x2fact * y2fact)
    taps = ((x1, y1), (x1, y2), (x2, y1), (x2, y2))
    total = None
    for (tx, ty), fact in zip(taps, facts):
        term = get_pixel_deep(frames, tx, ty, frame, edge, colours) * fact.astype(f32)[..., None]
        total = term if total is None else total + term
    return total.astype(f32), ok


def random_texels(n, w, h, seed):
    """n frames of float texels, float32 [n, h, w, 4]: most in -0.5 .. 1.5 (negatives and values above 1 among them), and
    planted in every frame that has the room NaN, both infinities, -0, a denormal, its negative, and a large value."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-0.5, 1.5, (n, h, w, 4)).astype(f32)
    tiny = np.finfo(f32).smallest_subnormal
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, tiny * 5, -tiny * 3, 3.0e38, -7.25], f32)
    for k in range(n):
        flat = t[k].reshape(-1)
        m = min(len(specials), flat.size // 2)
        flat[rng.permutation(flat.size)[:m]] = np.roll(specials, k)[:m]
    return t
