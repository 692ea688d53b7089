"""A NumPy restatement of the filtered clip (mmhip_render_clip_filtered, include/mmhip.h), written from the header's
statement: the kernel functions of one axis in Python floats (math.exp is the C library's double exp, the cubics in the
stated order), the normalised float32 taps of an edge class, the two sequential float32 sums over arrays of sub-sample
maps, the shutter's accumulation and, through tests/shutter_reference.py, the byte store.  It shares no code with the
library.  (tests/test_clip_filtered_api.py, tests/test_gpu_clip_filtered.py)"""
import math

import numpy as np

from tests import sample_grid_reference as G
from tests.fetch_reference import pack

f32, f64 = np.float32, np.float64
BOX, TENT, GAUSSIAN, MITCHELL = range(4)
KERNELS = {"box": BOX, "tent": TENT, "gaussian": GAUSSIAN, "mitchell": MITCHELL}
DEFAULT_RADII = {"box": 0.5, "tent": 1.0, "gaussian": 1.5, "mitchell": 2.0}


def reach(radius):
    """D = (int)ceil(radius - 0.5)."""
    return int(math.ceil(float(f32(radius)) - 0.5))


def k(kernel, d, radius):
    """The weight of one axis at distance d (Python floats are C doubles)."""
    d, big_r = float(d), float(f32(radius))
    ad = math.fabs(d)
    if ad >= big_r:
        return 0.0
    if kernel == BOX:
        return 1.0
    if kernel == TENT:
        return 1.0 - ad / big_r
    if kernel == GAUSSIAN:
        return math.exp(-2.0 * (d * d)) - math.exp(-2.0 * (big_r * big_r))
    u = (2.0 * ad) / big_r
    if u < 1.0:
        return (((7.0 * u - 12.0) * u) * u + 16.0 / 3.0) / 6.0
    return ((((-7.0 / 3.0) * u + 12.0) * u - 20.0) * u + 32.0 / 3.0) / 6.0


def taps(kernel, radius, n, lo, hi):
    """float32 [2 D + 1, n]: entry [dx + D, a] = (float)(k / norm) for the existing taps dx = -lo .. hi, 0 elsewhere; norm
    is the double sum of k over the existing taps in tap order.  None where norm is not a positive finite number."""
    big_d = reach(radius)
    offs = [float(o) for o in G.offsets(n)]
    norm = 0.0
    for dx in range(-lo, hi + 1):
        for a in range(n):
            norm = norm + k(kernel, float(dx) + offs[a], radius)
    if not (norm > 0.0 and math.isfinite(norm)):
        return None
    out = np.zeros((2 * big_d + 1, n), f32)
    for dx in range(-lo, hi + 1):
        for a in range(n):
            out[dx + big_d, a] = f32(k(kernel, float(dx) + offs[a], radius) / norm)
    return out


def edge_class(at, size, big_d):
    return min(big_d, at), min(big_d, size - 1 - at)


def weighted_sum(terms):
    """terms: [(float32 weight, float32 array)] in tap order, zero weights already dropped.  Each product is rounded on its
    own; the first starts the sum, every later one is added in order."""
    with np.errstate(all="ignore"):
        acc = None
        for w, f in terms:
            p = (f32(w) * f).astype(f32)
            acc = p if acc is None else (acc + p).astype(f32)
    return acc


def step(maps, kernel, radius):
    """s_j of one time step: maps float32 [sy, sx, H, W, 4] over the whole frame -> float32 [H, W, 4]."""
    maps = np.asarray(maps, f32)
    sy, sx, height, width = maps.shape[:4]
    big_d = reach(radius)
    tx = {c: taps(kernel, radius, sx, *c) for c in {edge_class(x, width, big_d) for x in range(width)}}
    ty = {c: taps(kernel, radius, sy, *c) for c in {edge_class(y, height, big_d) for y in range(height)}}
    h = np.zeros((sy, height, width, 4), f32)
    for c in range(width):
        w = tx[edge_class(c, width, big_d)]
        for b in range(sy):
            terms = [(w[dx + big_d, a], maps[b, a, :, c + dx]) for dx in range(-big_d, big_d + 1) for a in range(sx) if w[dx + big_d, a] != 0]
            h[b, :, c] = weighted_sum(terms)
    s = np.zeros((height, width, 4), f32)
    for r in range(height):
        w = ty[edge_class(r, height, big_d)]
        terms = [(w[dy + big_d, b], h[b, r + dy]) for dy in range(-big_d, big_d + 1) for b in range(sy) if w[dy + big_d, b] != 0]
        s[r] = weighted_sum(terms)
    return s


def frame(maps, kernel, radius):
    """m of one frame: maps float32 [K, sy, sx, H, W, 4] -> float32 [H, W, 4].  acc = s_0; acc = acc + s_j; m = acc *
    (float)(1.0 / (double)K)."""
    maps = np.asarray(maps, f32)
    count = maps.shape[0]
    with np.errstate(all="ignore"):
        acc = step(maps[0], kernel, radius)
        for j in range(1, count):
            acc = (acc + step(maps[j], kernel, radius)).astype(f32)
        return (acc * f32(1.0 / f64(count))).astype(f32)


def combine(maps, kernel, radius, bpp=4, floatmap=False):
    """The output of one whole frame: float32 [H, W, 4] with `floatmap`, else uint8 [H, W, bpp]."""
    m = frame(maps, kernel, radius)
    return m if floatmap else pack(m, bpp)
