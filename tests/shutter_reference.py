"""A NumPy restatement of the motion-blurred clip (mmhip_render_clip_shutter, include/mmhip.h): the times of the
sub-samples and the combine of their float maps.  It shares no code with the library: the sum is a loop of float32
additions in sub-sample order, the scale one float32 product, the bytes are tests/fetch_reference.py's `pack`.
(tests/test_clip_shutter_api.py, tests/test_gpu_clip_shutter.py)"""
import numpy as np

from tests.fetch_reference import pack

f32, f64 = np.float32, np.float64


def sample_ts(ts, samples, span):
    """float32 [N, samples]: t_ij = (float)((double)ts[i] + ((double)span * (double)j) / (double)samples), ts and span
    being C floats."""
    ts = [f32(t) for t in np.asarray(ts, f32).reshape(-1)]
    span = f32(span)
    out = np.empty((len(ts), samples), f32)
    for i, t in enumerate(ts):
        for j in range(samples):
            out[i, j] = f32(f64(t) + (f64(span) * f64(j)) / f64(samples))
    return out


def mean(maps):
    """maps: float32 [K, ..., 4].  acc = f_0; acc = acc + f_j, j = 1 .. K - 1; acc * (float)(1.0 / (double)K)."""
    maps = np.asarray(maps, f32)
    k = maps.shape[0]
    with np.errstate(all="ignore"):
        acc = maps[0].copy()
        for j in range(1, k):
            acc = (acc + maps[j]).astype(f32)
        return (acc * f32(1.0 / f64(k))).astype(f32)


def combine(maps, bpp=4, floatmap=False):
    """The output of one frame from its K sub-sample maps: float32 [..., 4] with `floatmap`, else uint8 [..., bpp]."""
    m = mean(maps)
    return m if floatmap else pack(m, bpp)


def same_floats(a, b):
    """NaNs at the same places, the same bit patterns everywhere else."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a.view(np.uint32)[ok], b.view(np.uint32)[ok])


def special_pixels(k, rng):
    """Sub-samples [n, k, 4] whose sums land on and beside the byte thresholds, overflow, cancel, and hold NaN (quiet), the
    infinities, -0 and denormals."""
    px = []
    for b in range(0, 256):
        for ulps in (-1, 0, 1):
            # a mean at b / 255 (and one ulp either side): k equal sub-samples
            target = f32(b / 255.0)
            for _ in range(abs(ulps)):
                target = np.nextafter(target, f32(2.0 if ulps > 0 else -1.0))
            s = np.full((k, 4), target, f32)
            px.append(s)
            # ... and the same sum split unevenly
            u = s.copy()
            u[0] = f32(target * f32(0.5))
            u[-1] = f32(target * f32(1.5))
            px.append(u)
    tiny = np.nextafter(f32(0), f32(1))
    singles = [np.nan, np.inf, -np.inf, -0.0, 0.0, tiny, -tiny, f32(1e-39), f32(5e-39), f32(1.1754942e-38), f32(3e38), f32(-3e38), 1.0, 0.5,
               f32(1) / f32(3), 255.0, -1.0]
    for v in singles:
        px.append(np.full((k, 4), v, f32))
        s = rng.uniform(-0.25, 1.25, (k, 4)).astype(f32)
        s[rng.integers(0, k)] = v                       # one sub-sample of the value among ordinary ones
        px.append(s)
        s = np.zeros((k, 4), f32)
        s[rng.integers(0, k), rng.integers(0, 4)] = v   # one channel only
        px.append(s)
    s = np.full((k, 4), np.inf, f32)
    s[-1] = -np.inf                                     # inf - inf
    px.append(s)
    s = np.full((k, 4), f32(5.877472e-39), f32)         # denormals that sum to a normal number
    px.append(s)
    return np.stack(px)
