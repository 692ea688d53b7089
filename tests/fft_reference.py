"""numpy float64 restatements of the three FFT native filters (convolve, half_convolve, visualize_fft of
native-filters/convolve.c) and the comparison the FFT tests share.  A helper: no tests in here.

The restatements are pinned against the oracle's direct long-double DFT (oracle/mm_oracle_fft.c) by
tests/test_fft_reference.py, so the GPU tests may use them at sizes the oracle's O(n (w+h)) sums cannot reach.

Every function takes and returns float32 [h,w,4] maps: `as_map(u8)` is what the filters see of a uint8 input
(byte / 255 in float, alpha 1.0 where the input has three channels).  n = w*h, cw = w//2+1, nhalf = w*(h//2) + w//2.
"""
import numpy as np

# the share of a map's elements that may differ from the reference at all (assert_fft_close)
MAX_DIFFERING_SHARE = 0.001
# the absolute term of the tolerance, as a fraction of the channel's largest reference magnitude
ZERO_FLOOR = 2.0 ** -40


def as_map(u8):
    """A uint8 [h,w,3|4] input as the float32 [h,w,4] map the native filters read."""
    u8 = np.asarray(u8)
    h, w, c = u8.shape
    out = np.ones((h, w, 4), np.float32)
    out[..., :c] = u8.astype(np.float32) / np.float32(255)
    return out


def random_rgba(w, h, seed):
    """Dense random RGBA bytes: every channel, alpha included, carries a texture of its own."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), np.uint8)


def textured_rgba(w, h, seed):
    """tests/filters.py's smooth synthetic image with a textured alpha plane (a fourth channel of the same make)."""
    from tests import filters as F
    alpha = F.synthetic_image(w, h, seed=seed + 40)[..., 1]
    return np.ascontiguousarray(np.dstack([F.synthetic_image(w, h, seed=seed), alpha]))


def blob_kernel(w, h):
    """The Gaussian blob of test_fft_native_filters_match_oracle as RGBA, green halved, alpha the blob itself."""
    yy, xx = np.mgrid[0:h, 0:w]
    blob = np.exp(-(((xx - w // 2) / 3.0) ** 2 + ((yy - (h // 2 - 1)) / 2.0) ** 2))
    kern = np.repeat((blob * 255).astype(np.uint8)[:, :, None], 4, axis=2)
    kern[:, :, 1] = kern[:, :, 1] // 2
    return kern


FLAGS = {          # filter of tests/filters.py -> every combination of its bool user values
    "convolve": [{"normalize": n, "copy_alpha": c} for n in (0, 1) for c in (0, 1)],
    "half_convolve": [{"copy_alpha": c} for c in (0, 1)],
    "visualize_fft": [{"ignore_alpha": i} for i in (0, 1)],
}
SECOND_IMAGE = {"convolve": "kernel", "half_convolve": "mask", "visualize_fft": None}

_ORACLES = {}


def oracle(src):
    """The CPU oracle of a filter of tests/filters.py or of .mm text, compiled once per process."""
    if src not in _ORACLES:
        import mathmap_amd as mm
        from oracle.ccgen import CpuFilter
        from tests import filters as F
        flt = F.load(src) if src in F.NAMES else mm.Filter(src)
        _ORACLES[src] = CpuFilter(flt.ir_json_raw)
    return _ORACLES[src]


def restated(name, uv, images):
    """The numpy restatement of filter `name` with user values `uv` on the uint8 `images` (all of the canvas's size)."""
    a = as_map(images["in"])
    if name == "convolve":
        return convolve(a, as_map(images["kernel"]), uv["normalize"], uv["copy_alpha"])
    if name == "half_convolve":
        return half_convolve(a, as_map(images["mask"]), uv["copy_alpha"])
    return visualize_fft(a, uv["ignore_alpha"])


def _nhalf(w, h):
    return w * (h // 2) + w // 2


def convolve(a, k, normalize, copy_alpha):
    h, w = a.shape[:2]
    n, nhalf = w * h, _nhalf(w, h)
    out = np.empty((h, w, 4), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(3 if copy_alpha else 4):
            kf = k[..., c].astype(np.float64).ravel()
            if normalize:
                kf = kf * (1.0 / kf.sum())
            kf = np.roll(kf, -(n - nhalf)).reshape(h, w)
            spec = np.fft.rfft2(a[..., c].astype(np.float64)) * np.fft.rfft2(kf)
            out[..., c] = np.fft.irfft2(spec, s=(h, w))
        res = out.astype(np.float32)
    if copy_alpha:
        res[..., 3] = a[..., 3]
    return res


def half_convolve(a, mask, copy_alpha):
    h, w = a.shape[:2]
    n, nhalf, cw = w * h, _nhalf(w, h), w // 2 + 1
    yy, xx = np.mgrid[0:h, 0:cw]
    idx = (xx + yy * w + nhalf) % n
    out = np.empty((h, w, 4), np.float64)
    for c in range(3 if copy_alpha else 4):
        spec = np.fft.rfft2(a[..., c].astype(np.float64))
        spec = spec * mask[..., c].astype(np.float64).ravel()[idx]
        # not irfft2: the product is not Hermitian in column 0, and the filter's c2r inverts the columns
        # first, then takes the real inverse of each row (test_oracle_dft_against_numpy_fft)
        out[..., c] = np.fft.irfft(np.fft.ifft(spec, axis=0), n=w, axis=1)
    res = out.astype(np.float32)
    if copy_alpha:
        res[..., 3] = a[..., 3]
    return res


def visualize_fft(a, ignore_alpha):
    h, w = a.shape[:2]
    n, cw = w * h, w // 2 + 1
    out = np.zeros((h, w, 4), np.float64)
    oy = (np.arange(h) + h // 2) % h
    for c in range(3 if ignore_alpha else 4):
        mag = np.abs(np.fft.rfft2(a[..., c].astype(np.float64))) / np.sqrt(float(n))
        for x in range(cw):                 # ascending: where two x land on one column the later one stays
            out[oy, cw - 1 - x, c] = mag[:, x]
            out[oy, x + w - cw, c] = mag[:, x]
    res = out.astype(np.float32)
    if ignore_alpha:
        res[..., 3] = 1.0
    return res


def fft_distance(got, want):
    """(largest |got - want| in units of the float spacing at the larger magnitude, share of elements that differ at
    all) over the elements finite in both: the two figures assert_fft_close bounds, for reports."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    fin = np.isfinite(got) & np.isfinite(want)
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    if not g.size:
        return 0.0, 0.0
    ulp = np.spacing(np.maximum(np.abs(got[fin]), np.abs(want[fin]))).astype(np.float64)
    return float((np.abs(g - w) / ulp).max()), float((g != w).sum()) / got.size


def assert_fft_close(got, want, what):
    """`got` against the reference map `want`, both float32 [h,w,4].  Per channel
      |got - want| <= spacing(float32(max(|got|, |want|))) + 2**-40 * max |want_channel|,
    at most 0.1 % of the map's elements differ at all, and NaN and infinity sit at the same places.

    The one-ulp term covers a double result that rounds to the neighbouring float.  2**-40 of the channel's largest
    magnitude is 4096 double epsilons: above the O(eps log n) error of any double FFT at the sizes tested, 65536 times
    below float precision, and needed only where the true value is 0.  The 0.1 % cap is what catches float-precision
    slips: they move many elements by one ulp, while two double FFTs disagree in the stored float on about 1e-6 of
    the elements."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32, (what, got.dtype, want.dtype)
    assert got.shape == want.shape and got.ndim == 3 and got.shape[2] == 4, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN at other places", int(np.isnan(got).sum()), int(np.isnan(want).sum()))
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), (what, "infinity at other places")
    fin = np.isfinite(want)
    differing = 0
    for c in range(4):
        f = fin[..., c]
        g32, w32 = got[..., c][f], want[..., c][f]
        if not w32.size:
            continue
        g, w = g32.astype(np.float64), w32.astype(np.float64)
        err = np.abs(g - w)
        tol = np.spacing(np.maximum(np.abs(g32), np.abs(w32))).astype(np.float64) + ZERO_FLOOR * np.abs(w).max()
        bad = err > tol
        if bad.any():
            i = int(np.argmax(err - tol))
            raise AssertionError((what, "channel %d" % c, "%d elements beyond the tolerance" % int(bad.sum()),
                                  "worst: got %r want %r tolerance %.3g" % (float(g[i]), float(w[i]), float(tol[i])),
                                  "(max ulps, differing share) = %r" % (fft_distance(got, want),)))
        differing += int((g != w).sum())
    assert differing <= MAX_DIFFERING_SHARE * got.size, (what, "%d of %d elements differ" % (differing, got.size),
                                                         "(max ulps, differing share) = %r" % (fft_distance(got, want),))
