"""numpy restatements of gaussian_blur's FIR path (native-filters/gauss.c:264-639: make_rle_curve, run_length_encode,
do_encoded_lre, do_full_lre, gauss_rle) and the inputs and comparisons the blur tests share.  A helper: no tests in here.

Written from gauss.c, not from the oracle (oracle/mm_oracle_rt.c) or the kernels (native_filters.hip), and pinned
against the oracle by tests/test_gauss_reference.py.  Two references:

* `fir_pass_f32` rounds every operation to float32 in gauss.c's order and keeps its types: exp in double, taps and
  cumulative sums stored as float, `int s2 = csum[i]`, `s1 = s2`, the int `ctotal` of the encoded branch.  A correct
  implementation equals it bit for bit, on either branch.
* `fir_pass_f64` evaluates the full branch (do_full_lre) with the same float32 taps but sums and divides in float64.
  The encoded branch is not a rounding of anything (its int-truncated sums make a constant line come out as
  total / (int)total: 1.0039 at length 1), so lines that take it are marked as not covered.

Maps are float32 [h,w,4]; axis 0 is the vertical pass (lines are columns), axis 1 the horizontal one (lines are rows).
"""
import math

import numpy as np

from tests.fft_reference import as_map, oracle, random_rgba  # noqa: F401  (re-exported for the blur tests)

# The bound on a float32 evaluation of the full branch against fir_pass_f64, per element, in units of
# 2**-24 * max |line| (the largest magnitude on the element's line and channel): L + 3 for a curve of length L.
# The centre and the L pairs make L + 1 terms; the first lands on 0.0 exactly, so L accumulations round, each a
# partial sum of at most total * max|line|, which the division by total brings back to one unit each: L.  The pair
# sums' roundings are weighted by their taps, which add up to total: after the division one unit for all of them
# together; likewise the products: one; the division itself rounds once: one.  (total leaves out the curve's last
# tap, gauss.c:295-302, which is below 1/255 of the centre's: 0.4 % of a unit per unit.)  Measured: 0.9 to 2.7 units
# at L = 1 and 2, 8.3 at L = 67, 87 at L = 8002.  float64's own error, (L + 3) * 2**-53, is 2**-29 of the bound.
def f64_bound_units(length):
    return length + 3


def sigmas(w, h, hdev, vdev):
    """(hs, vs): the deviations in pixels as gaussian_blur computes them (gauss.c:659-660, floatmap.c:39-41): float
    products with ax = (w - 1) / 2 and ay = -(h - 1) / 2.  A width of 1 makes hs 0 whatever hdev is."""
    ax = np.float32(np.float32(w - 1) / 2.0)
    ay = np.float32(np.float64(np.float32(np.float32(h - 1) / 2.0)) * -1.0)
    hs = np.float32(abs(float(np.float32(hdev) * ax)))
    vs = np.float32(abs(float(np.float32(vdev) * ay)))
    return hs, vs


def takes_fir(hs, vs):
    """gauss.c:662: a deviation below half a pixel on either axis."""
    return bool(hs < 0.5 or vs < 0.5)


def devs_for(w, h, hsig, vsig):
    """User values (hdev, vdev) that give about `hsig`, `vsig` pixels at w x h (sigmas() says what exactly)."""
    return (hsig / ((w - 1) / 2.0) if w > 1 else hsig), (vsig / ((h - 1) / 2.0) if h > 1 else vsig)


def rle_curve(sigma):
    """make_rle_curve (gauss.c:264-306): (length, taps, csum, total).  taps[length + i] for i in [-length, length] and
    csum[length + i] likewise, both float32; total = csum[length] - csum[-length] in float."""
    sigma = float(np.float32(sigma))
    sigma2 = 2 * sigma * sigma
    l = math.sqrt(-sigma2 * math.log(1.0 / 255.0))
    n = int(math.ceil(l) * 2)
    if n % 2 == 0:
        n += 1
    length = n // 2
    taps = np.empty(n, np.float32)
    taps[length] = 1.0
    for i in range(1, length + 1):
        temp = np.float32(math.exp(-(i * i) / sigma2))
        taps[length - i] = temp
        taps[length + i] = temp
    csum = np.zeros(2 * length + 1, np.float32)
    for i in range(1, 2 * length + 1):
        csum[i] = taps[i - 1] + csum[i - 1]             # float32 + float32
    total = np.float32(csum[2 * length] - csum[0])
    return length, taps, csum, total


def run_length_encode(line, border):
    """gauss.c:315-378 on one channel of one line: (same, pix, rle).  pix and rle cover positions -border .. n + border - 1
    (index = position + border).  The walk starts at the line's far end; an element equal to its successor's run value
    is written as that value (which matters only where +0 meets -0) and counted in `same`, the last element included."""
    vals = [float(v) for v in line]
    n = len(vals)
    pix = [0.0] * (n + 2 * border)
    rle = [0] * (n + 2 * border)
    p = n + 2 * border - 1
    last = vals[n - 1]
    count = same = 0
    for _ in range(border):
        count += 1
        pix[p], rle[p] = last, count
        p -= 1
    for k in range(n - 1, -1, -1):
        c = vals[k]
        if c == last:
            count += 1
            same += 1
        else:
            count = 1
            last = c
        pix[p], rle[p] = last, count
        p -= 1
    for _ in range(border):
        count += 1
        pix[p], rle[p] = last, count
        p -= 1
    return same, np.array(pix, np.float32), rle


def takes_encoded(same, n):
    """gauss.c:547,605: the switch between the two branches."""
    return same > (3 * n) // 4


def _full_f32(pix, n, length, taps, total):
    """do_full_lre (gauss.c:422-498): the centre, then the pairs outwards, every operation a float32 one."""
    at = np.arange(n) + length
    val = np.zeros(n, np.float32)
    val = val + pix[at] * taps[length]
    for i in range(1, length + 1):
        val = val + (pix[at + i] + pix[at - i]) * taps[length + i]
    return val / total


def _encoded_f32(pix, rle, n, length, csum, total):
    """do_encoded_lre (gauss.c:380-420): walks the runs inside the window; `int s2 = csum[i]`, `s1 = s2`, int ctotal."""
    f32 = np.float32
    ctotal = f32(int(total))
    out = np.empty(n, np.float32)
    for col in range(n):
        j = col                               # position col - length
        s1 = csum[0]
        nb = rle[j]
        i = -length + nb
        val = f32(0.0)
        while i <= length:
            s2 = int(csum[length + i])
            val = val + pix[j] * (f32(s2) - s1)
            s1 = f32(s2)
            j += nb
            nb = rle[j]
            i += nb
        val = val + pix[j] * (csum[2 * length] - s1)
        out[col] = val / ctotal
    return out


def _lines(m, axis):
    """(number of lines, line length, view [line, step, channel])."""
    v = m if axis == 1 else m.transpose(1, 0, 2)
    return v.shape[0], v.shape[1], v


def fir_pass_f32(m, sigma, axis):
    """One pass of gauss_rle in float32, gauss.c's order and types.  Returns (map, flags): flags[line, channel] is True
    where the line took the encoded branch."""
    m = np.asarray(m, np.float32)
    length, taps, csum, total = rle_curve(sigma)
    lines, n, src = _lines(m, axis)
    out = np.empty_like(m)
    dst = _lines(out, axis)[2]
    flags = np.zeros((lines, 4), bool)
    with np.errstate(all="ignore"):
        for ln in range(lines):
            for ch in range(4):
                same, pix, rle = run_length_encode(src[ln, :, ch], length)
                flags[ln, ch] = takes_encoded(same, n)
                if flags[ln, ch]:
                    dst[ln, :, ch] = _encoded_f32(pix, rle, n, length, csum, total)
                else:
                    dst[ln, :, ch] = _full_f32(pix, n, length, taps, total)
    return out, flags


def fir_pass_f64(m, sigma, axis):
    """The full branch of one pass in float64: float32 taps, sums in float64, divided by the float32 total.  Returns
    (map as float64, covered [h,w,4], length): covered is False on the lines that take the encoded branch."""
    m = np.asarray(m, np.float32)
    length, taps, _, total = rle_curve(sigma)
    lines, n, src = _lines(m, axis)
    taps64 = taps.astype(np.float64)
    idx = np.clip(np.arange(-length, n + length), 0, n - 1)
    pad = src.astype(np.float64)[:, idx, :]                    # edge replication
    at = np.arange(n) + length
    with np.errstate(all="ignore"):
        val = pad[:, at, :] * taps64[length]
        for i in range(1, length + 1):
            val = val + (pad[:, at + i, :] + pad[:, at - i, :]) * taps64[length + i]
        val = val / np.float64(total)
    covered = np.empty((lines, n, 4), bool)
    for ln in range(lines):
        for ch in range(4):
            covered[ln, :, ch] = not takes_encoded(run_length_encode(src[ln, :, ch], 0)[0], n)
    if axis == 0:
        val, covered = val.transpose(1, 0, 2), covered.transpose(1, 0, 2)
    return np.ascontiguousarray(val), np.ascontiguousarray(covered), length


def f64_distance(got, m, sigma, axis):
    """How far the float32 result `got` of one pass over `m` lies from fir_pass_f64, in units of 2**-24 * max |line|:
    (largest distance over the covered elements, share of elements covered, length).  f64_bound_units(length) bounds
    the first figure."""
    m = np.asarray(m, np.float32)
    want, covered, length = fir_pass_f64(m, sigma, axis)
    line_max = np.abs(m.astype(np.float64)).max(axis=0 if axis == 0 else 1, keepdims=True)
    unit = np.broadcast_to(line_max * 2.0 ** -24, m.shape)
    use = covered & (unit > 0)
    err = np.abs(np.asarray(got, np.float64) - want)
    assert not (covered & (unit == 0) & (err != 0)).any()       # a zero line stays zero
    return (float((err[use] / unit[use]).max()) if use.any() else 0.0), float(covered.mean()), length


def gauss_blur_map(m, hs, vs):
    """gauss_rle (gauss.c:500-639) on a float map: the vertical pass if vs > 0, then the horizontal one if hs > 0.
    Returns (map, {axis: flags}) with the flags of the passes that ran."""
    out, flags = np.array(m, np.float32), {}
    if vs > 0.0:
        out, flags[0] = fir_pass_f32(out, vs, 0)
    if hs > 0.0:
        out, flags[1] = fir_pass_f32(out, hs, 1)
    return out, flags


def same_maps(got, want):
    """The blur tests' comparison: NaN at the same places, every other element the same bits (the sign of zero and
    denormals included).  A NaN's sign and payload are not compared: x86 and the GPU make different default NaNs."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def describe_difference(got, want):
    """For assertion messages: how many NaN places and how many other elements differ, and the first of them."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan_diff = np.isnan(got) != np.isnan(want)
    bits = (got.view(np.uint32) != want.view(np.uint32)) & ~np.isnan(got) & ~np.isnan(want)
    where = np.argwhere(nan_diff | bits)
    first = tuple(int(v) for v in where[0]) if len(where) else None
    return {"nan places": int(nan_diff.sum()), "other elements": int(bits.sum()), "of": int(got.size), "first (row, col, ch)": first,
            "got": None if first is None else float(got[first]), "want": None if first is None else float(want[first])}


def special_census(m):
    """Per kind of special value, how many elements of each channel of the map hold it."""
    a = np.abs(m)
    kinds = {"+inf": np.isposinf(m), "-inf": np.isneginf(m), "nan": np.isnan(m), "-0": (m == 0) & np.signbit(m),
             "+0": (m == 0) & ~np.signbit(m), "denormal": (a > 0) & (a < np.finfo(np.float32).tiny)}
    return {k: [int(v[..., c].sum()) for c in range(4)] for k, v in kinds.items()}


# ---- inputs ---------------------------------------------------------------------------------------------------------

def threshold_sames(n):
    """The `same` counts threshold_rows gives its rows, in turn: around the switch `same > (3 * n) // 4`, and n."""
    return [min(max(s, 1), n) for s in ((3 * n) // 4 - 1, (3 * n) // 4, (3 * n) // 4 + 1, n)]


def threshold_rows(w, h):
    """RGBA bytes whose row r has, in every channel, exactly threshold_sames(w)[r % 4] elements that repeat their
    successor's value (run_length_encode's `same`, which counts the last element): the row ends in a run of that many
    equal bytes, and no element before the run equals its successor."""
    sames = threshold_sames(w)
    img = np.empty((h, w, 4), np.uint8)
    k = np.arange(w)
    for r in range(h):
        s = sames[r % 4]
        for c in range(4):
            row = (2 * k + 7 * c + 3 * r) % 200 + 1             # neighbours differ by 2 (mod 200): never equal
            row[w - s:] = 250 - c - (r % 4)                     # above every value before it
            img[r, :, c] = row
    return img


def stepped_flat(w, h):
    """A flat RGBA image with a few steps: every line of every channel has more than 3/4 of its elements in runs, so
    the first pass takes the encoded branch everywhere and the second one on the lines the first left flat."""
    img = np.empty((h, w, 4), np.uint8)
    img[...] = (40, 90, 160, 230)
    img[h // 3:h // 3 + max(h // 8, 1), w // 5:w - w // 8] = (200, 120, 30, 77)
    img[:, w // 2:w // 2 + max(w // 100, 1)] = (255, 0, 255, 128)
    return img


# The closure fills a float map with what no drawable holds; z = p[0] * 0 is +0 at run time (the compiler cannot fold it),
# exp(900 + z) overflows to +inf and inf * 0 is NaN (the language answers 1 / 0 with 0).
#   red:   +inf left of x = -0.6, -inf right of x = 0.6 in the upper half, values in [-1, 2] elsewhere
#   green: NaN in a block in the middle, values in [-1.5, 1.5] elsewhere
#   blue:  no inf, no NaN: rows of +0 and -0 in patches of three (y > 0.5), denormals (p[2] * 1e-40) in the middle band,
#          values in [-3, 0] below
#   alpha: -0 everywhere
SPECIAL_CLOSURE = """
stretched filter special (stretched image in)
  p = in(xy);
  z = p[0] * 0;
  nz = z * (0 - 1);
  big = exp(900 + z);
  vr = if x < -0.6 then big else if x > 0.6 && y > 0 then big * (0 - 1) else p[0] * 3 - 1 end end;
  vg = if abs(x) < 0.3 && abs(y) < 0.4 then big * z else p[1] * 3 - 1.5 end;
  vb = if y > 0.5 then
        if floor((x + 2) * 6.5) % 2 < 1 then z else nz end
      else
        if y > -0.4 then p[2] * 0.0000000000000000000000000000000000000001 else p[2] * (0 - 3) end
      end;
  rgba:[vr, vg, vb, nz]
end

stretched filter special_blur (stretched image in, float hdev: 0-100 (0.01), float vdev: 0-100 (0.01))
  b = gaussian_blur(special(in), hdev, vdev);
  b(xy)
end
"""

# an IIR blur whose float map (values that are no k / 255, tiny negatives) a FIR blur takes as it is
CHAINED = """
stretched filter chained (stretched image in, float wide: 0-1 (0.2), float narrow: 0-1 (0.01))
  soft = gaussian_blur(in, wide, wide);
  c = gaussian_blur(soft, narrow, narrow);
  c(xy)
end
"""
