"""A numpy float64 restatement of gaussian_blur's recursive path (native-filters/gauss.c:38-262: find_iir_constants,
transfer_pixels, gauss_iir) and the frames and deviations the tests of that path share.  A helper: no tests in here.

Written from gauss.c, not from the oracle (oracle/mm_oracle_rt.c) or the kernels (native_filters.hip), and pinned
against the oracle by tests/test_gauss_iir_reference.py.  Every step keeps gauss.c's operations in their order, each a
float64 operation of its own (numpy fuses nothing): the accumulator starts at +0; the terms i = 0 .. min(k, 4) add
n[i] * s[k-i] - d[i] * v[k-i], the i = 0 term with d[0] * acc in it, as written there; the terms above add
(n[j] - bd[j]) * initial; the stored value is (float)(val_p + val_m).  A correct implementation equals it bit for bit.

`iir_pass_segmented` restates what the scan kernels promise of a split line (native_filters.hip, "Segments"): the kept
values of segment [s0, s1) come from a causal sweep started at k0 = max(0, s0 - halo) as if k0 were the line's edge, and
from an anticausal sweep started at k1 - 1 (k1 = n for the last segment, else min(n, s1 + halo)) as if k1 were its end.

Maps are float32 [h,w,4]; axis 0 is the vertical pass (lines are columns), axis 1 the horizontal one (lines are rows).
"""
import math

import numpy as np

from tests import gauss_reference as G

# (w, h).  The vertical pass has n = h and lines = w, the horizontal one n = w and lines = h; the sweeps work in blocks
# of 16 steps, 16 lines make a wave's tile and 64 a workgroup.  2 and 4: both sweeps' edge steps inside one block;
# 15/16/17, 48/49, 63/64/65: around a block; 128/129, 144/145, 160/161: the anticausal sweep's first all-fast group at each
# residue of its groups of three blocks; 176/177 and 240/241: the causal sweep's first and second all-fast group of four.
FRAMES = [(2, 2), (3, 2), (2, 65), (4, 17), (17, 4), (15, 16), (16, 15), (33, 48), (49, 64), (65, 63), (129, 144), (145, 128),
          (161, 160), (177, 176), (193, 192), (241, 240), (240, 177)]
# (hs, vs) in pixels: the switch to the FIR path (poles exp(-3.5)); below a pixel on one axis; a deviation longer than
# most of the lines
SIGMA_PAIRS = [(0.5, 0.5), (0.9, 3.0), (7.0, 0.6), (50.0, 40.0)]
# float-map input (a closure's map): MapSrc in both passes
MAP_FRAMES = [(17, 4), (49, 64), (177, 176), (241, 240)]
MAP_SIGMA_PAIRS = [(0.5, 0.5), (7.0, 0.6)]
# (w, h, hs, vs): row windows whose halo the frame's ends cut off
ROW_WINDOW_CASES = [(65, 63, 0.9, 0.6), (240, 177, 2.0, 1.5)]
# (w, h, hs, vs) under MMHIP_GAUSS_SEGMENTS = each of FORCED_SEGMENTS
SEGMENT_CASES = [(193, 192, 0.6, 0.6), (241, 240, 0.9, 2.0), (700, 37, 2.0, 0.75)]
FORCED_SEGMENTS = ["2", "3", "5"]
# {forced: per case (segments of the vertical pass, of the horizontal pass)}, by the model's own rules (split_lines in
# native_filters.hip): the segment is n / count rounded up to a block, and a count is refused (1: the whole line) where
# the segment would be shorter than the halo -- 22.7 sigma + 2 rounded up to a block -- or the last segment empty.  The
# tests check the plan gaussian_blur reports against these; they are here so that a case's id can say what it runs.
SEGMENT_COUNTS = {"2": [(2, 2), (2, 2), (2, 2)], "3": [(3, 3), (3, 3), (1, 3)], "5": [(1, 5), (5, 1), (1, 5)]}
CLIP_FRAMES = [(17, 4), (49, 64), (129, 144), (177, 176), (241, 240)]
# (w, h, hs, vs) of the tolerance chain, and the bound tests/test_gpu_gauss_tolerance.py holds its float map to
TOLERANCE_CASES = [(97, 61, 20.0, 20.0), (301, 203, 0.55, 0.6), (700, 500, 3.0, 3.0)]
TOLERANCE_BOUND = 2.5e-7
PROPERTY_SIGMAS = [0.5, 0.75, 1.0, 2.0, 5.0, 20.0, 60.0]
IIR_BLOCK = 16


def iir_constants(sigma):
    """find_iir_constants (gauss.c:38-115) for the float `sigma`: (n_p, n_m, d, bd_p, bd_m), five doubles each
    (d_m is a copy of d_p)."""
    std_dev = float(np.float32(sigma))
    div = math.sqrt(2 * math.pi) * std_dev
    x0 = -1.783 / std_dev
    x1 = -1.723 / std_dev
    x2 = 0.6318 / std_dev
    x3 = 1.997 / std_dev
    x4 = 1.6803 / div
    x5 = 3.735 / div
    x6 = -0.6803 / div
    x7 = -0.2598 / div
    exp, sin, cos = math.exp, math.sin, math.cos
    n_p = [0.0] * 5
    n_p[0] = x4 + x6
    n_p[1] = (exp(x1) * (x7 * sin(x3) - (x6 + 2 * x4) * cos(x3)) +
              exp(x0) * (x5 * sin(x2) - (2 * x6 + x4) * cos(x2)))
    n_p[2] = (2 * exp(x0 + x1) *
              ((x4 + x6) * cos(x3) * cos(x2) - x5 * cos(x3) * sin(x2) -
               x7 * cos(x2) * sin(x3)) +
              x6 * exp(2 * x0) + x4 * exp(2 * x1))
    n_p[3] = (exp(x1 + 2 * x0) * (x7 * sin(x3) - x6 * cos(x3)) +
              exp(x0 + 2 * x1) * (x5 * sin(x2) - x4 * cos(x2)))
    n_p[4] = 0.0
    d = [0.0] * 5
    d[1] = -2 * exp(x1) * cos(x3) - 2 * exp(x0) * cos(x2)
    d[2] = 4 * cos(x3) * cos(x2) * exp(x0 + x1) + exp(2 * x1) + exp(2 * x0)
    d[3] = -2 * cos(x2) * exp(x0 + 2 * x1) - 2 * cos(x3) * exp(x1 + 2 * x0)
    d[4] = exp(2 * x0 + 2 * x1)
    n_m = [0.0] * 5
    for i in range(1, 5):
        n_m[i] = n_p[i] - d[i] * n_p[0]
    sum_n_p = sum_n_m = sum_d = 0.0
    for i in range(5):
        sum_n_p += n_p[i]
        sum_n_m += n_m[i]
        sum_d += d[i]
    a = sum_n_p / (1.0 + sum_d)
    b = sum_n_m / (1.0 + sum_d)
    bd_p = [d[i] * a for i in range(5)]
    bd_m = [d[i] * b for i in range(5)]
    return n_p, n_m, d, bd_p, bd_m


def _sweep(s, n, d, bd):
    """One sweep of gauss.c:175-196 over s[step, lane] (float64 copies of floats), from step 0 on: the line's edge is
    step 0 and `initial` its element.  The anticausal sweep is this one over the reversed line with n_m and bd_m."""
    steps = s.shape[0]
    v = np.zeros_like(s)
    initial = s[0]
    for k in range(steps):
        terms = min(k, 4)
        acc = np.zeros_like(initial)                          # memset: +0
        acc = acc + (n[0] * s[k] - d[0] * acc)                # i = 0: vp[-0] is the accumulator itself
        for i in range(1, terms + 1):
            acc = acc + (n[i] * s[k - i] - d[i] * v[k - i])
        for j in range(terms + 1, 5):
            acc = acc + (n[j] - bd[j]) * initial
        v[k] = acc
    return v


def _to_lines(m, axis):
    """float64 [step, lane] of a float32 map: lane = line * 4 + channel."""
    m = np.asarray(m, np.float32)
    h, w = m.shape[:2]
    v = m if axis == 0 else m.transpose(1, 0, 2)
    return np.ascontiguousarray(v.astype(np.float64).reshape(v.shape[0], -1)), (h, w)


def _from_lines(vals, axis, shape):
    """transfer_pixels' floats back as a map."""
    h, w = shape
    out = vals.astype(np.float32)
    return np.ascontiguousarray(out.reshape(h, w, 4) if axis == 0 else out.reshape(w, h, 4).transpose(1, 0, 2))


def iir_pass(m, axis, sigma):
    """One pass of gauss_iir over the float32 map `m`: (float)(val_p + val_m) for every line along `axis`."""
    n_p, n_m, d, bd_p, bd_m = iir_constants(sigma)
    s, shape = _to_lines(m, axis)
    with np.errstate(all="ignore"):
        val_p = _sweep(s, n_p, d, bd_p)
        val_m = _sweep(s[::-1], n_m, d, bd_m)[::-1]
        return _from_lines(val_p + val_m, axis, shape)


def iir_pass_segmented(m, axis, sigma, seg, halo):
    """The pass with every line split into segments of `seg` steps whose sweeps warm up over `halo` steps."""
    n_p, n_m, d, bd_p, bd_m = iir_constants(sigma)
    s, shape = _to_lines(m, axis)
    n = s.shape[0]
    assert seg >= 1 and halo >= 0
    total = np.empty_like(s)
    with np.errstate(all="ignore"):
        for s0 in range(0, n, seg):
            s1 = min(n, s0 + seg)
            k0 = max(0, s0 - halo)
            k1 = n if s1 == n else min(n, s1 + halo)
            val_p = _sweep(s[k0:s1], n_p, d, bd_p)[s0 - k0:]
            val_m = _sweep(s[s0:k1][::-1], n_m, d, bd_m)[::-1][:s1 - s0]
            total[s0:s1] = val_p + val_m
        return _from_lines(total, axis, shape)


def iir_blur(m, hs, vs):
    """gauss_iir (gauss.c:126-262) on a float map: the vertical pass, then the horizontal one."""
    return iir_pass(iir_pass(m, 0, vs), 1, hs)


def iir_blur_planned(m, hs, vs, plan_v, plan_h):
    """iir_blur with each pass split as its plan (seg, halo, count) says; a count of 1 is the whole line."""
    for axis, sigma, (seg, halo, count) in ((0, vs, plan_v), (1, hs, plan_h)):
        m = iir_pass_segmented(m, axis, sigma, seg, halo) if count > 1 else iir_pass(m, axis, sigma)
    return m


def true_gaussian_line(n, centre, sigma):
    """exp(-(k - centre)^2 / (2 sigma^2)) at k = 0 .. n - 1 in float64, scaled to sum 1."""
    k = np.arange(n, dtype=np.float64)
    g = np.exp(-((k - centre) ** 2) / (2.0 * float(sigma) ** 2))
    return g / g.sum()


def devs_at_least(w, h, hsig, vsig):
    """gauss_reference.devs_for as float32 values, each moved up float by float until gauss_reference.sigmas gives at
    least the wanted deviation: a wanted 0.5 px must not land at 0.49999997 and take the FIR path.  Returns Python
    floats that are float32 values, so that every consumer sees the same number."""
    hdev, vdev = (np.float32(v) for v in G.devs_for(w, h, hsig, vsig))
    while float(G.sigmas(w, h, hdev, vdev)[0]) < hsig:
        hdev = np.nextafter(hdev, np.float32(np.inf))
    while float(G.sigmas(w, h, hdev, vdev)[1]) < vsig:
        vdev = np.nextafter(vdev, np.float32(np.inf))
    return float(hdev), float(vdev)


def line_plan(n, lines, sigma, tolerance=False):
    """(seg, halo, count) of one pass as gaussian_blur plans it now (the self-test library's
    mmhip_selftest_gauss_line_plan: plan_segments, which reads MMHIP_GAUSS_SEGMENTS per call, or plan_tolerance)."""
    import ctypes as C
    from mathmap_amd._lib import selftest_lib
    out = (C.c_int * 3)()
    selftest_lib().mmhip_selftest_gauss_line_plan(n, lines, float(np.float32(sigma)), 1 if tolerance else 0, out)
    return out[0], out[1], out[2]


def frame_plans(w, h, hs, vs, tolerance=False):
    """The plans of the vertical pass (n = h, lines = w) and of the horizontal one (n = w, lines = h)."""
    return line_plan(h, w, vs, tolerance), line_plan(w, h, hs, tolerance)


def case_seed(w, h):
    return w * 1000 + h


def ulp_distance(a, b):
    """(largest distance in float32 ulps, number of elements that differ) of two finite float32 maps."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    d = np.abs(key(a) - key(b))
    return int(d.max()) if d.size else 0, int(np.count_nonzero(d))
