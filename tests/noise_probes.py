"""Cases of the float-for-float check of the noise builtins (noise, noiseBillow, noiseRidgedMulti, voronoiCells;
mathmap_amd/csrc/mm_noise_device.h) against the reference's libnoise, which the oracle links (oracle/noise_wrap.cpp).

Coordinates are xyz:[x * s + ox, y * s + oy, oz] over a 64 x 64 frame, so x runs over ox +- s and y over oy +- s: oy = -ox
puts the negative side of every edge into the same frame.  tests/make_noise_float.py records the oracle's floats as
tests/golden/noise_float/*.npy, for machines without the oracle's noise library; tests/test_noise_float_recording.py
checks the recording against a live render where the library is there, tests/test_gpu_noise_float.py holds the GPU to it."""
import os

import numpy as np

SIZE = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_float")
UV = ("s", "ox", "oy", "oz", "oct", "per", "lac")
HEAD = ("filter n (float s: 0-100 (1), float ox: 0-100 (0), float oy: 0-100 (0), float oz: 0-100 (0), float oct: 1-30 (6), "
        "float per: 0-1 (0.5), float lac: 0-4 (2))\n  p = xyz:[x * s + ox, y * s + oy, oz];\n")
# the three fractal sums with their parameters, and the cells
FULL = HEAD + "  rgba:[noise(oct, per, lac, p), noiseBillow(oct, per, lac, p), noiseRidgedMulti(oct, lac, p), voronoiCells(p)]\nend\n"
# the one-argument form: one octave
SIMPLE = HEAD + "  w = noise(p);\n  rgba:[w, w, w, w]\nend\n"
IDS = {"full": {"noise_perlin_full", "noise_billow", "noise_ridged_multi", "noise_voronoi"}, "simple": {"noise_perlin_simple"}}

# (name, s, ox, oz): fractional and exactly integral coordinates around every edge.  x * 31.5 + 0.5 is an integer for every
# pixel of a 64-pixel row; beyond 2^24 every float is one, and oz carries the fraction.
COORDINATES = [
    ("unit_frac", 2.5, 0.3, 0.37),                 # the lattice around 0 and +-1: (int)x - 1 for negative x
    ("unit_int", 31.5, 0.5, 3.0),                  # integers -31 .. 32
    ("byte_frac", 2.5, 255.3, 0.37),               # around +-255 and +-256: the hash's low byte
    ("byte_int", 31.5, 255.5, 3.0),
    ("p24_frac", 31.5, 16777216.0, 0.37), ("p24_int", 31.5, 16777216.0, 3.0),
    ("p30_frac", 4096.0, 1073741824.0, 0.37), ("p30_int", 4096.0, 1073741824.0, 3.0),        # 2^30 - 64 .. 2^30 + 128: the range reduction's edge
    ("p31_frac", 8192.0, 2147483648.0, 0.37), ("p31_int", 8192.0, 2147483648.0, 3.0),        # beyond int in voronoiCells
    ("3e9_frac", 10000.0, 3e9, 0.37), ("3e9_int", 10000.0, 3e9, 3.0),
    ("1e12_frac", 1e6, 1e12, 0.37), ("1e12_int", 1e6, 1e12, 3.0),
]
OCTAVES = (1, 6, 30)               # libnoise throws outside 1 .. 30
PERSISTENCE = (0.0, 0.5, 1.0)
LACUNARITY = (0.0, 1.0, 2.0, 3.1, -2.5, 1e10)
DEFAULT = (6, 0.5, 2.0)


def cases():
    """[(name, kind, user values)]: every coordinate case with the default parameters for both filters; every pair of
    octave count and lacunarity (the persistence taking its three values in turn) around 0; every lacunarity at 2^30"""
    out = []
    for name, s, o, oz in COORDINATES:
        for kind in ("full", "simple"):
            out.append(("%s_%s" % (kind, name), kind, (s, o, -o, oz) + DEFAULT))
    k = 0
    for octv in OCTAVES:
        for lac in LACUNARITY:
            per = PERSISTENCE[k % 3]
            k += 1
            if (octv, per, lac) != DEFAULT:
                out.append(("full_unit_frac_o%d_p%g_l%g" % (octv, per, lac), "full", (2.5, 0.3, -0.3, 0.37, octv, per, lac)))
    for lac in LACUNARITY:
        if lac != DEFAULT[2]:
            out.append(("full_p30_frac_l%g" % lac, "full", (4096.0, 1073741824.0, -1073741824.0, 0.37, 6, 1.0, lac)))
    # lacunarity 1e10 takes a double coordinate to inf only from 1e30 on (1e30 * 1e10^28): the sum is then NaN
    out.append(("full_1e30_o30_l1e+10", "full", (1e28, 1e30, -1e30, 0.37, 30, 0.5, 1e10)))
    assert len(set(c[0] for c in out)) == len(out)
    return out


def uservals(values):
    return dict(zip(UV, [float(np.float32(v)) for v in values]))


# the recording: full frames [n, 64, 64, 4] in files of at most 15 (under 1 MiB each), the one-channel frames of the
# one-argument form [n, 64, 64] in one file, and the names in order
PER_FILE = 15


def recorded():
    """name -> the oracle's floats ([64, 64, 4]; [64, 64] for the one-argument form)"""
    full = [c[0] for c in cases() if c[1] == "full"]
    simple = [c[0] for c in cases() if c[1] == "simple"]
    out = {}
    for i in range(0, len(full), PER_FILE):
        a = np.load(os.path.join(GOLDEN, "full_%d.npy" % (i // PER_FILE)))
        assert a.shape == (len(full[i:i + PER_FILE]), SIZE, SIZE, 4) and a.dtype == np.float32
        out.update(zip(full[i:i + PER_FILE], a))
    a = np.load(os.path.join(GOLDEN, "simple.npy"))
    assert a.shape == (len(simple), SIZE, SIZE) and a.dtype == np.float32
    out.update(zip(simple, a))
    return out


def differing(got, want):
    """(values that differ, NaN positions equal): NaN equals NaN, everything else bit for bit"""
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (nan_g & nan_w)
    return int((~same).sum()), bool(np.array_equal(nan_g, nan_w))
