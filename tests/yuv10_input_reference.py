"""NumPy restatement of 10-bit planar Y'CbCr 4:2:0 clip input to float frames (mmhip_clip_from_yuv420p10,
include/mmhip.h), written from the statement there and not from csrc/mm_yuv.h: the float32 coefficients derived from Kr
and Kb as exact rationals and proved nearest, the chroma a pixel sees at scale 16 as an exact integer, the matrix with
every step one explicit float32 operation, and a parser of YUV4MPEG2 files of either depth.  The layout helpers and the
standards' constants are those of tests/yuv10_reference.py."""
from fractions import Fraction

import numpy as np

from tests.yuv10_reference import (CONSTANTS, EXCURSIONS, MATRIX_IDS, MODES, RANGE_IDS, chroma_size, frame_bytes,  # noqa: F401
                                   frame_samples, plane_offsets)

CHROMAS = ("bilinear", "replicate")
CHROMA_IDS = {"bilinear": 0, "replicate": 1}
F32 = np.float32


def exact_coefficients(mode):
    """(rcr, gcb, gcr, bcb) as exact rationals per 1/16 chroma unit."""
    kr, kb = CONSTANTS[mode[0]]
    kg = 1 - kr - kb
    scale = 16 * EXCURSIONS[mode[1]][2]
    return (2 * (1 - kr) / scale, -2 * (1 - kb) * kb / (kg * scale), -2 * (1 - kr) * kr / (kg * scale), 2 * (1 - kb) / scale)


def nearest_float32(q):
    """The float32 nearest to the rational q, proved against both of its float32 neighbours."""
    f = F32(float(q))      # (float(Fraction) is correctly rounded to float64; the proof below does not rely on the second rounding)
    below, above = np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))
    here = abs(Fraction(float(f)) - q)
    assert here < abs(Fraction(float(below)) - q) and here < abs(Fraction(float(above)) - q), (q, f)
    return f


# mode -> off, E, (rcr, gcb, gcr, bcb) as float32
TABLES = {mode: (EXCURSIONS[mode[1]][0], EXCURSIONS[mode[1]][1], tuple(nearest_float32(q) for q in exact_coefficients(mode))) for mode in MODES}


def hex_table(mode):
    """The coefficients as C hex-float literals, the way the headers list them."""
    return tuple(float(c).hex().replace("0000000p", "p") + "f" for c in TABLES[mode][2])


def seen_chroma16(plane, w, h, chroma):
    """One chroma plane, integers [ch, cw] already limited to 0 .. 1023 -> int64 [h, w]: the chroma every pixel sees, at
    scale 16, exact."""
    cw, ch = chroma_size(w, h)
    c = np.asarray(plane).astype(np.int64).reshape(ch, cw)
    x, y = np.arange(w), np.arange(h)
    cx, cy = x >> 1, y >> 1
    if chroma == "replicate":
        return 16 * c[cy][:, cx]
    assert chroma == "bilinear", chroma
    nx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
    ny = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
    return 9 * c[cy][:, cx] + 3 * c[cy][:, nx] + 3 * c[ny][:, cx] + c[ny][:, nx]


def matrix(y, s_cb, s_cr, mode):
    """Integer arrays of Y (0 .. 1023) and of the seen chroma at scale 16 -> (R, G, B) float32 arrays.  Every line is one
    float32 operation, rounded to nearest."""
    off, e, (rcr, gcb, gcr, bcb) = TABLES[mode]
    yf = (np.asarray(y).astype(np.int64) - off).astype(F32)
    uf = (np.asarray(s_cb).astype(np.int64) - 8192).astype(F32)
    vf = (np.asarray(s_cr).astype(np.int64) - 8192).astype(F32)
    assert yf.dtype == uf.dtype == vf.dtype == F32
    lum = yf / F32(e)
    r_c = vf * rcr
    r = lum + r_c
    g_u = uf * gcb
    g_lu = lum + g_u
    g_v = vf * gcr
    g = g_lu + g_v
    b_c = uf * bcb
    b = lum + b_c
    for v in (lum, r_c, r, g_u, g_lu, g_v, g, b_c, b):
        assert v.dtype == F32
    return r, g, b


def planes_of(payload, w, h):
    """One frame's payload uint16 [frame_samples] -> (Y [h, w], Cb [ch, cw], Cr [ch, cw]), every sample min(s, 1023)."""
    cw, ch = chroma_size(w, h)
    _, cb_at, cr_at = plane_offsets(w, h)
    p = np.minimum(np.asarray(payload, np.uint16).reshape(-1), 1023)
    assert p.size == frame_samples(w, h), (p.size, w, h)
    return p[:cb_at].reshape(h, w), p[cb_at:cr_at].reshape(ch, cw), p[cr_at:].reshape(ch, cw)


def float_frame(payload, w, h, mode, chroma):
    """One frame's payload -> float32 [h, w, 4]: R, G, B and alpha 1."""
    y, cb, cr = planes_of(payload, w, h)
    r, g, b = matrix(y, seen_chroma16(cb, w, h, chroma), seen_chroma16(cr, w, h, chroma), mode)
    return np.stack([r, g, b, np.ones_like(r)], axis=-1)


def float_frames(yuv, w, h, mode, chroma):
    """uint16 [N, frame_samples] (or one frame) -> float32 [N, h, w, 4]."""
    yuv = np.asarray(yuv, np.uint16)
    if yuv.ndim == 1:
        yuv = yuv[None]
    return np.stack([float_frame(p, w, h, mode, chroma) for p in yuv])


def parse_y4m(data, max_frames=None):
    """A file's bytes -> (uint8 [N, frame_bytes] for an 8-bit stream or uint16 [N, frame_samples] for C420p10, w, h,
    (fps_num, fps_den), "limited" / "full" / None).  Samples of a 10-bit stream are little-endian.  Asserts on everything
    the header statement does not accept."""
    end = data.index(b"\n")
    tags = data[:end].decode("ascii").split()
    assert tags[0] == "YUV4MPEG2", tags
    w = h = None
    fps, rng, deep = (25, 1), None, False
    for tag in tags[1:]:
        key, value = tag[0], tag[1:]
        if key == "W":
            w = int(value)
        elif key == "H":
            h = int(value)
        elif key == "F":
            num, den = value.split(":")
            fps = (int(num), int(den))
        elif key == "I":
            assert value in ("p", "?"), tag
        elif key == "C":
            assert value in ("420jpeg", "420mpeg2", "420paldv", "420", "420p10"), tag
            deep = value == "420p10"
        elif key == "X":
            if value.startswith("COLORRANGE="):
                rng = {"FULL": "full", "LIMITED": "limited"}[value.split("=")[1]]
        else:
            assert key == "A", tag
    assert w and h and w > 0 and h > 0
    n = frame_samples(w, h)
    size = 2 * n if deep else n
    at, out = end + 1, []
    while at < len(data) and (max_frames is None or len(out) < max_frames):
        nl = data.index(b"\n", at)
        assert data[at:at + 5] == b"FRAME" and data[at + 5:at + 6] in (b" ", b"\n"), data[at:at + 16]
        at = nl + 1
        assert at + size <= len(data), "a truncated frame"
        out.append(np.frombuffer(data, "<u2", n, at).astype(np.uint16) if deep else np.frombuffer(data, np.uint8, n, at))
        at += size
    assert out, "no frames"
    return np.stack(out), w, h, fps, rng
