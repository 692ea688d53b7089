"""NumPy restatement of the 10-bit planar Y'CbCr 4:2:0 clip output from float frames (mmhip_clip_float_to_yuv420p10,
include/mmhip.h), written from the statement there and not from csrc/mm_yuv.h: the rule that gives the coefficient
tables, the quantisation in float32, the two formulas in int64 with floor division, the replication of an odd last column
and row, the layout of a frame in 16-bit samples, the framing of a C420p10 YUV4MPEG2 file and a parser for it."""
from fractions import Fraction

import numpy as np

MATRIX_IDS = {"bt601": 0, "bt709": 1}
RANGE_IDS = {"limited": 0, "full": 1}
# the standards' constants (Kr, Kb), exactly as they are written
CONSTANTS = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}
# range -> off, luma excursion, chroma excursion, with the channel in 0 .. 65535
EXCURSIONS = {"limited": (64, 876, 896), "full": (0, 1023, 1023)}
LUMA_SHIFT, CHROMA_SHIFT = 20, 19


def _round(x):
    """floor(|x| + 0.5) with the sign of x, exactly."""
    q = (abs(x) + Fraction(1, 2)).__floor__()
    return q if x >= 0 else -q


def derive_table(matrix, rng):
    """off, (yr, yg, yb), (cbr, cbg, cbb), (crr, crg, crb) by the rule of the header."""
    kr, kb = CONSTANTS[matrix]
    kg = 1 - kr - kb
    off, ey, ec = EXCURSIONS[rng]
    ys, cs = Fraction(ey, 65535) * 2 ** LUMA_SHIFT, Fraction(ec, 65535) * 2 ** CHROMA_SHIFT
    yr, yb = _round(kr * ys), _round(kb * ys)
    yg = _round(1 * ys) - yr - yb                       # the row sums to the rounded coefficient of k = 1
    cb_row = (-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), Fraction(1, 2))
    cr_row = (Fraction(1, 2), -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr)))
    cbr, cbb = _round(cb_row[0] * cs), _round(cb_row[2] * cs)
    crr, crb = _round(cr_row[0] * cs), _round(cr_row[2] * cs)
    return off, (yr, yg, yb), (cbr, -cbr - cbb, cbb), (crr, -crr - crb, crb)      # each chroma row sums to 0


TABLES = {(m, r): derive_table(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")}
MODES = list(TABLES)


def chroma_size(w, h):
    return (w + 1) >> 1, (h + 1) >> 1


def frame_samples(w, h):
    cw, ch = chroma_size(w, h)
    return w * h + 2 * cw * ch


def frame_bytes(w, h):
    return 2 * frame_samples(w, h)


def plane_offsets(w, h):
    """Sample offsets of Y, Cb and Cr in a frame (the byte offsets are twice these)."""
    cw, ch = chroma_size(w, h)
    return 0, w * h, w * h + cw * ch


def quant(v):
    """float32 [...] -> int32 [...]: CLAMP01 as the pixel store clamps (NaN and -0 give 0), one float32 product, rounded to
    nearest with ties to even."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(v > 0, np.where(v > 1, np.float32(1), v), np.float32(0)).astype(np.float32)
    return np.rint(c * np.float32(65535)).astype(np.int32)


def luma(q, mode):
    """q: integer [..., 3 or 4], quantised channels -> int64 [...]"""
    off, (yr, yg, yb), _, _ = TABLES[mode]
    p = np.asarray(q).astype(np.int64)
    return (yr * p[..., 0] + yg * p[..., 1] + yb * p[..., 2] + 2 ** 19) // 2 ** 20 + off


def chroma(sums, mode, clamp=True):
    """sums: integer [..., 3], the sums of a block's four quantised pixels -> (Cb, Cr) int64 [...]"""
    _, _, cb, cr = TABLES[mode]
    s = np.asarray(sums).astype(np.int64)
    out = []
    for kr, kg, kb in (cb, cr):
        c = (kr * s[..., 0] + kg * s[..., 1] + kb * s[..., 2] + 2 ** 20) // 2 ** 21 + 512
        out.append(np.clip(c, 0, 1023) if clamp else c)
    return out[0], out[1]


def block_sums(q):
    """q: integer [h, w, >= 3] -> int64 [ch, cw, 3]: the sums over (min(2 cx + i, w - 1), min(2 cy + j, h - 1))."""
    h, w = q.shape[:2]
    cw, ch = chroma_size(w, h)
    p = np.asarray(q)[..., :3].astype(np.int64)
    total = np.zeros((ch, cw, 3), np.int64)
    for j in (0, 1):
        rows = np.minimum(2 * np.arange(ch) + j, h - 1)
        for i in (0, 1):
            cols = np.minimum(2 * np.arange(cw) + i, w - 1)
            total += p[rows][:, cols]
    return total


def planes(pixels, mode):
    """One frame, float32 [h, w, 4] (or 3) -> (Y [h, w], Cb [ch, cw], Cr [ch, cw]) uint16."""
    q = quant(np.asarray(pixels, np.float32)[..., :3])
    y = luma(q, mode)
    cb, cr = chroma(block_sums(q), mode)
    assert y.min() >= 0 and y.max() <= 1023
    return y.astype(np.uint16), cb.astype(np.uint16), cr.astype(np.uint16)


def frame(pixels, mode):
    """One frame's payload: uint16 [frame_samples]."""
    return np.concatenate([p.reshape(-1) for p in planes(pixels, mode)])


def frames(clip, mode):
    """float32 [N, h, w, 4] -> uint16 [N, frame_samples]."""
    return np.stack([frame(f, mode) for f in clip])


def band_mask(w, h, first_row, last_row):
    """bool [frame_samples]: the samples a band writes -- Y rows [first_row, last_row), chroma rows [first_row / 2,
    (last_row + 1) / 2)."""
    cw, ch = chroma_size(w, h)
    y = np.zeros((h, w), bool)
    y[first_row:last_row] = True
    c = np.zeros((ch, cw), bool)
    c[first_row // 2:(last_row + 1) // 2] = True
    return np.concatenate([y.reshape(-1), c.reshape(-1), c.reshape(-1)])


def exact(rgb, mode):
    """The float64 formula the integers approximate: rgb float64 [..., 3] in 0 .. 1 (one colour for the whole block) ->
    (Y, Cb, Cr) float64, unrounded and unclamped."""
    kr, kb = [float(k) for k in CONSTANTS[mode[0]]]
    off, ey, ec = EXCURSIONS[mode[1]]
    p = np.asarray(rgb, np.float64)
    y = kr * p[..., 0] + (1 - kr - kb) * p[..., 1] + kb * p[..., 2]
    return off + ey * y, 512 + ec * (p[..., 2] - y) / (2 * (1 - kb)), 512 + ec * (p[..., 0] - y) / (2 * (1 - kr))


def y4m_header(w, h, fps=(25, 1), yuv_range="limited"):
    return ("YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420p10 XCOLORRANGE=%s\n" % (w, h, fps[0], fps[1], yuv_range.upper())).encode("ascii")


def y4m_file(payloads, w, h, fps=(25, 1), yuv_range="limited"):
    """The bytes of the file: the header, then FRAME and the payload per frame, every sample little-endian."""
    out = [y4m_header(w, h, fps, yuv_range)]
    for p in payloads:
        out += [b"FRAME\n", np.asarray(p).astype("<u2").tobytes()]
    return b"".join(out)


def parse_y4m(data):
    """(header fields as a dict of tag letter / X name -> text, uint16 [N, frame_samples]) of a C420p10 file's bytes."""
    end = data.index(b"\n")
    words = data[:end].decode("ascii").split(" ")
    assert words[0] == "YUV4MPEG2", words
    fields = {}
    for word in words[1:]:
        if word.startswith("X"):
            name, _, value = word[1:].partition("=")
            fields["X" + name] = value
        else:
            fields[word[0]] = word[1:]
    assert fields["C"] == "420p10", fields
    w, h = int(fields["W"]), int(fields["H"])
    n = frame_samples(w, h)
    at, out = end + 1, []
    while at < len(data):
        assert data[at:at + 6] == b"FRAME\n", data[at:at + 16]
        at += 6
        assert at + 2 * n <= len(data), "a truncated frame"
        out.append(np.frombuffer(data, "<u2", n, at).astype(np.uint16))
        at += 2 * n
    return fields, (np.stack(out) if out else np.zeros((0, n), np.uint16))
