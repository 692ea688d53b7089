"""NumPy and Python-int restatement of the four 4:2:0 converters with a chroma siting (the mmhip_..._sited entry points,
include/mmhip.h), written from the statement there and not from csrc/mm_yuv.h: left siting's six pixels with the weights
1, 2, 1 per row and the clamped columns, its two chroma formulas (Python ints for the 10-bit one, so nothing can wrap), and
the chroma a pixel sees from its own and its right chroma column.  The layout helpers, the mode tables, luma and the
matrix steps are those of tests/yuv_reference.py, yuv10_reference.py, yuv_input_reference.py and yuv10_input_reference.py;
with siting "center" every function here is the function there."""
import numpy as np

from tests import yuv10_input_reference as R10I
from tests import yuv10_reference as R10
from tests import yuv_input_reference as RI
from tests import yuv_reference as R8
from tests.yuv_reference import MATRIX_IDS, MODES, RANGE_IDS, chroma_size  # noqa: F401

SITINGS = ("center", "left")
SITING_IDS = {"center": 0, "left": 1}
CHROMAS = RI.CHROMAS
CHROMA_IDS = RI.CHROMA_IDS
# the weights of the pixel columns 2 cx - 1, 2 cx, 2 cx + 1 (each over two rows of weight 1), and of the chroma columns
# (own, right) an even and an odd pixel column see
OUT_WEIGHTS = (1, 2, 1)
IN_WEIGHTS = {0: (4, 0), 1: (2, 2)}


def _siting(siting):
    assert siting in SITINGS, siting
    return siting == "left"


def left_sums(p):
    """p: integer [h, w, >= 3] -> int64 [ch, cw, 3]: the weighted sums over the columns clamp(2 cx - 1 + i, 0, w - 1), weights
    1, 2, 1, and the rows min(2 cy + j, h - 1), weight 1 each."""
    h, w = p.shape[:2]
    cw, ch = chroma_size(w, h)
    p = np.asarray(p)[..., :3].astype(np.int64)
    total = np.zeros((ch, cw, 3), np.int64)
    for j in (0, 1):
        rows = np.minimum(2 * np.arange(ch) + j, h - 1)
        for i, weight in enumerate(OUT_WEIGHTS):
            cols = np.clip(2 * np.arange(cw) - 1 + i, 0, w - 1)
            total += weight * p[rows][:, cols]
    return total


def left_chroma(sums, table, shift, mid, top):
    """sums: integer [..., 3] -> (Cb, Cr) int64 [...]: clamp(floor((k . sums + 2^(shift - 1)) / 2^shift) + mid, 0, top), every
    product and sum a Python int."""
    _, _, cb, cr = table
    s = np.asarray(sums).astype(np.int64)
    flat = s.reshape(-1, 3).tolist()
    out = []
    for kr, kg, kb in (cb, cr):
        values = [min(max((kr * rs + kg * gs + kb * bs + (1 << (shift - 1))) // (1 << shift) + mid, 0), top) for rs, gs, bs in flat]
        out.append(np.array(values, np.int64).reshape(s.shape[:-1]))
    return out[0], out[1]


def left_intermediate(sums, row):
    """The value the chroma formula forms before its shift, without the rounding term, as a Python int."""
    return sum(int(k) * int(s) for k, s in zip(row, sums))


# ---- out, 8 bits: RGBA8 frames to payloads ----
def planes8(rgba, mode, siting):
    """One frame, uint8 [h, w, 4] (or 3) -> (Y [h, w], Cb [ch, cw], Cr [ch, cw]) uint8."""
    if not _siting(siting):
        return R8.planes(rgba, mode)
    y = R8.luma(rgba, mode)
    cb, cr = left_chroma(left_sums(rgba), R8.TABLES[mode], 19, 128, 255)
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def frame8(rgba, mode, siting):
    return np.concatenate([p.reshape(-1) for p in planes8(rgba, mode, siting)])


def frames8(clip, mode, siting):
    """uint8 [N, h, w, 4] -> uint8 [N, frame_bytes]."""
    return np.stack([frame8(f, mode, siting) for f in clip])


# ---- out, 10 bits: float frames to payloads of 16-bit samples ----
def planes10(pixels, mode, siting):
    """One frame, float32 [h, w, 4] (or 3) -> (Y [h, w], Cb [ch, cw], Cr [ch, cw]) uint16."""
    if not _siting(siting):
        return R10.planes(pixels, mode)
    q = R10.quant(np.asarray(pixels, np.float32)[..., :3])
    y = R10.luma(q, mode)
    cb, cr = left_chroma(left_sums(q), R10.TABLES[mode], 22, 512, 1023)
    return y.astype(np.uint16), cb.astype(np.uint16), cr.astype(np.uint16)


def frame10(pixels, mode, siting):
    return np.concatenate([p.reshape(-1) for p in planes10(pixels, mode, siting)])


def frames10(clip, mode, siting):
    """float32 [N, h, w, 4] -> uint16 [N, frame_samples]."""
    return np.stack([frame10(f, mode, siting) for f in clip])


# ---- in: the chroma a pixel sees ----
def left_seen16(plane, w, h):
    """One chroma plane, integers [ch, cw] -> int64 [h, w]: the chroma every pixel sees with left siting in bilinear mode,
    at scale 16 and exact: col(i) = 3 C[cy][i] + C[ny][i]; 4 col(cx) for an even x, 2 col(cx) + 2 col(r) for an odd one."""
    cw, ch = chroma_size(w, h)
    c = np.asarray(plane).astype(np.int64).reshape(ch, cw)
    x, y = np.arange(w), np.arange(h)
    cx, cy = x >> 1, y >> 1
    ny = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
    r = np.minimum(cx + 1, cw - 1)
    col = 3 * c[cy] + c[ny]                 # [h, cw]
    own = np.array([IN_WEIGHTS[int(v) & 1][0] for v in x], np.int64)
    right = np.array([IN_WEIGHTS[int(v) & 1][1] for v in x], np.int64)
    return own * col[:, cx] + right * col[:, r]


def seen8(plane, w, h, chroma, siting):
    if not _siting(siting) or chroma == "replicate":
        return RI.seen_chroma(plane, w, h, chroma)
    assert chroma == "bilinear", chroma
    return (left_seen16(plane, w, h) + 8) // 16


def seen16(plane, w, h, chroma, siting):
    if not _siting(siting) or chroma == "replicate":
        return R10I.seen_chroma16(plane, w, h, chroma)
    assert chroma == "bilinear", chroma
    return left_seen16(plane, w, h)


def rgba_frames(yuv, w, h, mode, chroma, siting):
    """uint8 [N, frame_bytes] (or one frame) -> uint8 [N, h, w, 4]."""
    yuv = np.asarray(yuv, np.uint8)
    if yuv.ndim == 1:
        yuv = yuv[None]
    out = []
    for payload in yuv:
        y, cb, cr = RI.planes_of(payload, w, h)
        r, g, b = RI.matrix(y, seen8(cb, w, h, chroma, siting), seen8(cr, w, h, chroma, siting), mode)
        out.append(np.stack([r, g, b, np.full_like(r, 255)], axis=-1).astype(np.uint8))
    return np.stack(out)


def float_frames(yuv, w, h, mode, chroma, siting):
    """uint16 [N, frame_samples] (or one frame) -> float32 [N, h, w, 4]."""
    yuv = np.asarray(yuv, np.uint16)
    if yuv.ndim == 1:
        yuv = yuv[None]
    out = []
    for payload in yuv:
        y, cb, cr = R10I.planes_of(payload, w, h)
        r, g, b = R10I.matrix(y, seen16(cb, w, h, chroma, siting), seen16(cr, w, h, chroma, siting), mode)
        out.append(np.stack([r, g, b, np.ones_like(r)], axis=-1))
    return np.stack(out)


def y4m_header(w, h, fps=(25, 1), yuv_range="limited", bits=8, siting="center"):
    tag = "C420p10" if bits == 10 else "C420mpeg2" if _siting(siting) else "C420jpeg"
    return ("YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=%s\n" % (w, h, fps[0], fps[1], tag, yuv_range.upper())).encode("ascii")
