"""NumPy restatement of planar Y'CbCr 4:2:0 clip input (mmhip_clip_from_yuv420, include/mmhip.h), written from the
statement there and not from csrc/mm_yuv.h: the table, the coefficients derived from Kr and Kb by the stated rule, both
chroma modes and the matrix in int64 with floor division, and a parser of YUV4MPEG2 files.  The layout helpers are those
of tests/yuv_reference.py."""
import math

import numpy as np

from tests.yuv_reference import MATRIX_IDS, MODES, RANGE_IDS, chroma_size, frame_bytes, plane_offsets  # noqa: F401

# (matrix, range) -> off, ky, rcr, gcb, gcr, bcb
TABLES = {
    ("bt601", "limited"): (16, 76309, 104597, -25675, -53279, 132201),
    ("bt601", "full"): (0, 65536, 91881, -22553, -46802, 116130),
    ("bt709", "limited"): (16, 76309, 117489, -13975, -34925, 138438),
    ("bt709", "full"): (0, 65536, 103206, -12276, -30679, 121609),
}
CHROMAS = ("bilinear", "replicate")
CHROMA_IDS = {"bilinear": 0, "replicate": 1}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def derived(mode):
    """The row of the table from the standard's constants: magnitudes rounded as floor(|k| * 2^16 + 0.5), the sign kept."""
    kr, kb = KR_KB[mode[0]]
    kg = 1 - kr - kb
    luma_scale, chroma_scale, off = (255 / 219, 255 / 224, 16) if mode[1] == "limited" else (1.0, 1.0, 0)

    def fixed(k):
        return int(math.copysign(math.floor(abs(k) * 2 ** 16 + 0.5), k))
    return (off, fixed(luma_scale), fixed(2 * (1 - kr) * chroma_scale), fixed(-2 * (1 - kb) * kb / kg * chroma_scale),
            fixed(-2 * (1 - kr) * kr / kg * chroma_scale), fixed(2 * (1 - kb) * chroma_scale))


def matrix(y, cb, cr, mode):
    """Integer arrays of Y and of the chroma the pixels see -> (R, G, B) int64 arrays, clamped to 0 .. 255."""
    off, ky, rcr, gcb, gcr, bcb = TABLES[mode]
    y = np.asarray(y).astype(np.int64) - off
    u = np.asarray(cb).astype(np.int64) - 128
    v = np.asarray(cr).astype(np.int64) - 128
    r = (ky * y + rcr * v + 2 ** 15) // 2 ** 16
    g = (ky * y + gcb * u + gcr * v + 2 ** 15) // 2 ** 16
    b = (ky * y + bcb * u + 2 ** 15) // 2 ** 16
    return np.clip(r, 0, 255), np.clip(g, 0, 255), np.clip(b, 0, 255)


def intermediates(y, cb, cr, mode):
    """Every value the matrix forms before a shift, as int64 arrays: what must stay inside int32."""
    off, ky, rcr, gcb, gcr, bcb = TABLES[mode]
    y = np.asarray(y).astype(np.int64) - off
    u = np.asarray(cb).astype(np.int64) - 128
    v = np.asarray(cr).astype(np.int64) - 128
    return [ky * y, rcr * v, gcb * u, gcr * v, bcb * u, ky * y + 2 ** 15, ky * y + rcr * v + 2 ** 15, ky * y + gcb * u, ky * y + gcb * u + gcr * v + 2 ** 15,
            ky * y + bcb * u + 2 ** 15]


def seen_chroma(plane, w, h, chroma):
    """One chroma plane uint8 [ch, cw] -> int64 [h, w]: the chroma every pixel sees."""
    cw, ch = chroma_size(w, h)
    c = np.asarray(plane).astype(np.int64).reshape(ch, cw)
    x, y = np.arange(w), np.arange(h)
    cx, cy = x >> 1, y >> 1
    if chroma == "replicate":
        return c[cy][:, cx]
    assert chroma == "bilinear", chroma
    nx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
    ny = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
    return (9 * c[cy][:, cx] + 3 * c[cy][:, nx] + 3 * c[ny][:, cx] + c[ny][:, nx] + 8) // 16


def planes_of(payload, w, h):
    """One frame's payload uint8 [frame_bytes] -> (Y [h, w], Cb [ch, cw], Cr [ch, cw])."""
    cw, ch = chroma_size(w, h)
    _, cb_at, cr_at = plane_offsets(w, h)
    p = np.asarray(payload, np.uint8).reshape(-1)
    assert p.size == frame_bytes(w, h), (p.size, w, h)
    return p[:cb_at].reshape(h, w), p[cb_at:cr_at].reshape(ch, cw), p[cr_at:].reshape(ch, cw)


def rgba_frame(payload, w, h, mode, chroma):
    """One frame's payload -> uint8 [h, w, 4]: R, G, B and alpha 255."""
    y, cb, cr = planes_of(payload, w, h)
    r, g, b = matrix(y, seen_chroma(cb, w, h, chroma), seen_chroma(cr, w, h, chroma), mode)
    return np.stack([r, g, b, np.full_like(r, 255)], axis=-1).astype(np.uint8)


def rgba_frames(yuv, w, h, mode, chroma):
    """uint8 [N, frame_bytes] (or one frame) -> uint8 [N, h, w, 4]."""
    yuv = np.asarray(yuv, np.uint8)
    if yuv.ndim == 1:
        yuv = yuv[None]
    return np.stack([rgba_frame(p, w, h, mode, chroma) for p in yuv])


def words(rgba):
    """uint8 [..., 4] RGBA -> uint32 [...]: the drawable's words R << 24 | G << 16 | B << 8 | A."""
    p = np.asarray(rgba).astype(np.uint32)
    return p[..., 0] << 24 | p[..., 1] << 16 | p[..., 2] << 8 | p[..., 3]


def parse_y4m(data, max_frames=None):
    """A file's bytes -> (uint8 [N, frame_bytes], w, h, (fps_num, fps_den), "limited" / "full" / None).  FRAME lines may
    carry parameters.  Accepts what the header statement accepts; asserts on everything else."""
    end = data.index(b"\n")
    tags = data[:end].decode("ascii").split()
    assert tags[0] == "YUV4MPEG2", tags
    w = h = None
    fps, rng = (25, 1), None
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
            assert value in ("420jpeg", "420mpeg2", "420paldv", "420"), tag
        elif key == "X":
            if value.startswith("COLORRANGE="):
                rng = {"FULL": "full", "LIMITED": "limited"}[value.split("=")[1]]
        else:
            assert key == "A", tag
    assert w and h and w > 0 and h > 0
    n = frame_bytes(w, h)
    at, out = end + 1, []
    while at < len(data) and (max_frames is None or len(out) < max_frames):
        nl = data.index(b"\n", at)
        assert data[at:at + 5] == b"FRAME" and data[at + 5:at + 6] in (b" ", b"\n"), data[at:at + 16]
        at = nl + 1
        assert at + n <= len(data), "a truncated frame"
        out.append(np.frombuffer(data, np.uint8, n, at))
        at += n
    assert out, "no frames"
    return np.stack(out), w, h, fps, rng
