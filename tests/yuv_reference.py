"""NumPy restatement of the planar Y'CbCr 4:2:0 clip output (mmhip_clip_to_yuv420, include/mmhip.h), written from the
statement there and not from csrc/mm_yuv.h: the tables, the two formulas in int64 with floor division, the replication of
an odd last column and row, the layout of a frame and the framing of a YUV4MPEG2 file."""
import numpy as np

# (matrix, range) -> off, (yr, yg, yb), (cbr, cbg, cbb), (crr, crg, crb)
TABLES = {
    ("bt601", "limited"): (16, (16829, 33039, 6416), (-9714, -19071, 28785), (28784, -24103, -4681)),
    ("bt601", "full"): (0, (19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329)),
    ("bt709", "limited"): (16, (11966, 40254, 4064), (-6596, -22189, 28785), (28784, -26145, -2639)),
    ("bt709", "full"): (0, (13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005)),
}
MODES = list(TABLES)
MATRIX_IDS = {"bt601": 0, "bt709": 1}
RANGE_IDS = {"limited": 0, "full": 1}


def chroma_size(w, h):
    return (w + 1) >> 1, (h + 1) >> 1


def frame_bytes(w, h):
    cw, ch = chroma_size(w, h)
    return w * h + 2 * cw * ch


def plane_offsets(w, h):
    """Byte offsets of Y, Cb and Cr in a frame."""
    cw, ch = chroma_size(w, h)
    return 0, w * h, w * h + cw * ch


def luma(rgb, mode):
    """rgb: integer [..., 3 or 4] -> int64 [...]"""
    off, (yr, yg, yb), _, _ = TABLES[mode]
    p = np.asarray(rgb).astype(np.int64)
    return (yr * p[..., 0] + yg * p[..., 1] + yb * p[..., 2] + 2 ** 15) // 2 ** 16 + off


def chroma(sums, mode):
    """sums: integer [..., 3], the sums of a block's four pixels -> (Cb, Cr) int64 [...]"""
    _, _, cb, cr = TABLES[mode]
    s = np.asarray(sums).astype(np.int64)
    out = []
    for kr, kg, kb in (cb, cr):
        out.append(np.clip((kr * s[..., 0] + kg * s[..., 1] + kb * s[..., 2] + 2 ** 17) // 2 ** 18 + 128, 0, 255))
    return out[0], out[1]


def block_sums(rgba):
    """rgba: uint8 [h, w, >= 3] -> int64 [ch, cw, 3]: the sums over (min(2 cx + i, w - 1), min(2 cy + j, h - 1))."""
    h, w = rgba.shape[:2]
    cw, ch = chroma_size(w, h)
    p = np.asarray(rgba)[..., :3].astype(np.int64)
    total = np.zeros((ch, cw, 3), np.int64)
    for j in (0, 1):
        rows = np.minimum(2 * np.arange(ch) + j, h - 1)
        for i in (0, 1):
            cols = np.minimum(2 * np.arange(cw) + i, w - 1)
            total += p[rows][:, cols]
    return total


def planes(rgba, mode):
    """One frame, uint8 [h, w, 4] (or 3) -> (Y [h, w], Cb [ch, cw], Cr [ch, cw]) uint8."""
    y = luma(rgba, mode)
    cb, cr = chroma(block_sums(rgba), mode)
    assert y.min() >= 0 and y.max() <= 255
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def frame(rgba, mode):
    """One frame's payload: uint8 [frame_bytes]."""
    return np.concatenate([p.reshape(-1) for p in planes(rgba, mode)])


def frames(clip, mode):
    """uint8 [N, h, w, 4] -> uint8 [N, frame_bytes]."""
    return np.stack([frame(f, mode) for f in clip])


def band_mask(w, h, first_row, last_row):
    """bool [frame_bytes]: the bytes a band writes -- Y rows [first_row, last_row), chroma rows [first_row / 2, (last_row + 1) / 2)."""
    cw, ch = chroma_size(w, h)
    y = np.zeros((h, w), bool)
    y[first_row:last_row] = True
    c = np.zeros((ch, cw), bool)
    c[first_row // 2:(last_row + 1) // 2] = True
    return np.concatenate([y.reshape(-1), c.reshape(-1), c.reshape(-1)])


def y4m_header(w, h, fps=(25, 1), yuv_range="limited"):
    return ("YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=%s\n" % (w, h, fps[0], fps[1], yuv_range.upper())).encode("ascii")


def y4m_file(payloads, w, h, fps=(25, 1), yuv_range="limited"):
    """The bytes of the file: the header, then FRAME and the payload per frame."""
    out = [y4m_header(w, h, fps, yuv_range)]
    for p in payloads:
        out += [b"FRAME\n", np.asarray(p, np.uint8).tobytes()]
    return b"".join(out)


def parse_y4m(data):
    """(header fields as a dict of tag letter / X name -> text, uint8 [N, frame_bytes]) of a file's bytes."""
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
    w, h = int(fields["W"]), int(fields["H"])
    n = frame_bytes(w, h)
    at, out = end + 1, []
    while at < len(data):
        assert data[at:at + 6] == b"FRAME\n", data[at:at + 16]
        at += 6
        assert at + n <= len(data), "a truncated frame"
        out.append(np.frombuffer(data, np.uint8, n, at))
        at += n
    return fields, (np.stack(out) if out else np.zeros((0, n), np.uint8))
