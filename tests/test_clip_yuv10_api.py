"""Clips as 10-bit planar Y'CbCr 4:2:0 without a GPU (mmhip_clip_float_to_yuv420p10, include/mmhip.h): the entry points
and the header's statement, the tables of tests/yuv10_reference.py re-derived by the rule, the restatement against values
worked out by hand, the int32 bounds, the distance to the float64 formula, the quantiser's edge cases, the layout and the
C420p10 framing, csrc/mm_yuv.h compiled for the host in a stand-alone program (plain and under the sanitizers), every
refusal by its name, the Python keywords and the command line's options."""
import ctypes as C
import io
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd import _lib
from mathmap_amd._lib import lib
from tests import yuv10_reference as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
CSRC = os.path.join(ROOT, "mathmap_amd", "csrc")
RED, GREEN, BLUE, WHITE, BLACK, GREY = (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 0, 0), (0.5, 0.5, 0.5)
CORNERS = [(r, g, b) for r in (0, 65535) for g in (0, 65535) for b in (0, 65535)]
# the table as the issue and the header give it, to hold the rule's result against
STATED = {
    ("bt601", "limited"): (64, (4191, 8227, 1598), (-1210, -2374, 3584), (3584, -3001, -583)),
    ("bt601", "full"): (0, (4894, 9608, 1866), (-1381, -2711, 4092), (4092, -3427, -665)),
    ("bt709", "limited"): (64, (2980, 10024, 1012), (-821, -2763, 3584), (3584, -3255, -329)),
    ("bt709", "full"): (0, (3480, 11706, 1182), (-938, -3154, 4092), (4092, -3717, -375)),
}
# (Y, Cb, Cr) of a block of one colour: the float64 formula rounded, by hand; at full range pure red's Cr and pure blue's
# Cb are 1023.5, which the integers make 1023 (the coefficient 4092.06 is rounded down)
BY_HAND = {
    ("bt709", "limited"): {RED: (250, 409, 960), GREEN: (690, 167, 105), BLUE: (127, 960, 471)},
    ("bt601", "limited"): {RED: (326, 361, 960), GREEN: (578, 215, 137), BLUE: (164, 960, 439)},
    ("bt709", "full"): {RED: (217, 395, 1023), GREEN: (732, 118, 47), BLUE: (74, 1023, 465)},
    ("bt601", "full"): {RED: (306, 339, 1023), GREEN: (600, 173, 84), BLUE: (117, 1023, 429)},
}


def err():
    return lib().mmhip_last_error().decode()


def test_entry_points_exist_and_are_declared():
    api = mm.api
    names = ("mmhip_clip_float_to_yuv420p10", "mmhip_yuv420p10_frame_bytes", "mmhip_y4m_header_p10", "mmhip_clip_float_to_yuv420p10_launches")
    for name in names:
        assert name in _lib.SYMBOLS and getattr(lib(), name) is not None, name
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name, value in (("MMHIP_YUV10_PATH_ALIGNED", 0), ("MMHIP_YUV10_PATH_BYTES", 1)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(_lib, name) == value
    assert api.PIXEL_FORMATS == ("yuv420p", "yuv420p10")
    assert api.YUV_MATRICES == X.MATRIX_IDS and api.YUV_RANGES == X.RANGE_IDS
    flat = " ".join(header.split())
    assert ("int mmhip_clip_float_to_yuv420p10(mmhip_invocation *inv, const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, "
            "int height, int first_row, int last_row, int num_frames, int matrix, int range, void *dst, int64_t dst_frame_stride, void *stream);") in flat
    assert "int64_t mmhip_yuv420p10_frame_bytes(int width, int height);" in flat
    assert "int mmhip_y4m_header_p10(char *buf, int cap, int width, int height, int fps_num, int fps_den, int range);" in flat
    assert "long mmhip_clip_float_to_yuv420p10_launches(mmhip_invocation *inv, int path);" in flat
    assert lib().mmhip_clip_float_to_yuv420p10.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_int] * 7 + [C.c_void_p, C.c_int64, C.c_void_p]
    for name in ("clip_float_to_yuv420p10", "clip_float_to_yuv420p10_launches"):
        assert hasattr(api.Invocation, name)
    # the kernel is in a file of its own, on the Makefile's list, declared in clip_kernels.h, over the shared header
    text = open(os.path.join(CSRC, "clip_yuv10.hip")).read()
    assert "k_float_to_yuv420p10_clip" in text and '#include "mm_yuv.h"' in text and '"yuv420p10_clip"' in text
    assert re.search(r"^HIP_SRCS\s*=.*\bclip_yuv10\.hip\b", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    assert "launch_float_to_yuv420p10_clip" in open(os.path.join(CSRC, "clip_kernels.h")).read()
    shared = open(os.path.join(CSRC, "mm_yuv.h")).read()
    for name in ("MM_YUV10_MODES", "mm_yuv10_quant", "mm_yuv10_luma", "mm_yuv10_chroma", "mm_yuv10_frame_host"):
        assert name in shared, name
    # both paths of the kernel convert with those functions
    for name in ("mm_yuv10_quant", "mm_yuv10_luma", "mm_yuv10_cb", "mm_yuv10_cr"):
        assert text.count(name + "(") >= 2, name


def test_the_header_states_the_arithmetic_and_the_tables():
    header = " ".join(open(os.path.join(ROOT, "include", "mmhip.h")).read().split())
    for phrase in ("q = (int)rintf(c * 65535.0f)", "np.rint(np.float32(c) * np.float32(65535)).astype(np.int32)",
                   "Y = ((yr * R + yg * G + yb * B + 2^19) >> 20) + off",
                   "Cb = clamp(((cbr * Rs + cbg * Gs + cbb * Bs + 2^20) >> 21) + 512, 0, 1023)",
                   "floor(k * E / 65535 * 2^20 + 0.5)", "sign(k) * floor(|k| * E / 65535 * 2^19 + 0.5)", "ties to even", "NaN and -0 give 0",
                   "16-bit little-endian samples with the value in the low 10 bits", "2 * (width * height + 2 * cw * ch)",
                   "C420p10", "yuv420p10_clip", "MMHIP_YUV10_LOADS", "MMHIP_YUV10_COLUMNS", "tests/yuv10_reference.py", "1 073 201 168",
                   "[-1 072 676 880, 1 073 725 456]"):
        assert phrase in header, phrase
    for (matrix, rng), (off, y, cb, cr) in STATED.items():
        row = "%s %s %d %s %s %s" % (matrix, rng, off, ", ".join(map(str, y)), ", ".join(map(str, cb)), ", ".join(map(str, cr)))
        assert row in header, row
    # mm_yuv.h holds the same rows
    shared = re.sub(r"\s+", "", open(os.path.join(CSRC, "mm_yuv.h")).read())
    for off, y, cb, cr in STATED.values():
        assert "{%s}" % ",".join(map(str, (off,) + y + cb + cr)) in shared


# ---- the rule, the restatement by hand, the bounds ----

def test_the_rule_gives_the_stated_tables():
    assert X.TABLES == STATED
    for (matrix, rng), (off, y, cb, cr) in X.TABLES.items():
        excursion = 876 if rng == "limited" else 1023
        assert off == (64 if rng == "limited" else 0)
        assert sum(y) == (excursion * 2 ** 20 * 2 + 65535) // (2 * 65535)       # floor(E / 65535 * 2^20 + 0.5)
        assert sum(cb) == 0 and sum(cr) == 0
        assert cb[2] == cr[0] == (3584 if rng == "limited" else 4092)


@pytest.mark.parametrize("mode", X.MODES, ids="-".join)
def test_white_black_grey_and_the_primaries_by_hand(mode):
    limited = mode[1] == "limited"
    colours = dict(BY_HAND[mode])
    colours[WHITE] = (940 if limited else 1023, 512, 512)
    colours[BLACK] = (64 if limited else 0, 512, 512)
    # 0.5 * 65535 = 32767.5 is a tie: 32768, and (sum(y) * 32768 + 2^19) >> 20 = sum(y) / 32 + 0.5 floored
    assert X.quant(0.5) == 32768
    colours[GREY] = (502 if limited else 512, 512, 512)
    assert (14016 * 32768 + 2 ** 19) >> 20 == 438 and (16368 * 32768 + 2 ** 19) >> 20 == 512
    for rgb, ycc in colours.items():
        px = np.array(rgb, np.float32).reshape(1, 1, 3)
        y, cb, cr = X.planes(px, mode)                                    # a 1 x 1 frame: the pixel replicated four times
        assert (int(y[0, 0]), int(cb[0, 0]), int(cr[0, 0])) == ycc, (mode, rgb)
        y, cb, cr = X.planes(np.broadcast_to(px, (2, 2, 3)), mode)
        assert (y == ycc[0]).all() and (int(cb[0, 0]), int(cr[0, 0])) == ycc[1:], (mode, rgb)
    # every grey has chroma 512 exactly, and luma does not decrease
    greys = np.repeat(np.linspace(0, 1, 4096, dtype=np.float32)[None, :, None], 3, axis=2)
    y, cb, cr = X.planes(greys, mode)
    assert (cb == 512).all() and (cr == 512).all() and (np.diff(y[0].astype(int)) >= 0).all()
    assert int(y[0, 0]) == colours[BLACK][0] and int(y[0, -1]) == colours[WHITE][0]
    # the corner colours, as blocks of one colour and of every pair
    sums = np.array([[2 * (a[k] + b[k]) for k in range(3)] for a in CORNERS for b in CORNERS])
    cb, cr = X.chroma(sums, mode, clamp=False)
    if limited:
        assert cb.min() == 64 and cb.max() == 960 and cr.min() == 64 and cr.max() == 960
    else:
        # 1023.5 in the real formula is the only case near the clamp: (4092 * 4 * 65535 + 2^20) >> 21 = 511, so the
        # integers stay in 1 .. 1023 and the clamp is a guard
        assert (4092 * 4 * 65535 + 2 ** 20) >> 21 == 511 and (-4092 * 4 * 65535 + 2 ** 20) >> 21 == -511
        assert cb.min() == 1 and cr.min() == 1 and cb.max() == 1023 and cr.max() == 1023
        clamped = X.chroma(sums, mode)
        assert np.array_equal(clamped[0], cb) and np.array_equal(clamped[1], cr)
    assert X.chroma(np.array([[0, 0, 10 ** 6], [10 ** 6, 10 ** 6, 0]]), mode)[0].tolist() == [1023, 0]      # the clamp itself


def test_no_intermediate_leaves_int32():
    """Interval arithmetic over the tables: a channel in [0, 65535] for luma, a sum in [0, 4 * 65535] for chroma."""
    luma_max, chroma_lo, chroma_hi = 0, 0, 0
    for off, y, cb, cr in X.TABLES.values():
        assert min(y) > 0
        luma_max = max(luma_max, sum(y) * 65535 + 2 ** 19)
        for row in (cb, cr):
            hi = sum(k for k in row if k > 0) * 4 * 65535 + 2 ** 20
            lo = sum(k for k in row if k < 0) * 4 * 65535              # (the sum of the products, before 2^20 is added)
            chroma_lo, chroma_hi = min(chroma_lo, lo), max(chroma_hi, hi)
            # partial sums in the order the formula is written stay inside as well
            for order in ((0, 1, 2),):
                acc_lo = acc_hi = 0
                for k in order:
                    acc_lo, acc_hi = acc_lo + min(row[k], 0) * 4 * 65535, acc_hi + max(row[k], 0) * 4 * 65535
                    assert -2 ** 31 <= acc_lo and acc_hi < 2 ** 31
    assert luma_max == 1073201168 < 2 ** 31
    assert (chroma_lo, chroma_hi) == (-1072676880, 1073725456) and -2 ** 31 <= chroma_lo and chroma_hi < 2 ** 31
    # at scale 2^20 the full-range chroma would come within 2^15 of the limit: hence 2^19
    assert 0 < 2 ** 31 - (8184 * 4 * 65535 + 2 ** 21) < 2 ** 15


@pytest.mark.parametrize("mode", X.MODES, ids="-".join)
def test_the_integers_stay_within_one_code_of_the_float64_formula(mode):
    rng = np.random.default_rng(20260)
    q = np.concatenate([rng.integers(0, 65536, (200000, 3)), np.array(CORNERS)])
    ey, ecb, ecr = X.exact(q / 65535.0, mode)
    y = X.luma(q, mode)
    cb, cr = X.chroma(4 * q, mode, clamp=False)
    worst = max(np.abs(y - ey).max(), np.abs(cb - ecb).max(), np.abs(cr - ecr).max())
    print("largest distance from the float64 formula, %s %s: %.4f codes" % (mode + (worst,)))
    assert worst < 1.0


def test_the_quantiser_at_its_edges():
    f = np.float32
    tiny = np.finfo(np.float32)
    cases = [(0.0, 0), (1.0, 65535), (np.nan, 0), (np.inf, 65535), (-np.inf, 0), (-0.0, 0), (tiny.smallest_subnormal, 0), (-tiny.smallest_subnormal, 0),
             (tiny.tiny, 0), (-1.0, 0), (2.0, 65535), (np.nextafter(f(1), f(0)), 65535), (np.nextafter(f(1), f(2)), 65535), (0.5, 32768), (0.25, 16384),
             (1.0 / 65535.0, 1)]
    got = X.quant(np.array([c[0] for c in cases], np.float32))
    assert got.dtype == np.int32 and got.tolist() == [c[1] for c in cases]
    # the ties k + 0.5 that float32 holds (k < 2^23 and far below: all of 0 .. 65534): c = (k + 0.5) / 65535 does not give
    # them in general, so walk the floats around each and keep those whose float32 product is the tie itself
    ks = np.arange(0, 65535, dtype=np.int64)
    c = ((ks + 0.5) / 65535.0).astype(np.float32)
    found = 0
    for step in range(-2, 3):
        cc = c.copy()
        for _ in range(abs(step)):
            cc = np.nextafter(cc, f(2) if step > 0 else f(-1))
        product = cc * f(65535)
        tie = product == (ks + 0.5).astype(np.float32)
        found += int(tie.sum())
        assert (X.quant(cc)[tie] == (ks + (ks & 1))[tie]).all()          # to even
        assert (np.abs(X.quant(cc) - product.astype(np.float64)) <= 0.5).all()
    assert found > 1000
    # 0.5 and 0.25 are ties by construction: 32767.5 and 16383.75 -- only the first is
    assert f(0.5) * f(65535) == f(32767.5) and X.quant(0.5) == 32768 and X.quant(f(1.5 / 65535)) in (1, 2)


# ---- layout and framing ----

def test_frame_bytes_and_plane_offsets_by_hand():
    by_hand = {(1, 1): (3, (0, 1, 2), (1, 1)), (2, 2): (6, (0, 4, 5), (1, 1)), (3, 5): (27, (0, 15, 21), (2, 3)), (17, 9): (243, (0, 153, 198), (9, 5))}
    for (w, h), (samples, offsets, (cw, ch)) in by_hand.items():
        assert lib().mmhip_yuv420p10_frame_bytes(w, h) == 2 * samples == mm.api.yuv420_frame_bytes(w, h, "yuv420p10") == X.frame_bytes(w, h), (w, h)
        assert mm.api.yuv420_frame_bytes(w, h) == samples == mm.api.yuv420_frame_bytes(w, h, pixel_format="yuv420p") == X.frame_samples(w, h)
        assert X.plane_offsets(w, h) == offsets and X.chroma_size(w, h) == (cw, ch)
        buf = (1000 * np.arange(2)[:, None] + np.arange(samples)[None, :]).astype(np.uint16)
        for planes in (mm.api.yuv420_planes(buf, w, h), mm.api.yuv420_planes(buf, w, h, pixel_format="yuv420p10")):
            y, cb, cr = planes
            assert y.dtype == np.uint16 and y.shape == (2, h, w) and cb.shape == (2, ch, cw) == cr.shape
            for plane, off in zip((y, cb, cr), offsets):
                assert plane[0, 0, 0] == off and plane[1, 0, 0] == 1000 + off
                assert np.shares_memory(plane, buf)
            assert y[0, h - 1, w - 1] == offsets[1] - 1 and cb[0, ch - 1, cw - 1] == offsets[2] - 1 and cr[0, ch - 1, cw - 1] == samples - 1
    assert lib().mmhip_yuv420p10_frame_bytes(0, 4) == -1 and "yuv420p10_frame_bytes" in err()
    assert lib().mmhip_yuv420p10_frame_bytes(65536, 65536) == 2 * (65536 * 65536 + 2 * 32768 * 32768)
    with pytest.raises(ValueError):
        mm.api.yuv420_planes(np.zeros((1, 26), np.uint16), 3, 5)
    with pytest.raises(ValueError):
        mm.api.yuv420_planes(np.zeros((1, 27), np.uint8), 3, 5, pixel_format="yuv420p10")
    with pytest.raises(ValueError):
        mm.api.yuv420_planes(np.zeros((1, 27), np.uint16), 3, 5, pixel_format="yuv420p")
    with pytest.raises(ValueError, match="pixel_format"):
        mm.api.yuv420_frame_bytes(3, 5, "yuv444p")


def test_y4m_header_bytes():
    def header(*args, cap=160):
        buf = C.create_string_buffer(cap)
        n = lib().mmhip_y4m_header_p10(buf, cap, *args)
        return n, buf.raw[:max(n, 0)]
    want = b"YUV4MPEG2 W1920 H1080 F25:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n"
    assert header(1920, 1080, 25, 1, 0) == (len(want), want)
    want = b"YUV4MPEG2 W17 H9 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL\n"
    assert header(17, 9, 30000, 1001, 1) == (len(want), want)
    assert want == X.y4m_header(17, 9, (30000, 1001), "full") == mm.api.y4m_header(17, 9, (30000, 1001), "full", pixel_format="yuv420p10")
    # the same line as the 8-bit header with the colour space replaced
    assert mm.api.y4m_header(17, 9, (30000, 1001), "full").replace(b"C420jpeg", b"C420p10") == want
    assert header(17, 9, 30000, 1001, 1, cap=len(want) + 1)[0] == len(want)
    assert header(17, 9, 30000, 1001, 1, cap=len(want))[0] == -1 and "y4m_header_p10" in err()
    for args, word in (((0, 9, 25, 1, 0), "width"), ((17, 9, 0, 1, 0), "fps"), ((17, 9, 25, 0, 0), "fps"), ((17, 9, 25, 1, 2), "range")):
        assert header(*args)[0] == -1 and word in err(), args
    assert lib().mmhip_y4m_header_p10(None, 160, 17, 9, 25, 1, 0) == -1
    with pytest.raises(ValueError, match="pixel_format"):
        mm.api.y4m_header(17, 9, pixel_format="yuv420p12")


def test_write_y4m_of_a_hand_made_clip(tmp_path):
    # 3 x 3: Y 9 samples, Cb and Cr 2 x 2 each: 17 samples, 34 bytes a frame; values with a high byte, so the byte order shows
    a = list(range(257, 266)) + [520, 521, 522, 523] + [1020, 1021, 1022, 1023]
    b = list(range(601, 610)) + [64, 65, 66, 67] + [0, 1, 2, 3]
    buf = np.array([a, b], np.uint16)
    little = lambda values: b"".join(bytes([v & 255, v >> 8]) for v in values)
    want = b"YUV4MPEG2 W3 H3 F25:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n" + b"FRAME\n" + little(a) + b"FRAME\n" + little(b)
    path = str(tmp_path / "two.y4m")
    mm.api.write_y4m(path, buf, 3, 3)
    assert open(path, "rb").read() == want == X.y4m_file(buf, 3, 3)
    assert len(want) == 58 + 2 * (6 + 34)
    # big-endian input is written little-endian too
    f = io.BytesIO()
    mm.api.write_y4m(f, buf.astype(">u2"), 3, 3, pixel_format="yuv420p10")
    assert f.getvalue() == want
    fields, frames = X.parse_y4m(want)
    assert fields == {"W": "3", "H": "3", "F": "25:1", "I": "p", "A": "1:1", "C": "420p10", "XCOLORRANGE": "LIMITED"}
    assert np.array_equal(frames, buf)
    y, cb, cr = mm.api.yuv420_planes(frames, 3, 3)
    assert y[1].tolist() == [[601, 602, 603], [604, 605, 606], [607, 608, 609]] and cb[0].tolist() == [[520, 521], [522, 523]] and cr[0, 1, 1] == 1023
    # a file object stays open; a frame rate and the full range go to the header; one frame may come without the first axis
    f = io.BytesIO()
    mm.api.write_y4m(f, buf[0], 3, 3, fps=(30000, 1001), yuv_range="full")
    assert f.getvalue() == b"YUV4MPEG2 W3 H3 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL\n" + b"FRAME\n" + little(a)
    with pytest.raises(ValueError):
        mm.api.write_y4m(io.BytesIO(), np.zeros((2, 16), np.uint16), 3, 3)
    with pytest.raises(ValueError):
        mm.api.write_y4m(io.BytesIO(), np.zeros((2, 34), np.uint8), 3, 3, pixel_format="yuv420p10")
    with pytest.raises(ValueError):
        mm.api.write_y4m(io.BytesIO(), buf, 3, 3, pixel_format="yuv420p")
    with pytest.raises(ValueError):
        mm.api.write_y4m(io.BytesIO(), buf, 3, 3, pixel_format="yuv422p10")
    # the reader keeps refusing 10-bit streams, by name
    with pytest.raises(ValueError, match="C420p10"):
        mm.api.read_y4m(io.BytesIO(want))
    with pytest.raises(ValueError, match="C420p10"):
        mm.api.y4m_parse_header(want[:58])


# ---- mm_yuv.h on the host ----

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mm_yuv.h"
// frame in width height row_stride matrix range out   |   quant in count out
int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "quant")) {
        const int n = atoi(argv[3]);
        std::vector<float> v((size_t)n);
        std::vector<int> q((size_t)n);
        FILE *f = fopen(argv[2], "rb");
        if (!f || fread(v.data(), sizeof(float), v.size(), f) != v.size()) return 4;
        fclose(f);
        for (int i = 0; i < n; ++i) q[i] = mm_yuv10_quant(v[i]);
        f = fopen(argv[4], "wb");
        if (!f || fwrite(q.data(), sizeof(int), q.size(), f) != q.size()) return 6;
        fclose(f);
        return 0;
    }
    if (argc != 9 || strcmp(argv[1], "frame")) return 2;
    const int w = atoi(argv[3]), h = atoi(argv[4]), stride = atoi(argv[5]), matrix = atoi(argv[6]), range = atoi(argv[7]);
    if (!mm_yuv_mode_known(matrix, range)) return 3;
    std::vector<unsigned char> src((size_t)stride * h);
    std::vector<uint16_t> dst((size_t)(mm_yuv10_frame_bytes(w, h) / 2));
    FILE *f = fopen(argv[2], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size()) return 4;
    fclose(f);
    if (mm_yuv10_frame_bytes(w, h) != 2 * mm_yuv_frame_bytes(w, h)) return 5;
    mm_yuv10_frame_host(MM_YUV10_MODES[matrix][range], (const float *)src.data(), stride, w, h, dst.data());
    f = fopen(argv[8], "wb");
    if (!f || fwrite(dst.data(), 2, dst.size(), f) != dst.size()) return 6;
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitizers"])
def host_program(request):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tempfile.mkdtemp(prefix="mm_yuv10_")
    open(os.path.join(d, "t.cpp"), "w").write(PROGRAM)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param else ["-O2"]
    exe = os.path.join(d, "t")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, "-o", exe, os.path.join(d, "t.cpp")], check=True)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])

    def convert(pixels, mode, pad=0):
        h, w = pixels.shape[:2]
        rows = np.full((h, w * 16 + pad), 0xEE, np.uint8)
        rows[:, :w * 16] = np.ascontiguousarray(pixels, np.float32).view(np.uint8).reshape(h, w * 16)
        rows.tofile(os.path.join(d, "in.bin"))
        run("frame", os.path.join(d, "in.bin"), w, h, w * 16 + pad, X.MATRIX_IDS[mode[0]], X.RANGE_IDS[mode[1]], os.path.join(d, "out.bin"))
        return np.fromfile(os.path.join(d, "out.bin"), "<u2")

    def quant(values):
        np.ascontiguousarray(values, np.float32).tofile(os.path.join(d, "q.bin"))
        run("quant", os.path.join(d, "q.bin"), len(values), os.path.join(d, "q.out"))
        return np.fromfile(os.path.join(d, "q.out"), np.int32)
    convert.quant = quant
    yield convert
    shutil.rmtree(d, ignore_errors=True)


def test_a_frame_worked_out_sample_by_sample(host_program):
    px = np.array([[RED, RED, GREEN, GREEN, BLUE], [GREEN, BLUE, GREEN, GREEN, BLUE], [WHITE, WHITE, BLACK, BLACK, GREY]], np.float32)
    alpha = np.array([[[0.5], [np.nan], [-3.0], [np.inf], [1.0]]] * 3, np.float32)       # some alpha, which is not read
    pixels = np.concatenate([px, alpha], axis=2)
    got = host_program(pixels, ("bt709", "limited"), pad=4)
    assert len(got) == 27
    # Y: the values by hand; grey 0.5 quantises to 32768 (a tie), (14016 * 32768 + 2^19) >> 20 = 438, plus 64
    assert got[:15].reshape(3, 5).tolist() == [[250, 250, 690, 690, 127], [690, 127, 690, 690, 127], [940, 940, 64, 64, 502]]
    # block (0, 0) is red, red / green, blue: Rs = 131070, Gs = 65535, Bs = 65535
    cb00 = ((-821 * 131070 - 2763 * 65535 + 3584 * 65535 + 2 ** 20) >> 21) + 512
    cr00 = ((3584 * 131070 - 3255 * 65535 - 329 * 65535 + 2 ** 20) >> 21) + 512
    assert (cb00, cr00) == (486, 624)
    # block (1, 0) is green; block (2, 0) is the last column twice: blue; row 1 is the last row twice: white, black, grey
    assert got[15:21].reshape(2, 3).tolist() == [[cb00, 167, 960], [512, 512, 512]]
    assert got[21:27].reshape(2, 3).tolist() == [[cr00, 105, 471], [512, 512, 512]]
    rng = np.random.default_rng(5)
    noisy = rng.uniform(-0.25, 1.25, (3, 5, 4)).astype(np.float32)
    noisy[1, 2, 0], noisy[0, 4, 1], noisy[2, 0, 2] = np.nan, np.inf, -np.inf
    for mode in X.MODES:
        assert np.array_equal(host_program(pixels, mode), X.frame(pixels, mode)), mode
        assert np.array_equal(host_program(noisy, mode, pad=12), X.frame(noisy, mode)), mode


def test_the_corner_colours_in_every_mode(host_program):
    pixels = np.zeros((2, 16, 4), np.float32)
    corners = [(r, g, b) for r in (0, 1) for g in (0, 1) for b in (0, 1)]
    for k, c in enumerate(corners):
        pixels[:, 2 * k:2 * k + 2, :3] = c
    for mode in X.MODES:
        got = host_program(pixels, mode)
        assert np.array_equal(got, X.frame(pixels, mode)), mode
        y, cb, cr = mm.api.yuv420_planes(got, 16, 2)
        for k, c in enumerate(corners):
            if c in BY_HAND[mode]:
                assert (int(y[0, 0, 2 * k]), int(cb[0, 0, k]), int(cr[0, 0, k])) == BY_HAND[mode][c], (mode, c)
        if mode[1] == "full":      # pure blue's Cb and pure red's Cr
            assert cb[0, 0, corners.index(BLUE)] == 1023 and cr[0, 0, corners.index(RED)] == 1023
            assert y[0, 0, 2 * corners.index(WHITE)] == 1023 and y[0, 0, 2 * corners.index(BLACK)] == 0


def test_the_host_quantiser_is_the_restatements(host_program):
    f = np.float32
    tiny = np.finfo(np.float32)
    ks = np.arange(0, 65535, dtype=np.int64)
    around = ((ks + 0.5) / 65535.0).astype(np.float32)
    values = np.concatenate([np.array([0.0, 1.0, np.nan, np.inf, -np.inf, -0.0, tiny.smallest_subnormal, -tiny.smallest_subnormal, tiny.tiny, -1.0, 2.0, 0.5],
                                      np.float32), around, np.nextafter(around, f(2)), np.nextafter(around, f(-1)),
                             np.random.default_rng(3).uniform(-0.5, 1.5, 4096).astype(np.float32)])
    got = host_program.quant(values)
    assert got[:12].tolist() == [0, 65535, 0, 65535, 0, 0, 0, 0, 0, 0, 65535, 32768]
    assert np.array_equal(got, X.quant(values))


# ---- refusals ----

def refused(**over):
    args = dict(src=0x1000, row_stride=None, frame_stride=None, w=16, h=8, first=0, last=None, n=2, matrix=1, rng=0, dst=0x2000, dst_stride=None)
    args.update(over)
    w, h = args["w"], args["h"]
    last = h if args["last"] is None else args["last"]
    row_stride = 16 * w if args["row_stride"] is None else args["row_stride"]
    frame_stride = row_stride * h if args["frame_stride"] is None else args["frame_stride"]
    dst_stride = X.frame_bytes(max(w, 1), max(h, 1)) if args["dst_stride"] is None else args["dst_stride"]
    rc = lib().mmhip_clip_float_to_yuv420p10(None, args["src"], row_stride, frame_stride, w, h, args["first"], last, args["n"], args["matrix"],
                                             args["rng"], args["dst"], dst_stride, None)
    assert rc == -1
    return err()


def test_the_call_refuses_bad_arguments_by_name():
    """Every check comes before the invocation is looked at: no GPU.  The wording is mmhip_clip_to_yuv420's where the
    condition is the same."""
    who = "clip_float_to_yuv420p10: "
    assert refused() == who + "no invocation"
    assert refused(w=0).startswith(who + "width and height must be at least 1")
    assert refused(h=-3).startswith(who + "width and height must be at least 1")
    assert refused(n=0) == who + "num_frames must be at least 1"
    assert refused(n=65536).startswith(who + "more than 65535 frames")
    assert refused(n=65535) == who + "no invocation"
    for matrix in (-1, 2):
        assert refused(matrix=matrix).startswith(who + "matrix must be MMHIP_YUV_BT601 or MMHIP_YUV_BT709")
    for rng in (-1, 2):
        assert refused(rng=rng).startswith(who + "range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL")
    for first, last in ((-2, 4), (0, 10), (4, 4), (6, 2)):
        assert "are not rows of a frame of 8" in refused(first=first, last=last)
    assert refused(first=1, last=4) == who + "first_row must be even, not 1"
    assert refused(first=0, last=3) == who + "last_row must be even or equal to height, not 3 of 8"
    assert refused(h=9, first=2, last=9) == who + "no invocation"          # an odd last row that is the height
    assert refused(h=9, first=2, last=7).startswith(who + "last_row must be even")
    assert refused(src=0).endswith("must be device pointers") and refused(dst=0).endswith("must be device pointers")
    assert refused(row_stride=255) == who + "src_row_stride 255 is smaller than one row (256 bytes)"
    for over in (dict(src=0x1002), dict(row_stride=258), dict(frame_stride=16 * 16 * 8 + 2)):
        assert refused(**over) == who + "src, src_row_stride and src_frame_stride must be multiples of 4 (the source holds floats)", over
    assert refused(src=0x1004, row_stride=260, frame_stride=260 * 8 + 4) == who + "no invocation"
    assert refused(dst_stride=382) == who + "dst_frame_stride 382 is smaller than one frame (384 bytes)"
    assert refused(dst_stride=384) == who + "no invocation"
    for over in (dict(dst=0x2001), dict(dst_stride=385)):
        assert refused(**over) == who + "dst and dst_frame_stride must be even (the samples are 16-bit)", over
    assert refused(dst=0x2002, dst_stride=386) == who + "no invocation"
    assert refused(w=65536, h=32769) == who + "a Y plane of more than 4 GiB"
    assert refused(w=65536, h=32768, last=2) == who + "no invocation"          # a plane of exactly 4 GiB, a band of two rows
    assert refused(w=16, h=8, row_stride=1 << 30).startswith(who + "a source frame of more than 4 GiB")
    assert refused(w=16384, h=16384, n=1) == who + "no invocation"             # a float frame of exactly 4 GiB
    assert refused(w=16384, h=16386, n=1).startswith(who + "a source frame of more than 4 GiB; convert the frame in row bands")
    assert refused(w=16384, h=16386, last=16384, n=1) == who + "no invocation"
    assert lib().mmhip_clip_float_to_yuv420p10_launches(None, 2) == -1 and "clip_float_to_yuv420p10_launches: path must be" in err()


def test_python_argument_errors():
    """Refused before anything else is looked at (an invocation needs a GPU; the checks do not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    inv.render_width, inv.render_height = 16, 9
    for fmt in ("yuv420p12", "yuv422p10", "YUV420P10", 10):
        with pytest.raises(ValueError, match="pixel_format must be one of yuv420p, yuv420p10"):
            inv.render_clip(num_frames=2, pixel_format=fmt)
    for keywords, word in ((dict(floatmap=True), "floatmap"), (dict(bpp=3), "bpp"), (dict(bpp=1), "bpp"), (dict(region=(0, 0, 8, 8)), "region"),
                           (dict(row_stride=64), "row_stride"), (dict(frame_stride=1024), "frame_stride")):
        with pytest.raises(ValueError, match="pixel_format is not combined with " + word):
            inv.render_clip(num_frames=2, out_ptr=0x1000, pixel_format="yuv420p10", **keywords)
    with pytest.raises(ValueError, match="yuv420p10.* is not combined with supersample=True"):
        inv.render_clip(num_frames=2, pixel_format="yuv420p10", supersample=True)
    for matrix in ("bt2020", "BT709", None, 1):
        with pytest.raises(ValueError, match="yuv_matrix"):
            inv.render_clip(num_frames=2, pixel_format="yuv420p10", yuv_matrix=matrix)
    for rng in ("tv", "Full", None, 0):
        with pytest.raises(ValueError, match="yuv_range"):
            inv.render_clip(num_frames=2, pixel_format="yuv420p10", yuv_range=rng)
    for rows in ((1, 4), (0, 3), (2, 7), (0, 10), (-2, 4), (4, 4)):
        with pytest.raises(ValueError, match="rows"):
            inv.render_clip(num_frames=2, out_ptr=0x1000, pixel_format="yuv420p10", rows=rows)
    with pytest.raises(ValueError, match="not both"):
        inv.render_clip(num_frames=2, pixel_format="yuv420p10", shutter_samples=2, shutter=0.5, shutter_span=0.1)
    with pytest.raises(ValueError, match="shutter is a fraction"):
        inv.render_clip(frames=[0, 1], ts=[0.0, 0.5], pixel_format="yuv420p10", shutter_samples=2, shutter=0.5)
    with pytest.raises(ValueError, match="yuv_matrix"):
        inv.clip_float_to_yuv420p10(0x1000, 0x2000, 1, yuv_matrix="bt2020")
    with pytest.raises(ValueError, match="path"):
        inv.clip_float_to_yuv420p10_launches("words")
    import inspect
    sig = inspect.signature(mm.api.Invocation.clip_float_to_yuv420p10).parameters
    assert list(sig)[1:4] == ["src_ptr", "dst_ptr", "num_frames"] and sig["yuv_matrix"].default == "bt709" and sig["yuv_range"].default == "limited"


def test_cli_help_and_argument_errors(tmp_path):
    p = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0
    for phrase in ("--pixel-format=FORMAT", "yuv420p (default", "yuv420p10", "C420p10", "not combined with -o"):
        assert phrase in p.stdout, phrase
    src = "filter f () rgba:[t, 0, 0, 1] end"
    cases = [(["--pixel-format=yuv420p10"], "f%d.png", ".y4m"), (["--pixel-format=yuv420p"], "f%d.png", ".y4m"),
             (["--pixel-format=yuv420p10"], "movie.y4m.png", ".y4m"), (["--pixel-format=yuv420p12"], "m.y4m", "--pixel-format"),
             (["--pixel-format="], "m.y4m", "--pixel-format"), (["--pixel-format=YUV420P10"], "m.y4m", "--pixel-format"),
             (["--pixel-format=yuv420p10", "-o"], "m.y4m", "-o")]
    for extra, out, word in cases:
        p = subprocess.run([CLI, "-F", "3", "-s", "8x8"] + extra + [src, str(tmp_path / out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=60)
        assert p.returncode != 0 and p.stderr.startswith("Error:") and word in p.stderr, (extra, p.stderr)
    assert not list(tmp_path.iterdir())
