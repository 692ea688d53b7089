"""Clips as planar Y'CbCr 4:2:0 without a GPU (mmhip_clip_to_yuv420, include/mmhip.h): the entry points and the header's
statement, the restatement tests/yuv_reference.py against the textbook values, the layout and the Y4M framing worked out
by hand, csrc/mm_yuv.h compiled for the host in a stand-alone program (plain and under the sanitizers), every refusal by
its name, the Python keywords and the command line's options."""
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
from tests import yuv_reference as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
CSRC = os.path.join(ROOT, "mathmap_amd", "csrc")
RED, GREEN, BLUE, WHITE, BLACK = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255), (0, 0, 0)
CORNERS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]


def err():
    return lib().mmhip_last_error().decode()


def test_entry_points_exist_and_are_declared():
    api = mm.api
    for name in ("mmhip_clip_to_yuv420", "mmhip_yuv420_frame_bytes", "mmhip_y4m_header"):
        assert name in _lib.SYMBOLS and getattr(lib(), name) is not None, name
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name, value in (("MMHIP_YUV_BT601", 0), ("MMHIP_YUV_BT709", 1), ("MMHIP_YUV_LIMITED", 0), ("MMHIP_YUV_FULL", 1)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(_lib, name) == value
    assert api.YUV_MATRICES == {"bt601": _lib.MMHIP_YUV_BT601, "bt709": _lib.MMHIP_YUV_BT709} == X.MATRIX_IDS
    assert api.YUV_RANGES == {"limited": _lib.MMHIP_YUV_LIMITED, "full": _lib.MMHIP_YUV_FULL} == X.RANGE_IDS
    flat = " ".join(header.split())
    assert ("int mmhip_clip_to_yuv420(mmhip_invocation *inv, const void *src_rgba, int64_t src_row_stride, int64_t src_frame_stride, int width, "
            "int height, int first_row, int last_row, int num_frames, int matrix, int range, void *dst, int64_t dst_frame_stride, void *stream);") in flat
    assert "int64_t mmhip_yuv420_frame_bytes(int width, int height);" in flat
    assert "int mmhip_y4m_header(char *buf, int cap, int width, int height, int fps_num, int fps_den, int range);" in flat
    assert lib().mmhip_clip_to_yuv420.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_int] * 7 + [C.c_void_p, C.c_int64, C.c_void_p]
    for name in ("clip_to_yuv420",):
        assert hasattr(api.Invocation, name)
    for name in ("yuv420_planes", "write_y4m", "yuv420_frame_bytes", "y4m_header"):
        assert hasattr(api, name)
    # the kernel is in a file of its own, on the Makefile's list, over the shared header
    assert "k_rgba8_to_yuv420_clip" in open(os.path.join(CSRC, "clip_yuv.hip")).read()
    assert re.search(r"^HIP_SRCS\s*=.*\bclip_yuv\.hip\b", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    for name in ("clip_yuv.hip", "runtime_clip.cpp"):
        assert '#include "mm_yuv.h"' in open(os.path.join(CSRC, name)).read(), name


def test_the_header_states_the_arithmetic_and_the_tables():
    header = " ".join(open(os.path.join(ROOT, "include", "mmhip.h")).read().split())
    for phrase in ("Y = ((yr * R + yg * G + yb * B + 2^15) >> 16) + off",
                   "Cb = clamp(((cbr * Rs + cbg * Gs + cbb * Bs + 2^17) >> 18) + 128, 0, 255)",
                   "cw = (width + 1) >> 1 and ch = (height + 1) >> 1", "first_row must be even and last_row even or equal to height",
                   "[first_row / 2, (last_row + 1) / 2)", "C420jpeg", "yuv420_clip", "floor division", "replicated"):
        assert phrase in header, phrase
    for (matrix, rng), (off, y, cb, cr) in X.TABLES.items():
        row = "%s %s %d %s %s %s" % (matrix, rng, off, ", ".join(map(str, y)), ", ".join(map(str, cb)), ", ".join(map(str, cr)))
        assert row in header, row


# ---- the restatement against the textbook ----

def test_the_restatement_gives_the_textbook_values():
    want = {("bt709", "limited"): {RED: (63, 102, 240), GREEN: (173, 42, 26), BLUE: (32, 240, 118)},
            ("bt601", "limited"): {RED: (81, 90, 240), GREEN: (145, 54, 34), BLUE: (41, 240, 110)}}
    for mode, colours in want.items():
        for rgb, ycc in list(colours.items()) + [(BLACK, (16, 128, 128)), (WHITE, (235, 128, 128))]:
            px = np.array(rgb, np.uint8).reshape(1, 1, 3)
            y, cb, cr = X.planes(px, mode)
            assert (int(y[0, 0]), int(cb[0, 0]), int(cr[0, 0])) == ycc, (mode, rgb)
            y, cb, cr = X.planes(np.broadcast_to(px, (2, 2, 3)), mode)
            assert (y == ycc[0]).all() and (int(cb[0, 0]), int(cr[0, 0])) == ycc[1:], (mode, rgb)
    for mode in X.MODES:
        white = X.planes(np.full((1, 1, 3), 255, np.uint8), mode)
        assert int(white[0][0, 0]) == (235 if mode[1] == "limited" else 255)
        assert int(X.planes(np.zeros((1, 1, 3), np.uint8), mode)[0][0, 0]) == (16 if mode[1] == "limited" else 0)
        # each row of the table sums exactly
        off, y, cb, cr = X.TABLES[mode]
        assert sum(cb) == 0 and sum(cr) == 0 and sum(y) == (65536 if mode[1] == "full" else 56284)


@pytest.mark.parametrize("mode", X.MODES, ids="-".join)
def test_grey_has_chroma_128_and_limited_chroma_stays_in_range(mode):
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)       # [1, 256, 3]: every grey, 128 blocks of two
    y, cb, cr = X.planes(ramp, mode)
    assert (cb == 128).all() and (cr == 128).all()
    assert (np.diff(y[0].astype(int)) >= 0).all()
    # the sums of every pair of corner colours twice over (blocks of two colours) and of single colours
    sums = np.array([[2 * (a[k] + b[k]) for k in range(3)] for a in CORNERS for b in CORNERS])
    cb, cr = X.chroma(sums, mode)
    if mode[1] == "limited":
        assert cb.min() == 16 and cb.max() == 240 and cr.min() == 16 and cr.max() == 240
    else:
        # unclamped, pure blue and pure red give 256
        _, _, kb, kr = X.TABLES[mode]
        assert (kb[2] * 1020 + 2 ** 17) // 2 ** 18 + 128 == 256 and (kr[0] * 1020 + 2 ** 17) // 2 ** 18 + 128 == 256
        assert cb.min() >= 0 and cb.max() == 255 and cr.max() == 255


# ---- layout and framing ----

def test_frame_bytes_and_plane_offsets_by_hand():
    by_hand = {(1, 1): (3, (0, 1, 2), (1, 1)), (2, 2): (6, (0, 4, 5), (1, 1)), (3, 5): (27, (0, 15, 21), (2, 3)), (17, 9): (243, (0, 153, 198), (9, 5))}
    for (w, h), (total, offsets, (cw, ch)) in by_hand.items():
        assert lib().mmhip_yuv420_frame_bytes(w, h) == total == mm.api.yuv420_frame_bytes(w, h) == X.frame_bytes(w, h), (w, h)
        assert X.plane_offsets(w, h) == offsets and X.chroma_size(w, h) == (cw, ch)
        buf = (np.arange(2 * total) % 256).astype(np.uint8).reshape(2, total)
        y, cb, cr = mm.api.yuv420_planes(buf, w, h)
        assert y.shape == (2, h, w) and cb.shape == (2, ch, cw) == cr.shape
        for plane, off in zip((y, cb, cr), offsets):
            assert plane[0, 0, 0] == off and plane[1, 0, 0] == (total + off) % 256
            assert np.shares_memory(plane, buf)
        assert y[0, h - 1, w - 1] == offsets[1] - 1 and cb[0, ch - 1, cw - 1] == offsets[2] - 1 and cr[0, ch - 1, cw - 1] == total - 1
    assert lib().mmhip_yuv420_frame_bytes(0, 4) == -1 and "yuv420_frame_bytes" in err()
    assert lib().mmhip_yuv420_frame_bytes(65536, 65536) == 65536 * 65536 + 2 * 32768 * 32768
    with pytest.raises(ValueError):
        mm.api.yuv420_planes(np.zeros((1, 26), np.uint8), 3, 5)


def test_y4m_header_bytes():
    def header(*args, cap=160):
        buf = C.create_string_buffer(cap)
        n = lib().mmhip_y4m_header(buf, cap, *args)
        return n, buf.raw[:max(n, 0)]
    want = b"YUV4MPEG2 W1920 H1080 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert header(1920, 1080, 25, 1, 0) == (len(want), want)
    want = b"YUV4MPEG2 W17 H9 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
    assert header(17, 9, 30000, 1001, 1) == (len(want), want)
    assert want == X.y4m_header(17, 9, (30000, 1001), "full") == mm.api.y4m_header(17, 9, (30000, 1001), "full")
    assert mm.api.y4m_header(8, 2) == b"YUV4MPEG2 W8 H2 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" == mm.api.y4m_header(8, 2, 25)
    # the NUL is written too, and needs its byte
    assert header(17, 9, 30000, 1001, 1, cap=len(want) + 1)[0] == len(want)
    assert header(17, 9, 30000, 1001, 1, cap=len(want))[0] == -1 and "y4m_header" in err()
    for args, word in (((0, 9, 25, 1, 0), "width"), ((17, 9, 0, 1, 0), "fps"), ((17, 9, 25, 0, 0), "fps"), ((17, 9, 25, 1, 2), "range")):
        assert header(*args)[0] == -1 and word in err(), args
    assert lib().mmhip_y4m_header(None, 160, 17, 9, 25, 1, 0) == -1


def test_write_y4m_of_a_hand_made_clip(tmp_path):
    # 3 x 3: Y 9 bytes, Cb and Cr 2 x 2 each: 17 bytes a frame
    a = bytes(range(1, 10)) + bytes([20, 21, 22, 23]) + bytes([30, 31, 32, 33])
    b = bytes(range(101, 110)) + bytes([120, 121, 122, 123]) + bytes([130, 131, 132, 133])
    buf = np.frombuffer(a + b, np.uint8).reshape(2, 17)
    want = b"YUV4MPEG2 W3 H3 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" + b"FRAME\n" + a + b"FRAME\n" + b
    path = str(tmp_path / "two.y4m")
    mm.api.write_y4m(path, buf, 3, 3)
    assert open(path, "rb").read() == want == X.y4m_file(buf, 3, 3)
    fields, frames = X.parse_y4m(want)
    assert fields == {"W": "3", "H": "3", "F": "25:1", "I": "p", "A": "1:1", "C": "420jpeg", "XCOLORRANGE": "LIMITED"}
    assert np.array_equal(frames, buf)
    y, cb, cr = mm.api.yuv420_planes(frames, 3, 3)
    assert y[1].tolist() == [[101, 102, 103], [104, 105, 106], [107, 108, 109]] and cb[0].tolist() == [[20, 21], [22, 23]] and cr[1, 1, 1] == 133
    # a file object stays open; a frame rate and the full range go to the header; one frame may come without the first axis
    f = io.BytesIO()
    mm.api.write_y4m(f, buf[0], 3, 3, fps=(30000, 1001), yuv_range="full")
    assert f.getvalue() == b"YUV4MPEG2 W3 H3 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n" + b"FRAME\n" + a
    with pytest.raises(ValueError):
        mm.api.write_y4m(io.BytesIO(), np.zeros((2, 16), np.uint8), 3, 3)
    with pytest.raises(ValueError):
        mm.api.write_y4m(io.BytesIO(), buf, 3, 3, yuv_range="wide")


# ---- mm_yuv.h on the host ----

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mm_yuv.h"
// in width height row_stride matrix range out
int main(int argc, char **argv) {
    if (argc != 8) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]), stride = atoi(argv[4]), matrix = atoi(argv[5]), range = atoi(argv[6]);
    if (!mm_yuv_mode_known(matrix, range) || mm_yuv_mode_known(2, 0) || mm_yuv_mode_known(0, -1)) return 3;
    std::vector<unsigned char> src((size_t)stride * h), dst((size_t)mm_yuv_frame_bytes(w, h));
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size()) return 4;
    fclose(f);
    if (mm_yuv_cb_offset(w, h) != (int64_t)w * h || mm_yuv_cr_offset(w, h) != (int64_t)w * h + (int64_t)mm_yuv_cw(w) * mm_yuv_ch(h)) return 5;
    mm_yuv_frame_host(MM_YUV_MODES[matrix][range], src.data(), stride, w, h, dst.data());
    f = fopen(argv[7], "wb");
    if (!f || fwrite(dst.data(), 1, dst.size(), f) != dst.size()) return 6;
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitizers"])
def host_program(request):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tempfile.mkdtemp(prefix="mm_yuv_")
    open(os.path.join(d, "t.cpp"), "w").write(PROGRAM)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param else ["-O2"]
    exe = os.path.join(d, "t")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, "-o", exe, os.path.join(d, "t.cpp")], check=True)

    def convert(rgba, mode, pad=0):
        h, w = rgba.shape[:2]
        rows = np.full((h, w * 4 + pad), 0xEE, np.uint8)
        rows[:, :w * 4] = rgba.reshape(h, w * 4)
        rows.tofile(os.path.join(d, "in.bin"))
        r = subprocess.run([exe, os.path.join(d, "in.bin"), str(w), str(h), str(w * 4 + pad), str(X.MATRIX_IDS[mode[0]]), str(X.RANGE_IDS[mode[1]]),
                            os.path.join(d, "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return np.fromfile(os.path.join(d, "out.bin"), np.uint8)
    yield convert
    shutil.rmtree(d, ignore_errors=True)


def test_a_frame_worked_out_sample_by_sample(host_program):
    grey = (128, 128, 128)
    px = np.array([[RED, RED, GREEN, GREEN, BLUE], [GREEN, BLUE, GREEN, GREEN, BLUE], [WHITE, WHITE, BLACK, BLACK, grey]], np.uint8)
    rgba = np.concatenate([px, np.array([[[7], [255], [0], [99], [200]]] * 3, np.uint8)], axis=2)       # some alpha
    got = host_program(rgba, ("bt709", "limited"), pad=3)
    # Y: the textbook values; grey 128 is ((11966 + 40254 + 4064) * 128 + 32768) >> 16 = 110, plus 16
    assert (56284 * 128 + 32768) >> 16 == 110
    assert got[:15].reshape(3, 5).tolist() == [[63, 63, 173, 173, 32], [173, 32, 173, 173, 32], [235, 235, 16, 16, 126]]
    # block (0, 0) is red, red / green, blue: Rs = 510, Gs = 255, Bs = 255
    cb00 = ((-6596 * 510 - 22189 * 255 + 28785 * 255 + 131072) >> 18) + 128
    cr00 = ((28784 * 510 - 26145 * 255 - 2639 * 255 + 131072) >> 18) + 128
    assert (cb00, cr00) == (122, 156)
    # block (1, 0) is green; block (2, 0) is the last column twice: blue; row 1 is the last row twice: white, black, grey
    assert got[15:21].reshape(2, 3).tolist() == [[cb00, 42, 240], [128, 128, 128]]
    assert got[21:27].reshape(2, 3).tolist() == [[cr00, 26, 118], [128, 128, 128]]
    assert len(got) == 27
    for mode in X.MODES:
        assert np.array_equal(host_program(rgba, mode), X.frame(rgba, mode)), mode


def test_the_corner_colours_in_every_mode(host_program):
    rgba = np.zeros((2, 16, 4), np.uint8)
    for k, c in enumerate(CORNERS):
        rgba[:, 2 * k:2 * k + 2, :3] = c
    textbook = {("bt709", "limited"): {RED: (63, 102, 240), GREEN: (173, 42, 26), BLUE: (32, 240, 118)},
                ("bt601", "limited"): {RED: (81, 90, 240), GREEN: (145, 54, 34), BLUE: (41, 240, 110)}}
    for mode in X.MODES:
        got = host_program(rgba, mode)
        assert np.array_equal(got, X.frame(rgba, mode)), mode
        y, cb, cr = mm.api.yuv420_planes(got, 16, 2)
        for k, c in enumerate(CORNERS):
            if c in textbook.get(mode, {}):
                assert (int(y[0, 0, 2 * k]), int(cb[0, 0, k]), int(cr[0, 0, k])) == textbook[mode][c], (mode, c)
        if mode[1] == "full":      # the clamp: pure blue's Cb and pure red's Cr
            assert cb[0, 0, CORNERS.index(BLUE)] == 255 and cr[0, 0, CORNERS.index(RED)] == 255
            assert y[0, 0, 2 * CORNERS.index(WHITE)] == 255 and y[0, 0, 2 * CORNERS.index(BLACK)] == 0


# ---- refusals ----

def refused(**over):
    args = dict(src=0x1000, row_stride=None, frame_stride=None, w=16, h=8, first=0, last=None, n=2, matrix=1, rng=0, dst=0x2000, dst_stride=None)
    args.update(over)
    w, h = args["w"], args["h"]
    last = h if args["last"] is None else args["last"]
    row_stride = 4 * w if args["row_stride"] is None else args["row_stride"]
    frame_stride = row_stride * h if args["frame_stride"] is None else args["frame_stride"]
    dst_stride = X.frame_bytes(max(w, 1), max(h, 1)) if args["dst_stride"] is None else args["dst_stride"]
    rc = lib().mmhip_clip_to_yuv420(None, args["src"], row_stride, frame_stride, w, h, args["first"], last, args["n"], args["matrix"], args["rng"],
                                    args["dst"], dst_stride, None)
    assert rc == -1
    return err()


def test_the_call_refuses_bad_arguments_by_name():
    """Every check comes before the invocation is looked at: no GPU."""
    assert refused() == "clip_to_yuv420: no invocation"
    assert refused(w=0).startswith("clip_to_yuv420: width and height must be at least 1")
    assert refused(h=-3).startswith("clip_to_yuv420: width and height must be at least 1")
    assert refused(n=0) == "clip_to_yuv420: num_frames must be at least 1"
    assert refused(n=65536).startswith("clip_to_yuv420: more than 65535 frames")
    assert refused(n=65535) == "clip_to_yuv420: no invocation"
    for matrix in (-1, 2):
        assert refused(matrix=matrix).startswith("clip_to_yuv420: matrix must be MMHIP_YUV_BT601 or MMHIP_YUV_BT709")
    for rng in (-1, 2):
        assert refused(rng=rng).startswith("clip_to_yuv420: range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL")
    for first, last in ((-2, 4), (0, 10), (4, 4), (6, 2)):
        assert "are not rows of a frame of 8" in refused(first=first, last=last)
    assert refused(first=1, last=4) == "clip_to_yuv420: first_row must be even, not 1"
    assert refused(first=0, last=3) == "clip_to_yuv420: last_row must be even or equal to height, not 3 of 8"
    assert refused(h=9, first=2, last=9) == "clip_to_yuv420: no invocation"          # an odd last row that is the height
    assert refused(h=9, first=2, last=7).startswith("clip_to_yuv420: last_row must be even")
    assert refused(src=0).endswith("must be device pointers") and refused(dst=0).endswith("must be device pointers")
    assert refused(row_stride=63) == "clip_to_yuv420: src_row_stride 63 is smaller than one row (64 bytes)"
    assert refused(dst_stride=191) == "clip_to_yuv420: dst_frame_stride 191 is smaller than one frame (192 bytes)"
    assert refused(dst_stride=192) == "clip_to_yuv420: no invocation"
    assert refused(w=65536, h=65537) == "clip_to_yuv420: a Y plane of more than 4 GiB"
    assert refused(w=65536, h=65536, last=2) == "clip_to_yuv420: no invocation"          # a plane of exactly 4 GiB, a band of two rows
    assert refused(w=16, h=8, row_stride=1 << 30).startswith("clip_to_yuv420: a source frame of more than 4 GiB")


def test_python_argument_errors():
    """Refused before anything else is looked at (an invocation needs a GPU; the checks do not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    inv.render_width, inv.render_height = 16, 9
    for fmt in ("yuv444p", "nv12", "", 420):
        with pytest.raises(ValueError, match="pixel_format"):
            inv.render_clip(num_frames=2, pixel_format=fmt)
    for keywords, word in ((dict(floatmap=True), "floatmap"), (dict(bpp=3), "bpp"), (dict(bpp=1), "bpp"), (dict(region=(0, 0, 8, 8)), "region"),
                           (dict(row_stride=64), "row_stride"), (dict(frame_stride=1024), "frame_stride")):
        with pytest.raises(ValueError, match="pixel_format is not combined with " + word):
            inv.render_clip(num_frames=2, out_ptr=0x1000, pixel_format="yuv420p", **keywords)
    for matrix in ("bt2020", "BT709", None, 1):
        with pytest.raises(ValueError, match="yuv_matrix"):
            inv.render_clip(num_frames=2, pixel_format="yuv420p", yuv_matrix=matrix)
    for rng in ("tv", "Full", None, 0):
        with pytest.raises(ValueError, match="yuv_range"):
            inv.render_clip(num_frames=2, pixel_format="yuv420p", yuv_range=rng)
    for rows in ((1, 4), (0, 3), (2, 7), (0, 10), (-2, 4), (4, 4)):
        with pytest.raises(ValueError, match="rows"):
            inv.render_clip(num_frames=2, out_ptr=0x1000, pixel_format="yuv420p", rows=rows)
    with pytest.raises(ValueError, match="not both"):
        inv.render_clip(num_frames=2, pixel_format="yuv420p", shutter_samples=2, shutter=0.5, shutter_span=0.1)
    with pytest.raises(ValueError, match="shutter is a fraction"):
        inv.render_clip(frames=[0, 1], ts=[0.0, 0.5], pixel_format="yuv420p", shutter_samples=2, shutter=0.5)
    # the modes' names
    assert mm.api.yuv_mode("bt709", "limited") == (1, 0) and mm.api.yuv_mode("bt601", "full") == (0, 1)
    # without pixel_format the two keywords are not looked at
    import inspect
    sig = inspect.signature(mm.api.Invocation.render_clip).parameters
    assert sig["pixel_format"].default is None and sig["yuv_matrix"].default == "bt709" and sig["yuv_range"].default == "limited"


def test_cli_help_and_argument_errors(tmp_path):
    p = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0
    for phrase in (".y4m", "YUV4MPEG2", "--yuv-matrix=MATRIX", "--yuv-range=RANGE", "--fps=N[:D]", "bt709 (default)", "limited (default", "(default 25)",
                   "standard output"):
        assert phrase in p.stdout, phrase
    src = "filter f () rgba:[t, 0, 0, 1] end"
    cases = [(["--yuv-matrix=bt601"], "f%d.png", ".y4m"), (["--yuv-range=full"], "f%d.png", ".y4m"), (["--fps=30"], "f%d.png", ".y4m"),
             (["--fps=30"], "movie.y4m.png", ".y4m"), (["--yuv-matrix=bt2020"], "m.y4m", "--yuv-matrix"), (["--yuv-matrix="], "m.y4m", "--yuv-matrix"),
             (["--yuv-range=tv"], "m.y4m", "--yuv-range"), (["--fps=0"], "m.y4m", "--fps"), (["--fps=25:0"], "m.y4m", "--fps"),
             (["--fps=25:"], "m.y4m", "--fps"), (["--fps=ntsc"], "m.y4m", "--fps"), (["--fps=-25"], "m.y4m", "--fps"),
             (["--fps=30000:1001x"], "m.y4m", "--fps"), (["--fps=29.97"], "m.y4m", "--fps")]
    for extra, out, word in cases:
        p = subprocess.run([CLI, "-F", "3", "-s", "8x8"] + extra + [src, str(tmp_path / out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=60)
        assert p.returncode != 0 and p.stderr.startswith("Error:") and word in p.stderr, (extra, p.stderr)
    assert not list(tmp_path.iterdir())
