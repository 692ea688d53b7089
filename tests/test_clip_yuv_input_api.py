"""Planar Y'CbCr 4:2:0 clip input without a GPU (mmhip_clip_from_yuv420, include/mmhip.h): the entry points and the
header's statement, the restatement tests/yuv_input_reference.py and its properties, csrc/mm_yuv.h compiled for the host
in a stand-alone program (plain and under the sanitizers), the round trip through the output direction, the Y4M header
parser and reader, every refusal by its name, the Python keywords and the command line's options."""
import ctypes as C
import inspect
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
from tests import yuv_input_reference as R
from tests import yuv_reference as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
CSRC = os.path.join(ROOT, "mathmap_amd", "csrc")
CORNERS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]


def err():
    return lib().mmhip_last_error().decode()


def test_entry_points_exist_and_are_declared():
    api = mm.api
    for name in ("mmhip_clip_from_yuv420", "mmhip_clip_from_yuv420_launches", "mmhip_set_image_sequence_yuv420_host", "mmhip_clip_yuv_input_groups",
                 "mmhip_y4m_parse_header"):
        assert name in _lib.SYMBOLS and getattr(lib(), name) is not None, name
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name, value in (("MMHIP_YUV_CHROMA_BILINEAR", 0), ("MMHIP_YUV_CHROMA_REPLICATE", 1), ("MMHIP_YUV_IN_PATH_ALIGNED", 0), ("MMHIP_YUV_IN_PATH_BYTES", 1)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(_lib, name) == value
    assert api.YUV_CHROMAS == {"bilinear": _lib.MMHIP_YUV_CHROMA_BILINEAR, "replicate": _lib.MMHIP_YUV_CHROMA_REPLICATE} == R.CHROMA_IDS
    flat = " ".join(header.split())
    assert ("int mmhip_clip_from_yuv420(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames, "
            "int matrix, int range, int chroma, void *dst_rgba32, int64_t dst_frame_stride, void *stream);") in flat
    assert ("int mmhip_set_image_sequence_yuv420_host(mmhip_invocation *inv, int index, const uint8_t *yuv, int64_t frame_stride, int width, "
            "int height, int num_frames, int matrix, int range, int chroma);") in flat
    assert "int mmhip_clip_yuv_input_groups(mmhip_invocation *inv);" in flat
    assert ("int mmhip_y4m_parse_header(const char *buf, int len, int *width, int *height, int *fps_num, int *fps_den, int *range, "
            "int *header_len);") in flat
    assert lib().mmhip_clip_from_yuv420.argtypes == [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int] * 6 + [C.c_void_p, C.c_int64, C.c_void_p]
    assert lib().mmhip_set_image_sequence_yuv420_host.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_int64] + [C.c_int] * 6
    for name in ("set_image_yuv420", "clip_from_yuv420", "clip_yuv_input_groups"):
        assert hasattr(api.Invocation, name)
    for name in ("read_y4m", "y4m_parse_header", "yuv_chroma"):
        assert hasattr(api, name)
    # the kernel is in a file on the Makefile's list, over the shared header
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    sources = re.search(r"^HIP_SRCS\s*=(.*)$", makefile, re.M).group(1).split()
    assert any("k_yuv420_to_rgba_clip" in open(os.path.join(CSRC, name)).read() and '#include "mm_yuv.h"' in open(os.path.join(CSRC, name)).read()
               for name in sources)
    text = open(os.path.join(CSRC, "mm_yuv.h")).read()
    for name in ("mm_yuv_rgba_mode", "MM_YUV_RGBA_MODES", "mm_yuv_to_rgba", "mm_yuv_chroma_replicate", "mm_yuv_chroma_bilinear", "mm_yuv_to_rgba_frame_host"):
        assert name in text, name


def test_the_header_states_the_arithmetic_and_the_table():
    header = " ".join(open(os.path.join(ROOT, "include", "mmhip.h")).read().split())
    for phrase in ("y = Y - off, u = Cb' - 128, v = Cr' - 128", "R = clamp((ky * y + rcr * v + 2^15) >> 16, 0, 255)",
                   "G = clamp((ky * y + gcb * u + gcr * v + 2^15) >> 16, 0, 255)", "B = clamp((ky * y + bcb * u + 2^15) >> 16, 0, 255)",
                   "R << 24 | G << 16 | B << 8 | 255", "C' = (9 * C[cy][cx] + 3 * C[cy][nx] + 3 * C[ny][cx] + C[ny][nx] + 8) >> 4",
                   "nx = clamp(cx + (x & 1 ? 1 : -1), 0, cw - 1)", "sample (x >> 1, y >> 1)", "floor(|k| * 2^16 + 0.5)", "yuv420_to_rgba_clip",
                   "MMHIP_YUV_IN_STORES", "MMHIP_CLIP_YUV_IN_BYTES", "read as centre-sited", "C420jpeg", "floor division"):
        assert phrase in header, phrase
    for (matrix, rng), row in R.TABLES.items():
        text = "%s %s %s" % (matrix, rng, " ".join(map(str, row)))
        assert text in header, text


@pytest.mark.parametrize("mode", R.MODES, ids="-".join)
def test_the_table_is_the_rule_applied_to_kr_and_kb(mode):
    assert R.derived(mode) == R.TABLES[mode]


# ---- the properties of the arithmetic ----

@pytest.mark.parametrize("mode", R.MODES, ids="-".join)
def test_white_black_and_grey(mode):
    limited = mode[1] == "limited"
    rgb = lambda y, cb, cr: tuple(int(c) for c in R.matrix(y, cb, cr, mode))
    assert rgb(235 if limited else 255, 128, 128) == (255, 255, 255)
    assert rgb(16 if limited else 0, 128, 128) == (0, 0, 0)
    v = np.arange(256)
    r, g, b = R.matrix(v, np.full(256, 128), np.full(256, 128), mode)
    if limited:
        assert (r == g).all() and (g == b).all() and (np.diff(r) >= 0).all() and r[:17].max() == 0 and r[235:].min() == 255
    else:
        assert np.array_equal(r, v) and np.array_equal(g, v) and np.array_equal(b, v)


@pytest.mark.parametrize("mode", R.MODES, ids="-".join)
def test_no_intermediate_leaves_int32_for_any_byte_triple(mode):
    # every intermediate is a sum of terms each monotone in one sample: its extremes over all triples lie at the corners
    y, cb, cr = [a.reshape(-1) for a in np.meshgrid([0, 255], [0, 255], [0, 255], indexing="ij")]
    worst = max(int(np.abs(v).max()) for v in R.intermediates(y, cb, cr, mode))
    assert worst < 2 ** 31 - 1
    assert worst < 2 ** 26          # (and by a wide margin)
    # and over a full sweep of two samples with the third at its corners
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for fixed in (0, 255):
        for args in ((a, b, np.full_like(a, fixed)), (a, np.full_like(a, fixed), b), (np.full_like(a, fixed), a, b)):
            assert max(int(np.abs(v).max()) for v in R.intermediates(*args, mode)) <= worst


def test_bilinear_equals_replicate_on_constant_chroma():
    rng = np.random.default_rng(4)
    for w, h in ((5, 3), (8, 2), (17, 9)):
        cw, ch = R.chroma_size(w, h)
        payload = np.concatenate([rng.integers(0, 256, w * h, dtype=np.uint8), np.full(cw * ch, 77, np.uint8), np.full(cw * ch, 201, np.uint8)])
        for mode in R.MODES:
            assert np.array_equal(R.rgba_frame(payload, w, h, mode, "bilinear"), R.rgba_frame(payload, w, h, mode, "replicate"))
    # and they differ on chroma that is not constant
    payload = rng.integers(0, 256, R.frame_bytes(8, 4), dtype=np.uint8)
    assert not np.array_equal(R.rgba_frame(payload, 8, 4, R.MODES[0], "bilinear"), R.rgba_frame(payload, 8, 4, R.MODES[0], "replicate"))


def test_bilinear_weights_by_hand():
    # 4 x 2: one chroma row of two samples, 100 and 200: rows blend with themselves, columns 0 and 3 with themselves
    plane = np.array([[100, 200]], np.uint8)
    seen = R.seen_chroma(plane, 4, 2, "bilinear")
    assert seen.tolist() == [[100, (12 * 100 + 4 * 200 + 8) >> 4, (12 * 200 + 4 * 100 + 8) >> 4, 200]] * 2 == [[100, 125, 175, 200]] * 2
    # 2 x 4: one chroma column of two samples
    seen = R.seen_chroma(np.array([[100], [200]], np.uint8), 2, 4, "bilinear")
    assert seen.tolist() == [[100, 100], [125, 125], [175, 175], [200, 200]]
    # the corner weights 9, 3, 3, 1 at pixel (1, 1) of a 4 x 4 frame
    plane = np.array([[16, 32], [64, 128]], np.uint8)
    assert R.seen_chroma(plane, 4, 4, "bilinear")[1, 1] == (9 * 16 + 3 * 32 + 3 * 64 + 128 + 8) >> 4 == 35
    assert R.seen_chroma(plane, 4, 4, "replicate").tolist() == [[16, 16, 32, 32], [16, 16, 32, 32], [64, 64, 128, 128], [64, 64, 128, 128]]


# ---- the round trip through the output direction ----

def block_clip(colours, bw):
    """uint8 [K, 3] -> one frame [1, 2 K / bw, 2 bw, 4] of 2 x 2 blocks of one colour each."""
    k = len(colours)
    assert k % bw == 0
    blocks = colours.reshape(k // bw, bw, 3)
    frame = np.repeat(np.repeat(blocks, 2, axis=0), 2, axis=1)
    return np.concatenate([frame, np.full(frame.shape[:2] + (1,), 255, np.uint8)], axis=2)[None]


@pytest.mark.parametrize("mode", R.MODES, ids="-".join)
def test_round_trip_of_constant_blocks_is_within_the_bound(mode):
    """RGB -> 4:2:0 (tests/yuv_reference.py) -> RGB on 2 x 2-constant blocks with replicate chroma: within 2 per channel at
    limited range, within 1 at full range, over 2 * 10^6 seeded random colours, the corners and the greys."""
    bound = 2 if mode[1] == "limited" else 1
    greys = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    # through whole frames: the corners, the greys and random colours, 32768 blocks
    rng = np.random.default_rng(20)
    colours = np.concatenate([np.array(CORNERS, np.uint8), greys, rng.integers(0, 256, (32768 - 264, 3), dtype=np.uint8)])
    clip = block_clip(colours, 256)
    h, w = clip.shape[1:3]
    back = R.rgba_frames(X.frames(clip, mode), w, h, mode, "replicate")
    diff = np.abs(back[..., :3].astype(int) - clip[..., :3].astype(int))
    print("round trip %s-%s frames: max %d" % (mode + (diff.max(),)))
    assert diff.max() <= bound and (back[..., 3] == 255).all()
    # the same arithmetic on 2 * 10^6 colours: a constant block's luma is its colour's, its sums four times the colour
    colours = rng.integers(0, 256, (2000000, 3), dtype=np.uint8)
    cb, cr = X.chroma(4 * colours.astype(np.int64), mode)
    r, g, b = R.matrix(X.luma(colours, mode), cb, cr, mode)
    diff = np.abs(np.stack([r, g, b], axis=1) - colours.astype(np.int64))
    print("round trip %s-%s colours: max %d" % (mode + (diff.max(),)))
    assert diff.max() <= bound


# ---- mm_yuv.h on the host ----

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mm_yuv.h"
// in width height matrix range chroma out
int main(int argc, char **argv) {
    if (argc != 8) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]), matrix = atoi(argv[4]), range = atoi(argv[5]), chroma = atoi(argv[6]);
    if (!mm_yuv_mode_known(matrix, range) || !mm_yuv_chroma_known(chroma) || mm_yuv_chroma_known(2) || mm_yuv_chroma_known(-1)) return 3;
    std::vector<unsigned char> src((size_t)mm_yuv_frame_bytes(w, h));
    std::vector<uint32_t> dst((size_t)w * h);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size()) return 4;
    fclose(f);
    mm_yuv_to_rgba_frame_host(MM_YUV_RGBA_MODES[matrix][range], chroma, src.data(), w, h, dst.data());
    f = fopen(argv[7], "wb");
    if (!f || fwrite(dst.data(), 4, dst.size(), f) != dst.size()) return 6;
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitizers"])
def host_program(request):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tempfile.mkdtemp(prefix="mm_yuv_in_")
    open(os.path.join(d, "t.cpp"), "w").write(PROGRAM)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param else ["-O2"]
    exe = os.path.join(d, "t")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, "-o", exe, os.path.join(d, "t.cpp")], check=True)

    def convert(payload, w, h, mode, chroma):
        """-> uint8 [h, w, 4] RGBA, from the words the program wrote"""
        np.asarray(payload, np.uint8).tofile(os.path.join(d, "in.bin"))
        r = subprocess.run([exe, os.path.join(d, "in.bin"), str(w), str(h), str(R.MATRIX_IDS[mode[0]]), str(R.RANGE_IDS[mode[1]]),
                            str(R.CHROMA_IDS[chroma]), os.path.join(d, "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        word = np.fromfile(os.path.join(d, "out.bin"), np.uint32).reshape(h, w)
        return np.stack([word >> 24, (word >> 16) & 255, (word >> 8) & 255, word & 255], axis=-1).astype(np.uint8)
    yield convert
    shutil.rmtree(d, ignore_errors=True)


def one_pixel(luma, cb, cr):
    """bt709 limited, with the table's numbers written out."""
    y, u, v = luma - 16, cb - 128, cr - 128
    clamp = lambda x: max(0, min(255, x))
    return [clamp((76309 * y + 117489 * v + 32768) >> 16), clamp((76309 * y - 13975 * u - 34925 * v + 32768) >> 16),
            clamp((76309 * y + 138438 * u + 32768) >> 16), 255]


def test_a_frame_worked_out_sample_by_sample(host_program):
    """5 x 3: Y 15 bytes, Cb and Cr 3 x 2 each.  The last column and the last row have chroma samples of their own."""
    luma = [[16, 235, 126, 63, 32], [173, 81, 145, 41, 210], [0, 255, 100, 16, 235]]
    cb = [[128, 102, 240], [42, 16, 255]]
    cr = [[128, 240, 118], [26, 0, 200]]
    payload = np.array(sum(luma, []) + sum(cb, []) + sum(cr, []), np.uint8)
    assert len(payload) == 27 == R.frame_bytes(5, 3)
    # a few samples through to the colour: black, white, the textbook red (63, 102, 240), green and blue -- each within 1
    # of the pure colour, exactly (255.51, 0.58, -0.20), (-0.05, 255.50, 1.14) and (0.70, 0.08, 255.22) before the floor --
    # and out-of-range samples, clamped: (0, 255, 0) is (-248.1, 22.50, 249.64), (255, 0, 255) is (505.97, 237.90, 7.90)
    assert one_pixel(16, 128, 128) == [0, 0, 0, 255] and one_pixel(235, 128, 128) == [255, 255, 255, 255]
    assert one_pixel(63, 102, 240) == [255, 1, 0, 255] and one_pixel(173, 42, 26) == [0, 255, 1, 255] and one_pixel(32, 240, 118) == [1, 0, 255, 255]
    assert one_pixel(0, 255, 0) == [0, 23, 250, 255] and one_pixel(255, 0, 255) == [255, 238, 8, 255]
    # replicate: pixel (x, y) takes sample (x >> 1, y >> 1)
    want = [[one_pixel(luma[y][x], cb[y >> 1][x >> 1], cr[y >> 1][x >> 1]) for x in range(5)] for y in range(3)]
    got = host_program(payload, 5, 3, ("bt709", "limited"), "replicate")
    assert got.tolist() == want
    assert got[0, 0].tolist() == [0, 0, 0, 255] and got[0, 1].tolist() == [255, 255, 255, 255]
    # bilinear: the neighbour column of x is cx - 1 (x even) or cx + 1 (x odd) inside 0 .. 2, the neighbour row of y is
    # cy - 1 (y even) or cy + 1 (y odd) inside 0 .. 1; weights 9, 3, 3, 1, rounded once
    nx = [0, 1, 0, 2, 1]      # x = 0 .. 4: cx = 0, 0, 1, 1, 2
    ny = [0, 1, 0]            # y = 0 .. 2: cy = 0, 0, 1
    def seen(c, x, y):
        return (9 * c[y >> 1][x >> 1] + 3 * c[y >> 1][nx[x]] + 3 * c[ny[y]][x >> 1] + c[ny[y]][nx[x]] + 8) >> 4
    assert seen(cb, 0, 0) == 128 and seen(cb, 1, 0) == (12 * 128 + 4 * 102 + 8) >> 4 == 122
    assert seen(cb, 1, 1) == (9 * 128 + 3 * 102 + 3 * 42 + 16 + 8) >> 4 == 100 and seen(cr, 4, 2) == (9 * 200 + 3 * 0 + 3 * 118 + 240 + 8) >> 4 == 150
    want = [[one_pixel(luma[y][x], seen(cb, x, y), seen(cr, x, y)) for x in range(5)] for y in range(3)]
    got = host_program(payload, 5, 3, ("bt709", "limited"), "bilinear")
    assert got.tolist() == want
    for mode in R.MODES:
        for chroma in R.CHROMAS:
            assert np.array_equal(host_program(payload, 5, 3, mode, chroma), R.rgba_frame(payload, 5, 3, mode, chroma)), (mode, chroma)


def test_the_corner_colours_in_every_mode(host_program):
    """16 x 2: the planes tests/yuv_reference.py makes of the 8 corner colours, one 2 x 2 block each, and back."""
    rgba = np.zeros((2, 16, 4), np.uint8)
    for k, c in enumerate(CORNERS):
        rgba[:, 2 * k:2 * k + 2, :3] = c
    for mode in R.MODES:
        payload = X.frame(rgba, mode)
        for chroma in R.CHROMAS:
            got = host_program(payload, 16, 2, mode, chroma)
            assert np.array_equal(got, R.rgba_frame(payload, 16, 2, mode, chroma)), (mode, chroma)
        back = host_program(payload, 16, 2, mode, "replicate")
        assert np.abs(back[..., :3].astype(int) - rgba[..., :3].astype(int)).max() <= (2 if mode[1] == "limited" else 1)
        assert (back[..., 3] == 255).all()
    # every byte value in every plane: out-of-range samples are clamped, not refused
    payload = np.random.default_rng(9).integers(0, 256, R.frame_bytes(17, 9), dtype=np.uint8)
    payload[:4] = (0, 255, 1, 254)
    for mode in R.MODES:
        for chroma in R.CHROMAS:
            assert np.array_equal(host_program(payload, 17, 9, mode, chroma), R.rgba_frame(payload, 17, 9, mode, chroma)), (mode, chroma)


# ---- the header parser and the reader ----

def parse(text):
    data = text if isinstance(text, bytes) else text.encode()
    out = [C.c_int(-7) for _ in range(6)]
    rc = lib().mmhip_y4m_parse_header(data, len(data), *[C.byref(v) for v in out])
    return rc, tuple(v.value for v in out)


def test_parse_header_accepts_what_the_statement_lists():
    line = mm.api.y4m_header(1920, 1080, (30000, 1001), "full")
    assert parse(line + b"FRAME\n") == (0, (1920, 1080, 30000, 1001, 1, len(line)))
    line = mm.api.y4m_header(17, 9)
    assert parse(line) == (0, (17, 9, 25, 1, 0, len(line)))
    for tag in ("C420jpeg", "C420mpeg2", "C420paldv", "C420"):
        assert parse("YUV4MPEG2 W8 H6 F24:1 Ip A1:1 %s\n" % tag) == (0, (8, 6, 24, 1, -1, 31 + len(tag))), tag
    assert parse("YUV4MPEG2 W8 H6 F24:1\n") == (0, (8, 6, 24, 1, -1, 22))                      # no C tag
    assert parse("YUV4MPEG2 W8 H6\nFRAME\n") == (0, (8, 6, 25, 1, -1, 16))                     # no F: 25:1
    assert parse("YUV4MPEG2 H6 W8 I? A0:0\n")[:2] == (0, (8, 6, 25, 1, -1, 24))
    assert parse("YUV4MPEG2 W8 H6 XYSCSS=420JPEG XCOLORRANGE=LIMITED XFOO\n")[1][4] == 0       # other X tags are ignored
    assert parse("YUV4MPEG2 W8 H6 XCOLORRANGE=FULL XYSCSS=420JPEG\n")[1][4] == 1
    assert mm.api.y4m_parse_header(b"YUV4MPEG2 W8 H6 F50:2 XCOLORRANGE=FULL\nrest") == (8, 6, (50, 2), "full", 39)
    assert mm.api.y4m_parse_header(b"YUV4MPEG2 W8 H6\n")[3] is None
    assert mm.api.y4m_parse_header(X.y4m_header(3, 5, (25, 1), "limited"))[:4] == (3, 5, (25, 1), "limited")


def test_parse_header_refuses_by_name():
    cases = [("YUV4MPEG3 W8 H6\n", "magic word YUV4MPEG2"), ("RIFF....AVI \n", "magic word"), ("", "magic word"), ("YUV4MPEG2X W8 H6\n", "magic word"),
             ("YUV4MPEG2 H6\n", "W and H"), ("YUV4MPEG2 W8\n", "W and H"), ("YUV4MPEG2 W0 H6\n", "W and H"), ("YUV4MPEG2 W8 H-6\n", "W and H"),
             ("YUV4MPEG2 W8 H6 It\n", "interlaced"), ("YUV4MPEG2 W8 H6 Ib\n", "interlaced"), ("YUV4MPEG2 W8 H6 Im\n", "interlaced"),
             ("YUV4MPEG2 W8 H6 C422\n", "colour space `C422'"), ("YUV4MPEG2 W8 H6 C444\n", "colour space `C444'"),
             ("YUV4MPEG2 W8 H6 C420p10\n", "colour space `C420p10'"), ("YUV4MPEG2 W8 H6 Cmono\n", "colour space `Cmono'"),
             ("YUV4MPEG2 W8 H6 C444alpha\n", "colour space"), ("YUV4MPEG2 W8 H6 F25\n", "frame rate"), ("YUV4MPEG2 W8 H6 F0:1\n", "frame rate"),
             ("YUV4MPEG2 W8 H6 F25:1", "no newline"), ("YUV4MPEG2 W8 H6 " + "A" * 80, "no newline")]
    for text, word in cases:
        rc, _ = parse(text)
        assert rc == -1 and err().startswith("y4m_parse_header: ") and word in err(), (text, err())
        with pytest.raises(ValueError, match="y4m_parse_header"):
            mm.api.y4m_parse_header(text.encode())


def test_read_y4m_round_trip_frame_parameters_and_refusals(tmp_path):
    rng = np.random.default_rng(12)
    for w, h in ((3, 3), (8, 2), (17, 9)):
        buf = rng.integers(0, 256, (4, R.frame_bytes(w, h)), dtype=np.uint8)
        path = str(tmp_path / ("clip%dx%d.y4m" % (w, h)))
        mm.api.write_y4m(path, buf, w, h, fps=(30000, 1001), yuv_range="full")
        yuv, gw, gh, fps, yuv_range = mm.api.read_y4m(path)
        assert (gw, gh, fps, yuv_range) == (w, h, (30000, 1001), "full")
        assert yuv.dtype == np.uint8 and np.array_equal(yuv, buf)
        want = R.parse_y4m(open(path, "rb").read())
        assert np.array_equal(want[0], buf) and want[1:] == (w, h, (30000, 1001), "full")
        assert np.array_equal(mm.api.read_y4m(path, max_frames=2)[0], buf[:2]) and np.array_equal(mm.api.read_y4m(path, max_frames=9)[0], buf)
        with open(path, "rb") as f:      # a file object stays open and stands behind the frames read
            assert np.array_equal(mm.api.read_y4m(f, max_frames=1)[0], buf[:1])
            assert f.read(6) == b"FRAME\n"
    # FRAME parameters, no XCOLORRANGE, no F
    w, h = 17, 9
    data = b"YUV4MPEG2 W17 H9 C420mpeg2\n" + b"FRAME Ip\n" + buf[0].tobytes() + b"FRAME\n" + buf[1].tobytes() + b"FRAME XFOO=1 Ip\n" + buf[2].tobytes()
    yuv, gw, gh, fps, yuv_range = mm.api.read_y4m(io.BytesIO(data))
    assert (gw, gh, fps, yuv_range) == (17, 9, (25, 1), None) and np.array_equal(yuv, buf[:3])
    assert np.array_equal(R.parse_y4m(data)[0], buf[:3])
    with pytest.raises(ValueError, match="frame 2 is truncated: 242 of 243 bytes"):
        mm.api.read_y4m(io.BytesIO(data[:-1]))
    assert np.array_equal(mm.api.read_y4m(io.BytesIO(data[:-1]), max_frames=2)[0], buf[:2])      # (never read, never missed)
    with pytest.raises(ValueError, match="frame 1 does not begin with a FRAME line"):
        mm.api.read_y4m(io.BytesIO(data.replace(b"FRAME\n", b"FRAMES\n")))
    with pytest.raises(ValueError, match="frame 0 does not begin with a FRAME line"):
        mm.api.read_y4m(io.BytesIO(b"YUV4MPEG2 W17 H9\n" + buf[0].tobytes()))
    with pytest.raises(ValueError, match="the file has no frames"):
        mm.api.read_y4m(io.BytesIO(b"YUV4MPEG2 W17 H9\n"))
    with pytest.raises(ValueError, match="colour space `C444'"):
        mm.api.read_y4m(io.BytesIO(b"YUV4MPEG2 W17 H9 C444\nFRAME\n"))
    with pytest.raises(ValueError, match="max_frames"):
        mm.api.read_y4m(io.BytesIO(data), max_frames=0)


# ---- refusals ----

def refused(**over):
    args = dict(src=0x1000, stride=None, w=16, h=8, n=2, matrix=1, rng=0, chroma=0, dst=0x2000, dst_stride=None)
    args.update(over)
    w, h = args["w"], args["h"]
    stride = R.frame_bytes(max(w, 1), max(h, 1)) if args["stride"] is None else args["stride"]
    dst_stride = 4 * w * h if args["dst_stride"] is None else args["dst_stride"]
    rc = lib().mmhip_clip_from_yuv420(None, args["src"], stride, w, h, args["n"], args["matrix"], args["rng"], args["chroma"], args["dst"], dst_stride, None)
    assert rc == -1
    return err()


def test_the_call_refuses_bad_arguments_by_name():
    """Every check comes before the invocation is looked at: no GPU."""
    assert refused() == "clip_from_yuv420: no invocation"
    assert refused(w=0).startswith("clip_from_yuv420: width and height must be at least 1")
    assert refused(h=-3).startswith("clip_from_yuv420: width and height must be at least 1")
    assert refused(n=0) == "clip_from_yuv420: num_frames must be at least 1"
    assert refused(n=65536).startswith("clip_from_yuv420: more than 65535 frames")
    assert refused(n=65535) == "clip_from_yuv420: no invocation"
    for matrix in (-1, 2):
        assert refused(matrix=matrix).startswith("clip_from_yuv420: matrix must be MMHIP_YUV_BT601 or MMHIP_YUV_BT709")
    for rng in (-1, 2):
        assert refused(rng=rng).startswith("clip_from_yuv420: range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL")
    for chroma in (-1, 2):
        assert refused(chroma=chroma).startswith("clip_from_yuv420: chroma must be MMHIP_YUV_CHROMA_BILINEAR or MMHIP_YUV_CHROMA_REPLICATE")
    assert refused(src=0).endswith("must be device pointers") and refused(dst=0).endswith("must be device pointers")
    assert refused(stride=191) == "clip_from_yuv420: src_frame_stride 191 is smaller than one frame (192 bytes)"
    assert refused(stride=192) == "clip_from_yuv420: no invocation"
    assert refused(dst_stride=511) == "clip_from_yuv420: dst_frame_stride 511 is not a multiple of 4"
    assert refused(dst_stride=514) == "clip_from_yuv420: dst_frame_stride 514 is not a multiple of 4"
    assert refused(dst_stride=508) == "clip_from_yuv420: dst_frame_stride 508 is smaller than one frame (512 bytes)"
    assert refused(dst_stride=516) == "clip_from_yuv420: no invocation"
    assert refused(w=32768, h=32769) == "clip_from_yuv420: a destination frame of more than 4 GiB"
    assert refused(w=32768, h=32768) == "clip_from_yuv420: no invocation"          # exactly 4 GiB


def test_python_argument_errors():
    """Refused before anything else is looked at (an invocation needs a GPU; the checks do not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    inv.render_width, inv.render_height = 16, 8
    good = np.zeros((2, 192), np.uint8)
    for matrix in ("bt2020", "BT709", None, 1):
        with pytest.raises(ValueError, match="yuv_matrix"):
            inv.set_image_yuv420("in", good, 16, 8, yuv_matrix=matrix)
        with pytest.raises(ValueError, match="yuv_matrix"):
            inv.clip_from_yuv420(0x1000, 0x2000, 2, yuv_matrix=matrix)
    for rng in ("tv", "Full", None, 0):
        with pytest.raises(ValueError, match="yuv_range"):
            inv.set_image_yuv420("in", good, 16, 8, yuv_range=rng)
        with pytest.raises(ValueError, match="yuv_range"):
            inv.clip_from_yuv420(0x1000, 0x2000, 2, yuv_range=rng)
    for chroma in ("nearest", "Bilinear", None, 0, ""):
        with pytest.raises(ValueError, match="chroma must be one of bilinear, replicate"):
            inv.set_image_yuv420("in", good, 16, 8, chroma=chroma)
        with pytest.raises(ValueError, match="chroma must be one of"):
            inv.clip_from_yuv420(0x1000, 0x2000, 2, chroma=chroma)
    for bad in (np.zeros((2, 191), np.uint8), np.zeros((2, 193), np.uint8), np.zeros((2, 192), np.int8), np.zeros((0, 192), np.uint8),
                np.zeros((2, 8, 24), np.uint8), np.zeros((2, 8, 16, 3), np.uint8)):
        with pytest.raises(ValueError, match=r"set_image_yuv420: uint8 \[N, 192\] for frames of 16 x 8"):
            inv.set_image_yuv420("in", bad, 16, 8)
    with pytest.raises(ValueError, match="at least 1"):
        inv.set_image_yuv420("in", good, 0, 8)
    assert mm.api.yuv_chroma("bilinear") == 0 and mm.api.yuv_chroma("replicate") == 1
    sig = inspect.signature(mm.api.Invocation.set_image_yuv420).parameters
    assert sig["yuv_matrix"].default == "bt709" and sig["yuv_range"].default == "limited" and sig["chroma"].default == "bilinear"
    assert inspect.signature(mm.api.read_y4m).parameters["max_frames"].default is None


def test_cli_help_and_argument_errors(tmp_path):
    p = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0
    for phrase in ("-D<name>=FILE.y4m", "standard input", "--input-yuv-matrix=MATRIX", "--input-yuv-range=RANGE", "--input-chroma=MODE", "bilinear (default",
                   "replicate", "XCOLORRANGE", "--input-frames=NUM", "without -F every input", "takes the stream's frame rate"):
        assert phrase in p.stdout, phrase
    one = "filter f (image in) in(xy, frame) end"
    two = "filter f (image a, image b) a(xy, frame) + b(xy, frame) end"
    good = str(tmp_path / "good.y4m")
    mm.api.write_y4m(good, np.full((2, R.frame_bytes(8, 6)), 128, np.uint8), 8, 6)
    bad = {}
    for name, data in (("c444", b"YUV4MPEG2 W8 H6 C444\nFRAME\n" + bytes(144)), ("interlaced", b"YUV4MPEG2 W8 H6 It\nFRAME\n" + bytes(72)),
                       ("short", open(good, "rb").read()[:-5]), ("empty", b"YUV4MPEG2 W8 H6\n"), ("noframe", b"YUV4MPEG2 W8 H6\nFRAMING\n" + bytes(72)),
                       ("png", b"\x89PNG\r\n\x1a\n")):
        bad[name] = str(tmp_path / (name + ".y4m"))
        open(bad[name], "wb").write(data)
    out = str(tmp_path / "out.y4m")
    cases = [(["--input-yuv-matrix=bt2020", "-Din=" + good], one, "--input-yuv-matrix"), (["--input-yuv-range=tv", "-Din=" + good], one, "--input-yuv-range"),
             (["--input-chroma=nearest", "-Din=" + good], one, "--input-chroma"), (["--input-chroma=", "-Din=" + good], one, "--input-chroma"),
             (["--input-yuv-matrix=bt601", "-Din=in.png"], one, "go with an input image whose file name ends in .y4m"),
             (["--input-yuv-range=full", "-s", "8x8"], "filter f () rgba:[t, 0, 0, 1] end", "go with an input image"),
             (["--input-chroma=replicate", "-Din=movie.y4m.png"], one, "go with an input image"),
             (["-Da=-", "-Db=-"], two, "At most one input image can be read from standard input"),
             (["-Din=" + bad["c444"]], one, "colour space `C444'"), (["-Din=" + bad["interlaced"]], one, "interlaced"),
             (["-Din=" + bad["short"]], one, "frame 1 is truncated"), (["-Din=" + bad["empty"]], one, "has no frames"),
             (["-Din=" + bad["noframe"]], one, "frame 0 does not begin with a FRAME line"), (["-Din=" + bad["png"]], one, "magic word YUV4MPEG2"),
             (["-Din=" + str(tmp_path / "missing.y4m")], one, "Could not read input stream")]
    for extra, src, word in cases:
        p = subprocess.run([CLI] + extra + [src, out], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and p.stderr.startswith("Error:") and word in p.stderr, (extra, p.stderr)
    assert not os.path.exists(out)
