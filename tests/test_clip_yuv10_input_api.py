"""10-bit planar Y'CbCr 4:2:0 clip input without a GPU (mmhip_clip_from_yuv420p10, include/mmhip.h): the properties of the
restatement tests/yuv10_input_reference.py, its Fraction-derived tables against the ones the headers list, csrc/mm_yuv.h
compiled for the host in a stand-alone program and compared bit for bit, the stream header of either depth, read_y4m in its
three modes and the ValueErrors of set_image_yuv420p10."""
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
from tests import yuv10_input_reference as R
from tests import yuv10_reference as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mathmap_amd", "csrc")
CASES = [(mode, chroma) for mode in R.MODES for chroma in R.CHROMAS]
# the legal luma codes of a range
LEGAL = {"limited": (64, 940), "full": (0, 1023)}
# The largest distance of a sample after out -> in -> out from the sample after out, over the 200 000 colours of
# round_trip_colours(): measured with the two restatements, per mode.
ROUND_TRIP_MAX = {("bt601", "limited"): 1, ("bt601", "full"): 1, ("bt709", "limited"): 1, ("bt709", "full"): 1}


def err():
    return lib().mmhip_last_error().decode()


def test_entry_points_exist_and_are_declared():
    names = ("mmhip_clip_from_yuv420p10", "mmhip_clip_from_yuv420p10_launches", "mmhip_set_image_sequence_yuv420p10_host",
             "mmhip_clip_yuv10_input_groups", "mmhip_y4m_parse_stream_header")
    for name in names:
        assert name in _lib.SYMBOLS and getattr(lib(), name) is not None, name
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name, value in (("MMHIP_YUV10_IN_PATH_ALIGNED", 0), ("MMHIP_YUV10_IN_PATH_SAMPLES", 1)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(_lib, name) == value
    flat = " ".join(header.split())
    assert ("int mmhip_clip_from_yuv420p10(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, "
            "int num_frames, int matrix, int range, int chroma, void *dst_float4, int64_t dst_frame_stride, void *stream);") in flat
    assert ("int mmhip_set_image_sequence_yuv420p10_host(mmhip_invocation *inv, int index, const uint16_t *yuv, int64_t frame_stride, int width, "
            "int height, int num_frames, int matrix, int range, int chroma);") in flat
    assert ("int mmhip_y4m_parse_stream_header(const char *buf, int len, int *width, int *height, int *fps_num, int *fps_den, int *range, int *bits, "
            "int *header_len);") in flat
    for name in ("set_image_yuv420p10", "clip_from_yuv420p10", "clip_from_yuv420p10_launches", "clip_yuv10_input_groups"):
        assert hasattr(mm.api.Invocation, name), name
    text = open(os.path.join(CSRC, "clip_yuv10_in.hip")).read()
    assert "k_yuv420p10_to_float_clip" in text and '#include "mm_yuv.h"' in text and '"yuv420p10_to_float_clip"' in text
    assert "__shared__" not in text                                        # nothing is staged through LDS
    assert re.search(r"^HIP_SRCS\s*=.*\bclip_yuv10_in\.hip\b", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    kernels = open(os.path.join(CSRC, "clip_kernels.h")).read()
    assert "launch_yuv420p10_to_float_clip" in kernels and "check_yuv420p10_to_float_clip" in kernels
    for phrase in ("S = 9 * C[cy][cx] + 3 * C[cy][nx] + 3 * C[ny][cx] + C[ny][nx]", "min(s, 1023)", "G = (L + uf * gcb) + vf * gcr", "__fdiv_rn",
                   "There is no clamp", "MMHIP_YUV10_IN_COLUMNS", "MMHIP_YUV10_IN_STORES", "tests/yuv10_input_reference.py", "-0.07305936f", "1.0947489f"):
        assert phrase in flat, phrase


# ---- the restatement's own properties ----

def test_the_coefficients_are_the_nearest_floats():
    """nearest_float32 proves each against both neighbours when the module is imported; here the exact values by hand for
    one mode and the signs and sizes of all."""
    from fractions import Fraction as F
    rcr, gcb, gcr, bcb = R.exact_coefficients(("bt709", "limited"))
    assert rcr == F(7874, 5000) / (16 * 896) and bcb == F(9278, 5000) / (16 * 896)
    assert gcb == -F(9278, 5000) * F(722, 10000) / F(7152, 10000) / (16 * 896)
    assert gcr == -F(7874, 5000) * F(2126, 10000) / F(7152, 10000) / (16 * 896)
    for mode in R.MODES:
        off, e, (rcr, gcb, gcr, bcb) = R.TABLES[mode]
        assert (off, e) == ((64, 876) if mode[1] == "limited" else (0, 1023))
        assert all(c.dtype == np.float32 for c in (rcr, gcb, gcr, bcb))
        assert rcr > 0 and bcb > 0 and gcb < 0 and gcr < 0
        for c, q in zip((rcr, gcb, gcr, bcb), R.exact_coefficients(mode)):
            assert abs(F(float(c)) - q) <= abs(q) * F(1, 2 ** 24)          # half a unit in the last place at most
    with pytest.raises(AssertionError):
        R.nearest_float32(F(float(np.float32(1) + np.float32(2.0 ** -23)) + float(np.float32(1))) / 2)      # a tie has no nearest


def test_the_headers_list_the_derived_tables():
    header = " ".join(open(os.path.join(ROOT, "include", "mmhip.h")).read().split())
    shared = re.sub(r"\s+", "", open(os.path.join(CSRC, "mm_yuv.h")).read())
    for mode in R.MODES:
        off, e, coefficients = R.TABLES[mode]
        texts = R.hex_table(mode)
        for text, c in zip(texts, coefficients):
            assert np.float32(float.fromhex(text[:-1])) == c and float.fromhex(text[:-1]) == float(c), text      # the literal is the float, exactly
        assert "%s %s %d %d %s" % (mode[0], mode[1], off, e, " ".join(texts)) in header, mode
        assert "{%d,%d.0f,%s}" % (off, e, ",".join(texts)) in shared, mode


@pytest.mark.parametrize("mode", R.MODES, ids="-".join)
def test_grey_black_white_and_the_ends_of_the_code_range(mode):
    off, e, _ = R.TABLES[mode]
    y = np.arange(1024)
    grey = np.full(1024, 16 * 512)
    r, g, b = R.matrix(y, grey, grey, mode)
    assert np.array_equal(r.view(np.uint32), g.view(np.uint32)) and np.array_equal(g.view(np.uint32), b.view(np.uint32))
    assert r.dtype == np.float32 and (np.diff(r) > 0).all()
    assert r[off].view(np.uint32) == 0 and r[off + e] == np.float32(1.0)          # +0.0 and 1.0, exactly
    if mode[1] == "limited":
        assert r[0] == np.float32(-0.07305936) and r[1023] == np.float32(1.0947489)
    else:
        assert r[0] == 0 and r[1023] == 1
    # a grey frame on through the 10-bit writer's quantiser and luma returns every legal code
    lo, hi = LEGAL[mode[1]]
    q = X.quant(np.stack([r, g, b], axis=-1))
    back = X.luma(q, mode)
    assert np.array_equal(back[lo:hi + 1], y[lo:hi + 1]), mode
    cb, cr = X.chroma(4 * q.astype(np.int64), mode)
    assert (cb[lo:hi + 1] == 512).all() and (cr[lo:hi + 1] == 512).all()


def test_samples_above_ten_bits_read_as_1023_and_both_chroma_modes_agree_on_flat_chroma():
    w, h = 6, 4
    yuv = np.random.default_rng(3).integers(0, 65536, R.frame_samples(w, h)).astype(np.uint16)
    capped = np.minimum(yuv, 1023)
    for mode, chroma in CASES:
        assert np.array_equal(R.float_frame(yuv, w, h, mode, chroma).view(np.uint32), R.float_frame(capped, w, h, mode, chroma).view(np.uint32))
    flat = capped.copy()
    flat[w * h:w * h + 6] = 300
    flat[w * h + 6:] = 700
    a, b = R.float_frame(flat, w, h, ("bt709", "limited"), "bilinear"), R.float_frame(flat, w, h, ("bt709", "limited"), "replicate")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (a[..., 3] == 1).all()
    # the seen chroma is exact at scale 16: 9 + 3 + 3 + 1 parts
    plane = np.array([[0, 1023], [512, 4]])
    seen = R.seen_chroma16(plane, 4, 4, "bilinear")
    assert seen[0, 0] == 0 and seen[0, 1] == 12 * 0 + 4 * 1023 and seen[1, 1] == 9 * 0 + 3 * 1023 + 3 * 512 + 4
    assert seen[3, 3] == 16 * 4 and seen[2, 2] == 9 * 4 + 3 * 512 + 3 * 1023 + 0
    assert np.array_equal(R.seen_chroma16(plane, 4, 4, "replicate"), 16 * np.repeat(np.repeat(plane, 2, 0), 2, 1))


def round_trip_colours():
    """200 000 colours in gamut, seeded: float32 [250, 1600, 3] laid out as a frame of 2 x 2-constant blocks 500 x 3200."""
    blocks = np.random.default_rng(2024).random((250, 1600, 3), dtype=np.float32)
    return np.repeat(np.repeat(blocks, 2, axis=0), 2, axis=1)


@pytest.mark.parametrize("mode", R.MODES, ids="-".join)
def test_out_in_out_over_a_seeded_set(mode):
    """out -> in -> out with block-constant chroma and replicate mode: the largest move of any sample, measured over the
    seeded set and pinned."""
    frame = round_trip_colours()
    h, w = frame.shape[:2]
    first = X.frame(frame, mode)
    again = X.frame(R.float_frame(first, w, h, mode, "replicate"), mode)
    worst = int(np.abs(again.astype(np.int64) - first.astype(np.int64)).max())
    print("out -> in -> out, %s %s: max %d" % (mode[0], mode[1], worst))
    assert worst == ROUND_TRIP_MAX[mode]


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
    if (!mm_yuv_mode_known(matrix, range) || !mm_yuv_chroma_known(chroma)) return 3;
    std::vector<uint16_t> src((size_t)(mm_yuv10_frame_bytes(w, h) / 2));
    std::vector<float> dst((size_t)w * h * 4);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(src.data(), 2, src.size(), f) != src.size()) return 4;
    fclose(f);
    mm_yuv10_to_float_frame_host(MM_YUV10_FLOAT_MODES[matrix][range], chroma, src.data(), w, h, dst.data());
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
    d = tempfile.mkdtemp(prefix="mm_yuv10_in_")
    open(os.path.join(d, "t.cpp"), "w").write(PROGRAM)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param else ["-O2"]
    exe = os.path.join(d, "t")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + ["-I", CSRC, "-o", exe, os.path.join(d, "t.cpp")], check=True)

    def convert(yuv, w, h, mode, chroma):
        np.ascontiguousarray(yuv, np.uint16).tofile(os.path.join(d, "in.bin"))
        r = subprocess.run([exe, os.path.join(d, "in.bin"), str(w), str(h), str(R.MATRIX_IDS[mode[0]]), str(R.RANGE_IDS[mode[1]]),
                            str(R.CHROMA_IDS[chroma]), os.path.join(d, "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return np.fromfile(os.path.join(d, "out.bin"), np.float32).reshape(h, w, 4)
    yield convert
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("size", [(1, 1), (2, 1), (1, 2), (3, 5), (8, 2), (17, 9)], ids=lambda s: "%dx%d" % s)
def test_the_host_frame_is_the_restatements_bit_for_bit(host_program, size):
    w, h = size
    yuv = np.random.default_rng(10 * w + h).integers(0, 65536, R.frame_samples(w, h)).astype(np.uint16)      # the min is exercised
    assert (yuv > 1023).any()
    for mode, chroma in CASES:
        got = host_program(yuv, w, h, mode, chroma)
        assert np.array_equal(got.view(np.uint32), R.float_frame(yuv, w, h, mode, chroma).view(np.uint32)), (size, mode, chroma)


def test_the_host_frame_over_every_code_at_grey(host_program):
    w, h = 1024, 2
    yuv = np.concatenate([np.tile(np.arange(1024, dtype=np.uint16), 2), np.full(2 * 512, 512, np.uint16)])
    for mode, chroma in CASES:
        got = host_program(yuv, w, h, mode, chroma)
        assert np.array_equal(got.view(np.uint32), R.float_frame(yuv, w, h, mode, chroma).view(np.uint32)), (mode, chroma)
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 1], got[..., 2])


# ---- the stream header of either depth ----

def test_the_stream_header_of_either_depth():
    parse = mm.api.y4m_parse_stream_header
    assert parse(b"YUV4MPEG2 W8 H6 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL\nFRAME\n") == (8, 6, (30000, 1001), "full", 61, "yuv420p10")
    assert parse(X.y4m_header(17, 9, (24, 1), "limited")) == (17, 9, (24, 1), "limited", len(X.y4m_header(17, 9, (24, 1), "limited")), "yuv420p10")
    assert parse(b"YUV4MPEG2 W8 H6 C420p10\n") == (8, 6, (25, 1), None, 24, "yuv420p10")
    # everything the 8-bit parser accepts, with the same values
    for line in (b"YUV4MPEG2 W8 H6\n", b"YUV4MPEG2 W8 H6 C420jpeg\n", b"YUV4MPEG2 W8 H6 C420mpeg2 XCOLORRANGE=LIMITED\n", b"YUV4MPEG2 W8 H6 C420paldv I?\n",
                 b"YUV4MPEG2 H6 W8 C420 F24:1 A4:3 XYSCSS=420JPEG\n", mm.api.y4m_header(640, 480, (25, 1), "full")):
        assert parse(line) == mm.api.y4m_parse_header(line) + ("yuv420p",), line
    # and the same refusals, under its own name
    for line, word in ((b"YUV4MPEG2 W8 H6 C444\n", "colour space `C444'"), (b"YUV4MPEG2 W8 H6 C420p12\n", "colour space `C420p12'"),
                       (b"YUV4MPEG2 W8 H6 C422p10\n", "colour space `C422p10'"), (b"YUV4MPEG2 W8 H6 Cmono\n", "colour space `Cmono'"),
                       (b"YUV4MPEG2 W8 H6 It\n", "interlaced"), (b"YUV4MPEG W8 H6\n", "magic word"), (b"YUV4MPEG2 W8\n", "W and H"),
                       (b"YUV4MPEG2 W0 H6 C420p10\n", "W and H"), (b"YUV4MPEG2 W8 H6 F25\n", "frame rate"), (b"YUV4MPEG2 W8 H6 C420p10", "no newline"),
                       (b"YUV4MPEG2 W8 H6 C420p10 Q1\n", "header tag `Q1'")):
        with pytest.raises(ValueError, match=re.escape(word)) as e:
            parse(line)
        assert str(e.value).startswith("y4m_parse_stream_header: "), str(e.value)
    # the C function with null outputs
    line = b"YUV4MPEG2 W8 H6 C420p10\n"
    assert lib().mmhip_y4m_parse_stream_header(line, len(line), *[None] * 7) == 0
    bits = C.c_int(0)
    assert lib().mmhip_y4m_parse_stream_header(line, len(line), None, None, None, None, None, C.byref(bits), None) == 0 and bits.value == 10
    # the old parser keeps refusing the 10-bit colour space, in its own words
    with pytest.raises(ValueError, match=r"y4m_parse_header: the colour space `C420p10' is not 8-bit 4:2:0 \(C420jpeg, C420mpeg2, C420paldv or C420\)"):
        mm.api.y4m_parse_header(line)


# ---- read_y4m ----

def test_read_y4m_in_its_three_modes(tmp_path):
    w, h, n = 5, 3, 3
    deep = np.random.default_rng(1).integers(0, 1024, (n, R.frame_samples(w, h))).astype(np.uint16)
    flat = np.random.default_rng(2).integers(0, 256, (n, R.frame_samples(w, h)), dtype=np.uint8)
    deep_path, flat_path = str(tmp_path / "deep.y4m"), str(tmp_path / "flat.y4m")
    mm.api.write_y4m(deep_path, deep, w, h, fps=(30, 1), yuv_range="full")
    mm.api.write_y4m(flat_path, flat, w, h, fps=(24, 1))
    assert open(deep_path, "rb").read() == X.y4m_file(deep, w, h, (30, 1), "full")
    for pixel_format in ("yuv420p10", "any"):
        yuv, gw, gh, fps, rng = mm.api.read_y4m(deep_path, pixel_format=pixel_format)
        assert yuv.dtype == np.uint16 and np.array_equal(yuv, deep) and (gw, gh, fps, rng) == (w, h, (30, 1), "full")
    yuv = mm.api.read_y4m(io.BytesIO(open(deep_path, "rb").read()), max_frames=2, pixel_format="yuv420p10")[0]
    assert yuv.shape == (2, R.frame_samples(w, h)) and np.array_equal(yuv, deep[:2])
    want = R.parse_y4m(open(deep_path, "rb").read())
    assert np.array_equal(want[0], deep) and want[1:] == (w, h, (30, 1), "full")
    # the samples are little-endian in the file: 0x0123 is the bytes 23 01
    one = np.full((1, R.frame_samples(2, 2)), 0x0123, np.uint16)
    data = io.BytesIO()
    mm.api.write_y4m(data, one, 2, 2)
    assert data.getvalue().endswith(b"FRAME\n" + b"\x23\x01" * 6)
    assert np.array_equal(mm.api.read_y4m(io.BytesIO(data.getvalue()), pixel_format="any")[0], one)
    # 8-bit streams: the default and "any" read them, "yuv420p10" refuses them by name
    for keywords in ({}, dict(pixel_format="yuv420p"), dict(pixel_format="any")):
        yuv, gw, gh, fps, rng = mm.api.read_y4m(flat_path, **keywords)
        assert yuv.dtype == np.uint8 and np.array_equal(yuv, flat) and (gw, gh, fps, rng) == (w, h, (24, 1), "limited")
    with pytest.raises(ValueError, match="reads streams of colour space C420p10, and this one holds 8-bit samples"):
        mm.api.read_y4m(flat_path, pixel_format="yuv420p10")
    # the default keeps refusing 10-bit streams
    for keywords in ({}, dict(pixel_format="yuv420p")):
        with pytest.raises(ValueError, match="y4m_parse_header: the colour space `C420p10' is not 8-bit"):
            mm.api.read_y4m(deep_path, **keywords)
    with pytest.raises(ValueError, match="pixel_format must be one of yuv420p, yuv420p10, any"):
        mm.api.read_y4m(deep_path, pixel_format="yuv422p10")
    # a truncated 10-bit frame, with its byte counts
    data = open(deep_path, "rb").read()
    fb = R.frame_bytes(w, h)
    with pytest.raises(ValueError, match="read_y4m: frame 2 is truncated: %d of %d bytes" % (fb - 3, fb)):
        mm.api.read_y4m(io.BytesIO(data[:-3]), pixel_format="yuv420p10")
    with pytest.raises(ValueError, match="read_y4m: frame 1 is truncated: 1 of %d bytes" % fb):
        mm.api.read_y4m(io.BytesIO(data[:len(data) - fb - 6 - fb + 1]), pixel_format="any")
    assert inspect.signature(mm.api.read_y4m).parameters["pixel_format"].default == "yuv420p"


# ---- the Python setter's own refusals ----

def test_python_argument_errors():
    """Refused before anything else is looked at (an invocation needs a GPU; the checks do not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    inv.render_width, inv.render_height = 16, 8
    good = np.zeros((2, 192), np.uint16)
    for matrix in ("bt2020", "BT709", None, 1):
        with pytest.raises(ValueError, match="yuv_matrix"):
            inv.set_image_yuv420p10("in", good, 16, 8, yuv_matrix=matrix)
        with pytest.raises(ValueError, match="yuv_matrix"):
            inv.clip_from_yuv420p10(0x1000, 0x2000, 2, yuv_matrix=matrix)
    for rng in ("tv", "Full", None, 0):
        with pytest.raises(ValueError, match="yuv_range"):
            inv.set_image_yuv420p10("in", good, 16, 8, yuv_range=rng)
        with pytest.raises(ValueError, match="yuv_range"):
            inv.clip_from_yuv420p10(0x1000, 0x2000, 2, yuv_range=rng)
    for chroma in ("nearest", "Bilinear", None, 0, ""):
        with pytest.raises(ValueError, match="chroma must be one of bilinear, replicate"):
            inv.set_image_yuv420p10("in", good, 16, 8, chroma=chroma)
        with pytest.raises(ValueError, match="chroma must be one of"):
            inv.clip_from_yuv420p10(0x1000, 0x2000, 2, chroma=chroma)
    for bad in (np.zeros((2, 191), np.uint16), np.zeros((2, 193), np.uint16), np.zeros((2, 192), np.int16), np.zeros((2, 192), np.uint8),
                np.zeros((2, 384), np.uint8), np.zeros((2, 192), np.float32), np.zeros((0, 192), np.uint16), np.zeros((2, 8, 24), np.uint16)):
        with pytest.raises(ValueError, match=r"set_image_yuv420p10: uint16 \[N, 192\] for frames of 16 x 8"):
            inv.set_image_yuv420p10("in", bad, 16, 8)
    with pytest.raises(ValueError, match="at least 1"):
        inv.set_image_yuv420p10("in", good, 0, 8)
    with pytest.raises(ValueError, match="path must be"):
        inv.clip_from_yuv420p10_launches("bytes")
    sig = inspect.signature(mm.api.Invocation.set_image_yuv420p10).parameters
    assert sig["yuv_matrix"].default == "bt709" and sig["yuv_range"].default == "limited" and sig["chroma"].default == "bilinear"


def test_the_call_refuses_bad_arguments_by_name():
    """The converter's checks come before the invocation is looked at: without one, a call that passes them all says so."""
    def refused(src=0x1000, stride=384, w=16, h=8, n=2, matrix=1, rng=0, chroma=0, dst=0x2000, dst_stride=2048):
        assert lib().mmhip_clip_from_yuv420p10(None, C.c_void_p(src), stride, w, h, n, matrix, rng, chroma, C.c_void_p(dst), dst_stride, None) == -1
        return err()
    assert refused() == "clip_from_yuv420p10: no invocation"
    assert refused(w=0) == "clip_from_yuv420p10: width and height must be at least 1, not 0 x 8"
    assert refused(n=0) == "clip_from_yuv420p10: num_frames must be at least 1"
    assert refused(n=65536) == "clip_from_yuv420p10: more than 65535 frames in one call (65536); convert the clip in groups"
    assert refused(matrix=2) == "clip_from_yuv420p10: matrix must be MMHIP_YUV_BT601 or MMHIP_YUV_BT709 (0 or 1), not 2"
    assert refused(rng=-1) == "clip_from_yuv420p10: range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL (0 or 1), not -1"
    assert refused(chroma=2) == "clip_from_yuv420p10: chroma must be MMHIP_YUV_CHROMA_BILINEAR or MMHIP_YUV_CHROMA_REPLICATE (0 or 1), not 2"
    assert refused(src=0) == refused(dst=0) == "clip_from_yuv420p10: src_yuv and dst_float4 must be device pointers"
    assert refused(src=0x1001) == refused(stride=385) == "clip_from_yuv420p10: src_yuv and src_frame_stride must be even (the samples are 16-bit)"
    assert refused(stride=382) == "clip_from_yuv420p10: src_frame_stride 382 is smaller than one frame (384 bytes)"
    assert refused(dst=0x2008) == "clip_from_yuv420p10: dst_float4 is not 16-byte aligned (float4 texels)"
    assert refused(dst_stride=2056) == "clip_from_yuv420p10: dst_frame_stride 2056 is not a multiple of 16"
    assert refused(dst_stride=2032) == "clip_from_yuv420p10: dst_frame_stride 2032 is smaller than one frame (2048 bytes)"
    assert refused(w=16384, h=16385, stride=1 << 40, dst_stride=1 << 40) == "clip_from_yuv420p10: a destination frame of more than 4 GiB"
    assert refused(w=16384, h=16384, stride=1 << 40, dst_stride=1 << 40) == "clip_from_yuv420p10: no invocation"          # exactly 4 GiB
    assert lib().mmhip_set_image_sequence_yuv420p10_host(None, 0, None, 384, 16, 8, 2, 1, 0, 0) == -1
    assert err() == "set_image_sequence_yuv420p10_host: the pixels are a null pointer"
